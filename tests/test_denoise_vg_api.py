"""The variance-guided denoiser, the interface, without a GPU: the entry points are declared, bound and exported, the struct layout,
the code object holds the kernels, and denoise_vg_config / render_denoised check their arguments before any device call."""
import ctypes as C
import os
import re

import pytest

from accum_helpers import ERR_INVALID, ROOT, kernel_id

NEW_SYMBOLS = ("srt_denoise_features_vg", "srt_denoise_vg_kat", "srt_denoise_estimate_last_ms")
INF, NAN = float("inf"), float("nan")


def header():
    return open(os.path.join(ROOT, "include", "srt_c_api.h")).read()


def test_new_symbols_are_declared_bound_and_exported(srt):
    text = header()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, text), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, fp, cfg = C.c_uint32, C.POINTER(C.c_float), C.POINTER(srt.binding.DenoiseVG)
    assert srt.binding.PROTOTYPES["srt_denoise_features_vg"] == (C.c_int, [C.c_void_p, cfg, fp, fp, fp, fp, u32, u32])
    assert srt.binding.PROTOTYPES["srt_denoise_vg_kat"] == (C.c_int, [C.c_void_p, cfg, fp, fp, u32, u32, u32, fp, fp])
    assert srt.binding.PROTOTYPES["srt_denoise_estimate_last_ms"] == (C.c_int, [C.c_void_p, fp])
    assert "denoise_vg_config" in srt.__all__ and callable(srt.denoise_vg_config)
    for attr in ("denoise_vg", "denoise_vg_kat", "denoise_estimate_last_ms"):
        assert hasattr(srt.Renderer, attr), attr
    assert not hasattr(srt.Comm, "denoise_vg")      # a gathered denoise is out of scope
    # the filter is part of the contract the header states
    for phrase in ("if (g > 0 && (Y_q - Y_q) == 0) { s0 += g;  s1 += g * Y_q;  s2 += g * (Y_q * Y_q); }",
                   "mu = s1 / s0;  m2 = s2 / s0;  v = m2 - mu * mu;  v_p = (s0 > 0 && v > 0) ? v : 0.",
                   "k = b[dy+1] * b[dx+1];  bk += k;  bv += k * v_q;   vb_p = bv / bk.", "kc_p = ks * vb_p + vf.",
                   "wt = wt * e(dl, kc_p);", "if (wt > 0 && (dc - dc) == 0) { sw += wt;", "sv += (wt * wt) * v_q; }",
                   "sw > 0 ? (sx / sw, sy / sw, sz / sw, sv / (sw * sw)) : (c_p, v_p)."):
        assert phrase in text, phrase


def test_struct_layout_is_32_bytes(srt):
    D = srt.binding.DenoiseVG
    assert C.sizeof(D) == 32
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [("levels", 0), ("sigma_variance", 4), ("sigma_normal", 8), ("sigma_albedo", 12),
                                                                  ("sigma_depth", 16), ("variance_floor", 20), ("reserved", 24)]
    assert ("typedef struct srt_denoise_vg { uint32_t levels; float sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor; "
            "uint32_t reserved[2]; } srt_denoise_vg;") in header()


def test_code_object_holds_the_variance_guided_kernels_beside_the_plain_ones(srt):
    names = [n for n, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH) if "denoise" in n]
    for want in ("denoise_variance_kernel", "denoise_level_vg_kernelILb1E", "denoise_level_vg_kernelILb0E", "denoise_var_out_kernel",
                 "denoise_level_kernelILb1E", "denoise_level_kernelILb0E"):
        assert sum(want in n for n in names) == 1, (want, names)


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    cfg = srt.denoise_vg_config()
    assert lib.srt_denoise_features_vg(None, C.byref(cfg), None, None, None, None, 1, 1) == ERR_INVALID
    assert lib.srt_denoise_vg_kat(None, C.byref(cfg), None, None, 1, 1, 1, None, None) == ERR_INVALID
    assert lib.srt_denoise_estimate_last_ms(None, None) == ERR_INVALID


def test_denoise_vg_config_defaults_and_values(srt):
    c = srt.denoise_vg_config()
    assert (c.levels, c.sigma_variance, c.sigma_normal, c.sigma_albedo) == (5, 2.0, 0.5, 0.25)
    assert abs(c.sigma_depth - 0.1) < 1e-8 and abs(c.variance_floor - 1e-8) < 1e-15 and list(c.reserved) == [0, 0]
    c = srt.denoise_vg_config(levels=0, sigma_variance=1e30, sigma_normal=INF, sigma_albedo=1e39, sigma_depth=1e-30, variance_floor=INF)
    assert c.levels == 0 and c.sigma_variance > 1e29 and c.sigma_normal == INF and c.sigma_albedo == INF and c.sigma_depth > 0 and c.variance_floor == INF
    assert srt.denoise_vg_config(levels=8, variance_floor=1e39).variance_floor == INF
    assert "starting values" in srt.denoise_vg_config.__doc__


BAD_CONFIGS = [dict(levels=9), dict(levels=-1), dict(levels=2.5), dict(levels=True), dict(levels="3"),
               dict(sigma_variance=0.0), dict(sigma_variance=-1.0), dict(sigma_variance=NAN), dict(sigma_variance=INF), dict(sigma_variance=1e39),
               dict(sigma_variance=-INF), dict(sigma_variance=1e-50), dict(sigma_variance=None), dict(sigma_variance=True),
               dict(sigma_normal=NAN), dict(sigma_normal=0.0), dict(sigma_albedo=-INF), dict(sigma_albedo=-0.0), dict(sigma_depth=1e-50),
               dict(sigma_depth="wide"), dict(sigma_depth=-2.0),
               dict(variance_floor=0.0), dict(variance_floor=-0.0), dict(variance_floor=-1e-8), dict(variance_floor=NAN), dict(variance_floor=-INF),
               dict(variance_floor=1e-50), dict(variance_floor="low"), dict(sigma_color=1.0)]


@pytest.mark.parametrize("kw", BAD_CONFIGS, ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_denoise_vg_config_rejects(srt, kw):
    with pytest.raises((ValueError, TypeError) if "sigma_color" in kw else ValueError):
        srt.denoise_vg_config(**kw)


@pytest.mark.parametrize("kw", [dict(passes=[]), dict(passes=[4, -1]), dict(passes=[4], levels=9), dict(passes=[4], sigma_variance=INF),
                                dict(passes=[4], sigma_variance=0.0), dict(passes=[4], variance_floor=0.0), dict(passes=[4], variance_floor=NAN),
                                dict(passes=[4], sigma_depth=NAN)],
                         ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_render_denoised_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_denoised created a device context for arguments it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_denoised(None, None, 16, 16, bounce_limit=8, variance_guided=True, **kw)


def test_the_two_modes_take_their_own_keywords(srt, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device context was created")))
    with pytest.raises(TypeError):      # sigma_variance belongs to the variance-guided mode, sigma_color to the plain one
        srt.render_denoised(None, None, 16, 16, [4], 8, sigma_variance=1.0)
    with pytest.raises(TypeError):
        srt.render_denoised(None, None, 16, 16, [4], 8, variance_guided=True, sigma_color=1.0)


def test_renderer_methods_check_the_config_before_the_library(srt):
    r = object.__new__(srt.Renderer)      # no device context: a checked config never reaches the handle
    r._h = None
    with pytest.raises(ValueError):
        r.denoise_vg(4, 4, levels=9)
    with pytest.raises(ValueError):
        r.denoise_vg_kat(None, None, 1, variance_floor=0.0)
