"""The denoiser, the interface, without a GPU: the entry points are declared, bound and exported, the struct layout, the code object
holds the kernels, and denoise_config / render_denoised check their arguments before any device call."""
import ctypes as C
import os
import re

import pytest

from accum_helpers import ERR_INVALID, ROOT, kernel_id

NEW_SYMBOLS = ("srt_denoise_features", "srt_denoise_kat", "srt_denoise_last_ms")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, fp, cfg = C.c_uint32, C.POINTER(C.c_float), C.POINTER(srt.binding.Denoise)
    assert srt.binding.PROTOTYPES["srt_denoise_features"] == (C.c_int, [C.c_void_p, cfg, fp, fp, fp, u32, u32])
    assert srt.binding.PROTOTYPES["srt_denoise_kat"] == (C.c_int, [C.c_void_p, cfg, fp, fp, u32, u32, u32, fp])
    for name in ("denoise_config", "render_denoised"):
        assert name in srt.__all__ and callable(getattr(srt, name)), name
    for attr in ("denoise", "denoise_kat"):
        assert hasattr(srt.Renderer, attr), attr
    assert not hasattr(srt.Comm, "denoise")      # a gathered denoise is out of scope
    # the filter is part of the contract the header states
    for phrase in ("t = 1 - d2 / k;  t = (t > 0) ? t : 0;  return t * t", "h = {1/16, 1/4, 3/8, 1/4, 1/16}", "sigma_color * 2^-i",
                   "if (wt > 0) { sw += wt;", "z_p = F[7] > 0 ? F[6] / F[7] : 0", "adaptive + features is the intended next step"):
        assert phrase in header, phrase


def test_struct_layout_is_32_bytes(srt):
    D = srt.binding.Denoise
    assert C.sizeof(D) == 32
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [("levels", 0), ("sigma_color", 4), ("sigma_normal", 8), ("sigma_albedo", 12),
                                                                  ("sigma_depth", 16), ("reserved", 20)]
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    assert ("typedef struct srt_denoise { uint32_t levels; float sigma_color, sigma_normal, sigma_albedo, sigma_depth; uint32_t reserved[3]; } "
            "srt_denoise;") in header


def test_code_object_holds_the_denoise_kernels(srt):
    names = [n for n, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH) if "denoise" in n]
    for want in ("denoise_prepass_kernel", "denoise_level_kernelILb1E", "denoise_level_kernelILb0E", "denoise_epilogue_kernel"):
        assert sum(want in n for n in names) == 1, (want, names)


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    cfg = srt.denoise_config()
    assert lib.srt_denoise_features(None, C.byref(cfg), None, None, None, 1, 1) == ERR_INVALID
    assert lib.srt_denoise_kat(None, C.byref(cfg), None, None, 1, 1, 1, None) == ERR_INVALID
    assert lib.srt_denoise_last_ms(None, None, None, None, None) == ERR_INVALID


def test_denoise_config_defaults_and_values(srt):
    c = srt.denoise_config()
    assert (c.levels, c.sigma_color, c.sigma_normal, c.sigma_albedo) == (5, 1.0, 0.5, 0.25) and abs(c.sigma_depth - 0.1) < 1e-8
    assert list(c.reserved) == [0, 0, 0]
    c = srt.denoise_config(levels=0, sigma_color=float("inf"), sigma_normal=1e39, sigma_albedo=2, sigma_depth=1e-30)
    assert c.levels == 0 and c.sigma_color == float("inf") and c.sigma_normal == float("inf") and c.sigma_albedo == 2.0 and c.sigma_depth > 0
    assert srt.denoise_config(levels=8).levels == 8


BAD_CONFIGS = [dict(levels=9), dict(levels=-1), dict(levels=2.5), dict(levels=True), dict(levels="3"),
               dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")), dict(sigma_albedo=-float("inf")),
               dict(sigma_depth=1e-50), dict(sigma_depth="wide"), dict(sigma_normal=None), dict(sigma_color=True)]


@pytest.mark.parametrize("kw", BAD_CONFIGS, ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_denoise_config_rejects(srt, kw):
    with pytest.raises(ValueError):
        srt.denoise_config(**kw)


@pytest.mark.parametrize("kw", [dict(passes=[]), dict(passes=[0]), dict(passes=[4, -1]), dict(passes=[65535, 1]),
                                dict(passes=[4], levels=9), dict(passes=[4], sigma_color=0.0), dict(passes=[4], sigma_depth=float("nan"))],
                         ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_render_denoised_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_denoised created a device context for arguments it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_denoised(None, None, 16, 16, bounce_limit=8, **kw)


def test_renderer_methods_check_the_config_before_the_library(srt):
    r = object.__new__(srt.Renderer)      # no device context: a checked config never reaches the handle
    r._h = None
    with pytest.raises(ValueError):
        r.denoise(4, 4, levels=9)
    with pytest.raises(ValueError):
        r.denoise_kat(None, None, 1, sigma_color=-1.0)
