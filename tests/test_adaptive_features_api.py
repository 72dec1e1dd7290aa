"""Adaptive featured accumulations and the measured-variance denoise, the interface, without a GPU: the entry points are declared,
bound and exported, the code object holds render_kernel<8, ...> for every shape the launcher picks and the two new denoise kernels, the
header states what the tests hold, and the Python side checks its arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from accum_helpers import ERR_INVALID, ROOT, SHAPES, kernel_id

NEW_SYMBOLS = ("srt_accum_reset_adaptive_features", "srt_denoise_features_mv", "srt_denoise_mv_kat", "srt_comm_accum_reset_adaptive_features")
MODE8_SYM = re.compile(r"^_ZN3srt13render_kernelILi8ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, fp, up = C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    ad, vg = C.POINTER(srt.binding.Adaptive), C.POINTER(srt.binding.DenoiseVG)
    P = srt.binding.PROTOTYPES
    assert P["srt_accum_reset_adaptive_features"] == (C.c_int, [C.c_void_p, ad]) == P["srt_accum_reset_adaptive"]
    assert P["srt_comm_accum_reset_adaptive_features"] == (C.c_int, [C.c_void_p, ad])
    assert P["srt_denoise_features_mv"] == (C.c_int, [C.c_void_p, vg, fp, fp, fp, fp, u32, u32]) == P["srt_denoise_features_vg"]
    assert P["srt_denoise_mv_kat"] == (C.c_int, [C.c_void_p, vg, fp, fp, up, fp, u32, u32, fp, fp])
    assert "render_adaptive_denoised" in srt.__all__ and callable(srt.render_adaptive_denoised)
    for attr in ("accum_reset_adaptive_features", "denoise_mv", "denoise_mv_kat"):
        assert hasattr(srt.Renderer, attr), attr
    assert hasattr(srt.Comm, "accum_reset_adaptive_features") and not hasattr(srt.Comm, "denoise_mv")
    # the claims and the estimator are part of the contract the header states
    for phrase in ("mean = S1 / n;  v = S2 / n - mean * mean;  v = v > 0 ? v : 0;  vm = v / (n - 1.0f);  v_p = (n_p >= 2 && (vm - vm) == 0) ? vm : 0",
                   "inv = 1.0f / (float)n_p", "render_kernel MODE 8", "bit-identical to an adaptive accumulation's (MODE 4)",
                   "holds the feature row of a PLAIN featured n-spp frame at that pixel, bit for bit",
                   "a converged pixel's row is not touched by later passes", "spp_total >= 2",
                   "equals srt_denoise_features at sigma_color = +inf"):
        assert phrase in header, phrase


def test_code_object_holds_every_adaptive_featured_variant_and_the_new_denoise_kernels(srt):
    found, names = set(), []
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        names.append(name)
        m = MODE8_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)
    hs = kernel_id().render_code_hashes(srt.binding.LIB_PATH)
    assert {k[1:] for k in hs if k[0] == 8} == SHAPES
    # six kernels of their own: no MODE 8 variant is the code of its MODE 4 or MODE 7 counterpart
    for shape in SHAPES:
        assert len({hs[(m,) + shape] for m in (4, 7, 8)}) == 3, shape
    for kernel in ("denoise_prepass_counts_kernel", "denoise_measured_kernel", "denoise_prepass_kernel", "denoise_variance_kernel"):
        assert any(kernel in n for n in names), kernel


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    cfg, vg = srt.binding.Adaptive(0.1, 0.0, 4, 0), srt.denoise_vg_config()
    assert lib.srt_accum_reset_adaptive_features(None, C.byref(cfg)) == ERR_INVALID
    assert lib.srt_comm_accum_reset_adaptive_features(None, C.byref(cfg)) == ERR_INVALID
    assert lib.srt_denoise_features_mv(None, C.byref(vg), None, None, None, None, 1, 1) == ERR_INVALID
    assert lib.srt_denoise_mv_kat(None, C.byref(vg), None, None, None, None, 1, 1, None, None) == ERR_INVALID


def no_device(*a, **k):
    raise AssertionError("a device context was created for arguments that must be rejected")


@pytest.mark.parametrize("kw", [dict(rel_tol=0.0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(rel_tol=0.1, abs_tol=float("inf")),
                                dict(rel_tol=0.1, min_spp=1), dict(rel_tol=0.1, min_spp=2.5), dict(rel_tol=0.1, step=0),
                                dict(rel_tol=0.1, min_spp=32, max_spp=16), dict(rel_tol=0.1, max_spp=65536), dict(rel_tol=0.1, variance="temporal"),
                                dict(rel_tol=0.1, variance=True), dict(rel_tol=0.1, levels=9), dict(rel_tol=0.1, sigma_variance=0.0),
                                dict(rel_tol=0.1, variance="measured", sigma_color=1.0), dict(rel_tol=0.1, variance=None, sigma_variance=1.0),
                                dict(rel_tol=0.1, variance=None, sigma_color=-1.0), dict(rel_tol=0.1, variance_floor=0.0)],
                         ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_render_adaptive_denoised_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises((ValueError, TypeError)):
        srt.render_adaptive_denoised(None, None, 16, 16, 8, **kw)


def test_render_adaptive_denoised_accepts_each_variance_mode_lazily(srt, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    for kw in (dict(variance="measured", sigma_variance=1.5), dict(variance="spatial", variance_floor=float("inf")), dict(variance=None, sigma_color=0.5), dict()):
        gen = srt.render_adaptive_denoised(None, None, 16, 16, 8, 0.1, **kw)      # a generator: nothing runs before the first next()
        assert hasattr(gen, "__next__")
        gen.close()


def test_denoise_mv_kat_checks_its_arrays_before_the_library(srt):
    r = srt.Renderer.__new__(srt.Renderer)      # no context: every case below must fail before the library is called
    r._h = None
    S, rows = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32)
    n, s2 = np.full((3, 5), 4, np.uint32), np.zeros((3, 5), np.float32)
    zero = n.copy(); zero[1, 2] = 0
    for args in ((S, rows[:, :4], n, s2), (S[..., :2], rows, n, s2), (S, rows, n[:2], s2), (S, rows, n, s2[:, :4]), (S, rows, zero, s2),
                 (S, rows, n.astype(np.float32), s2), (S, rows, -n.astype(np.int64), s2), (S, rows, n.astype(np.int64) << 31, s2)):
        with pytest.raises(ValueError):
            srt.Renderer.denoise_mv_kat(r, *args)
    with pytest.raises(ValueError):
        srt.Renderer.denoise_mv_kat(r, S, rows, n, s2, levels=9)
