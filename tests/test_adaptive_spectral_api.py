"""Adaptive spectral accumulations, the interface, without a GPU: the entry points are declared, bound and exported, the code object holds
render_kernel<10, ...> and <11, ...> for every shape the launcher picks and the two per-pixel-count kernels, the header states what the
tests hold, and the Python side checks its arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from accum_helpers import ERR_INVALID, ROOT, SHAPES, kernel_id

NEW_SYMBOLS = ("srt_accum_reset_adaptive_spectral", "srt_accum_reset_adaptive_spectral_features", "srt_comm_accum_reset_adaptive_spectral",
               "srt_comm_accum_reset_adaptive_spectral_features", "srt_denoise_developed_counts_kat")
NEW_SYM = re.compile(r"^_ZN3srt13render_kernelILi(10|11)ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, fp, vp = C.c_uint32, C.POINTER(C.c_float), C.c_void_p
    dn, ad = C.POINTER(srt.binding.Denoise), C.POINTER(srt.binding.Adaptive)
    P = srt.binding.PROTOTYPES
    for name in NEW_SYMBOLS[:4]:
        assert P[name] == (C.c_int, [vp, ad]) == P["srt_accum_reset_adaptive"], name
    assert P["srt_denoise_developed_counts_kat"] == (C.c_int, [vp, dn, fp, fp, fp, u32, C.POINTER(u32), u32, u32, fp, fp])
    assert "render_adaptive_spectral" in srt.__all__ and callable(srt.render_adaptive_spectral)
    for attr in ("accum_reset_adaptive_spectral", "accum_reset_adaptive_spectral_features"):
        assert hasattr(srt.Renderer, attr) and hasattr(srt.Comm, attr), attr
    assert hasattr(srt.Renderer, "denoise_developed_counts_kat") and not hasattr(srt.Comm, "denoise_developed_counts_kat")


def test_the_header_states_the_claims():
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    for phrase in ("render_kernel MODE 10 / MODE 11",
                   "state are bit-identical to an adaptive accumulation's (MODE 4)",
                   "holds the film row of a plain spectral n-spp frame at that pixel, bit for bit",
                   "a converged pixel's film row is never touched again",
                   "the eight feature sums are bit-identical to an adaptive featured accumulation's (MODE 8)",
                   "none of this depends on launch shape, partition, world size, chunk offset or the split into passes",
                   "d_p[k] = inv_p * D_p[k]", "inv_p = 1.0f / (float)n_p", "srt_accum_reset_adaptive_spectral, below",
                   "With a constant map it equals"):
        assert phrase in header, phrase


def test_code_object_holds_every_new_variant_and_the_per_pixel_count_kernels(srt):
    K = kernel_id()
    found, names = set(), []
    for name, _ in K.gfx950_functions(srt.binding.LIB_PATH):
        names.append(name)
        m = NEW_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == {(m,) + s for m in (10, 11) for s in SHAPES}, sorted(found)
    hs = K.render_code_hashes(srt.binding.LIB_PATH, K.RENDER_ALL)
    assert len(hs) == 72, len(hs)
    # twelve kernels of their own: no new variant is the code of a parent's counterpart, or of the other new mode's
    for shape in SHAPES:
        assert len({hs[(m,) + shape] for m in (4, 5, 8, 9, 10, 11)}) == 6, shape
    for kernel in ("develop_srgb_counts_kernel", "denoise_payload_prepass_counts_kernel"):
        assert sum(kernel in n for n in names) == 1, kernel
    # ... behind the kernels that were there
    for kernel in ("develop_srgb_kernel", "denoise_payload_prepass_kernel", "denoise_prepass_counts_kernel", "denoise_level_dev_kernelILb1E"):
        assert sum(kernel in n for n in names) == 1, kernel


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    cfg, dn = srt.binding.Adaptive(0.1, 0.0, 4, 0), srt.denoise_config()
    for name in NEW_SYMBOLS[:4]:
        assert getattr(lib, name)(None, C.byref(cfg)) == ERR_INVALID, name
    assert lib.srt_denoise_developed_counts_kat(None, C.byref(dn), None, None, None, 1, None, 1, 1, None, None) == ERR_INVALID


def no_device(*a, **k):
    raise AssertionError("a device context was created for arguments that must be rejected")


@pytest.mark.parametrize("kw", [dict(rel_tol=0.0), dict(rel_tol=-0.1), dict(rel_tol=float("nan")), dict(rel_tol=0.1, abs_tol=float("inf")),
                                dict(rel_tol=0.1, min_spp=1), dict(rel_tol=0.1, min_spp=2.5), dict(rel_tol=0.1, step=0),
                                dict(rel_tol=0.1, min_spp=32, max_spp=16), dict(rel_tol=0.1, max_spp=65536), dict(rel_tol=0.1, features=1),
                                # without features there is nothing to develop or denoise
                                dict(rel_tol=0.1, response=np.ones(95)), dict(rel_tol=0.1, filter=np.ones(95)), dict(rel_tol=0.1, levels=2),
                                dict(rel_tol=0.1, scale=2.0),
                                dict(rel_tol=0.1, features=True, response=np.zeros((17, 95))), dict(rel_tol=0.1, features=True, response=np.full(95, np.nan)),
                                dict(rel_tol=0.1, features=True, filter=np.ones(3)), dict(rel_tol=0.1, features=True, scale=float("nan")),
                                dict(rel_tol=0.1, features=True, levels=9), dict(rel_tol=0.1, features=True, sigma_color=0.0)],
                         ids=lambda kw: ",".join(sorted(kw)) + "-%d" % len(repr(kw)))
def test_render_adaptive_spectral_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_adaptive_spectral(None, None, 16, 16, 8, **kw)


def test_render_adaptive_spectral_rejects_an_unknown_keyword_before_touching_a_device(srt, monkeypatch):
    """a keyword that is not one of denoise_config's (here the variance-guided filter's) is a TypeError from denoise_config, as in
    render_developed_denoised; without features any such keyword is the ValueError of the cases above"""
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(TypeError):
        srt.render_adaptive_spectral(None, None, 16, 16, 8, 0.1, features=True, sigma_variance=1.0)
    with pytest.raises(ValueError):
        srt.render_adaptive_spectral(None, None, 16, 16, 8, 0.1, sigma_variance=1.0)


def test_render_adaptive_spectral_is_lazy(srt, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    for kw in (dict(), dict(abs_tol=0.01, min_spp=2, step=2, max_spp=6), dict(features=True),
               dict(features=True, response=np.ones((5, 95)), filter=np.full(95, 0.5), levels=2, scale=2.0)):
        gen = srt.render_adaptive_spectral(None, None, 16, 16, 8, 0.1, **kw)      # a generator: nothing runs before the first next()
        assert hasattr(gen, "__next__")
        gen.close()


def test_renderer_methods_check_their_arguments_before_the_library(srt):
    r = object.__new__(srt.Renderer)      # no device context: a checked argument never reaches the handle
    r._h = None
    c = object.__new__(srt.Comm)
    c._h = None
    for obj in (r, c):
        for method in (obj.accum_reset_adaptive_spectral, obj.accum_reset_adaptive_spectral_features):
            for args in ((0.0,), (-1.0,), (float("nan"),), (0.1, -1.0), (0.1, 0.0, 1), (0.1, 0.0, 2.5), ("x",)):
                with pytest.raises(ValueError):
                    method(*args)
    S, rows, dev = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32), np.zeros((3, 5, 4), np.float32)
    n = np.full((3, 5), 2, np.uint32)
    zero = n.copy(); zero[1, 2] = 0
    for args in ((S, rows[:, :4], dev, n), (S[..., :2], rows, dev, n), (S, rows, dev[:2], n), (S, rows, dev[..., :0], n),
                 (S, rows, np.zeros((3, 5, 17), np.float32), n), (S, rows, dev, 2), (S, rows, dev, n[:2]), (S, rows, dev, zero),
                 (S, rows, dev, n.astype(np.float32)), (S, rows, dev, n.astype(np.int64) - 3), (S, rows, dev, n.astype(bool))):
        with pytest.raises(ValueError):
            r.denoise_developed_counts_kat(*args)
    with pytest.raises(ValueError):
        r.denoise_developed_counts_kat(S, rows, dev, n, sigma_albedo=-1.0)
