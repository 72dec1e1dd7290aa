"""Spectral featured accumulations and the denoised developed film, the interface, without a GPU: the entry points are declared, bound
and exported, the code object holds render_kernel<9, ...> for every shape the launcher picks and the payload kernels, the header states
what the tests hold, and the Python side checks its arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from accum_helpers import ERR_INVALID, ROOT, SHAPES, kernel_id

NEW_SYMBOLS = ("srt_accum_reset_spectral_features", "srt_comm_accum_reset_spectral_features", "srt_denoise_developed", "srt_denoise_developed_kat")
MODE9_SYM = re.compile(r"^_ZN3srt13render_kernelILi9ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, f, fp, vp = C.c_uint32, C.c_float, C.POINTER(C.c_float), C.c_void_p
    dn = C.POINTER(srt.binding.Denoise)
    P = srt.binding.PROTOTYPES
    assert P["srt_accum_reset_spectral_features"] == (C.c_int, [vp]) == P["srt_accum_reset_spectral"] == P["srt_accum_reset_features"]
    assert P["srt_comm_accum_reset_spectral_features"] == (C.c_int, [vp])
    assert P["srt_denoise_developed"] == (C.c_int, [vp, dn, fp, u32, f, fp, fp, u32, u32])
    assert P["srt_denoise_developed_kat"] == (C.c_int, [vp, dn, fp, fp, fp, u32, u32, u32, u32, fp, fp])
    assert "render_developed_denoised" in srt.__all__ and callable(srt.render_developed_denoised)
    for attr in ("accum_reset_spectral_features", "denoise_developed", "denoise_developed_kat"):
        assert hasattr(srt.Renderer, attr), attr
    assert hasattr(srt.Comm, "accum_reset_spectral_features") and not hasattr(srt.Comm, "denoise_developed")


def test_the_header_states_the_claims_and_the_payload_operation():
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    for phrase in ("render_kernel MODE 9",
                   "the image, all nine planes, the XYZ sums, the RNG state and the 95 film sums are bit-identical to a spectral accumulation's (MODE 5)",
                   "the eight feature sums are bit-identical to a featured accumulation's (MODE 7)",
                   "independent of partition, world size, launch shape and split into passes",
                   "d_p[k] = inv * D_p[k]", "sd[k] += wt * d_q[k]", "sw > 0 ? sd[k] / sw : d_p[k]", "levels == 0 returns (c_p, d_p)",
                   "never on the payload", "bit-identical to srt_denoise_features' out_xyz",
                   # the sentences the earlier suites pin stay, with the pointer behind them
                   "adaptive + spectral is not supported", "adaptive + features is the intended next step",
                   "features combined with the spectral film or"):
        assert phrase in header, phrase
    assert header.count("srt_accum_reset_spectral_features, below") >= 2


def test_code_object_holds_every_spectral_featured_variant_and_the_payload_kernels(srt):
    found, names = set(), []
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        names.append(name)
        m = MODE9_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)
    hs = kernel_id().render_code_hashes(srt.binding.LIB_PATH)
    assert {k[1:] for k in hs if k[0] == 9} == SHAPES
    assert len(hs) == 60, len(hs)
    # six kernels of their own: no MODE 9 variant is the code of its MODE 5 or MODE 7 counterpart
    for shape in SHAPES:
        assert len({hs[(m,) + shape] for m in (5, 7, 9)}) == 3, shape
    for kernel in ("denoise_level_dev_kernelILb1E", "denoise_level_dev_kernelILb0E", "denoise_payload_prepass_kernel", "denoise_dev_out_kernel"):
        assert sum(kernel in n for n in names) == 1, kernel
    # ... behind the kernels that were there
    for kernel in ("denoise_level_kernelILb1E", "denoise_level_kernelILb0E", "denoise_prepass_kernel", "denoise_epilogue_kernel", "develop_kernelILi16E"):
        assert any(kernel in n for n in names), kernel


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    cfg = srt.denoise_config()
    assert lib.srt_accum_reset_spectral_features(None) == ERR_INVALID
    assert lib.srt_comm_accum_reset_spectral_features(None) == ERR_INVALID
    assert lib.srt_denoise_developed(None, C.byref(cfg), None, 1, 1.0, None, None, 1, 1) == ERR_INVALID
    assert lib.srt_denoise_developed_kat(None, C.byref(cfg), None, None, None, 1, 1, 1, 1, None, None) == ERR_INVALID


def no_device(*a, **k):
    raise AssertionError("a device context was created for arguments that must be rejected")


@pytest.mark.parametrize("kw", [dict(passes=[]), dict(passes=[0]), dict(passes=[65535, 1]), dict(passes=[4], response=np.zeros((17, 95))),
                                dict(passes=[4], response=np.full(95, np.nan)), dict(passes=[4], filter=np.ones(3)),
                                dict(passes=[4], scale=float("nan")), dict(passes=[4], response=np.ones(95), scale="big"),
                                dict(passes=[4], levels=9), dict(passes=[4], sigma_color=0.0), dict(passes=[4], sigma_depth=float("nan")),
                                dict(passes=[4], sigma_variance=1.0)],
                         ids=lambda kw: ",".join(sorted(kw)) + "-%d" % len(repr(kw)))
def test_render_developed_denoised_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises((ValueError, TypeError)):
        srt.render_developed_denoised(None, None, 16, 16, bounce_limit=8, **kw)


def test_render_developed_denoised_is_lazy(srt, monkeypatch):
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    for kw in (dict(), dict(response=np.ones((5, 95)), filter=np.full(95, 0.5), levels=2), dict(scale=2.0, sigma_color=float("inf"))):
        gen = srt.render_developed_denoised(None, None, 16, 16, [4, 4], 8, **kw)      # a generator: nothing runs before the first next()
        assert hasattr(gen, "__next__")
        gen.close()


def test_renderer_methods_check_their_arguments_before_the_library(srt):
    r = object.__new__(srt.Renderer)      # no device context: a checked argument never reaches the handle
    r._h = None
    with pytest.raises(ValueError):
        r.denoise_developed(4, 4, np.zeros((17, 95)))
    with pytest.raises(ValueError):
        r.denoise_developed(4, 4, np.ones(95), scale=float("inf"))
    with pytest.raises(ValueError):
        r.denoise_developed(4, 4, np.ones(95), filter=np.ones(4))
    with pytest.raises(ValueError):
        r.denoise_developed(4, 4, np.ones(95), levels=9)
    S, rows, dev = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5, 8), np.float32), np.zeros((3, 5, 4), np.float32)
    for args in ((S, rows[:, :4], dev, 1), (S[..., :2], rows, dev, 1), (S, rows, dev[:2], 1), (S, rows, dev[..., :0], 1),
                 (S, rows, np.zeros((3, 5, 17), np.float32), 1), (S, rows, dev[..., 0], 1), (S, rows, dev, 0), (S, rows, dev, 1.5)):
        with pytest.raises(ValueError):
            r.denoise_developed_kat(*args)
    with pytest.raises(ValueError):
        r.denoise_developed_kat(S, rows, dev, 1, sigma_albedo=-1.0)
