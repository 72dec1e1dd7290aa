"""Adaptive sampling without a GPU: the new entry points are declared, bound and exported, the library's gfx950 code object holds the
adaptive render kernel (render_kernel<4, ...>) for every shape the launcher picks, render_adaptive checks its arguments before any
device is touched, and the float32 restatement of the stopping criterion (which the GPU tests hold the kernel's decisions to) decides
the hand-made edge cases as the C-ABI documents them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from accum_helpers import ROOT, SHAPES, converged_f32, kernel_id

NEW_SYMBOLS = ("srt_accum_reset_adaptive", "srt_accum_active", "srt_read_accum_stats", "srt_comm_accum_reset_adaptive", "srt_comm_accum_active")
ADAPT_SYM = re.compile(r"^_ZN3srt13render_kernelILi4ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    assert re.search(r"typedef struct \{ float rel_tol, abs_tol; uint32_t min_spp, reserved; \} srt_adaptive;", header)
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    assert C.sizeof(srt.binding.Adaptive) == 16
    assert "render_adaptive" in srt.__all__ and callable(srt.render_adaptive)
    for attr in ("accum_reset_adaptive", "accum_active", "accum_stats"):
        assert hasattr(srt.Renderer, attr), attr
    for attr in ("accum_reset_adaptive", "accum_active"):
        assert hasattr(srt.Comm, attr), attr


def test_code_object_holds_every_adaptive_variant(srt):
    found = set()
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        m = ADAPT_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)


def test_production_kernels_are_still_found_by_kernel_id(srt):
    hs = kernel_id().code_hashes(srt.binding.LIB_PATH)
    assert set(hs) == {(1, 1, 1), (0, 0, 1), (1, 1), (1, 0), (0, 1), (0, 0)}, sorted(hs)


@pytest.mark.parametrize("kw", [
    dict(rel_tol=0.0), dict(rel_tol=0.0, abs_tol=0.0), dict(rel_tol=-0.1), dict(rel_tol=0.1, abs_tol=-1e-3), dict(rel_tol=math.nan),
    dict(rel_tol=math.inf), dict(rel_tol=0.1, abs_tol=math.inf), dict(rel_tol=1e39), dict(rel_tol="x"),
    dict(rel_tol=0.1, min_spp=1), dict(rel_tol=0.1, min_spp=0), dict(rel_tol=0.1, min_spp=2.5), dict(rel_tol=0.1, min_spp=True),
    dict(rel_tol=0.1, step=0), dict(rel_tol=0.1, step=-4), dict(rel_tol=0.1, step=1.5), dict(rel_tol=0.1, max_spp=65536),
    dict(rel_tol=0.1, min_spp=32, max_spp=16), dict(rel_tol=0.1, max_spp=None),
], ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_render_adaptive_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_adaptive created a device context for arguments it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_adaptive(None, None, 16, 16, 8, **kw)


def test_adaptive_schedule(srt):
    S = srt.renderer.adaptive_schedule
    assert S(8, 4, 24) == [8, 4, 4, 4, 4]
    assert S(16, 16, 1024) == [16] * 64
    assert S(16, 64, 1024) == [64] * 16
    assert S(16, 64, 100) == [64, 36]            # the last pass is clipped: the total reaches max_spp exactly
    assert S(32, 4, 40) == [32, 4, 4]            # the first pass is max(min_spp, step)
    assert S(2, 100, 50) == [50]
    assert sum(S(16, 7, 65535)) == 65535


def test_criterion_restatement_on_edge_cases():
    f = np.float32
    # zero variance: converged exactly when n reaches min_spp
    for n in (15, 16, 17):
        assert bool(converged_f32(f(0.5) * n, f(0.25) * n, n, 16, 1e-6, 0.0)) == (n >= 16), n
    # S2 / n < mean^2 by rounding: v < 0 is clamped to 0, so any tolerance > 0 stops the pixel
    s1, s2, n = f(1.0), f(0.0999), 10
    assert f(s2) / f(n) - (f(s1) / f(n)) * (f(s1) / f(n)) < 0
    assert bool(converged_f32(s1, s2, n, 2, 1e-6, 0.0))
    # NaN / inf anywhere: never converged, whatever the tolerance
    for a, b in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (3e38, 1.0)):
        assert not bool(converged_f32(f(a), f(b), 4, 2, 1e6, 1e6)), (a, b)
    # mean = 0: a black pixel (S1 = S2 = 0) stops on a relative tolerance alone; with S2 > 0 (not a real pixel: the restatement
    # only) it needs an absolute one
    assert bool(converged_f32(0.0, 0.0, 8, 2, 0.1, 0.0))
    assert not bool(converged_f32(0.0, 1e-3, 8, 2, 0.1, 0.0))
    assert bool(converged_f32(0.0, 1e-3, 8, 2, 0.1, 0.02))
    # a pixel just inside / just outside its tolerance: var_mean = (S2/n - mean^2) / (n - 1)
    n, mean = 16, f(0.5)
    s1 = mean * f(n)
    s2 = (mean * mean + f(0.01) * f(n - 1)) * f(n)        # var_mean ~ 0.01 -> needs tol >= ~0.1
    assert bool(converged_f32(s1, s2, n, 2, 0.21, 0.0))
    assert not bool(converged_f32(s1, s2, n, 2, 0.19, 0.0))
    # arrays: element-wise, float32 throughout
    out = converged_f32(np.array([0.0, 8.0, np.nan], f), np.array([0.0, 8.0, 0.0], f), np.array([4, 8, 8]), 4, 0.1, 0.0)
    assert out.tolist() == [True, True, False]
