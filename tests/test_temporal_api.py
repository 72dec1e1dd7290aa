"""The Python face of the temporal reprojection without a GPU: temporal_config refuses what the library refuses, render_interactive checks
its arguments before any device is touched, and the binding declares the new symbols."""
import ctypes as C

import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")
SYMBOLS = ("srt_temporal_reset", "srt_temporal_accum", "srt_temporal_kat", "srt_denoise_features_temporal", "srt_present_temporal", "srt_temporal_last_ms")


def test_new_symbols_are_in_the_binding_and_the_library(srt):
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in SYMBOLS:
        assert name in srt.binding.PROTOTYPES and getattr(L, name) is not None, name
    B = srt.binding
    assert C.sizeof(B.Temporal) == 32 and C.sizeof(B.TemporalResult) == 48
    assert [f[0] for f in B.Temporal._fields_] == ["alpha_min", "max_len", "sigma_normal", "sigma_albedo", "sigma_depth", "reserved"]
    assert [f[0] for f in B.TemporalResult._fields_] == ["blended", "fresh", "offscreen", "rejected", "nonfinite", "history_frames", "history_dropped"]


def test_temporal_config_defaults_and_limits(srt):
    t = srt.temporal_config()
    assert (t.alpha_min, t.max_len, t.sigma_normal, t.sigma_albedo, t.sigma_depth) == tuple(float(np.float32(v)) for v in (0.1, 32, 0.5, 0.25, 0.1))
    assert list(t.reserved) == [0, 0, 0]
    assert srt.temporal_config(alpha_min=1.0, max_len=1).alpha_min == 1.0
    off = srt.temporal_config(sigma_normal=INF, sigma_albedo=INF, sigma_depth=1e60)      # (beyond float32: +inf, which switches the test off)
    assert off.sigma_normal == INF and off.sigma_albedo == INF and off.sigma_depth == INF
    assert srt.temporal_config(alpha_min=np.float32(1e-30)).alpha_min > 0


@pytest.mark.parametrize("kw", [
    dict(alpha_min=0.0), dict(alpha_min=-0.1), dict(alpha_min=1.0000001), dict(alpha_min=NAN), dict(alpha_min=1e-60), dict(alpha_min=INF),
    dict(alpha_min=True), dict(alpha_min="half"), dict(alpha_min=None),
    dict(max_len=0.99), dict(max_len=0), dict(max_len=-3), dict(max_len=INF), dict(max_len=NAN), dict(max_len=1e60), dict(max_len=None),
    dict(sigma_normal=0.0), dict(sigma_normal=-1.0), dict(sigma_normal=NAN), dict(sigma_albedo=0.0), dict(sigma_albedo=NAN), dict(sigma_albedo=-INF),
    dict(sigma_depth=0.0), dict(sigma_depth=NAN), dict(sigma_depth=-0.1), dict(sigma_depth=1e-60), dict(sigma_depth=False),
], ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_temporal_config_refuses(srt, kw):
    with pytest.raises(ValueError, match="temporal: " + next(iter(kw))):
        srt.temporal_config(**kw)


def test_temporal_stats_reads_the_result(srt):
    res = srt.binding.TemporalResult(5, 4, 3, 1, 2, 7, 1)
    assert srt.temporal_stats(res) == dict(blended=5, fresh=4, offscreen=3, rejected=1, nonfinite=2, history_frames=7, history_dropped=True)


def test_render_interactive_checks_before_the_device(srt):
    """every refusal is raised by the call itself -- a generator function would only raise at the first next() -- and with device=99, which
    does not exist: no device was touched"""
    cam = srt.camera_init(16, 12, 40.0, (0, 0, 5), (0, 0, 0))
    scene = object()      # (never looked at)
    call = lambda cams=(cam,), spp=4, **kw: srt.render_interactive(scene, cams, 16, 12, spp, 3, device=99, **kw)
    with pytest.raises(ValueError, match="no camera"):
        call(cams=[])
    with pytest.raises(TypeError, match=r"cameras\[1\] is no CameraData"):
        call(cams=[cam, (1, 2, 3)])
    with pytest.raises(ValueError):
        call(spp=0)
    with pytest.raises(ValueError):
        call(spp=70000)
    with pytest.raises(TypeError, match="unknown temporal keyword"):
        call(temporal=dict(alpha=0.5))
    with pytest.raises(ValueError, match="temporal: alpha_min"):
        call(temporal=dict(alpha_min=2.0))
    with pytest.raises(TypeError, match="unknown despeckle keyword"):
        call(despeckle=dict(size=2))
    with pytest.raises(ValueError, match="despeckle: radius"):
        call(despeckle=dict(radius=3))
    with pytest.raises(ValueError, match="denoise: levels"):
        call(levels=9)
    with pytest.raises(TypeError, match="denoise=False"):
        call(denoise=False, levels=2)
    with pytest.raises(ValueError, match="despeckle given with denoise=False"):
        call(denoise=False, despeckle={})
    gen = call(cams=iter([cam, cam]), temporal=dict(max_len=8), despeckle=dict(radius=1), levels=2)      # accepted: nothing runs before the first next()
    assert hasattr(gen, "__next__")
    gen.close()
