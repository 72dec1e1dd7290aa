"""The Python face of the variance measured across frames without a GPU: the binding declares the new symbols and structs, the
configuration builders refuse what the library refuses before a device is touched, and render_interactive / render_animated make exactly
the calls they made before unless variance_guided=True asks for the new chain."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srt_denoise_features_temporal_vg", "srt_present_temporal_vg", "srt_temporal_moments_kat", "srt_temporal_variance_kat",
           "srt_read_temporal_moments", "srt_temporal_variance_last_ms")


def test_symbols_prototypes_and_struct_sizes(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    B = srt.binding
    for name in SYMBOLS:
        assert "SRT_API int %s(" % name in header, name
        assert name in B.PROTOTYPES and getattr(L, name) is not None, name
    assert "typedef struct srt_temporal_vg { uint32_t min_len; uint32_t moving; uint32_t reserved[2]; } srt_temporal_vg;" in header
    assert C.sizeof(B.TemporalVG) == 16 and [f[0] for f in B.TemporalVG._fields_] == ["min_len", "moving", "reserved"]
    # the result struct did not grow: n_temporal is a parameter
    assert C.sizeof(B.TemporalResult) == 48 and C.sizeof(B.Temporal) == 32 and C.sizeof(B.DenoiseVG) == 32 and C.sizeof(B.PresentCfg) == 184
    vp, fp, u32, u64p = C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint64)
    t, ds, vg, tv = C.POINTER(B.Temporal), C.POINTER(B.Despeckle), C.POINTER(B.DenoiseVG), C.POINTER(B.TemporalVG)
    tres, mres, cam = C.POINTER(B.TemporalResult), C.POINTER(B.MotionResult), C.POINTER(B.CameraData)
    P = B.PROTOTYPES
    assert P["srt_denoise_features_temporal_vg"] == (C.c_int, [vp, t, ds, vg, tv, fp, fp, fp, fp, tres, u64p, mres, u32, u32])
    assert P["srt_present_temporal_vg"] == (C.c_int, [vp, C.POINTER(B.PresentCfg), t, ds, tv, C.POINTER(C.c_uint8), C.c_size_t, u32, u32,
                                                      C.POINTER(B.PresentResult), tres, u64p, mres])
    assert P["srt_temporal_moments_kat"] == (C.c_int, P["srt_temporal_kat"][1] + [fp, fp, fp])
    assert P["srt_temporal_kat"][1] == [vp, t, cam, cam, fp, fp, fp, fp, u32, u32, u32, u32, fp, fp, fp, tres]
    assert P["srt_temporal_variance_kat"] == (C.c_int, [vp, fp, fp, fp, u32, u32, u32, fp, u64p])
    assert P["srt_read_temporal_moments"] == (C.c_int, [vp, fp, u32, u32])
    assert P["srt_temporal_variance_last_ms"] == (C.c_int, [vp, fp])
    assert "temporal_vg_config" in srt.__all__


def test_the_header_states_the_operations():
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    for text in ("s1 += wt * Hm_q.x;  s2 += wt * Hm_q.y;  sm += wt * Hm_q.z", "Hm' = (Y, Q, 1, 0)", "Hm' = (0, 0, 0, 0)",
                 "g1 + b * (Y - g1), g2 + b * (Q - g2)", "d = m2' - m1' * m1';  d = d > 0 ? d : 0;  vt = d / len'",
                 "use = (mlen' >= ml_min) && (len' > 0) && ((vt - vt) == 0)", "an approximation once alpha_min or"):
        assert text in header, text


def test_temporal_vg_config_values(srt):
    v = srt.temporal_vg_config()
    assert (v.min_len, v.moving, list(v.reserved)) == (4, 0, [0, 0])
    v = srt.temporal_vg_config(np.int64(2 ** 24), np.bool_(True))
    assert (v.min_len, v.moving) == (2 ** 24, 1)
    assert srt.temporal_vg_config(min_len=2).min_len == 2


@pytest.mark.parametrize("kw", [dict(min_len=1), dict(min_len=0), dict(min_len=-4), dict(min_len=2 ** 24 + 1), dict(min_len=4.0), dict(min_len=True),
                                dict(min_len=None), dict(min_len="4"), dict(moving=1), dict(moving=None), dict(moving="yes")],
                         ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_temporal_vg_config_refuses(srt, kw):
    with pytest.raises(ValueError, match="temporal_vg: " + next(iter(kw))):
        srt.temporal_vg_config(**kw)


def test_bad_arguments_are_refused_before_a_device_is_touched(srt):
    """a Renderer that holds no context: a method that reached the library would fail on the null handle with another exception"""
    r = object.__new__(srt.Renderer)
    r._h = None
    cam = srt.camera_init(4, 4, 40.0, (0, 0, 5), (0, 0, 0))
    img, g = np.ones((4, 4, 3), np.float32), np.ones((4, 4, 8), np.float32)
    q = np.ones((4, 4, 4), np.float32)
    for call, exc in ((lambda: r.denoise_temporal_vg(8, 8, min_len=1), ValueError), (lambda: r.denoise_temporal_vg(8, 8, moving=2), ValueError),
                      (lambda: r.denoise_temporal_vg(8, 8, levels=9), ValueError), (lambda: r.denoise_temporal_vg(8, 8, sigma_variance=0.0), ValueError),
                      (lambda: r.denoise_temporal_vg(8, 8, sigma_color=1.0), TypeError), (lambda: r.denoise_temporal_vg(8, 8, temporal=dict(alpha_min=2.0)), ValueError),
                      (lambda: r.denoise_temporal_vg(8, 8, temporal=dict(alpha=1.0)), TypeError),
                      (lambda: r.denoise_temporal_vg(8, 8, despeckle=dict(radius=5)), ValueError),
                      (lambda: r.present_temporal_vg(8, 8, min_len=2 ** 25), ValueError), (lambda: r.present_temporal_vg(8, 8, gain=0.0), ValueError),
                      (lambda: r.present_temporal_vg(8, 8, variance_floor=-1.0), ValueError),
                      (lambda: r.temporal_moments_kat(cam, img, g[..., :7]), ValueError), (lambda: r.temporal_moments_kat(cam, img, g, alpha_min=0.0), ValueError),
                      (lambda: r.temporal_moments_kat(cam, img, g, prev_cam=cam), ValueError),
                      (lambda: r.temporal_moments_kat(cam, img, g, hist_moments=q), ValueError),
                      (lambda: r.temporal_moments_kat(cam, img, g, cam, q, g, hist_moments=q[:2]), ValueError),
                      (lambda: r.temporal_moments_kat(cam, img, g, prev_point=q[..., :3]), ValueError),
                      (lambda: r.temporal_variance_kat(q, q[..., 0], q[..., 0], min_len=1), ValueError),
                      (lambda: r.temporal_variance_kat(q[..., :3], q[..., 0], q[..., 0]), ValueError),
                      (lambda: r.temporal_variance_kat(q, q[..., 0], q[:2, :, 0]), ValueError),
                      (lambda: r.temporal_moments(), ValueError)):
        with pytest.raises(exc):
            call()
    r._h = None      # (nothing to close)


class _Recorder:
    """stands in for a Renderer: records every method call and answers with a dict that has the keys the generators read"""
    _h = 1
    gather_planes = 9
    geom = {}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def method(*args, **kw):
            self.calls.append((name, args, kw))
            return {"stats": {"history_frames": len(self.calls)}}
        return method


def _names(rec):
    return [c[0] for c in rec.calls]


def test_render_interactive_default_path_makes_no_new_call(srt):
    cams = [srt.camera_init(16, 12, 40.0, (0, 0, 5), (0, 0, 0)), srt.camera_init(16, 12, 40.0, (0.1, 0, 5), (0, 0, 0))]
    scene = object()
    frame = ["set_camera", "accum_reset_features", "render_chunk_accum", "scatter_tiles", "CHAIN", "read_fb", "read_fb_aux", "read_fb_aux",
             "read_fb_rowmajor", "stats", "last_kernel_ms", "read_features"]
    setup = ["upload_scene", "set_camera", "init_device_params", "set_partition", "set_count_traversal", "set_gather_planes", "temporal_reset"]

    def expected(chain):
        return setup + [chain if n == "CHAIN" else n for n in frame] * 2 + ["set_gather_planes"]

    tkw, dkw = dict(max_len=8), dict(radius=1)
    rec = _Recorder()
    list(srt.render_interactive(scene, cams, 16, 12, 4, 3, renderer=rec, temporal=tkw, despeckle=dkw, levels=2))
    assert _names(rec) == expected("denoise_temporal")
    chain = [c for c in rec.calls if c[0] == "denoise_temporal"]
    assert all(c[1] == (16, 12, tkw, dkw) and c[2] == dict(levels=2) for c in chain)
    same = _Recorder()
    list(srt.render_interactive(scene, cams, 16, 12, 4, 3, renderer=same, temporal=tkw, despeckle=dkw, variance_guided=False, levels=2))
    assert same.calls == rec.calls
    plain = _Recorder()
    list(srt.render_interactive(scene, cams, 16, 12, 4, 3, renderer=plain, denoise=False))
    assert _names(plain) == expected("temporal")
    # variance_guided=True: the new chain in the old one's place, nothing else moves
    vg = _Recorder()
    list(srt.render_interactive(scene, cams, 16, 12, 4, 3, renderer=vg, temporal=tkw, despeckle=dkw, variance_guided=True, min_len=3, levels=2,
                                sigma_variance=1.5))
    assert _names(vg) == expected("denoise_temporal_vg")
    chain = [c for c in vg.calls if c[0] == "denoise_temporal_vg"]
    assert all(c[1] == (16, 12, tkw, dkw, 3, False) and c[2] == dict(levels=2, sigma_variance=1.5) for c in chain)
    assert [c for c in vg.calls if c[0] != "denoise_temporal_vg"] == [c for c in rec.calls if c[0] != "denoise_temporal"]
    # ... and its arguments are checked by the call itself, with a device that does not exist
    call = lambda **kw: srt.render_interactive(scene, cams, 16, 12, 4, 3, device=99, **kw)
    with pytest.raises(ValueError, match="temporal_vg: min_len"):
        call(variance_guided=True, min_len=1)
    with pytest.raises(TypeError):
        call(variance_guided=True, sigma_color=1.0)      # (denoise_config's keyword, not denoise_vg_config's)
    with pytest.raises(ValueError, match="denoise: sigma_variance"):
        call(variance_guided=True, sigma_variance=float("inf"))
    with pytest.raises(ValueError, match="variance_guided=True with denoise=False"):
        call(variance_guided=True, denoise=False)
    with pytest.raises(TypeError, match="variance_guided must be a bool"):
        call(variance_guided=1)
    with pytest.raises(TypeError):
        call(min_len=3)      # (without variance_guided it is no keyword of denoise_config)


def test_render_animated_selects_the_moving_stage_with_tracking(srt):
    cam = srt.camera_init(16, 12, 40.0, (0, 0, 5), (0, 0, 0))
    frames = [np.zeros((3, 3, 3), np.float32), np.ones((3, 3, 3), np.float32)]
    scene = object()
    for track in (False, True):
        old, new = _Recorder(), _Recorder()
        list(srt.render_animated(scene, cam, frames, 16, 12, 4, 3, renderer=old, track_motion=track, levels=2))
        list(srt.render_animated(scene, cam, frames, 16, 12, 4, 3, renderer=new, track_motion=track, variance_guided=True, levels=2))
        chain = "denoise_temporal_moving" if track else "denoise_temporal"
        assert _names(old).count(chain) == 2 and "denoise_temporal_vg" not in _names(old)
        assert [n if n != chain else "denoise_temporal_vg" for n in _names(old)] == _names(new)
        got = [c for c in new.calls if c[0] == "denoise_temporal_vg"]
        assert all(c[1] == (16, 12, {}, None) and c[2] == (dict(moving=True, levels=2, min_len=4) if track else dict(levels=2, min_len=4)) for c in got)
    with pytest.raises(ValueError, match="temporal_vg: min_len"):
        srt.render_animated(scene, cam, frames, 16, 12, 4, 3, device=99, variance_guided=True, min_len=0)
