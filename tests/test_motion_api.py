"""Surface motion's C-ABI and Python face without a GPU: header, binding and library agree on the new symbols, null arguments are refused
without a device, the Python wrappers refuse bad rectangles, shapes and dtypes before any library call, and render_animated takes its
track_motion keyword."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srt_temporal_track_motion", "srt_temporal_tracking", "srt_surface_motion", "srt_surface_motion_kat", "srt_motion_last_ms",
           "srt_temporal_accum_moving", "srt_temporal_moving_kat", "srt_denoise_features_temporal_moving", "srt_present_temporal_moving")


def test_new_symbols_are_in_header_binding_and_library(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    B, P = srt.binding, srt.binding.PROTOTYPES
    vp, fp, sz, i, u32 = C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_uint32
    mr, ip = C.POINTER(B.MotionResult), C.POINTER(C.c_int32)
    assert P["srt_temporal_track_motion"] == (i, [vp, i]) and P["srt_temporal_tracking"] == (i, [vp, C.POINTER(i), C.POINTER(u32)])
    assert P["srt_surface_motion"] == (i, [vp, u32, u32, u32, u32, fp, ip, fp, mr])
    assert P["srt_surface_motion_kat"] == (i, [vp, C.POINTER(B.CameraData), fp, fp, sz, u32, u32, u32, u32, fp, ip, fp, mr])
    # every *_moving call is its sibling's signature plus one trailing argument
    for name, last in (("srt_temporal_accum", mr), ("srt_denoise_features_temporal", mr), ("srt_present_temporal", mr)):
        assert P[name + "_moving"] == (P[name][0], P[name][1] + [last]), name
    assert P["srt_temporal_moving_kat"] == (P["srt_temporal_kat"][0], P["srt_temporal_kat"][1] + [fp])
    assert C.sizeof(B.MotionResult) == 32 and [f[0] for f in B.MotionResult._fields_] == ["hit", "miss", "moved", "degenerate"]
    assert re.search(r"typedef struct srt_motion_result \{ uint64_t hit, miss, moved, degenerate; \} srt_motion_result;", header)
    # the statement: every operation of step 4, the vertex state, the stated limitation
    for phrase in ("den = d11 * d22 - d12 * d12", "disp = (Da + beta * (Db - Da)) + gamma * (Dc - Da)", "THE TEMPORAL\n *                           HISTORY IS KEPT",
                   "THE CALLER'S PROMISE", "expected-normal correction", "refits_pending"):
        assert phrase in header, phrase
    for attr in ("track_motion", "tracking", "surface_motion", "surface_motion_kat", "temporal_moving", "temporal_moving_kat", "denoise_temporal_moving",
                 "present_temporal_moving", "motion_last_ms"):
        assert hasattr(srt.Renderer, attr), attr
    assert isinstance(srt.Renderer.tracking, property)
    assert "motion_stats" in srt.__all__


def test_null_arguments_are_refused_without_a_device(srt):
    L, B = srt.binding.lib(), srt.binding
    ms, on, n, res = C.c_float(), C.c_int(), C.c_uint32(), B.MotionResult()
    v = np.zeros((2, 3, 3), np.float32)
    cam, t = B.CameraData(), srt.temporal_config()
    assert L.srt_temporal_track_motion(None, 1) == -1
    assert L.srt_temporal_tracking(None, C.byref(on), C.byref(n)) == -1
    assert L.srt_surface_motion(None, 4, 4, 0, 0, None, None, None, C.byref(res)) == -1
    assert L.srt_surface_motion_kat(None, C.byref(cam), None, B.fptr(v), 2, 4, 4, 0, 0, None, None, None, C.byref(res)) == -1
    assert L.srt_motion_last_ms(None, C.byref(ms)) == -1
    assert L.srt_temporal_accum_moving(None, C.byref(t), None, None, None, None, None, None, 4, 4, C.byref(res)) == -1
    assert L.srt_temporal_moving_kat(None, C.byref(t), C.byref(cam), None, None, None, None, None, 4, 4, 0, 0, None, None, None, None, None) == -1
    assert L.srt_denoise_features_temporal_moving(None, C.byref(t), None, None, None, None, None, None, 4, 4, None) == -1
    assert L.srt_present_temporal_moving(None, None, C.byref(t), None, None, 16, 4, 4, None, None, None) == -1


def test_wrappers_refuse_bad_arguments_before_the_library(srt):
    r = srt.Renderer.__new__(srt.Renderer)      # no context: every refusal below must come before the first library call
    r.device = 0
    cam = srt.camera_init(16, 16, 40.0, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    good = np.zeros((4, 3, 3), np.float32)
    for w, h, ox, oy in ((0, 4, 0, 0), (4, 0, 0, 0), (-1, 4, 0, 0), (4, 4, -1, 0), (4.5, 4, 0, 0), (True, 4, 0, 0), (2 ** 16, 2 ** 15, 0, 0),
                         (4, 4, 2 ** 24 - 3, 0), (4, 4, 0, 2 ** 24 - 3)):
        with pytest.raises(ValueError, match="surface_motion"):
            r.surface_motion(w, h, ox, oy)
        with pytest.raises(ValueError, match="surface_motion_kat"):
            r.surface_motion_kat(cam, good, w, h, ox, oy)
    with pytest.raises(TypeError, match="CameraData"):
        r.surface_motion_kat(None, good, 4, 4)
    for wrong, exc in ((good.astype(np.float64), TypeError), (good.reshape(4, 9), ValueError), (good[:0], ValueError), (good.tolist(), TypeError)):
        with pytest.raises(exc, match="cur_verts"):
            r.surface_motion_kat(cam, wrong, 4, 4)
        with pytest.raises(exc, match="prev_verts"):
            r.surface_motion_kat(cam, good, 4, 4, prev_verts=wrong)
    with pytest.raises(ValueError, match="differ in shape"):
        r.surface_motion_kat(cam, good, 4, 4, prev_verts=good[:3])
    img, g, pts = np.zeros((4, 5, 3), np.float32), np.zeros((4, 5, 8), np.float32), np.zeros((4, 5, 4), np.float32)
    with pytest.raises(ValueError, match="prev_point"):
        r.temporal_moving_kat(cam, img, g, pts[:3])
    with pytest.raises(ValueError, match="guides"):
        r.temporal_moving_kat(cam, img, g[:, :4], pts)
    with pytest.raises(ValueError, match="history is prev_cam"):
        r.temporal_moving_kat(cam, img, g, pts, prev_cam=cam)
    with pytest.raises(TypeError, match="unknown temporal keyword"):
        r.temporal_moving(4, 4, sigma_colour=1.0)
    with pytest.raises(TypeError, match="unknown temporal keyword"):
        r.denoise_temporal_moving(4, 4, temporal=dict(bogus=1))
    with pytest.raises(ValueError, match="present_temporal_moving"):
        r.present_temporal_moving(4, 4, "develop", 1.0)


def test_render_animated_keyword(srt):
    sig = inspect.signature(srt.render_animated)
    assert sig.parameters["track_motion"].default is False
    cam = srt.camera_init(16, 16, 40.0, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    frames = [np.zeros((4, 3, 3), np.float32)]
    with pytest.raises(TypeError, match="track_motion must be a bool"):
        srt.render_animated(None, cam, frames, 16, 16, 2, 3, track_motion=1)
    # the other checks still run first-come: a bad frame is refused whatever the keyword says
    for track in (False, True):
        with pytest.raises(ValueError, match="frames"):
            srt.render_animated(None, cam, [np.zeros((4, 9), np.float32)], 16, 16, 2, 3, track_motion=track)
        with pytest.raises(TypeError, match="unknown temporal keyword"):
            srt.render_animated(None, cam, frames, 16, 16, 2, 3, temporal=dict(bogus=1), track_motion=track)
    # False is today's generator, True the tracked one: neither touches a device before its first frame is asked for
    import importlib
    R = importlib.import_module("cuda-spectral-ray-tracer_amd.renderer")
    assert srt.render_animated(None, cam, frames, 16, 16, 2, 3).gi_code is R._animated_frames.__code__
    assert srt.render_animated(None, cam, frames, 16, 16, 2, 3, track_motion=True).gi_code is R._animated_frames_tracked.__code__
    src = inspect.getsource(R._animated_frames_tracked)
    assert src.index("track_motion(True)") < src.index("_image_session") and "denoise_temporal_moving" in src and "temporal_moving(" in src
