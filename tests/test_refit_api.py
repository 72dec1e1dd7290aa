"""The refit's C-ABI and Python face without a GPU: header, binding and library agree on the new symbols, the argument checks that need
no device refuse, and Renderer.refit / render_animated refuse wrong shapes and dtypes before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srt_scene_refit", "srt_scene_refit_schedule", "srt_refit_vertices", "srt_refit_vertices_dev", "srt_refit_last_ms", "srt_read_scene_image", "srt_comm_refit_vertices")


def test_new_symbols_are_in_header_binding_and_library(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    vp, fp, sz, i, u32 = C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_uint32
    P = srt.binding.PROTOTYPES
    assert P["srt_scene_refit"] == (i, [vp, fp, sz])
    assert P["srt_scene_refit_schedule"] == (i, [vp, C.POINTER(u32), sz, C.POINTER(u32)])
    assert P["srt_refit_vertices"] == (i, [vp, fp, sz]) and P["srt_comm_refit_vertices"] == (i, [vp, fp, sz])
    assert P["srt_refit_vertices_dev"] == (i, [vp, vp, sz])
    assert P["srt_refit_last_ms"] == (i, [vp, fp, fp, C.POINTER(u32)])
    assert P["srt_read_scene_image"] == (i, [vp, i, vp, sz, C.POINTER(sz)])
    m = re.search(r"enum \{ SRT_IMAGE_NODES = 0, SRT_IMAGE_NODES_SW = 1, SRT_IMAGE_FRINGE = 2, SRT_IMAGE_TRIS = 3, SRT_IMAGE_SHADE = 4 \};", header)
    assert m and srt.binding.SCENE_IMAGES == dict(nodes=0, nodes_sw=1, fringe=2, tris=3, shade=4)
    # the header lists both entries among the calls that synchronise, and says what is out of scope
    sync = header[header.index("The calls that synchronise"):header.index("What is NOT ordered")]
    assert "srt_refit_vertices and srt_refit_vertices_dev" in sync and "srt_read_scene_image" in sync
    for phrase in ("topology", "motion vectors", "refit of materials"):
        assert phrase in header
    assert "render_animated" in srt.__all__ and callable(srt.render_animated)
    for attr in ("refit", "refit_last_ms", "scene_image"):
        assert hasattr(srt.Renderer, attr), attr
    assert hasattr(srt.Comm, "refit") and hasattr(srt.Scene, "refit")


def test_null_arguments_are_refused_without_a_device(srt):
    L = srt.binding.lib()
    v = np.zeros((2, 3, 3), np.float32)
    n, ms, lv = C.c_size_t(), C.c_float(), C.c_uint32()
    assert L.srt_refit_vertices(None, srt.binding.fptr(v), 2) == -1
    assert L.srt_refit_vertices_dev(None, None, 2) == -1
    assert L.srt_refit_last_ms(None, C.byref(ms), C.byref(ms), C.byref(lv)) == -1
    assert L.srt_read_scene_image(None, 0, None, 0, C.byref(n)) == -1
    assert L.srt_comm_refit_vertices(None, srt.binding.fptr(v), 2) == -1
    assert L.srt_scene_refit(None, srt.binding.fptr(v), 2) == -1


def test_renderer_refit_refuses_shapes_and_dtypes_before_the_device(srt):
    r = srt.Renderer.__new__(srt.Renderer)      # no context: every refusal below must come before the first library call
    r.device = 0
    good = np.zeros((4, 3, 3), np.float32)
    for wrong, exc in ((good.astype(np.float64), TypeError), (good.astype(np.int32), TypeError), (good.reshape(4, 9), ValueError),
                       (good[:, :, :2], ValueError), (good[:0], ValueError), (good.tolist(), TypeError), (None, TypeError), ("verts", TypeError)):
        with pytest.raises(exc, match="Renderer.refit"):
            srt.Renderer.refit(r, wrong)
    with pytest.raises(ValueError, match="scene_image: unknown image"):
        srt.Renderer.scene_image(r, "materials")
    import torch
    t = torch.zeros((4, 3, 3), dtype=torch.float32)
    for wrong, exc in ((t.double(), TypeError), (t.reshape(4, 9), ValueError), (t[:0], ValueError), (t, ValueError)):      # (t itself: a CPU tensor)
        with pytest.raises(exc, match="Renderer.refit"):
            srt.Renderer.refit(r, wrong)


def test_render_animated_checks_before_the_device(srt):
    cam = srt.camera_init(16, 12, 40.0, (0, 0, 5), (0, 0, 0))
    scene = object()      # (never looked at)
    v = np.zeros((3, 3, 3), np.float32)
    call = lambda frames=(v,), spp=4, cam=cam, **kw: srt.render_animated(scene, cam, frames, 16, 12, spp, 3, device=99, **kw)
    with pytest.raises(ValueError, match="no frame"):
        call(frames=[])
    with pytest.raises(TypeError, match="no CameraData"):
        call(cam=(1, 2, 3))
    with pytest.raises(ValueError, match=r"frames\[1\]"):
        call(frames=[v, v.reshape(3, 9)])
    with pytest.raises(TypeError, match=r"frames\[0\]"):
        call(frames=[v.astype(np.float64)])
    with pytest.raises(ValueError):
        call(spp=0)
    with pytest.raises(TypeError, match="unknown temporal keyword"):
        call(temporal=dict(alpha=0.5))
    with pytest.raises(ValueError, match="denoise: levels"):
        call(levels=9)
    with pytest.raises(TypeError, match="denoise=False"):
        call(denoise=False, levels=2)
    gen = call(frames=iter([v, v]), levels=2)      # accepted: nothing runs before the first next()
    assert hasattr(gen, "__next__")
    gen.close()
