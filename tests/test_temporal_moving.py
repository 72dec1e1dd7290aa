"""The temporal stage on tracked points (srt_temporal_moving_kat, srt_temporal_accum_moving, srt_denoise_features_temporal_moving,
srt_present_temporal_moving) and the vertex state of a tracking context: the moving kernel equals tests/surface_motion_reference.py bit
for bit and counter for counter, equals the static kernel when it is fed the static point, the history survives a refit exactly when
tracking is on, and every refusal leaves history and vertex state alone."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as D
import surface_motion_reference as M
import temporal_reference as T
from accum_helpers import ERR_INVALID, expect_error, fresh_context, named_workload
from helpers import bits
from path_ends_reference import assert_same_floats
from test_temporal import SIZES, _device_inputs, _frame, _levels

pytestmark = pytest.mark.gpu
F = np.float32
FP = C.POINTER(C.c_float)
BOX = slice(12, 24)


def _assert_stage(got, want, what):
    assert_same_floats(got["colour"], want["colour"], what + " colour and len")
    assert_same_floats(got["guides"], want["guides"], what + " guides")
    assert_same_floats(got["motion"], want["motion"], what + " motion")
    stats = {k: v for k, v in got["stats"].items() if k in want["stats"]}
    assert stats == want["stats"], (what, stats, want["stats"])


def _cameras(srt, IW, IH):
    prev = srt.camera_init(IW, IH, 40.0, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0))
    return prev, [("static", prev), ("translate", srt.camera_init(IW, IH, 40.0, (0.2, 0.1, 6.0), (0.2, 0.1, 0.0))),
                  ("rotate", srt.camera_init(IW, IH, 40.0, (0.0, 0.0, 6.0), (0.3, 0.05, 0.0))), ("behind", T.move_camera(prev, yaw_deg=180.0))]


@pytest.mark.parametrize("w,h", SIZES)
def test_moving_kat_equals_the_restatement(srt, gpu, w, h):
    """explicit inputs at the temporal suite's sizes: displaced points, valid = 0 holes, non-finite coordinates under valid = 1"""
    ox, oy = 5, 3
    prev, pairs = _cameras(srt, w + ox + 2, h + oy + 1)
    c, g, hc, hg = T.random_case(w, h, 1)
    rng = np.random.default_rng(100 * w + h)
    total = dict(blended=0, fresh=0, offscreen=0, rejected=0, nonfinite=0)
    for name, cur in pairs:
        for off in ((0, 0), (ox, oy)):
            pts = M.static_points(g, cur, off[0], off[1])
            pts[..., :3] += rng.normal(0, 0.02, (h, w, 3)).astype(F)
            pts[rng.random((h, w)) < 0.2, 3] = 0.0
            if w * h >= 4:
                pts[rng.integers(h), rng.integers(w), 3] = 0.5      # (only exactly 1 is valid)
                pts[rng.integers(h), rng.integers(w), 0] = np.nan
            hist = dict(colour=hc, guides=hg, cam=prev)
            want = M.temporal_moving(c, g, cur, pts, hist, off[0], off[1], **T.DEFAULTS)
            got = gpu.temporal_moving_kat(cur, c, g, pts, prev, hc, hg, off[0], off[1], **T.DEFAULTS)
            _assert_stage(got, want, "%d x %d %s at %r" % (w, h, name, off))
            assert got["stats"]["history_frames"] == 2
            for k in total:
                total[k] += want["stats"][k]
        got = gpu.temporal_moving_kat(cur, c, g, pts, offx=ox, offy=oy)
        _assert_stage(got, T.temporal(c, g, cur, None, ox, oy, **T.DEFAULTS), "%d x %d %s without history" % (w, h, name))
    print("%d x %d: %r" % (w, h, total))
    if w * h > 100:
        assert min(total.values()) > 0, total


@pytest.mark.parametrize("w,h", SIZES)
def test_moving_kat_fed_the_static_point_equals_the_static_kat(srt, gpu, w, h):
    ox, oy = 5, 3
    prev, pairs = _cameras(srt, w + ox + 2, h + oy + 1)
    c, g, hc, hg = T.random_case(w, h, 2)
    for name, cur in pairs:
        for off in ((0, 0), (ox, oy)):
            want = gpu.temporal_kat(cur, c, g, prev, hc, hg, off[0], off[1], **T.DEFAULTS)
            got = gpu.temporal_moving_kat(cur, c, g, M.static_points(g, cur, off[0], off[1]), prev, hc, hg, off[0], off[1], **T.DEFAULTS)
            for key in ("colour", "guides", "motion"):
                assert_same_floats(got[key], want[key], "%d x %d %s %s" % (w, h, name, key))
            assert got["stats"] == want["stats"]


# ---- a real scene across refits ---------------------------------------------------------------------------------------------------------
def _workload(srt):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    v0 = scene.vertices()
    extent = float(np.linalg.norm(v0.reshape(-1, 3).max(axis=0) - v0.reshape(-1, 3).min(axis=0)))
    assert v0.shape[0] == 42

    def sideways(v, amount):      # one object moves along x: triangles 12 .. 23 are the tall box
        out = v.copy()
        out[BOX, :, 0] = (out[BOX, :, 0] + F(amount * extent)).astype(F)
        return out

    return scene, cam, W, H, depth, v0, sideways(v0, 0.02), sideways(v0, 0.035)


def _history_of(first, guides):
    return np.concatenate([first["xyz"], first["len"][..., None]], axis=-1).astype(F), guides


def _first_frame(gpu, scene, cam, W, H, depth, moving=True):
    fresh_context(gpu, scene, cam, W, H, depth)
    _frame(gpu, cam, W, H, (3, 2))
    c, g = _device_inputs(gpu, W, H)
    first = gpu.temporal_moving(W, H) if moving else gpu.temporal(W, H)
    assert first["stats"]["history_frames"] == 1 and np.array_equal(bits(first["xyz"]), bits(c))
    return first, g


def test_history_survives_a_refit_and_equals_the_kat(srt, gpu):
    scene, cam, W, H, depth, v0, v1, _ = _workload(srt)
    gpu.track_motion(True)
    try:
        first, g0 = _first_frame(gpu, scene, cam, W, H, depth)
        assert first["surface"]["moved"] == 0 and first["surface"]["hit"] > W * H // 2 and gpu.tracking == (True, 0)
        gpu.refit(v1)
        assert gpu.tracking == (True, 1)
        _frame(gpu, cam, W, H, (3, 2))
        c, g = _device_inputs(gpu, W, H)
        pts = gpu.surface_motion(W, H)
        kat_pts = gpu.surface_motion_kat(cam, v1, W, H, prev_verts=v0)
        assert np.array_equal(bits(pts["point"]), bits(kat_pts["point"])) and pts["stats"] == kat_pts["stats"] and pts["stats"]["moved"] > 0
        assert gpu.tracking == (True, 1)      # (the query moved nothing)
        got = gpu.temporal_moving(W, H)
        assert got["stats"]["history_frames"] == 2 and got["stats"]["blended"] > 0 and gpu.tracking == (True, 0)
        assert got["surface"] == pts["stats"]
        hc, hg = _history_of(first, g0)
        kat = gpu.temporal_moving_kat(cam, c, g, pts["point"], cam, hc, hg, **T.DEFAULTS)
        assert_same_floats(got["xyz"], kat["colour"][..., :3], "second call xyz")
        assert_same_floats(got["len"], kat["colour"][..., 3], "second call len")
        assert_same_floats(got["motion"], kat["motion"], "second call motion")
        assert {k: got["stats"][k] for k in ("blended", "fresh", "offscreen", "rejected", "nonfinite")} == \
               {k: kat["stats"][k] for k in ("blended", "fresh", "offscreen", "rejected", "nonfinite")}
        want = M.temporal_moving(c, g, cam, pts["point"], dict(colour=hc, guides=hg, cam=cam), **T.DEFAULTS)
        assert_same_floats(got["xyz"], want["xyz"], "second call against the restatement")
        # the tracked points are not the static ones: on the moved triangles the motion vector is their motion, not zero
        moved = (pts["bary"][..., 0] > 0) & np.isin(pts["tri"], np.arange(BOX.start, BOX.stop))
        assert moved.any() and np.nanmax(np.abs(got["motion"][moved][:, 0])) > 0.25
        still = (pts["tri"] >= 0) & ~moved
        assert np.nanmax(np.abs(got["motion"][still])) < 1e-3
        assert gpu.motion_last_ms() > 0 and gpu.temporal_last_ms() > 0
    finally:
        gpu.track_motion(False)


def test_without_tracking_a_refit_drops_the_history(srt, gpu):
    """today's behaviour, asserted so that it stays"""
    scene, cam, W, H, depth, v0, v1, _ = _workload(srt)
    assert gpu.tracking == (False, 0)
    _first_frame(gpu, scene, cam, W, H, depth, moving=False)
    gpu.refit(v1)
    assert gpu.tracking == (False, 0)
    _frame(gpu, cam, W, H, (3, 2))
    got = gpu.temporal(W, H)
    assert got["stats"]["history_frames"] == 1 and got["stats"]["blended"] == 0


def test_a_static_call_after_a_refit_is_a_first_frame(srt, gpu):
    scene, cam, W, H, depth, v0, v1, _ = _workload(srt)
    gpu.track_motion(True)
    try:
        _first_frame(gpu, scene, cam, W, H, depth)
        gpu.refit(v1)
        _frame(gpu, cam, W, H, (3, 2))
        assert gpu.tracking == (True, 1)
        got = gpu.temporal(W, H)
        assert got["stats"]["history_frames"] == 1 and got["stats"]["blended"] == 0 and gpu.tracking == (True, 0)
        # ... and the new history shows V_cur: the next moving call finds nothing moved and blends
        _frame(gpu, cam, W, H, (3, 2))
        got = gpu.temporal_moving(W, H)
        assert got["stats"]["history_frames"] == 2 and got["stats"]["blended"] > 0 and got["surface"]["moved"] == 0
    finally:
        gpu.track_motion(False)


def test_two_refits_reproject_against_the_vertices_of_the_history(srt, gpu):
    scene, cam, W, H, depth, v0, v1, v2 = _workload(srt)
    gpu.track_motion(True)
    try:
        first, g0 = _first_frame(gpu, scene, cam, W, H, depth)
        gpu.refit(v1)
        gpu.refit(v2)
        assert gpu.tracking == (True, 2)
        _frame(gpu, cam, W, H, (3, 2))
        c, g = _device_inputs(gpu, W, H)
        pts = gpu.surface_motion(W, H)
        from_v0 = gpu.surface_motion_kat(cam, v2, W, H, prev_verts=v0)
        from_v1 = gpu.surface_motion_kat(cam, v2, W, H, prev_verts=v1)
        assert np.array_equal(bits(pts["point"]), bits(from_v0["point"])) and (bits(pts["point"]) != bits(from_v1["point"])).any()
        got = gpu.temporal_moving(W, H)
        hc, hg = _history_of(first, g0)
        kat = gpu.temporal_moving_kat(cam, c, g, from_v0["point"], cam, hc, hg, **T.DEFAULTS)
        assert_same_floats(got["xyz"], kat["colour"][..., :3], "two refits xyz")
        assert_same_floats(got["motion"], kat["motion"], "two refits motion")
        assert got["stats"]["history_frames"] == 2 and got["stats"]["blended"] > 0 and gpu.tracking == (True, 0)
    finally:
        gpu.track_motion(False)


def test_chained_calls_equal_the_separate_calls(srt, gpu):
    """denoise_temporal_moving and present_temporal_moving against the motion pass, the moving KAT on the read-back guides, the restated
    levels and present_kat, byte for byte"""
    scene, cam, W, H, depth, v0, v1, _ = _workload(srt)
    sig = {k: v for k, v in D.DEFAULTS.items() if k != "levels"}
    gpu.track_motion(True)
    try:
        for chained in ("denoise", "present accum", "present denoise"):
            first, g0 = _first_frame(gpu, scene, cam, W, H, depth)
            gpu.refit(v1)
            _frame(gpu, cam, W, H, (3, 2))
            c, g = _device_inputs(gpu, W, H)
            pts = gpu.surface_motion(W, H)
            hc, hg = _history_of(first, g0)
            stage = gpu.temporal_moving_kat(cam, c, g, pts["point"], cam, hc, hg, **T.DEFAULTS)
            o = stage["colour"][..., :3]
            if chained == "denoise":
                got = gpu.denoise_temporal_moving(W, H, levels=2)
                assert_same_floats(got["xyz"], _levels(o, g, 2, sig), chained)
                tstats, surface = got["stats"], got["surface"]
            else:
                source = chained.split()[1]
                kw = dict(levels=1) if source == "denoise" else {}
                got = gpu.present_temporal_moving(W, H, source, 1.3, **kw)
                want = gpu.present_kat(o if source == "accum" else _levels(o, g, 1, sig), 1.3)
                assert np.array_equal(got["rgba"], want["rgba"]) and got["clip"] == want["clip"], chained
                tstats, surface = got["temporal"], got["surface"]
            assert tstats["history_frames"] == 2 and tstats["blended"] > 0 and surface == pts["stats"] and gpu.tracking == (True, 0)
            assert {k: tstats[k] for k in ("blended", "fresh", "offscreen", "rejected", "nonfinite")} == \
                   {k: stage["stats"][k] for k in ("blended", "fresh", "offscreen", "rejected", "nonfinite")}
    finally:
        gpu.track_motion(False)


def test_refusals_leave_history_and_vertex_state_alone(srt, gpu):
    scene, cam, W, H, depth, v0, v1, _ = _workload(srt)
    L, B = srt.binding.lib(), srt.binding
    good, dcfg = srt.temporal_config(), srt.denoise_config(levels=1)
    res, mres, pres = B.TemporalResult(), B.MotionResult(), B.PresentResult()
    out = np.zeros((H, W, 3), F)
    op = out.ctypes.data_as(FP)
    rgba = np.zeros((H, W, 4), np.uint8)
    rp = rgba.ctypes.data_as(C.POINTER(C.c_uint8))

    def accum(t=good, o=op):
        return L.srt_temporal_accum_moving(gpu._h, C.byref(t) if t is not None else None, o, None, None, None, None, None, W, H, C.byref(mres))

    def chain(t=good):
        return L.srt_denoise_features_temporal_moving(gpu._h, C.byref(t), None, C.byref(dcfg), op, None, None, C.byref(res), W, H, C.byref(mres))

    def present(t=good, source="accum"):
        p = srt.present_config(source, 1.0)
        return L.srt_present_temporal_moving(gpu._h, C.byref(p), C.byref(t), None, rp, 4 * W, W, H, C.byref(pres), C.byref(res), C.byref(mres))

    # tracking off: the static calls build a history, the moving ones refuse and leave it
    _first_frame(gpu, scene, cam, W, H, depth, moving=False)
    assert accum() == ERR_INVALID and chain() == ERR_INVALID and present() == ERR_INVALID
    assert b"tracking is off" in L.srt_last_error(gpu._h)
    assert gpu.temporal(W, H)["stats"]["history_frames"] == 2
    gpu.track_motion(True)
    try:
        # switched on: the history is gone and the vertices are unknown
        assert gpu.tracking == (True, 0)
        assert accum() == ERR_INVALID and chain() == ERR_INVALID and present() == ERR_INVALID
        assert b"unknown" in L.srt_last_error(gpu._h)
        assert gpu.temporal(W, H)["stats"]["history_frames"] == 1
        # known vertices, a history, a refit pending: bad arguments change nothing
        _first_frame(gpu, scene, cam, W, H, depth)
        gpu.refit(v1)
        _frame(gpu, cam, W, H, (3, 2))
        bad = srt.temporal_config()
        bad.alpha_min = 0.0
        assert accum(bad) == ERR_INVALID and chain(bad) == ERR_INVALID and present(bad) == ERR_INVALID
        assert accum(None) == ERR_INVALID and L.srt_temporal_accum_moving(gpu._h, C.byref(good), None, None, None, None, None, None, W, H, None) == ERR_INVALID
        assert present(source="develop") != 0
        expect_error(srt, lambda: gpu.refit(v1[:-1]), ERR_INVALID, "a refused refit")
        pts = np.zeros((H, W, 4), F)
        img, gd = np.ones((H, W, 3), F), np.ones((H, W, 8), F)
        assert L.srt_temporal_moving_kat(gpu._h, C.byref(good), C.byref(cam), None, B.fptr(img), B.fptr(gd), None, None, W, H, 0, 0, B.fptr(pts), None, None,
                                         None, None) == ERR_INVALID      # (no prev_point)
        assert gpu.tracking == (True, 1)
        got = gpu.temporal_moving(W, H)
        assert got["stats"]["history_frames"] == 2 and got["stats"]["blended"] > 0 and gpu.tracking == (True, 0)
        # a partition other than (0, 1): refused as the static stage refuses; set_partition itself drops the history
        gpu.set_partition(1, 2)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, 2)
        assert accum() != 0 and chain() != 0 and present() != 0
        gpu.surface_motion(W, H)      # (the query runs under any partition)
        gpu.set_partition(0, 1)
        # switching off forgets everything again
        gpu.track_motion(False)
        assert gpu.tracking == (False, 0)
        assert accum() == ERR_INVALID
    finally:
        gpu.track_motion(False)
