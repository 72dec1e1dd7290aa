"""The surface-motion pass on the device (srt_surface_motion / srt_surface_motion_kat): the device equals tests/surface_motion_reference.py
in every bit of point, tri and bary and in every counter.  The closest hits (t, k) the restatement starts from are srt_trace_rays' answers
for the centre rays the test forms in numpy, which pins tri and t to the path the CPU oracle pins.  Every tree shape, both FRINGE strides,
a camera inside the geometry, a rectangle of sky; no motion, jitter, a power-of-two translation, degenerate triangles on either side."""
import numpy as np
import pytest

import helpers as H
import refit_cases as R
import surface_motion_reference as M
from accum_helpers import ERR_INVALID, expect_error, fresh_context, named_workload, read_frame
from features_reference import stack_features
from helpers import bits

pytestmark = pytest.mark.gpu
F = np.float32
RECTS = [(1, 1), (7, 5), (33, 9), (67, 35)]      # one lane, a partial wave, two tiles across and partial rows, 3 x 5 tiles
OFFSET = (11, 6)


def _assert_pass(gpu, cam, cur, prev, w, h, ox, oy, what, got=None):
    t, k = M.hits_of_trace(gpu.trace_rays(M.trace_inputs(cam, w, h, ox, oy)), w, h)
    want = M.surface_motion(cam, t, k, cur, prev, ox, oy)
    if got is None:
        got = gpu.surface_motion_kat(cam, cur, w, h, ox, oy, prev_verts=prev)
    for key in ("tri", "point", "bary"):
        same = bits(got[key]) == bits(want[key]) if key != "tri" else got[key] == want[key]
        assert same.all(), "%s %s: %d of %d words differ, first at %r" % (what, key, (~same).sum(), same.size, tuple(np.argwhere(~same)[0]))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    return want


def _sweep(gpu, cam, cur, motions, what, rects=RECTS):
    total = dict(hit=0, miss=0, moved=0, degenerate=0)
    for name, prev in motions:
        for w, h in rects:
            for ox, oy in ((0, 0), OFFSET):
                want = _assert_pass(gpu, cam, cur, prev, w, h, ox, oy, "%s %s %dx%d at (%d, %d)" % (what, name, w, h, ox, oy))
                for key in total:
                    total[key] += want["stats"][key]
    print(what, total)
    return total


def _translated(v0, which, shift):
    v = v0.copy()
    v[which] = (v[which] + np.asarray(shift, F)).astype(F)
    return v


def _motions(v0, seed):
    """(name, V_prev) for V_cur = v0: none, jitter, a power-of-two translation of the first third of the triangles, a triangle that is
    degenerate in V_prev (it must still be valid), and -- last -- previous vertices so far apart that Db - Da overflows: the previous
    point is not finite, the pixel degenerate"""
    n = v0.shape[0]
    flat = v0.copy()
    flat[n // 2, 2] = flat[n // 2, 1]
    apart = v0.copy()
    apart[:max(1, n // 3), 0, 0], apart[:max(1, n // 3), 1, 0] = 3e38, -3e38
    return [("none", None), ("jitter", R.jitter(v0, seed)), ("translation", _translated(v0, slice(0, max(1, n // 3)), (0.25, 0.0, -0.5))),
            ("degenerate before", flat), ("overflow", apart)]


@pytest.mark.parametrize("case", ["one_triangle", "two_triangles"])
def test_smallest_trees(srt, gpu, case):
    """the root-is-a-leaf tree goes through trav_begin alone; the two-triangle tree is one FRINGE record"""
    scene, cam, W, Hh, _, depth = H.edge_case_scene(srt, case)
    fresh_context(gpu, scene, cam, W, Hh, depth)
    total = _sweep(gpu, cam, scene.vertices(), _motions(scene.vertices(), 1), case)
    assert total["hit"] > 0 and total["miss"] > 0 and total["moved"] > 0


@pytest.mark.parametrize("seed", [1, 2, 9])
def test_fuzz_cases(srt, gpu, seed):
    scene, cam, W, Hh, _, depth, _, _ = H.fuzz_case(srt, seed)
    fresh_context(gpu, scene, cam, W, Hh, depth)
    total = _sweep(gpu, cam, scene.vertices(), _motions(scene.vertices(), seed), "fuzz %d" % seed)
    assert total["hit"] > 0 and total["moved"] > 0 and total["degenerate"] > 0


def test_unpaired_sah_tree(srt, gpu):
    scene, cam, W, Hh, _, depth = R.unpaired_scene(srt, "sah_odd_outlier")
    assert not scene.is_paired
    fresh_context(gpu, scene, cam, W, Hh, depth)
    total = _sweep(gpu, cam, scene.vertices(), _motions(scene.vertices(), 4), "unpaired")
    assert total["hit"] > 0 and total["moved"] > 0


@pytest.mark.parametrize("knobs,stride_env", [(dict(wide_refs=True), None), (dict(lds_cache_max=0), None), (dict(lds_cache_max=0), "128")],
                         ids=["wide_refs", "lds_cache_max=0", "lds_cache_max=0, 128-byte FRINGE stride"])
def test_under_test_knobs(srt, gpu, monkeypatch, knobs, stride_env):
    """both FRINGE strides: the pass reads the records the upload laid out for the render launch"""
    scene, cam, W, Hh, _, depth, _, _ = H.fuzz_case(srt, 10)
    if stride_env:
        monkeypatch.setenv("SRT_FRINGE_STRIDE", stride_env)
    try:
        gpu.set_test_knobs(**knobs)
        fresh_context(gpu, scene, cam, W, Hh, depth)
        if stride_env:
            assert gpu.scene_image("fringe").size % 32 == 0
        total = _sweep(gpu, cam, scene.vertices(), _motions(scene.vertices(), 10)[:2], "knobs %r %r" % (knobs, stride_env), RECTS[1:])
        assert total["hit"] > 0
    finally:
        gpu.set_test_knobs()
        monkeypatch.delenv("SRT_FRINGE_STRIDE", raising=False)
        gpu.upload_scene(scene)


def test_camera_inside_the_geometry_and_a_rectangle_of_sky(srt, gpu):
    scene, _, W, Hh, _, depth, _, _ = H.fuzz_case(srt, 9)
    inside = srt.camera_init(W, Hh, 70.0, (0.1, 0.2, -0.3), (1.0, 0.3, 0.2))
    fresh_context(gpu, scene, inside, W, Hh, depth)
    total = _sweep(gpu, inside, scene.vertices(), _motions(scene.vertices(), 9)[:2], "inside", RECTS[2:])
    assert total["hit"] > 0
    # far off the image every centre ray leaves the scene sideways: no hit, no vertex row read, every output word zero (tri -1)
    cam = srt.camera_init(W, Hh, 30.0, (0.0, 0.0, 40.0), (0.0, 0.0, 0.0))
    got = gpu.surface_motion_kat(cam, scene.vertices(), 33, 9, 4000, 3000, prev_verts=R.jitter(scene.vertices(), 9))
    _assert_pass(gpu, cam, scene.vertices(), R.jitter(scene.vertices(), 9), 33, 9, 4000, 3000, "sky", got)
    assert got["stats"] == dict(hit=0, miss=33 * 9, moved=0, degenerate=0)
    assert not bits(got["point"]).any() and not bits(got["bary"]).any() and (got["tri"] == -1).all()


def test_degenerate_in_the_current_vertices_and_the_bound_entry(srt, gpu):
    """tracking on: the bound entry uses the context's own vertex state and equals the KAT entry; a triangle refitted to a needle is
    never hit, and one that was a needle when the history was written stays valid"""
    scene, cam, W, Hh, _, depth = H.edge_case_scene(srt, "degenerate_and_odd_materials")
    v0 = scene.vertices()
    gpu.track_motion(True)
    try:
        fresh_context(gpu, scene, cam, W, Hh, depth)
        assert gpu.tracking == (True, 0)
        for w, h in RECTS:
            for ox, oy in ((0, 0), OFFSET):
                got = gpu.surface_motion(w, h, ox, oy)
                _assert_pass(gpu, cam, v0, None, w, h, ox, oy, "bound, no refit", got)
                kat = gpu.surface_motion_kat(cam, v0, w, h, ox, oy)
                assert all(np.array_equal(bits(got[key]), bits(kat[key])) for key in ("point", "tri", "bary")) and got["stats"] == kat["stats"]
        assert gpu.motion_last_ms() > 0
        # a refit without a history: V_hist stays none, nothing has "moved"
        v1 = v0.copy()
        v1[0] = [[1, 1, 0], [1, 1, 0], [1, 1, 0]]          # a wall triangle collapses to a point
        v1[6] = (v1[6] + F([0.5, 0.0, 0.0])).astype(F)
        gpu.refit(v1)
        assert gpu.tracking == (True, 0)
        got = gpu.surface_motion(W, Hh)
        want = _assert_pass(gpu, cam, v1, None, W, Hh, 0, 0, "bound, refit without history", got)
        assert want["stats"]["moved"] == 0 and not (want["tri"] == 0).any()
        # the KAT on the refitted images: degenerate now (never hit), and degenerate before
        total = _sweep(gpu, cam, v1, [("degenerate now", v0), ("jitter", R.jitter(v1, 3))], "degenerate", RECTS[2:])
        assert total["moved"] > 0
    finally:
        gpu.track_motion(False)
    assert gpu.tracking == (False, 0)


def test_the_pass_changes_nothing(srt, gpu):
    """a frame before and a frame after: images, accumulation, RNG state and temporal history are what they are without the calls"""
    scene, cam, W, Hh, depth, _ = named_workload(srt, "dielectric")
    v0 = scene.vertices()

    def run(with_calls):
        gpu.track_motion(True)
        try:
            fresh_context(gpu, scene, cam, W, Hh, depth)
            gpu.accum_reset_features()
            gpu.render_chunk_accum(W, Hh, 3)
            first = gpu.temporal(W, Hh)
            images = {k: gpu.scene_image(k) for k in R.IMAGES}
            if with_calls:
                gpu.surface_motion(W, Hh)
                gpu.surface_motion(33, 9, 7, 5)
                gpu.surface_motion_kat(cam, v0, W, Hh, prev_verts=R.jitter(v0, 1))
                assert gpu.tracking == (True, 0)
                for k in R.IMAGES:
                    assert np.array_equal(images[k], gpu.scene_image(k)), k
            gpu.render_chunk_accum(W, Hh, 2)
            frame = read_frame(gpu, W, Hh)
            return first, frame, gpu.read_features(W, Hh), gpu.temporal(W, Hh), gpu.accum_samples
        finally:
            gpu.track_motion(False)

    a, b = run(False), run(True)
    for key in ("xyz", "len", "motion"):
        assert np.array_equal(bits(a[0][key]), bits(b[0][key])) and np.array_equal(bits(a[3][key]), bits(b[3][key])), key
    assert a[3]["stats"] == b[3]["stats"] and a[3]["stats"]["history_frames"] == 2 and a[4] == b[4] == 5
    for key in ("fb", "lin", "xyz"):
        for p, q in zip(a[1][key], b[1][key]):
            assert np.array_equal(bits(p), bits(q)), key
    assert np.array_equal(bits(stack_features(a[2])), bits(stack_features(b[2])))


def test_refusals(srt, gpu):
    scene, cam, W, Hh, _, depth = H.edge_case_scene(srt, "two_triangles")
    fresh_context(gpu, scene, cam, W, Hh, depth)
    v0 = scene.vertices()
    expect_error(srt, lambda: gpu.surface_motion(8, 8), ERR_INVALID, "tracking off")
    gpu.track_motion(True)
    try:
        expect_error(srt, lambda: gpu.surface_motion(8, 8), ERR_INVALID, "vertices unknown after the switch")
        gpu.upload_scene(scene)
        gpu.surface_motion(8, 8)
    finally:
        gpu.track_motion(False)
    other = srt.Renderer(0)
    try:
        expect_error(srt, lambda: other.surface_motion_kat(cam, v0, 8, 8), ERR_INVALID, "no scene uploaded")
    finally:
        other.close()
    expect_error(srt, lambda: gpu.surface_motion_kat(cam, np.concatenate([v0, v0]), 8, 8), ERR_INVALID, "wrong n_tris")
    bad = v0.copy()
    bad[1, 2, 0] = np.inf
    expect_error(srt, lambda: gpu.surface_motion_kat(cam, bad, 8, 8), ERR_INVALID, "non-finite current vertex")
    expect_error(srt, lambda: gpu.surface_motion_kat(cam, v0, 8, 8, prev_verts=bad), ERR_INVALID, "non-finite previous vertex")
    L, B = srt.binding.lib(), srt.binding
    res = B.MotionResult()
    import ctypes as C
    for w, h, ox, oy in ((0, 4, 0, 0), (4, 0, 0, 0), (4, 4, 2 ** 24 - 3, 0), (4, 4, 0, 2 ** 24 - 3), (2 ** 16, 2 ** 15, 0, 0)):
        assert L.srt_surface_motion_kat(gpu._h, C.byref(cam), None, B.fptr(v0), v0.shape[0], w, h, ox, oy, None, None, None, C.byref(res)) == ERR_INVALID
    assert L.srt_surface_motion_kat(gpu._h, C.byref(cam), None, B.fptr(v0), v0.shape[0], 4, 4, 0, 0, None, None, None, None) == ERR_INVALID
