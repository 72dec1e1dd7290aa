"""srt_scene_refit on the host (no GPU): new vertices on the built topology leave the scene a fresh build of the moved triangles with
that topology would leave -- triangle records bit for bit, node boxes against a numpy restatement and against the oracle's own sweep --
and every refusal leaves the scene as it was.  The specification of the device path (tests/test_refit.py)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import refit_cases as R

SEEDS = (0, 1, 2, 3, 5, 8)


def _check_refitted(srt, orc, scene, v, mode, cam, W, Hh, topo):
    fresh = R.moved(srt, scene, v)
    assert np.array_equal(scene.tri_records().view(np.uint32), fresh.tri_records().view(np.uint32)), "triangle records differ from a fresh scene's"
    assert bytes(scene.triangles()) == bytes(fresh.triangles())
    left, right, prim, boxes = scene.bvh()
    for name, a in zip(("left", "right", "prim"), (left, right, prim)):
        assert np.array_equal(a, topo[name]), "refit changed " + name
    want = R.restated_boxes(scene)
    # bit for bit away from ties of zeros with opposite signs (numpy's fmin / fmax may pick either, like the C library's), as values there
    tie = (boxes == 0) & (want == 0)
    assert np.array_equal(boxes.view(np.uint32)[~tie], want.view(np.uint32)[~tie])
    R.assert_values_equal(boxes, want, "node boxes against the restatement")
    # the oracle, fed the moved triangles and the imported topology, recomputes the boxes itself and renders
    osc = H.oracle_scene_for(orc, scene, 1)
    R.assert_values_equal(osc.bvh()[3], boxes, "node boxes against the oracle's")
    res = osc.render(cam, W, Hh, 1, 2, threads=4)
    assert res["stats"]["paths"] > 0


def test_refit_matches_a_fresh_scene(srt, orc):
    modes = set()
    for seed in SEEDS:
        scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, seed)
        modes.add(mode)
        before = R.scene_state(scene)
        v0 = scene.vertices()
        assert v0.shape == (n, 3, 3)
        v1 = R.jitter(v0, seed)
        scene.refit(v1)
        _check_refitted(srt, orc, scene, v1, mode, cam, W, Hh, before)
        assert scene.is_paired == before["paired"] and scene.n_nodes == before["nodes"]
        v2 = R.smooth(v0)
        scene.refit(v2)
        _check_refitted(srt, orc, scene, v2, mode, cam, W, Hh, before)
        scene.refit(v0)
        R.assert_state_equal(before, R.scene_state(scene), "refit(v0) after two motions (seed %d)" % seed)
    assert modes == {srt.BVH_REFERENCE, srt.BVH_SAH}, "the seeds must cover both builders"


@pytest.mark.parametrize("case", ["degenerate", "axis_aligned", "thin", "signed_zero"])
def test_refit_edge_motions(srt, orc, case):
    scene, cam, W, Hh, spp, depth, v1, v2 = R.motion_scene(srt, case)
    before = R.scene_state(scene)
    v0 = scene.vertices()
    for v in (v1, v2):
        scene.refit(v)
        _check_refitted(srt, orc, scene, v, 0, cam, W, Hh, before)
    if case == "axis_aligned":      # the motions really change the projection planes (record word 5)
        planes = [R.moved(srt, scene, v).tri_records()[:, 5] for v in (v0, v1, v2)]
        assert not np.array_equal(planes[0], planes[1]) and not np.array_equal(planes[1], planes[2])
    if case == "thin":              # ... and the padding really applies: a box wider than its vertices' extent
        scene.refit(v1)
        rec = scene.tri_records()
        assert rec[2, 11] - rec[2, 10] > v1[2, :, 2].max() - v1[2, :, 2].min()
    scene.refit(v0)
    R.assert_state_equal(before, R.scene_state(scene), "refit(v0)")


@pytest.mark.parametrize("which", R.UNPAIRED)
def test_refit_unpaired_sah_trees(srt, orc, which):
    """trees with a leaf + INNER node: a FRINGE record whose internal child is an INNER record, in front of it in the record order"""
    scene, cam, W, Hh, spp, depth = R.unpaired_scene(srt, which)
    assert R.leaf_plus_inner_nodes(scene) >= 1 and not scene.is_paired
    before = R.scene_state(scene)
    v0 = scene.vertices()
    for v in (R.jitter(v0, 11), R.smooth(v0)):
        scene.refit(v)
        _check_refitted(srt, orc, scene, v, 1, cam, W, Hh, before)
    scene.refit(v0)
    R.assert_state_equal(before, R.scene_state(scene), "refit(v0)")


def test_refit_schedule_is_the_restated_heights(srt):
    """the level schedule of the device refit (srt_scene_refit_schedule) against the heights restated from the node dump: every record in
    exactly one level, children below parents -- for both builders, optimised trees, the trees with a leaf + INNER node (where record
    indices do not order parents and children), the root-is-a-leaf tree and the single FRINGE record"""
    scenes = [H.fuzz_case(srt, seed)[0] for seed in range(14)]
    scenes += [H.fuzz_case(srt, seed)[0].build_bvh(srt.BVH_SAH, 1984).optimise_bvh(3) for seed in (1, 6, 14)]
    scenes += [R.unpaired_scene(srt, which)[0] for which in R.UNPAIRED]
    assert sum(R.leaf_plus_inner_nodes(s) > 0 for s in scenes) >= 6
    for k, scene in enumerate(scenes):
        got, want = scene.refit_schedule(), R.restated_schedule(scene)
        assert np.array_equal(got, want), (k, got, want)
        assert int(got.sum()) == scene.n_tris - 1      # a binary tree with one triangle per leaf
    assert H.edge_case_scene(srt, "one_triangle")[0].refit_schedule().size == 0
    assert list(H.edge_case_scene(srt, "two_triangles")[0].refit_schedule()) == [1]
    B = srt.binding
    n = C.c_uint32()
    assert B.lib().srt_scene_refit_schedule(None, None, 0, C.byref(n)) == -1
    assert B.lib().srt_scene_refit_schedule(scenes[0].handle, None, 0, None) == -1
    one = (C.c_uint32 * 1)()
    assert B.lib().srt_scene_refit_schedule(scenes[1].handle, one, 1, C.byref(n)) == -1      # cap too small
    assert B.lib().srt_scene_refit_schedule(R.moved(srt, scenes[0], scenes[0].vertices()).handle, None, 0, C.byref(n)) == -1      # no BVH


def test_gpu_fuzz_seeds_cover_both_builders(srt):
    """the seeds tests/test_refit.py refits on the device: both builders, paired and unpaired trees"""
    cases = [H.fuzz_case(srt, seed) for seed in (0, 1, 3, 7, 11)]
    assert {c[6] for c in cases} == {srt.BVH_REFERENCE, srt.BVH_SAH}
    assert {c[0].is_paired for c in cases} == {True, False}


def test_refit_refusals_leave_the_scene_unchanged(srt):
    B = srt.binding
    scene, *_ = H.fuzz_case(srt, 1)
    before = R.scene_state(scene)
    v = scene.vertices()
    n = v.shape[0]
    L = B.lib()
    good = R.jitter(v, 99)
    assert L.srt_scene_refit(None, B.fptr(good), n) == -1
    assert L.srt_scene_refit(scene.handle, None, n) == -1
    assert L.srt_scene_refit(scene.handle, B.fptr(good), n - 1) == -1
    assert L.srt_scene_refit(scene.handle, B.fptr(good), n + 1) == -1
    for poison in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[n - 1, 2, 1] = poison      # the very last triangle: everything before it must stay untouched too
        with pytest.raises(B.SrtError) as e:
            scene.refit(bad)
        assert e.value.code == -1
        R.assert_state_equal(before, R.scene_state(scene), "a refused refit (%r)" % poison)
    R.assert_state_equal(before, R.scene_state(scene), "refused refits")
    # a scene whose BVH is not built
    unbuilt = R.moved(srt, scene, v)
    with pytest.raises(B.SrtError) as e:
        unbuilt.refit(good)
    assert e.value.code == -1
    assert bytes(unbuilt.triangles()) == bytes(R.moved(srt, scene, v).triangles())
    # the Python face refuses wrong shapes and dtypes itself
    for wrong, exc in ((good.astype(np.float64), TypeError), (good.reshape(-1, 9), ValueError), (good[:, :2], ValueError), (good.tolist(), TypeError),
                       (np.zeros((0, 3, 3), np.float32), ValueError)):
        with pytest.raises(exc):
            scene.refit(wrong)
    R.assert_state_equal(before, R.scene_state(scene), "refused arguments")
