"""The segment dump of the instrumented kernel and the ray-weighted step of srt_tune_tree_for_throughput on the GPU."""
import collections
import ctypes as C
import hashlib

import numpy as np
import pytest

import ground_truth as G
from helpers import assert_planes_equal, edge_case_scene, oracle_scene_for

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
FRAME = (1920, 1080)      # the frame the trees are tuned FOR: far above 6 pixels per lane on one GPU (the renders below are 64 x 64)


def _built(srt, sid):
    return srt.Scene.builtin(sid, 0).build_bvh(srt.BVH_SAH, 1984)


def _sha(scene):
    h = hashlib.sha256()
    for a in scene.bvh():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _production_frame(srt, gpu, scene, W, H, spp, depth):
    out = srt.render_image(scene, scene.default_camera(W, H), W, H, spp, depth, renderer=gpu)
    return [np.array(p, copy=True) for p in out["fb"] + out["xyz"]], out["stats"]["rays"]


def test_segment_dump(srt, gpu):
    """Scene 100 at 64 x 64 x 2 spp, depth 4.  Every finished query with a direction that is not NaN takes a ticket, so the tickets are
    stats()["rays"] minus the NaN-direction queries of the dump's own frame, and the segments written are the tickets t with (t + seed %
    stride) % stride == 0 -- for stride 1 (every query; the array is the same in a second dump), 7 and 64, and for a capacity below that
    number the capacity.  Every t_end is positive, every origin finite, no direction NaN; without a lens the camera rays start at the camera.  The
    production frame rendered before and after the dumps is the same, bit for bit in its framebuffer and XYZ planes."""
    W, H, spp, depth = 64, 64, 2, 4
    scene = _built(srt, 100)
    cam = scene.default_camera(W, H)
    before, rays_before = _production_frame(srt, gpu, scene, W, H, spp, depth)
    first = None
    for stride, seed, capacity in ((1, 0, None), (1, 5, None), (7, 3, None), (64, 1984, None), (7, 3, 100)):
        gpu.upload_scene(scene); gpu.set_camera(cam)
        segs, queries = gpu.collect_ray_segments(W, H, spp, depth, stride=stride, seed=seed, capacity=capacity)
        st = gpu.stats()
        assert st["rays"] == rays_before and queries == st["rays"] - st["util"][2]
        predicted = len(range((-(seed % stride)) % stride, queries, stride))
        print("stride %d seed %d: %d queries (%d NaN directions), %d segments" % (stride, seed, queries, st["util"][2], len(segs)))
        assert len(segs) == (predicted if capacity is None else min(predicted, capacity)) > 0
        assert (segs[:, 6] > 0).all() and np.isfinite(segs[:, 0:3]).all() and not np.isnan(segs[:, 3:6]).any()
        if stride == 1:
            assert len(segs) == queries
            centre = np.array(list(cam.camera_center), np.float32)
            if not cam.defocus_angle > 0:      # (no lens: the camera rays, one per path, start at the camera's centre)
                assert int((segs[:, 0:3] == centre).all(axis=1).sum()) == W * H * spp
            if first is None:
                first = segs
            else:
                assert first.tobytes() == segs.tobytes()
    after, rays_after = _production_frame(srt, gpu, scene, W, H, spp, depth)
    assert rays_after == rays_before
    assert_planes_equal(after, before, "production frame after the dumps")


DUMPED_FRAMES = ("random spheres, lens", "42 triangles", "42 triangles, reference tree", "two_triangles")
_dumps = {}


def _dump(srt, gpu, which):
    """the stride 1 dump of one of the dumped frames, taken once per session -> scene, cam, W, H, spp, depth, rows, queries, stats"""
    if which not in _dumps:
        if which == "two_triangles":
            scene, cam, W, H, spp, depth = edge_case_scene(srt, "two_triangles")
        else:
            scene = _built(srt, 100) if which == "random spheres, lens" else srt.Scene.builtin(0, 0).build_bvh(
                srt.BVH_REFERENCE if which.endswith("reference tree") else srt.BVH_SAH, 1984)
            cam, W, H, spp, depth = scene.default_camera(32, 32), 32, 32, 2, 4
        gpu.upload_scene(scene); gpu.set_camera(cam)
        segs, queries = gpu.collect_ray_segments(W, H, spp, depth, stride=1)
        _dumps[which] = (scene, cam, W, H, spp, depth, segs, queries, gpu.stats())
    return _dumps[which]


def _oracle_closest_hits(orc, osc, segs):
    """orc_trace_ray on origin and direction of every row (the words of the row itself: no copy, no conversion) -> hit flags, t"""
    orc.lib()
    fn = C.CDLL(orc.ORACLE_SO).orc_trace_ray
    fn.argtypes, fn.restype = [C.c_void_p] * 4, C.c_int
    segs = np.ascontiguousarray(segs, np.float32)
    out9 = np.zeros(9, np.float32)
    hit, t = np.zeros(len(segs), bool), np.zeros(len(segs), np.float32)
    base, po = segs.ctypes.data, out9.ctypes.data
    for k in range(len(segs)):
        if fn(osc.h, base + 28 * k, base + 28 * k + 12, po):
            hit[k], t[k] = True, out9[0]
    return hit, t


def _from_camera(cam, segs):
    return (segs[:, 0:3] == np.array(list(cam.camera_center), np.float32)).all(axis=1)


@pytest.mark.parametrize("which", DUMPED_FRAMES)
def test_segment_dump_rows_are_true_closest_hits(srt, gpu, orc, which):
    """Stride 1 dumps of scene 100 (SAH tree; the camera has a lens) and scene 0 (SAH tree, reference tree) at 32 x 32 x 2 spp, depth 4,
    and of the two-triangle scene at 45 x 37 x 6 spp, depth 6, row by row:
      order    the rows ascend lexicographically by the uint32 bit patterns of their seven words (np.lexsort is the restatement)
      oracle   orc_trace_ray fed the row's own origin and direction finds a hit with t bit-equal to t_end, or misses where t_end is
               FLT_MAX -- the same float32 arithmetic on the same tree and the same t interval (orc_trace_ray and the oracle's path tracer
               both query [0, FLT_MAX], as the kernel does, so every row is compared): 0 differing rows.  A t_end of another lane's query,
               an origin or direction the shading pass had already replaced, or a hit stored as a miss fails here.
      counts   rows with t_end == FLT_MAX number queries - stats()["hits"]; without a lens the rows from the camera centre number W H spp
    Measured on one MI355X, rows compared (hits + misses), all with 0 differing: scene 100 4 762 (2 975 + 1 787), scene 0 6 267 (5 266 +
    1 001) on the SAH tree and on the reference tree alike, two triangles 14 850 (4 860 + 9 990).  (Before the builder split leaf pairs
    too thin for the slab test, scene 0's SAH tree gave 5 326 rows, 4 084 + 1 242: the paths that lost the back wall ended early.)"""
    scene, cam, W, H, spp, depth, segs, queries, st = _dump(srt, gpu, which)
    assert len(segs) == queries == st["rays"] - st["util"][2] > 0
    words = np.ascontiguousarray(segs).view(np.uint32)
    assert np.array_equal(np.lexsort(words.T[::-1]), np.arange(len(words))), "the rows are not in canonical order"
    hit, t = _oracle_closest_hits(orc, oracle_scene_for(orc, scene, 1), segs)
    missed = segs[:, 6] == FLT_MAX
    differ = (hit == missed) | (hit & (t.view(np.uint32) != np.ascontiguousarray(segs[:, 6]).view(np.uint32)))
    print("%s: %d rows, %d hits, %d misses, %d differ from the oracle" % (which, len(segs), (~missed).sum(), missed.sum(), differ.sum()))
    assert not differ.any(), ("first differing row", int(np.nonzero(differ)[0][0]), segs[np.nonzero(differ)[0][0]], hit[differ][0], t[differ][0])
    assert int(missed.sum()) == queries - st["hits"] and 0 < missed.sum() < len(segs)
    assert (cam.defocus_angle > 0) == (which == "random spheres, lens")
    if not cam.defocus_angle > 0:
        assert int(_from_camera(cam, segs).sum()) == W * H * spp


@pytest.mark.parametrize("which", DUMPED_FRAMES[1:])
def test_segment_dump_camera_rows_against_the_truth(srt, gpu, which):
    """The rows from the camera centre (no lens: one per path) against ground_truth.closest_hit over ALL triangles, no tree: every row at
    least EDGE_MARGIN from every edge agrees in hit / miss and has |t_end - t| <= C_T t_bound; at most MAX_EXCLUDED of the rows are left
    out.  The rows are bit for bit what the oracle finds (the test above), so the share the reference leaves out is the same: 0 rows.
    Measured on one MI355X: scene 0, on the SAH and on the reference builder's tree alike, 2 048 rows, 1 867 hits in the truth, 0 inside the margin, 0 differ,
    largest |dt| / t_bound 0.792; two triangles 9 990 rows, 4 860 hits, 0 inside the margin, 0 differ, 0.283.

    "42 triangles" (scene 0 on this build's SAH tree) is the case that found a fault: 374 of its 2 048 camera rows (18 %; truth's triangles
    4 and 5, the back wall at z = 555) were stored as misses, by device and oracle alike -- the SAH builder had paired the wall's two
    coplanar triangles under a node whose box, two ulps thick, the reference's slab test (aabb.cu:7-40, max <= min rejects) cannot resolve
    from 1 355 away; leaves carry no box test, so the reference builder's tree lost none.  The builders now split such pairs
    (srt_host.cpp, split_pairs_too_thin_for_slab_test), and the case passes on the device."""
    scene, cam, W, H, spp, depth, segs, queries, st = _dump(srt, gpu, which)
    rows = segs[_from_camera(cam, segs)]
    assert len(rows) == W * H * spp
    V, o, d = G.f64(scene.vertices()), G.f64(rows[:, 0:3]), G.f64(rows[:, 3:6])
    t64, tri, _, near = G.closest_hit(V, o, d)
    held = near >= G.EDGE_MARGIN
    want_hit, got_hit = tri >= 0, rows[:, 6] < FLT_MAX
    k = np.maximum(tri, 0)
    with np.errstate(all="ignore"):
        ratio = np.where(got_hit & want_hit, np.abs(rows[:, 6].astype(np.float64) - t64) / G.t_bound(G.normals(V)[1][k], V[k, 0], o, d, t64), 0.0)
    bad = held & (got_hit != want_hit)
    print("%s: %d camera rows, %d hit in the truth, %d inside the margin, %d differ in hit / miss (truth's triangles %s), largest |dt| / t_bound %.3f" %
          (which, len(rows), want_hit.sum(), (~held).sum(), bad.sum(), sorted(set(tri[bad].tolist())), ratio[held].max()))
    assert not bad.any(), "%d of %d camera rows differ from the truth in hit / miss, first %r" % (bad.sum(), len(rows), rows[np.nonzero(bad)[0][0]])
    assert ratio[held].max() <= G.C_T and (~held).mean() <= G.MAX_EXCLUDED and want_hit.any()


def test_a_strided_dump_is_part_of_the_full_one(srt, gpu):
    """The stride 7 dump of scene 0's frame is a sub-multiset of its stride 1 dump, rows compared as byte strings: a sampled ticket writes
    the query it belongs to, whole"""
    scene, cam, W, H, spp, depth, segs, queries, st = _dump(srt, gpu, "42 triangles")
    gpu.upload_scene(scene); gpu.set_camera(cam)
    some, q7 = gpu.collect_ray_segments(W, H, spp, depth, stride=7, seed=3)
    assert q7 == queries and len(some) == len(range((-(3 % 7)) % 7, queries, 7)) > 0
    have = collections.Counter(r.tobytes() for r in segs)
    want = collections.Counter(r.tobytes() for r in some)
    assert all(have[r] >= n for r, n in want.items()), "a row of the stride 7 dump is not a row of the stride 1 dump"


@pytest.mark.parametrize("sid", [100, 0], ids=["random spheres", "42 triangles"])
def test_parity_on_the_tuned_tree(srt, gpu, orc, sid):
    """srt_tune_tree_for_throughput, gated, for a 1920 x 1080 frame (throughput-bound: the gate lets it through), then 64 x 64 x 4 spp at
    depth 16 through the production and the instrumented kernel against the oracle walking the same tree: 0 differing values in all
    nine planes and equal ray counts.  The recipe took its ray-weighted step (kept, undone for LDS or vetoed by the counters -- it says
    which), a tree that was LDS resident still is, a paired tree is still paired, and a second copy of the scene arrives at the same tree."""
    W, H, spp, depth = 64, 64, 4, 16
    scene = _built(srt, sid)
    gpu.upload_scene(scene)
    resident, paired = gpu.launch_plan()["all_cached"], scene.is_paired
    t = srt.tree_tuning(gpu, scene, FRAME[0], FRAME[1], depth, gate=True)
    print("tree tuning: %r" % (t,))
    assert t["throughput_bound"] == 1 and t["order_status"] == 0 and t["reinsertion"] in (2, 3, 4)
    assert 0 < t["segments"] <= 2048
    gpu.upload_scene(scene)
    assert gpu.launch_plan()["all_cached"] or not resident
    assert scene.is_paired == paired
    again = _built(srt, sid)
    assert srt.tree_tuning(gpu, again, FRAME[0], FRAME[1], depth, gate=True) == t and _sha(again) == _sha(scene)
    cam = scene.default_camera(W, H)
    ref = oracle_scene_for(orc, scene, 1).render(cam, W, H, spp, depth)
    for counting in (False, True):
        out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=counting)
        for name in ("fb", "lin", "xyz"):
            assert_planes_equal(out[name], ref[name], "%s kernel, %s" % ("instrumented" if counting else "production", name))
        assert out["stats"]["rays"] == ref["stats"]["rays"]


def test_useless_sample_keeps_the_tree_that_walked_in(srt, gpu):
    """The recipe fed a sample of zero-length segments (srt_tune_tree_with_segments): none of them is usable, the topology is the one that
    walked in, and the report says so -- the tree equals a second copy taken through the child-order step alone."""
    depth = 16
    scene, hand = _built(srt, 100), _built(srt, 100)
    segs = np.zeros((4096, 7), np.float32)
    segs[:, 0:3] = np.array(list(scene.default_camera(64, 64).camera_center), np.float32)
    segs[:, 3:6] = np.random.default_rng(3).normal(size=(4096, 3)).astype(np.float32)
    gpu.upload_scene(scene)
    t = srt.tree_tuning(gpu, scene, FRAME[0], FRAME[1], depth, gate=True, segments=segs)
    print("tree tuning: %r" % (t,))
    assert t["throughput_bound"] == 1 and t["reinsertion"] == 5 and t["segments"] == 0 and t["order_status"] == 0
    gpu.upload_scene(hand)
    swapped, _ = srt.profile_child_order(gpu, hand, FRAME[0], FRAME[1], depth)
    assert swapped == t["nodes_swapped"] and _sha(hand) == _sha(scene)
    assert "no usable ray segment" in srt.tune_tree_for_throughput(gpu, _built(srt, 100), FRAME[0], FRAME[1], depth, gate=True, segments=segs)
