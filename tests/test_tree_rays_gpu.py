"""The segment dump of the instrumented kernel and the ray-weighted step of srt_tune_tree_for_throughput on the GPU."""
import hashlib

import numpy as np
import pytest

from helpers import assert_planes_equal, oracle_scene_for

pytestmark = pytest.mark.gpu

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
