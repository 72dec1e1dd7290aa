"""First-hit feature buffers (srt_accum_reset_features + srt_render_chunk_accum, render_kernel MODE 7).  Per pixel eight raw fp32 sums
-- face-forwarded normal, the material's colour, distance and hits of every sample's camera ray -- held bit for bit to a CPU prediction
built from the oracle (tests/features_reference.py): on three workloads, for every split of the samples, every partition, every launch
shape, on a leaf-root tree and with bounce_limit 0; and the image, the XYZ sums and the RNG state of a featured accumulation are those
of a plain one."""
import numpy as np
import pytest

from accum_helpers import (EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, assert_same_image, forced_shape, fresh_context, named_workload,
                           read_frame, read_sum_y, split_passes)
from features_reference import predict_features, shape_prediction, stack_features, workload_prediction
from helpers import bits, custom_scene

NAMES = ("normal x", "normal y", "normal z", "albedo r", "albedo g", "albedo b", "distance", "hits")


def features_run(gpu, scene, cam, W, H, depth, passes, spp=12):
    """a featured accumulation of `passes`; returns (frame after the last pass, rows (H, W, 8))"""
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp)
    gpu.accum_reset_features()
    for s in passes:
        gpu.render_chunk_accum(W, H, s)
    return read_frame(gpu, W, H), stack_features(gpu.read_features(W, H))


def assert_rows_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for c in range(8):
        a, b = bits(got[..., c]), bits(want[..., c])
        bad = np.argwhere(a != b)
        print("%s %s: %d of %d pixels differ" % (what, NAMES[c], len(bad), a.size))
        assert len(bad) == 0, "%s %s: %d of %d pixels differ, first (y, x) = %r: got %r want %r" % (
            what, NAMES[c], len(bad), a.size, tuple(bad[0]), got[..., c][tuple(bad[0])], want[..., c][tuple(bad[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "random_spheres", "dielectric"])
def test_features_equal_the_cpu_prediction(srt, gpu, orc, name):
    n = 6
    (scene, cam, W, H, depth, _), want = workload_prediction(srt, orc, name, n)
    hits = want["rows"][..., 7]
    # the prediction itself covers the three kinds of pixel, and a pixel whose samples hit different materials (the sum's order)
    assert (hits == 0).any() and (hits == n).any() and ((hits > 0) & (hits < n)).any(), (name, np.unique(hits, return_counts=True))
    mats = want["mats"]
    first = np.where(mats >= 0, mats, 1 << 30).min(axis=0)
    assert ((mats >= 0) & (mats != first)).any(), name + ": no pixel whose first hits differ in material between samples"
    _, got = features_run(gpu, scene, cam, W, H, depth, [n])
    assert_rows_equal(got, want["rows"], name)
    assert gpu.accum_samples == n and gpu.stats()["paths"] == W * H * n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "dielectric"])
def test_the_image_is_untouched(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    passes = [3, 2, 4]
    featured, _ = features_run(gpu, scene, cam, W, H, depth, passes, spp=3)
    sum_y = read_sum_y(gpu, W, H)
    gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
    after = read_frame(gpu, W, H)
    fresh_context(gpu, scene, cam, W, H, depth, spp=3)
    gpu.accum_reset()
    for s in passes:
        gpu.render_chunk_accum(W, H, s)
    plain = read_frame(gpu, W, H)
    plain_y = read_sum_y(gpu, W, H)
    gpu.render_chunk(W, H)
    plain_after = read_frame(gpu, W, H)
    assert_same_image(featured, plain, name + " featured vs plain")
    assert_same_image(after, plain_after, name + " RNG state: plain launch after the passes")
    assert np.array_equal(bits(sum_y), bits(plain_y))


@pytest.mark.gpu
def test_splits_and_partitions(srt, gpu, orc):
    n = 6
    (scene, cam, W, H, depth, _), want = workload_prediction(srt, orc, "random_spheres", n)
    for passes in ([n], [1] * n, split_passes(n)):
        _, got = features_run(gpu, scene, cam, W, H, depth, passes)
        assert_rows_equal(got, want["rows"], "passes %r" % (passes,))
    world = 3
    parts = []
    for rank in range(world):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.set_partition(rank, world)
        gpu.accum_reset_features()
        for s in split_passes(n):
            gpu.render_chunk_accum(W, H, s)
        parts.append(stack_features(gpu.read_features(W, H)))
    gpu.set_partition(0, 1)
    # every pixel's row is on exactly one rank (its tile's owner) and +0 on the others
    nonzero = np.stack([(bits(p) != 0).any(axis=-1) for p in parts])
    assert (nonzero.sum(axis=0) <= 1).all()
    assert (nonzero.sum(axis=0) == (want["rows"][..., 7] > 0)).all()
    assert all(nz.any() for nz in nonzero), "a rank without a hit pixel"
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    assert_rows_equal(total, want["rows"], "sum of %d ranks" % world)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_shape_equals_the_prediction(srt, gpu, orc, knobs, paired, expect):
    n = 4
    (scene, cam, W, H, depth), want = shape_prediction(srt, orc, paired, n)
    assert (want["rows"][..., 7] > 0).any() and (want["rows"][..., 7] < n).any()
    with forced_shape(gpu, scene, knobs, expect):
        _, got = features_run(gpu, scene, cam, W, H, depth, [1, 3])
    assert_rows_equal(got, want["rows"], "shape %r" % (expect,))


@pytest.mark.gpu
def test_leaf_root_and_bounce_limit_zero(srt, gpu, orc):
    scene = custom_scene(srt, [((-3, -2, 0), (3, -2, 0), (0, 3, 0), 0, 0)], [(0, (0.25, 0.25, 0.25), 0.0, 0.0)]).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, n = 45, 37, 4
    cam = srt.camera_init(W, H, 60.0, (0.3, 0.2, 9.0), (0.0, 0.0, 0.0))
    want = predict_features(orc, scene, cam, W, H, n, 6, 0)
    assert (want["rows"][..., 7] == n).any() and (want["rows"][..., 7] == 0).any()
    _, got = features_run(gpu, scene, cam, W, H, 6, [1, 3])
    assert_rows_equal(got, want["rows"], "one triangle")
    assert (got[..., 3:6][got[..., 7] == n] == np.float32(0.25 * n)).all()      # (grey: the table-free bake; random_spheres has the colours)
    # bounce_limit 0: no query is made, nothing is deposited
    for sc, cm, w, h in ((scene, cam, W, H),) + (named_workload(srt, "prism")[:4],):
        _, got = features_run(gpu, sc, cm, w, h, 0, [2, 2])
        assert not bits(got).any(), "bounce_limit 0 deposited something"
        assert gpu.accum_samples == 4


@pytest.mark.gpu
def test_chunk_placement(srt, gpu, orc):
    """a 30 x 21 chunk (no multiple of 8 x 8 or 28 x 16) at (17, 9) of a 64 x 40 image: only its rectangle is written, with the rows the
    prediction gives for that chunk (the camera ray of a pixel follows its image coordinates, its RNG stream its lane of the chunk's grid)"""
    scene, _, _, _, depth, _ = named_workload(srt, "random_spheres")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    fresh_context(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset_features()
    for s in (1, 2):
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    lib = srt.binding.lib()
    sentinel = np.float32(-7.0)
    out = np.full((IH, IW, 8), sentinel, np.float32)
    gpu._ck(lib.srt_read_features(gpu._h, srt.binding.fptr(out), IW, IH))
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert (out[~inside] == sentinel).all()
    assert (out[inside] >= np.float32(-3.0)).all() and out[inside][:, 7].max() > 0
    zeros = stack_features(gpu.read_features(IW, IH))
    assert not bits(zeros[~inside]).any() and np.array_equal(bits(zeros[inside]), bits(out[inside]))
    want = predict_features(orc, scene, cam, cw, ch, 3, depth, 1, offx=ox, offy=oy)
    assert_rows_equal(out[oy:oy + ch, ox:ox + cw], want["rows"], "offset chunk")
