"""Adaptive sampling with first-hit features in one accumulation (srt_accum_reset_adaptive_features + srt_render_chunk_accum,
render_kernel MODE 8).  Everything the adaptive accumulation keeps -- image, nine planes, sums, S2, sample map, active counts, RNG state
-- is bit-identical to a MODE 4 run under the same cfg and schedule; every pixel's feature row is the CPU prediction
(tests/features_reference.py) of a plain featured frame of the pixel's own count; a converged pixel's row is never touched again; and
the result does not depend on launch shape, partition, chunk offset or the split into passes."""
import ctypes as C

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, MIN_SPP, NEVER, SCHED, adaptive_run,
                           assert_same_image, expect_error, forced_shape, fresh_context, gather_ranks, gpu_lib, lane_of, named_workload,
                           pick_tolerance, predict_stops, read_frame, shape_case)
from features_reference import predict_features, shape_prediction, stack_features, workload_prediction
from helpers import assert_planes_equal, bits, custom_scene, oracle_scene_for

NAMES = ("normal x", "normal y", "normal z", "albedo r", "albedo g", "albedo b", "distance", "hits")
SMALL_SCHED, SMALL_MIN = [2, 2, 2], 2       # counts 2, 4, 6: the feature predictions of tests/test_features.py reach 6 samples


def adaptive_features_run(gpu, scene, cam, W, H, depth, rel_tol, sched=SCHED, min_spp=MIN_SPP, abs_tol=0.0, spp=12):
    """accum_helpers.adaptive_run on an adaptive FEATURED accumulation; per pass also rows (H, W, 8)"""
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp)
    gpu.accum_reset_adaptive_features(rel_tol, abs_tol, min_spp)
    assert gpu.accum_active == 0
    out = []
    for s in sched:
        gpu.render_chunk_accum(W, H, s)
        out.append(dict(total=gpu.accum_samples, active=gpu.accum_active, paths=gpu.stats()["paths"], stats=gpu.accum_stats(W, H),
                        frame=read_frame(gpu, W, H), rows=stack_features(gpu.read_features(W, H))))
    return out


def assert_rows_equal(got, want, what, mask=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for c in range(8):
        a, b = bits(np.ascontiguousarray(got[..., c])), bits(np.ascontiguousarray(want[..., c]))
        differ = (a != b) if mask is None else (a != b) & mask
        bad = np.argwhere(differ)
        assert len(bad) == 0, "%s %s: %d pixels differ, first (y, x) = %r: got %r want %r" % (
            what, NAMES[c], len(bad), tuple(bad[0]), got[..., c][tuple(bad[0])], want[..., c][tuple(bad[0])])


def assert_same_pass(got, want, what):
    """everything an adaptive accumulation keeps after a pass"""
    assert got["total"] == want["total"] and got["active"] == want["active"] and got["paths"] == want["paths"], (what, got["total"], got["active"], want["active"])
    for k in ("samples", "sum_y", "sum_y2"):
        assert np.array_equal(got["stats"][k].view(np.uint32), want["stats"][k].view(np.uint32)), (what, k)
    assert_same_image(got["frame"], want["frame"], what)


def small_tolerance(never):
    """pick_tolerance for SMALL_SCHED: the tolerance that ends the schedule with the most distinct counts while a pixel is still active"""
    best, best_n = None, 0
    for rel in np.geomspace(1e-3, 10.0, 121):
        maps, stop, _ = predict_stops(never, float(rel), 0.0, SMALL_MIN)
        n = len(np.unique(stop[stop > 0]))
        if (stop == 0).any() and n > best_n:
            best, best_n = float(rel), n
    assert best is not None
    return best


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "cornell", "random_spheres", "dielectric"])
def test_everything_adaptive_equals_mode_4(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    rel = pick_tolerance(never)
    want = adaptive_run(gpu, scene, cam, W, H, depth, rel)
    gpu.render_chunk(W, H)                # a plain launch continues every pixel's RNG stream from where its own count left it
    want_after = read_frame(gpu, W, H)
    assert len(np.unique(want[-1]["stats"]["samples"])) >= 3 and want[-1]["active"] > 0
    got = adaptive_features_run(gpu, scene, cam, W, H, depth, rel)
    gpu.render_chunk(W, H)
    got_after = read_frame(gpu, W, H)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_pass(g, w, "%s pass %d" % (name, k))
    assert_same_image(got_after, want_after, name + " RNG state: a plain launch after the run")
    assert (got[-1]["rows"][..., 7] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dielectric", "random_spheres"])
def test_every_row_is_the_prediction_at_the_pixels_own_count(srt, gpu, orc, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER, sched=SMALL_SCHED, min_spp=SMALL_MIN)
    rel = small_tolerance(never)
    maps, stop, actives = predict_stops(never, rel, 0.0, SMALL_MIN)
    # the prediction: pixels stopped at two or more distinct counts, and a pixel still active
    stopped = np.unique(stop[stop > 0])
    print("%s rel %g: stopped at %r, %d active" % (name, rel, {int(c): int((stop == c).sum()) for c in stopped}, int((stop == 0).sum())))
    assert len(stopped) >= 2 and (stop == 0).any()
    run = adaptive_features_run(gpu, scene, cam, W, H, depth, rel, sched=SMALL_SCHED, min_spp=SMALL_MIN)
    for p, want, act in zip(run, maps, actives):
        assert np.array_equal(p["stats"]["samples"], want) and p["active"] == act
    counts = run[-1]["stats"]["samples"].reshape(H, W)
    checked = np.zeros((H, W), bool)
    for c in np.unique(counts):
        _, pred = workload_prediction(srt, orc, name, int(c))
        assert_rows_equal(run[-1]["rows"], pred["rows"], "%s: %d pixels at %d spp" % (name, (counts == c).sum(), c), mask=counts == c)
        checked |= counts == c
    assert checked.all()
    # ... and after every pass: a pixel's row is that of its count then (an active pixel: the running total)
    for p in run[:-1]:
        cnt = p["stats"]["samples"].reshape(H, W)
        for c in np.unique(cnt):
            assert_rows_equal(p["rows"], workload_prediction(srt, orc, name, int(c))[1]["rows"], "%s after %d: at %d spp" % (name, p["total"], c), mask=cnt == c)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_shape(srt, gpu, orc, knobs, paired, expect):
    scene, cam, W, H, depth = shape_case(srt, paired)
    gpu.set_test_knobs()
    sched, mn, rel = [2, 2], 2, 0.2
    want = adaptive_run(gpu, scene, cam, W, H, depth, rel, sched=sched, min_spp=mn)
    counts = want[-1]["stats"]["samples"].reshape(H, W)
    assert set(np.unique(counts)) == {2, 4} and want[-1]["active"] > 0
    with forced_shape(gpu, scene, knobs, expect):
        got = adaptive_features_run(gpu, scene, cam, W, H, depth, rel, sched=sched, min_spp=mn)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_pass(g, w, "shape %r pass %d" % (expect, k))
    for c in (2, 4):
        _, pred = shape_prediction(srt, orc, paired, c)
        assert_rows_equal(got[-1]["rows"], pred["rows"], "shape %r at %d spp" % (expect, c), mask=counts == c)


@pytest.mark.gpu
def test_partitions_offset_chunk_and_split_into_passes(srt, gpu, orc):
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    rel = 0.1
    ref = adaptive_features_run(gpu, scene, cam, W, H, depth, rel)[-1]
    assert len(np.unique(ref["stats"]["samples"])) >= 2 and ref["active"] > 0
    for world in (2, 3):
        def one_rank(rank):
            fresh_context(gpu, scene, cam, W, H, depth)
            gpu.set_partition(rank, world)
            gpu.accum_reset_adaptive_features(rel, 0.0, MIN_SPP)
            for s in SCHED:
                gpu.render_chunk_accum(W, H, s)
            gpu.synchronize()
            return gpu.accum_stats(W, H)["samples"], gpu.accum_active, stack_features(gpu.read_features(W, H))      # (pixels of the other ranks read 0)
        samples, actives, rows = zip(*gather_ranks(gpu, world, one_rank))
        assert np.array_equal(sum(samples), ref["stats"]["samples"]), world
        assert sum(actives) == ref["active"], world
        assert_planes_equal(gpu.read_fb(), ref["frame"]["fb"], "world %d fb" % world)
        assert_planes_equal(gpu.read_fb_aux(2), ref["frame"]["xyz"], "world %d xyz" % world)
        nonzero = np.stack([(bits(r) != 0).any(axis=-1) for r in rows])
        assert (nonzero.sum(axis=0) <= 1).all() and all(nz.any() for nz in nonzero)
        total = rows[0]
        for r in rows[1:]:
            total = total + r
        assert_rows_equal(total, ref["rows"], "sum of %d ranks" % world)

    # a 30 x 21 chunk at (17, 9) of a 64 x 40 image: MODE 4's frame and map, and at each count the rows of a plain featured chunk
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam2 = scene.default_camera(IW, IH)
    sched, mn = [2, 2, 2], 2

    def chunk(kind, passes):
        fresh_context(gpu, scene, cam2, cw, ch, depth)
        {"both": lambda: gpu.accum_reset_adaptive_features(rel, 0.0, mn), "adaptive": lambda: gpu.accum_reset_adaptive(rel, 0.0, mn),
         "features": gpu.accum_reset_features}[kind]()
        for s in passes:
            gpu.render_chunk_accum(cw, ch, s, ox, oy)
        return (read_frame(gpu, IW, IH), gpu.accum_stats(IW, IH)["samples"].reshape(IH, IW) if kind != "features" else None,
                stack_features(gpu.read_features(IW, IH)) if kind != "adaptive" else None)
    frame, counts, rows = chunk("both", sched)
    frame4, counts4, _ = chunk("adaptive", sched)
    assert_same_image(frame, frame4, "offset chunk against MODE 4")
    assert np.array_equal(counts, counts4)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert not bits(rows[~inside]).any() and (counts[~inside] == 0).all() and (counts[inside] >= mn).all()
    assert len(np.unique(counts[inside])) >= 2
    for c in np.unique(counts[inside]):
        assert_rows_equal(rows, chunk("features", [int(c)])[2], "offset chunk at %d spp" % c, mask=inside & (counts == c))
    want = predict_features(orc, scene, cam2, cw, ch, 2, depth, 1, offx=ox, offy=oy)
    assert_rows_equal(rows[oy:oy + ch, ox:ox + cw], want["rows"], "offset chunk, the prediction at 2 spp", mask=counts[oy:oy + ch, ox:ox + cw] == 2)

    # at NEVER with min_spp = the total no pixel stops before the end: one pass, two and six give the same bits
    (_, _, _, _, _, _), pred = workload_prediction(srt, orc, "random_spheres", 6)
    one = adaptive_features_run(gpu, scene, cam, W, H, depth, NEVER, sched=[6], min_spp=6)[-1]
    assert (one["stats"]["samples"] == 6).all()
    assert_rows_equal(one["rows"], pred["rows"], "one pass of 6")
    for passes in ([2, 4], [1] * 6):
        got = adaptive_features_run(gpu, scene, cam, W, H, depth, NEVER, sched=passes, min_spp=6)[-1]
        assert_rows_equal(got["rows"], one["rows"], "passes %r" % (passes,))
        assert_same_image(got["frame"], one["frame"], "passes %r" % (passes,))
        for k in ("samples", "sum_y", "sum_y2"):
            assert np.array_equal(got["stats"][k].view(np.uint32), one["stats"][k].view(np.uint32)), (passes, k)


@pytest.mark.gpu
def test_a_converged_pixels_row_is_frozen(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    run = adaptive_features_run(gpu, scene, cam, W, H, depth, 0.25, sched=[4, 4], min_spp=4)
    counts = run[-1]["stats"]["samples"].reshape(H, W)
    done = counts < 8                       # stopped at 4 (or at 8 with the flag -- those are not needed here)
    hit_done = done & (run[-1]["rows"][..., 7] > 0)
    assert hit_done.any() and run[-1]["active"] > 0
    before = run[-1]["rows"]
    for _ in range(2):
        gpu.render_chunk_accum(W, H, 4)
    after = stack_features(gpu.read_features(W, H))
    later = gpu.accum_stats(W, H)["samples"].reshape(H, W)
    assert np.array_equal(later[done], counts[done])
    assert_rows_equal(after, before, "rows of the pixels that had stopped", mask=done)
    grew = later > counts
    assert grew.any() and (after[..., 7][grew] >= before[..., 7][grew]).all() and (after[..., 7][grew] > before[..., 7][grew]).any()
    stopped_since = (later == counts) & ~done          # converged exactly at 8: frozen as well
    assert_rows_equal(after, before, "rows of the pixels that stopped at the last boundary", mask=stopped_since)


@pytest.mark.gpu
def test_leaf_root_and_bounce_limit_zero(srt, gpu, orc):
    """a leaf-root tree (no traversal step at all) deposits what the prediction says; bounce_limit 0 makes no query: every row stays +0"""
    scene = custom_scene(srt, [((-3, -2, 0), (3, -2, 0), (0, 3, 0), 0, 0)], [(0, (0.25, 0.25, 0.25), 0.0, 0.0)]).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H = 45, 37
    cam = srt.camera_init(W, H, 60.0, (0.3, 0.2, 9.0), (0.0, 0.0, 0.0))
    run = adaptive_features_run(gpu, scene, cam, W, H, 6, 0.05, sched=[2, 2], min_spp=2)
    counts = run[-1]["stats"]["samples"].reshape(H, W)
    assert set(np.unique(counts)) == {2, 4}
    for c in (2, 4):
        want = predict_features(orc, scene, cam, W, H, c, 6, 0)
        assert_rows_equal(run[-1]["rows"], want["rows"], "one triangle at %d spp" % c, mask=counts == c)
    assert (run[-1]["rows"][..., 7] > 0).any()
    for sc, cm, w, h in ((scene, cam, W, H),) + (named_workload(srt, "prism")[:4],):
        got = adaptive_features_run(gpu, sc, cm, w, h, 0, 0.05, sched=[2, 2], min_spp=2)[-1]
        assert not bits(got["rows"]).any(), "bounce_limit 0 deposited something"
        assert gpu.accum_samples == 4


@pytest.mark.gpu
def test_refusals_and_invalidation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(0.1, 0.0, 4)
    assert gpu.accum_active == 0
    expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features before the first pass")
    expect_error(srt, lambda: gpu.accum_stats(W, H), ERR_INVALID, "accum_stats before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first, rows, active = read_frame(gpu, W, H), stack_features(gpu.read_features(W, H)), gpu.accum_active
    bad = [(0.0, 0.0, 4, 0), (-0.1, 0.0, 4, 0), (0.1, -1.0, 4, 0), (float("nan"), 0.0, 4, 0), (float("inf"), 0.0, 4, 0),
           (0.1, 0.0, 1, 0), (0.1, 0.0, 0, 0), (0.1, 0.0, 4, 1)]
    for rel, ab, mn, res in bad:        # straight through the C-ABI: the Python check would refuse most of them first
        cfg = srt.binding.Adaptive(rel, ab, mn, res)
        assert L.srt_accum_reset_adaptive_features(gpu._h, C.byref(cfg)) == ERR_INVALID, (rel, ab, mn, res)
        assert gpu.accum_samples == 4 and gpu.accum_active == active, (rel, ab, mn, res)
    assert L.srt_accum_reset_adaptive_features(gpu._h, None) == ERR_INVALID
    assert L.srt_accum_reset_adaptive_features(None, C.byref(srt.binding.Adaptive(0.1, 0.0, 4, 0))) == ERR_INVALID
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.accum_reset_adaptive_features(0.1), ERR_UNSUPPORTED, "instrumented context")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_UNSUPPORTED, "instrumented pass")
    gpu.set_count_traversal(False)
    for k, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, first[k], "after the refusals " + k)
    assert_rows_equal(stack_features(gpu.read_features(W, H)), rows, "rows after the refusals")
    gpu.render_chunk_accum(W, H, 4)         # the accumulation survived the refusals
    assert gpu.accum_samples == 8
    cont, cont_rows = read_frame(gpu, W, H), stack_features(gpu.read_features(W, H))
    again = adaptive_features_run(gpu, scene, cam, W, H, depth, 0.1, sched=[4, 4], min_spp=4)[-1]
    assert_same_image(cont, again["frame"], "continued after the refusals")
    assert_rows_equal(cont_rows, again["rows"], "rows continued after the refusals")
    # a context without device parameters: refused (srt_accum_reset_features' and srt_accum_reset_adaptive's rule)
    r = srt.Renderer(0)
    try:
        expect_error(srt, lambda: r.accum_reset_adaptive_features(0.1), ERR_INVALID, "no device parameters")
    finally:
        r.close()
    # srt_set_gather_planes ends it, as it ends an adaptive accumulation; so do the other invalidations
    gpu.set_gather_planes(9)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, "pass after srt_set_gather_planes")
    expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active after srt_set_gather_planes")
    expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features after srt_set_gather_planes")
    for what, call in (("srt_set_camera", lambda: gpu.set_camera(cam)), ("srt_render_chunk", lambda: gpu.render_chunk(W, H)),
                       ("srt_upload_scene", lambda: gpu.upload_scene(scene)), ("srt_set_partition", lambda: gpu.set_partition(0, 1))):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_adaptive_features(0.1, 0.0, 4)
        gpu.render_chunk_accum(W, H, 4)
        call()
        expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, what)
    # one accumulation per context and chunk, and the 65535-sample limit
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(0.1, 0.0, 4)
    gpu.render_chunk_accum(W, H, 4)
    expect_error(srt, lambda: gpu.render_chunk_accum(W - 8, H, 4), ERR_INVALID, "another chunk")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 65535), ERR_INVALID, "more than 65535 samples")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 0), ERR_INVALID, "no samples")
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == 8


@pytest.mark.gpu
def test_neighbouring_kinds(srt, gpu):
    """what the new kind's neighbours still refuse, and every other reset makes the next accumulation something else again"""
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
    resets = {"plain": gpu.accum_reset, "adaptive": lambda: gpu.accum_reset_adaptive(0.1, 0.0, 4), "features": gpu.accum_reset_features,
              "spectral": gpu.accum_reset_spectral, "streams": lambda: gpu.accum_reset_streams(2)}
    for kind, reset in resets.items():
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_adaptive_features(0.1, 0.0, 4)
        gpu.render_chunk_accum(W, H, 4)
        assert gpu.accum_active >= 0 and gpu.read_features(W, H)["hits"].max() > 0
        reset()
        gpu.render_chunk_accum(W, H, 4)
        if kind != "adaptive":
            expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active on a %s accumulation" % kind)
        else:
            assert gpu.accum_stats(W, H)["samples"].max() == 4
        if kind != "features":
            expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features on a %s accumulation" % kind)
            expect_error(srt, lambda: gpu.denoise(W, H), ERR_INVALID, "denoise on a %s accumulation" % kind)
        else:
            assert gpu.read_features(W, H)["hits"].max() == 4
        expect_error(srt, lambda: gpu.denoise_mv(W, H), ERR_INVALID, "denoise_mv on a %s accumulation" % kind)
    # a plain accumulation after the new kind behaves as before: passes of 5 + 7 are the one-shot 12-spp frame
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(0.1, 0.0, 4)
    gpu.render_chunk_accum(W, H, 4)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset()
    for s in (5, 7):
        gpu.render_chunk_accum(W, H, s)
    got = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(got[k], one_shot[k], "plain accumulation after an adaptive featured one " + k)
    gpu.set_gather_planes(3)


@pytest.mark.gpu
def test_plain_render_after_the_run_continues_each_pixels_stream(srt, gpu, orc):
    """a plain launch after an adaptive featured run equals the oracle continued from each pixel's RNG state after its own count"""
    scene, cam, W, H, depth, mode = named_workload(srt, "prism")
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    rel = pick_tolerance(never)
    spp_next = 3
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp_next)
    gpu.accum_reset_adaptive_features(rel, 0.0, MIN_SPP)
    for s in SCHED:
        gpu.render_chunk_accum(W, H, s)
    counts = gpu.accum_stats(W, H)["samples"]
    assert len(np.unique(counts)) >= 3
    gpu.render_chunk(W, H)
    after = read_frame(gpu, W, H)
    osc = oracle_scene_for(orc, scene, mode)
    n = gpu.geom["n_lanes"]
    init = np.zeros(6 * n, np.uint32)
    for idx in range(n):
        s = orc.Rng()
        orc.lib().orc_rng_init(1984 + idx, C.byref(s))
        init[6 * idx: 6 * idx + 6] = [s.d] + list(s.v)
    states = init.copy()
    lane = lane_of(gpu.geom, W, H)
    for c in np.unique(counts):
        st = init.copy()
        osc.render(cam, W, H, int(c), depth, states=st)
        for p in lane[counts == c]:
            states[6 * p: 6 * p + 6] = st[6 * p: 6 * p + 6]
    ref = osc.render(cam, W, H, spp_next, depth, states=states)
    assert_planes_equal(after["xyz"], ref["xyz"], "plain launch after the adaptive featured run, XYZ")
    assert_planes_equal(after["fb"], ref["fb"], "plain launch after the adaptive featured run, fb")


@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    from accum_helpers import run_mock_transport_child
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
from features_reference import stack_features
from helpers import assert_planes_equal, bits
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth, rel = 80, 45, 16, 0.1
cam = scene.default_camera(W, H)
steps = list(srt.render_adaptive_denoised(scene, cam, W, H, depth, rel, min_spp=4, step=4, max_spp=12, variance=None))
total, active, ref, feat, _ = steps[-1]
assert total == 12 and active > 0 and len(np.unique(ref['samples'])) >= 2, (total, active)
def reset(comm):
    comm.accum_reset_adaptive_features(rel, 0.0, 4)
    assert comm.accum_active == 0
for _, comm in comm_accumulations(srt, 2, (9,), scene, cam, W, H, depth, 12, reset, (4, 4, 4)):
    assert comm.accum_active == active
    assert_planes_equal(comm.root.read_fb_aux(2), ref['xyz'], 'xyz')
    rows = sum(stack_features(r.read_features(W, H)) for r in comm.renderers)
    assert np.array_equal(bits(rows), bits(stack_features(feat)))
r = srt.Renderer(0)
c1 = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
c1.upload_scene(scene); c1.set_camera(cam); c1.init_device_params(W, H, 12, depth, 1984)
try:
    c1.accum_reset_adaptive_features(rel)
    raise SystemExit('process-per-GPU adaptive featured reset was accepted')
except srt.SrtError as e:
    assert e.code == -5, e
c1.close(); r.close()
print('adaptive features mock transport ok')
""", "adaptive features mock transport ok", timeout=300)
