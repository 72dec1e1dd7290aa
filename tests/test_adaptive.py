"""Adaptive sampling (srt_accum_reset_adaptive + srt_render_chunk_accum, render_kernel MODE 4).  A pixel that stopped after n samples
holds exactly what a plain n-spp launch gives it (the RNG stream belongs to the pixel), so the adaptive image is a patchwork of exact
one-shot frames; every comparison here is bit for bit, and every stop decision is reproduced by a numpy float32 restatement of the
criterion (accum_helpers.converged_f32).  S1 and S2 themselves, and with them the stop map, are held to the CPU oracle: each sample's Y is
orc_spectrum_to_XYZ of the oracle's path end (tests/path_ends_reference.py), summed and squared sequentially in float32."""
import ctypes as C

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, MIN_SPP, NEVER, SCHED, adaptive_run,
                           assert_pixels_equal, expect_error, forced_shape, fresh_context, gather_ranks, gpu_lib, lane_of, named_workload,
                           pick_tolerance, predict_stops, read_frame, read_sum_y, run_mock_transport_child, shape_case)
from helpers import assert_planes_equal, bits, oracle_scene_for
from path_ends_reference import assert_sums_at_counts, boundary_sums, cached_ends


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "cornell", "random_spheres", "dielectric"])
def test_each_pixel_equals_the_one_shot_frame_of_its_count(srt, gpu, orc, name):
    scene, cam, W, H, depth, mode = named_workload(srt, name)
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    rel = pick_tolerance(never)
    run = adaptive_run(gpu, scene, cam, W, H, depth, rel)
    last = run[-1]
    counts = last["stats"]["samples"]
    assert last["total"] == sum(SCHED) and last["active"] > 0
    assert len(np.unique(counts)) >= 3, np.unique(counts)
    lane = lane_of(gpu.geom, W, H)
    osc = oracle_scene_for(orc, scene, mode) if name in ("prism", "cornell") else None
    for c in np.unique(counts):
        mask = counts == c
        one_shot = srt.render_image(scene, cam, W, H, int(c), depth, renderer=gpu)
        assert_pixels_equal(last["frame"], one_shot, mask, lane, "%s: %d pixels at %d spp" % (name, mask.sum(), c))
        if osc is not None:
            ref = osc.render(cam, W, H, int(c), depth)
            for k in ("fb", "lin", "xyz"):
                for p in range(3):
                    assert np.array_equal(bits(last["frame"][k][p])[lane[mask]], bits(ref[k][p])[lane[mask]]), (name, c, k, p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "dielectric"])
def test_decisions_match_the_float32_restatement(srt, gpu, name):
    """which pixels stop at which boundary, after every pass, with no tolerance; and the sums a pixel holds are those of the run that
    never stops at the same count (S1, S2 exact across runs)"""
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    for rel, ab in ((pick_tolerance(never), 0.0), (0.05, 1e-3), (0.5, 0.0)):
        run = adaptive_run(gpu, scene, cam, W, H, depth, rel, abs_tol=ab)
        maps, _, actives = predict_stops(never, rel, ab)
        for k, (p, want, act) in enumerate(zip(run, maps, actives)):
            got = p["stats"]["samples"]
            assert np.array_equal(got, want), "rel %g abs %g pass %d: %d pixels differ" % (rel, ab, k, int((got != want).sum()))
            assert p["active"] == act, (rel, ab, k, p["active"], act)
        final = run[-1]["stats"]
        for k, p in enumerate(never):
            at = final["samples"] == p["total"]
            for key in ("sum_y", "sum_y2"):
                assert np.array_equal(bits(final[key])[at], bits(p["stats"][key])[at]), (rel, key, k)


@pytest.mark.gpu
def test_s2_is_the_sequential_float32_sum_of_squares(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    N = 12
    fresh_context(gpu, scene, cam, W, H, depth)
    ys = []
    for _ in range(N):           # accum_reset zeroes the sums and does not re-seed: pass k's Y sum is sample k's Y
        gpu.accum_reset()
        gpu.render_chunk_accum(W, H, 1)
        ys.append(read_sum_y(gpu, W, H))
    ys = np.array(ys, np.float32)
    run = adaptive_run(gpu, scene, cam, W, H, depth, NEVER, sched=[2, 4, 6], min_spp=2)
    st = run[-1]["stats"]
    s1 = np.zeros(W * H, np.float32); s2 = np.zeros(W * H, np.float32)
    want1 = np.zeros(W * H, np.float32); want2 = np.zeros(W * H, np.float32)
    for k in range(N):
        s1 = s1 + ys[k]
        s2 = s2 + ys[k] * ys[k]
        at = st["samples"] == k + 1
        want1[at], want2[at] = s1[at], s2[at]
    assert (st["samples"] == N).sum() > W * H // 2
    assert np.array_equal(bits(st["sum_y"]), bits(want1))
    assert np.array_equal(bits(st["sum_y2"]), bits(want2))


def _oracle_sums(srt, orc, name):
    """(scene, cam, W, H, depth) of a named workload and, per pass boundary of SCHED, dict(total, stats = dict(sum_y, sum_y2)) from the
    oracle's path ends alone -- the layout predict_stops and pick_tolerance take"""
    scene, cam, W, H, depth, mode = named_workload(srt, name)
    n = sum(SCHED)
    ends = cached_ends(orc, ("named", name, n), lambda: oracle_scene_for(orc, scene, mode), cam, W, H, n, depth)
    sums = boundary_sums(orc, ends, SCHED)
    return (scene, cam, W, H, depth), sums


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dielectric", "prism"])
def test_sums_equal_the_oracles_at_every_pass_boundary(srt, gpu, orc, name):
    """tolerance NEVER: only a pixel without any variance stops (at min_spp, as the criterion on the oracle's sums says); every other
    one holds the oracle's S1 and S2 of the pass total, after every pass"""
    wl, oracle = _oracle_sums(srt, orc, name)
    maps, _, actives = predict_stops(oracle, NEVER)
    assert actives[-1] >= 100, actives          # (prism is mostly black background: those pixels stop at min_spp)
    run = adaptive_run(gpu, *wl, NEVER)
    for p, o, want, act in zip(run, oracle, maps, actives):
        assert p["total"] == o["total"] and p["active"] == act
        assert np.array_equal(p["stats"]["samples"], want), "pass to %d: %d pixels differ" % (o["total"], int((p["stats"]["samples"] != want).sum()))
        assert_sums_at_counts(p["stats"], oracle, "%s after %d samples" % (name, o["total"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dielectric", "prism"])
def test_stop_map_equals_the_criterion_on_the_oracles_sums(srt, gpu, orc, name):
    """the stop map and the active count after every pass == converged_f32 applied to the oracle's S1 and S2: nothing in the
    prediction is read from the GPU"""
    wl, oracle = _oracle_sums(srt, orc, name)
    for rel, ab in ((pick_tolerance(oracle), 0.0), (0.05, 1e-3)):
        maps, _, actives = predict_stops(oracle, rel, ab)
        run = adaptive_run(gpu, *wl, rel, abs_tol=ab)
        for k, (p, want, act) in enumerate(zip(run, maps, actives)):
            got = p["stats"]["samples"]
            assert np.array_equal(got, want), "rel %g abs %g pass %d: %d pixels differ" % (rel, ab, k, int((got != want).sum()))
            assert p["active"] == act, (rel, ab, k, p["active"], act)
        assert len(np.unique(maps[-1])) >= 2, (rel, ab)
        assert_sums_at_counts(run[-1]["stats"], oracle, "%s rel %g abs %g" % (name, rel, ab))


@pytest.mark.gpu
def test_plain_render_after_adaptive_run_continues_each_pixels_stream(srt, gpu, orc):
    """a plain launch after an adaptive run equals the oracle continued from each pixel's RNG state after its own count"""
    scene, cam, W, H, depth, mode = named_workload(srt, "prism")
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    rel = pick_tolerance(never)
    spp_next = 3
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp_next)
    gpu.accum_reset_adaptive(rel, 0.0, MIN_SPP)
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
    assert_planes_equal(after["xyz"], ref["xyz"], "plain launch after the adaptive run, XYZ")
    assert_planes_equal(after["fb"], ref["fb"], "plain launch after the adaptive run, fb")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_adaptive_shape_gives_the_same_image(srt, gpu, knobs, paired, expect):
    scene, cam, W, H, depth = shape_case(srt, paired)
    gpu.set_test_knobs()
    ref = adaptive_run(gpu, scene, cam, W, H, depth, 0.2)[-1]
    assert len(np.unique(ref["stats"]["samples"])) >= 2
    with forced_shape(gpu, scene, knobs, expect):
        got = adaptive_run(gpu, scene, cam, W, H, depth, 0.2)[-1]
    assert np.array_equal(got["stats"]["samples"], ref["stats"]["samples"])
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(got["frame"][k], ref["frame"][k], "shape %r %s" % (expect, k))
    assert got["active"] == ref["active"]


@pytest.mark.gpu
def test_partitions_and_offset_chunk(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    rel = 0.1
    ref = adaptive_run(gpu, scene, cam, W, H, depth, rel)[-1]
    assert len(np.unique(ref["stats"]["samples"])) >= 2
    for world in (2, 3):
        def one_rank(rank):
            fresh_context(gpu, scene, cam, W, H, depth)
            gpu.set_partition(rank, world)
            gpu.accum_reset_adaptive(rel, 0.0, MIN_SPP)
            for s in SCHED:
                gpu.render_chunk_accum(W, H, s)
            gpu.synchronize()
            return gpu.accum_stats(W, H)["samples"], gpu.accum_active      # (pixels of the other ranks read 0)
        samples, actives = zip(*gather_ranks(gpu, world, one_rank))
        assert np.array_equal(sum(samples), ref["stats"]["samples"]), world
        assert sum(actives) == ref["active"], world
        assert_planes_equal(gpu.read_fb(), ref["frame"]["fb"], "world %d fb" % world)
        assert_planes_equal(gpu.read_fb_aux(1), ref["frame"]["lin"], "world %d lin" % world)
        assert_planes_equal(gpu.read_fb_aux(2), ref["frame"]["xyz"], "world %d xyz" % world)

    # a 30 x 20 chunk at (17, 9) of a 64 x 40 image: each pixel of the chunk equals the one-shot chunk of its count
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 20, 17, 9
    cam = scene.default_camera(IW, IH)

    def chunk(spp=None):
        fresh_context(gpu, scene, cam, cw, ch, depth, spp=spp or 12)
        if spp is None:
            gpu.accum_reset_adaptive(rel, 0.0, MIN_SPP)
            for s in SCHED:
                gpu.render_chunk_accum(cw, ch, s, ox, oy)
        else:
            gpu.render_chunk(cw, ch, ox, oy)
        return dict(read_frame(gpu, IW, IH), samples=gpu.accum_stats(IW, IH)["samples"] if spp is None else None)
    got = chunk()
    counts = got["samples"]
    inside = np.zeros((IH, IW), bool); inside[oy:oy + ch, ox:ox + cw] = True
    inside = inside.ravel()
    assert (counts[~inside] == 0).all() and (counts[inside] > 0).all()
    j, i = np.divmod(np.arange(IW * IH), IW)
    lane = np.zeros(IW * IH, np.int64)
    geom = gpu.geom
    ci, cj = i[inside] - ox, j[inside] - oy
    lane_c = lane_of(geom, cw, ch)
    lane[inside] = lane_c[cj * cw + ci]
    for c in np.unique(counts[inside]):
        mask = inside & (counts == c)
        assert_pixels_equal(got, chunk(int(c)), mask, lane, "offset chunk, %d spp" % c)


@pytest.mark.gpu
def test_comm_two_and_three_ranks_one_gpu_mock_transport():
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth, rel = 150, 90, 16, 0.1
cam = scene.default_camera(W, H)
steps = list(srt.render_adaptive(scene, cam, W, H, depth, rel, min_spp=8, step=4, max_spp=24))
total, active, ref = steps[-1]
assert total == 24 and active > 0 and len(np.unique(ref['samples'])) >= 2, (total, active)
def reset(comm):
    comm.accum_reset_adaptive(rel, 0.0, 8)
    assert comm.accum_active == 0
for world in (2, 3):
    for _, comm in comm_accumulations(srt, world, (9,), scene, cam, W, H, depth, 24, reset, (8, 4, 4, 4, 4)):
        assert comm.accum_active == active, (world, comm.accum_active, active)
        root = comm.root
        assert_planes_equal(root.read_fb(), ref['fb'], 'world %d fb' % world)
        assert_planes_equal(root.read_fb_aux(1), ref['lin'], 'world %d lin' % world)
        assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'world %d xyz' % world)
        samples = sum(r.accum_stats(W, H)['samples'] for r in comm.renderers)
        assert np.array_equal(samples, ref['samples']), world
r = srt.Renderer(0)
c1 = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
c1.upload_scene(scene); c1.set_camera(cam); c1.init_device_params(W, H, 24, depth, 1984)
try:
    c1.accum_reset_adaptive(rel)
    raise SystemExit('process-per-GPU adaptive reset was accepted')
except srt.SrtError as e:
    assert e.code == -5, e
c1.close(); r.close()
print('adaptive mock transport ok')
""", "adaptive mock transport ok", timeout=300)


@pytest.mark.gpu
def test_compaction_counts_and_the_pass_after_convergence(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    run = adaptive_run(gpu, scene, cam, W, H, depth, pick_tolerance(never))
    before = W * H
    for p, s in zip(run, SCHED):
        assert p["paths"] == before * s, (p["total"], p["paths"], before, s)
        before = p["active"]
    # everything stops after the first pass (min_spp samples); a later pass renders nothing and changes nothing but the total
    spp_next = 3
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp_next)
    gpu.accum_reset_adaptive(1e3, 1e3, MIN_SPP)
    gpu.render_chunk_accum(W, H, MIN_SPP)
    first = read_frame(gpu, W, H)
    assert gpu.accum_active == 0 and gpu.stats()["paths"] == W * H * MIN_SPP
    stats_first = gpu.accum_stats(W, H)
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.stats()["paths"] == 0 and gpu.accum_active == 0 and gpu.accum_samples == MIN_SPP + 4
    again = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(again[k], first[k], "pass after convergence " + k)
    stats_again = gpu.accum_stats(W, H)
    for k in ("samples", "sum_y", "sum_y2"):
        assert np.array_equal(stats_again[k].view(np.uint32), stats_first[k].view(np.uint32)), k
    gpu.render_chunk(W, H)           # the RNG states are those after MIN_SPP samples: a plain launch continues from there
    after = read_frame(gpu, W, H)
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp_next)
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, MIN_SPP)
    gpu.render_chunk(W, H)
    want = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(after[k], want[k], "plain launch after the converged adaptive run " + k)


@pytest.mark.gpu
def test_refusals_and_invalidation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
    L = gpu_lib()
    fresh_context(gpu, scene, cam, W, H, depth)
    expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active without an adaptive accumulation")
    gpu.accum_reset_adaptive(0.1, 0.0, 4)
    gpu.render_chunk_accum(W, H, 4)
    first = read_frame(gpu, W, H)
    active = gpu.accum_active
    bad = [(0.0, 0.0, 4, 0), (-0.1, 0.0, 4, 0), (0.1, -1.0, 4, 0), (float("nan"), 0.0, 4, 0), (float("inf"), 0.0, 4, 0),
           (0.1, 0.0, 1, 0), (0.1, 0.0, 0, 0), (0.1, 0.0, 4, 1)]
    for rel, ab, mn, res in bad:        # straight through the C-ABI: the Python check would refuse most of them first
        cfg = srt.binding.Adaptive(rel, ab, mn, res)
        rc = L.srt_accum_reset_adaptive(gpu._h, C.byref(cfg))
        assert rc == ERR_INVALID, (rel, ab, mn, res, rc)
        assert gpu.accum_samples == 4 and gpu.accum_active == active, (rel, ab, mn, res)
    assert L.srt_accum_reset_adaptive(gpu._h, None) == ERR_INVALID
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.accum_reset_adaptive(0.1), ERR_UNSUPPORTED, "instrumented context")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_UNSUPPORTED, "instrumented pass")
    gpu.set_count_traversal(False)
    for k, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, first[k], "after the refusals " + k)
    gpu.render_chunk_accum(W, H, 4)         # the accumulation survived the refusals
    assert gpu.accum_samples == 8
    # srt_set_gather_planes ends an adaptive accumulation (not a plain one: test_progressive)
    gpu.set_gather_planes(9)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, "pass after srt_set_gather_planes")
    expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active after srt_set_gather_planes")
    # the other invalidations of an accumulation hold for an adaptive one too
    for what, call in (("srt_set_camera", lambda: gpu.set_camera(cam)), ("srt_render_chunk", lambda: gpu.render_chunk(W, H))):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_adaptive(0.1, 0.0, 4)
        gpu.render_chunk_accum(W, H, 4)
        call()
        expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, what)
    # a plain accumulation after an adaptive one behaves as before: passes of 5 + 7 are the one-shot 12-spp frame
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive(0.1, 0.0, 4)
    gpu.render_chunk_accum(W, H, 4)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset()
    expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active on a plain accumulation")
    for s in (5, 7):
        gpu.render_chunk_accum(W, H, s)
    assert gpu.stats()["paths"] == W * H * 7
    got = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(got[k], one_shot[k], "plain accumulation after an adaptive one " + k)
    gpu.set_gather_planes(3)


@pytest.mark.gpu
def test_render_adaptive_generator(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    steps = list(srt.render_adaptive(scene, cam, W, H, depth, 0.05, min_spp=8, step=4, max_spp=24, renderer=gpu))
    assert [t for t, _, _ in steps] == [8, 12, 16, 20, 24][:len(steps)]
    for t, active, res in steps:
        assert set(res) == {"fb", "lin", "xyz", "rowmajor", "stats", "kernel_ms", "geom", "samples"}
        assert res["samples"].max() == t and 0 < active <= int((res["samples"] == t).sum())
    # a tolerance every pixel meets at once: one pass, then stop
    steps = list(srt.render_adaptive(scene, cam, W, H, depth, 1e3, abs_tol=1e3, min_spp=8, step=4, max_spp=24, renderer=gpu))
    assert len(steps) == 1 and steps[0][:2] == (8, 0)
