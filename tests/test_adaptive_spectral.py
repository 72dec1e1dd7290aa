"""Adaptive sampling of the spectral film (srt_accum_reset_adaptive_spectral / _features + srt_render_chunk_accum, render_kernel MODE 10
and MODE 11).  Everything the adaptive accumulation keeps -- image, nine planes, sums, S2, sample map, active counts, paths, RNG state --
is bit-identical to a MODE 4 run under the same cfg and schedule; every pixel's film row is the CPU prediction
(tests/path_ends_reference.py) of a plain spectral frame of the pixel's own count; the featured kind's rows are MODE 8's; a converged
pixel's film row is never touched again; nothing depends on launch shape, partition, chunk offset or the split into passes; and the
consumers that normalise (srt_develop_spectral_srgb, srt_denoise_developed) divide every pixel by its own count.  All comparisons are on
bit patterns (same bits, or both NaN)."""
import ctypes as C

import numpy as np
import pytest

import denoise_developed_reference as DD
import denoise_mv_reference as MV
import denoise_reference as D
from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, MIN_SPP, NEVER, SCHED, adaptive_run, assert_same_image,
                           convert_xyz, expect_error, forced_shape, fresh_context, gather_ranks, gpu_lib, lane_of, named_workload, pick_tolerance,
                           predict_stops, read_frame, shape_case, spectral_run)
from develop_reference import CIE_SCALE, develop
from features_reference import predict_features, shape_prediction, stack_features
from helpers import assert_planes_equal, bits, custom_scene
from path_ends_reference import assert_same_floats, bits_equal_or_both_nan, boundary_sums, predict_film, shape_ends, workload_ends

F = np.float32
KINDS = ("unfeatured", "featured")
SMALL_SCHED, SMALL_MIN = [2, 2, 2], 2       # counts 2, 4, 6: the path ends of tests/path_ends_reference.py reach 6 samples


def reset_of(gpu, kind):
    return gpu.accum_reset_adaptive_spectral_features if kind == "featured" else gpu.accum_reset_adaptive_spectral


def adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, rel_tol, sched=SCHED, min_spp=MIN_SPP, abs_tol=0.0, spp=12):
    """accum_helpers.adaptive_run on an adaptive SPECTRAL (FEATURED) accumulation; per pass also film (H, W, 95) and, featured, rows (H, W, 8)"""
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp)
    reset_of(gpu, kind)(rel_tol, abs_tol, min_spp)
    assert gpu.accum_active == 0
    out = []
    for s in sched:
        gpu.render_chunk_accum(W, H, s)
        out.append(dict(total=gpu.accum_samples, active=gpu.accum_active, paths=gpu.stats()["paths"], stats=gpu.accum_stats(W, H),
                        frame=read_frame(gpu, W, H), film=gpu.read_spectral(W, H),
                        rows=stack_features(gpu.read_features(W, H)) if kind == "featured" else None))
    return out


def adaptive_features_run(gpu, scene, cam, W, H, depth, rel_tol, sched=SCHED, min_spp=MIN_SPP):
    """the MODE 8 parent: the rows after every pass"""
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(rel_tol, 0.0, min_spp)
    out = []
    for s in sched:
        gpu.render_chunk_accum(W, H, s)
        out.append(stack_features(gpu.read_features(W, H)))
    return out


def assert_masked(got, want, mask, what):
    """bit-identical (or both NaN) on the pixels of `mask` (H, W); got, want: (H, W, C)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~bits_equal_or_both_nan(got, want).all(axis=-1) & mask)
    assert len(bad) == 0, "%s: %d of %d pixels differ, first (y, x) = %r" % (what, len(bad), int(mask.sum()), tuple(bad[0]))


def assert_same_pass(got, want, what):
    """everything an adaptive accumulation keeps after a pass"""
    assert got["total"] == want["total"] and got["active"] == want["active"] and got["paths"] == want["paths"], (what, got["total"], got["active"], want["active"])
    for k in ("samples", "sum_y", "sum_y2"):
        assert np.array_equal(got["stats"][k].view(np.uint32), want["stats"][k].view(np.uint32)), (what, k)
    assert_same_image(got["frame"], want["frame"], what)


def small_tolerance(never):
    """pick_tolerance for SMALL_SCHED: the tolerance that ends the schedule with the most distinct stop counts while a pixel is still active"""
    best, best_n = None, 0
    for rel in np.geomspace(1e-3, 10.0, 121):
        maps, stop, _ = predict_stops(never, float(rel), 0.0, SMALL_MIN)
        n = len(np.unique(stop[stop > 0]))
        if (stop == 0).any() and n > best_n:
            best, best_n = float(rel), n
    assert best is not None
    return best


_films = {}


def film_at(key, ends, c):
    """predict_film(ends, 0, c), once per (key, c)"""
    if (key, c) not in _films:
        _films[(key, c)] = predict_film(ends, 0, int(c))
    return _films[(key, c)]


def xyz_sums_rowmajor(gpu, frame, W, H):
    lane = lane_of(gpu.geom, W, H)
    return np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)


def curves(k, seed=11):
    return np.random.default_rng(seed).uniform(-0.25, 1.0, (k, 95)).astype(F)


# ---- 1: everything adaptive is MODE 4's ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["prism", "cornell", "random_spheres", "dielectric"])
def test_everything_adaptive_equals_mode_4(srt, gpu, name, kind):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER)
    rel = pick_tolerance(never)
    want = adaptive_run(gpu, scene, cam, W, H, depth, rel)
    gpu.render_chunk(W, H)                # a plain launch continues every pixel's RNG stream from where its own count left it
    want_after = read_frame(gpu, W, H)
    assert len(np.unique(want[-1]["stats"]["samples"])) >= 3 and want[-1]["active"] > 0
    got = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, rel)
    gpu.render_chunk(W, H)
    got_after = read_frame(gpu, W, H)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_pass(g, w, "%s %s pass %d" % (name, kind, k))
    assert_same_image(got_after, want_after, name + " RNG state: a plain launch after the run")
    assert bits(got[-1]["film"]).any()


# ---- 2: the film at the pixel's own count, from the oracle alone ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["dielectric", "random_spheres"])
def test_every_film_row_is_the_prediction_at_the_pixels_own_count(srt, gpu, orc, name, kind):
    (scene, cam, W, H, n, depth, _), ends = workload_ends(srt, orc, name)
    assert n == sum(SMALL_SCHED)
    never = boundary_sums(orc, ends, SMALL_SCHED)          # S1 and S2 at every boundary, from the path ends: no GPU run chooses the tolerance
    rel = small_tolerance(never)
    maps, stop, actives = predict_stops(never, rel, 0.0, SMALL_MIN)
    stopped = np.unique(stop[stop > 0])
    print("%s rel %g: stopped at %r, %d active" % (name, rel, {int(c): int((stop == c).sum()) for c in stopped}, int((stop == 0).sum())))
    assert len(stopped) >= 2 and (stop == 0).any()
    run = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, rel, sched=SMALL_SCHED, min_spp=SMALL_MIN)
    for p, want, act in zip(run, maps, actives):
        assert np.array_equal(p["stats"]["samples"], want) and p["active"] == act
    for p in run:           # after every pass: a pixel's row is that of its count then (an active pixel: the running total)
        counts = p["stats"]["samples"].reshape(H, W)
        checked = np.zeros((H, W), bool)
        for c in np.unique(counts):
            assert_masked(p["film"], film_at(name, ends, c), counts == c, "%s after %d: %d pixels at %d spp" % (name, p["total"], (counts == c).sum(), c))
            checked |= counts == c
        assert checked.all()
    assert len(np.unique(run[-1]["stats"]["samples"])) >= 3


# ---- 3: the featured kind against its parents ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_spheres", "dielectric"])
def test_the_featured_kind_against_its_parents(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    rel = 0.1
    plain = adaptive_spectral_run(gpu, "unfeatured", scene, cam, W, H, depth, rel)
    assert len(np.unique(plain[-1]["stats"]["samples"])) >= 2 and plain[-1]["active"] > 0
    both = adaptive_spectral_run(gpu, "featured", scene, cam, W, H, depth, rel)
    rows8 = adaptive_features_run(gpu, scene, cam, W, H, depth, rel)
    for k, (b, p, r8) in enumerate(zip(both, plain, rows8)):
        assert_same_pass(b, p, "%s pass %d, featured against unfeatured" % (name, k))
        assert_same_floats(b["film"], p["film"], "%s pass %d film" % (name, k))
        assert_same_floats(b["rows"], r8, "%s pass %d rows against MODE 8" % (name, k))
    assert (both[-1]["rows"][..., 7] > 0).any()


# ---- 4: every launch shape ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_shape(srt, gpu, orc, knobs, paired, expect, kind):
    scene, cam, W, H, depth = shape_case(srt, paired)
    gpu.set_test_knobs()
    sched, mn, rel = [2, 2], 2, 0.2
    want = adaptive_run(gpu, scene, cam, W, H, depth, rel, sched=sched, min_spp=mn)
    counts = want[-1]["stats"]["samples"].reshape(H, W)
    assert set(np.unique(counts)) == {2, 4} and want[-1]["active"] > 0
    with forced_shape(gpu, scene, knobs, expect):
        got = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, rel, sched=sched, min_spp=mn)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_pass(g, w, "shape %r pass %d" % (expect, k))
    _, ends = shape_ends(srt, orc, paired, 4)
    for c in (2, 4):
        assert_masked(got[-1]["film"], film_at(("shape", paired), ends, c), counts == c, "shape %r film at %d spp" % (expect, c))
        if kind == "featured":       # (MODE 11 finds its rows behind the film: the address is formed in every shape)
            assert_masked(got[-1]["rows"], shape_prediction(srt, orc, paired, c)[1]["rows"], counts == c, "shape %r rows at %d spp" % (expect, c))


# ---- 5: partitions, an offset chunk, the split into passes ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_partitions_offset_chunk_and_split_into_passes(srt, gpu, kind):
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    rel = 0.1
    ref = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, rel)[-1]
    assert len(np.unique(ref["stats"]["samples"])) >= 2 and ref["active"] > 0
    for world in (2, 3):
        def one_rank(rank):
            fresh_context(gpu, scene, cam, W, H, depth)
            gpu.set_partition(rank, world)
            reset_of(gpu, kind)(rel, 0.0, MIN_SPP)
            for s in SCHED:
                gpu.render_chunk_accum(W, H, s)
            gpu.synchronize()
            return gpu.accum_stats(W, H)["samples"], gpu.accum_active, gpu.read_spectral(W, H)      # (pixels of the other ranks read 0)
        samples, actives, films = zip(*gather_ranks(gpu, world, one_rank))
        assert np.array_equal(sum(samples), ref["stats"]["samples"]), world
        assert sum(actives) == ref["active"], world
        assert_planes_equal(gpu.read_fb(), ref["frame"]["fb"], "world %d fb" % world)
        assert_planes_equal(gpu.read_fb_aux(2), ref["frame"]["xyz"], "world %d xyz" % world)
        nonzero = np.stack([(bits(f) != 0).any(axis=-1) for f in films])
        assert (nonzero.sum(axis=0) <= 1).all() and all(nz.any() for nz in nonzero)      # each pixel is non-zero on one rank only: the sum is exact
        total = films[0]
        for f in films[1:]:
            total = total + f
        assert_same_floats(total, ref["film"], "films summed over %d ranks" % world)

    # a 30 x 21 chunk at (17, 9) of a 64 x 40 image: MODE 4's frame and map, zeros outside, and at each count the film of a plain spectral chunk
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam2 = scene.default_camera(IW, IH)
    sched, mn = [2, 2, 2], 2

    def chunk(which, passes):
        fresh_context(gpu, scene, cam2, cw, ch, depth)
        {"new": lambda: reset_of(gpu, kind)(rel, 0.0, mn), "adaptive": lambda: gpu.accum_reset_adaptive(rel, 0.0, mn), "spectral": gpu.accum_reset_spectral}[which]()
        for s in passes:
            gpu.render_chunk_accum(cw, ch, s, ox, oy)
        return (read_frame(gpu, IW, IH), gpu.accum_stats(IW, IH)["samples"].reshape(IH, IW) if which != "spectral" else None,
                gpu.read_spectral(IW, IH) if which != "adaptive" else None)
    frame, counts, film = chunk("new", sched)
    frame4, counts4, _ = chunk("adaptive", sched)
    assert_same_image(frame, frame4, "offset chunk against MODE 4")
    assert np.array_equal(counts, counts4)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert not bits(film[~inside]).any() and (counts[~inside] == 0).all() and (counts[inside] >= mn).all()
    assert len(np.unique(counts[inside])) >= 2
    for c in np.unique(counts[inside]):
        assert_masked(film, chunk("spectral", [int(c)])[2], inside & (counts == c), "offset chunk at %d spp" % c)

    # at NEVER with min_spp = the total no pixel stops before the end: one pass, two and six give the same bits
    one = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, NEVER, sched=[6], min_spp=6)[-1]
    assert (one["stats"]["samples"] == 6).all()
    assert_same_floats(one["film"], spectral_run(gpu, scene, cam, W, H, depth, [6])[1], "one pass of 6 against a plain spectral frame")
    for passes in ([2, 4], [1] * 6):
        got = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, NEVER, sched=passes, min_spp=6)[-1]
        assert_same_floats(got["film"], one["film"], "passes %r" % (passes,))
        assert_same_image(got["frame"], one["frame"], "passes %r" % (passes,))
        if kind == "featured":
            assert_same_floats(got["rows"], one["rows"], "rows, passes %r" % (passes,))
        for k in ("samples", "sum_y", "sum_y2"):
            assert np.array_equal(got["stats"][k].view(np.uint32), one["stats"][k].view(np.uint32)), (passes, k)


# ---- 6: a converged pixel's film is frozen ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_a_converged_pixels_film_row_is_frozen(srt, gpu, kind):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    run = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, 0.25, sched=[4, 4], min_spp=4)
    counts = run[-1]["stats"]["samples"].reshape(H, W)
    done = counts < 8                       # stopped at 4
    lit_done = done & (bits(run[-1]["film"]) != 0).any(axis=-1)
    assert lit_done.any() and run[-1]["active"] > 0
    before = run[-1]["film"]
    for _ in range(2):
        gpu.render_chunk_accum(W, H, 4)
    after = gpu.read_spectral(W, H)
    later = gpu.accum_stats(W, H)["samples"].reshape(H, W)
    assert np.array_equal(later[done], counts[done])
    assert_masked(after, before, done, "film rows of the pixels that had stopped")
    grew = later > counts
    changed = (bits(after) != bits(before)).any(axis=-1)
    assert grew.any() and (changed & grew).any() and not (changed & ~grew).any()
    stopped_since = (later == counts) & ~done          # converged exactly at 8: frozen as well
    assert_masked(after, before, stopped_since, "film rows of the pixels that stopped at the last boundary")
    if kind == "featured":
        assert_masked(stack_features(gpu.read_features(W, H)), run[-1]["rows"], done | stopped_since, "feature rows of the stopped pixels")


# ---- 7: a leaf-root tree and bounce_limit = 0 --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_leaf_root_and_bounce_limit_zero(srt, gpu, orc, kind):
    """a leaf-root tree (no traversal step at all) deposits what a plain spectral frame deposits (and, featured, what the prediction says);
    bounce_limit 0 makes no query and converts no path: film and rows stay +0"""
    scene = custom_scene(srt, [((-3, -2, 0), (3, -2, 0), (0, 3, 0), 0, 0)], [(0, (0.25, 0.25, 0.25), 0.0, 0.0)]).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H = 45, 37
    cam = srt.camera_init(W, H, 60.0, (0.3, 0.2, 9.0), (0.0, 0.0, 0.0))
    run = adaptive_spectral_run(gpu, kind, scene, cam, W, H, 6, 0.05, sched=[2, 2], min_spp=2)
    counts = run[-1]["stats"]["samples"].reshape(H, W)
    assert set(np.unique(counts)) == {2, 4}
    film, rows = run[-1]["film"], run[-1]["rows"]
    for c in (2, 4):
        assert_masked(film, spectral_run(gpu, scene, cam, W, H, 6, [c])[1], counts == c, "one triangle, film at %d spp" % c)
        if kind == "featured":
            assert_masked(rows, predict_features(orc, scene, cam, W, H, c, 6, 0)["rows"], counts == c, "one triangle, rows at %d spp" % c)
    assert bits(film).any()
    for sc, cm, w, h in ((scene, cam, W, H),) + (named_workload(srt, "prism")[:4],):
        got = adaptive_spectral_run(gpu, kind, sc, cm, w, h, 0, 0.05, sched=[2, 2], min_spp=2)[-1]
        assert not bits(got["film"]).any(), "bounce_limit 0 deposited something into the film"
        assert kind != "featured" or not bits(got["rows"]).any(), "bounce_limit 0 deposited something into the rows"
        assert gpu.accum_samples == 4


# ---- 8: develop --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_develop_and_the_srgb_variant_at_each_pixels_own_count(srt, gpu, orc, kind):
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    run = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, 0.1)[-1]
    counts = run["stats"]["samples"].reshape(H, W)
    assert len(np.unique(counts)) >= 2 and (counts >= MIN_SPP).all()          # (a scalar normalisation would fail below)
    resp = curves(3)
    got = gpu.develop_spectral(W, H, resp, 0.5)
    assert_same_floats(got, gpu.develop_kat(run["film"].reshape(-1, 95), resp, 0.5).reshape(H, W, 3), "develop_spectral against develop_kat of the film")
    assert_same_floats(got, develop(run["film"], resp, 0.5), "develop_spectral against the restatement (still sums)")
    res = gpu.develop_spectral_srgb(W, H)
    assert_same_floats(res["xyz"], develop(run["film"], srt.renderer.cie_response(), CIE_SCALE), "sRGB variant, developed sums")
    sums = res["xyz"].reshape(-1, 3)
    flat = counts.reshape(-1)
    lin, q = np.zeros_like(sums), np.zeros_like(sums)
    for c in np.unique(flat):          # inv = 1 / (float32)n_p, then the conversion restatement the scalar variant is held to
        at = flat == c
        l3, q3 = convert_xyz(orc, [sums[at, k] for k in range(3)], int(c))
        lin[at], q[at] = np.stack(l3, axis=1), np.stack(q3, axis=1)
    assert_same_floats(res["lin"].reshape(-1, 3), lin, "sRGB variant, unquantised, each pixel by its own count")
    assert_same_floats(res["fb"].reshape(-1, 3), q, "sRGB variant, quantised, each pixel by its own count")
    # ... which the scalar total would not give
    l_tot, _ = convert_xyz(orc, [sums[:, k] for k in range(3)], run["total"])
    assert (bits(np.stack(l_tot, axis=1)) != bits(lin)).any()
    ms = gpu.develop_last_ms()
    assert ms["contract"] > 0 and ms["epilogue"] > 0
    assert_same_image(read_frame(gpu, W, H), run["frame"], "frame after the calls")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_srgb_variant_on_a_rank_of_two_leaves_the_other_ranks_pixels_zero(srt, gpu, orc, kind):
    """a pixel owned by another rank holds no sample (count 0) and a +0 film row: it is normalised by 1, never by 1 / 0, so its XYZ sums
    are +0 and its sRGB is the conversion of +0 -- no NaN; the rank's own pixels are normalised by their own counts"""
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    fresh_context(gpu, scene, cam, W, H, depth)
    try:
        gpu.set_partition(1, 2)
        reset_of(gpu, kind)(0.1, 0.0, MIN_SPP)
        for s in SCHED:
            gpu.render_chunk_accum(W, H, s)
        flat = gpu.accum_stats(W, H)["samples"]
        res = gpu.develop_spectral_srgb(W, H)
    finally:
        gpu.set_partition(0, 1)
    other = flat == 0
    assert other.any() and (~other).any() and len(np.unique(flat[~other])) >= 2
    sums = res["xyz"].reshape(-1, 3)
    assert not bits(sums[other]).any(), "a pixel of the other rank has a developed sum"
    lin0, q0 = convert_xyz(orc, [np.zeros(1, F)] * 3, 1)
    lin, q = np.zeros_like(sums), np.zeros_like(sums)
    lin[other], q[other] = np.stack(lin0, axis=1), np.stack(q0, axis=1)
    for c in np.unique(flat[~other]):
        at = flat == c
        l3, q3 = convert_xyz(orc, [sums[at, k] for k in range(3)], int(c))
        lin[at], q[at] = np.stack(l3, axis=1), np.stack(q3, axis=1)
    assert np.isfinite(res["lin"]).all() and np.isfinite(res["fb"]).all()
    assert np.array_equal(bits(res["lin"].reshape(-1, 3)), bits(lin)) and np.array_equal(bits(res["fb"].reshape(-1, 3)), bits(q))


# ---- 9: the developed denoise ------------------------------------------------------------------------------------------------------------------
def restated_counts(S, rows, P, n, levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1):
    """denoise_developed_reference.denoise_developed with both prepasses on the pixel's own count: inv_p = 1 / (float32)n_p; d_p = inv_p * D_p"""
    c, N, A, z = MV.prepass_counts(S, rows, n)
    with np.errstate(all="ignore"):
        inv = (F(1) / np.asarray(n).astype(F)).astype(F)[..., None]
        d = (inv * np.asarray(P, F)).astype(F)
    for i in range(levels):
        c, d = DD.filter_level(c, d, N, A, z, i, D.level_constants(i, sigma_color, sigma_normal, sigma_albedo, sigma_depth))
    return d, c


_sigmas = {}


def sigmas():
    """the sigmas of every size are those picked on the 67 x 35 input (tests/test_denoise.py does the same)"""
    if not _sigmas:
        _sigmas.update(D.pick_sigmas(*D.synthetic_case(35, 67))[0])
    return _sigmas


def check_counts_kat(gpu, h, w, k, levels=5):
    S, rows, n, _ = MV.varying_case(h, w)
    P = DD.random_payload(h, w, k)
    assert len(np.unique(n)) >= min(3, n.size), np.unique(n)
    want_dev, want_xyz = restated_counts(S, rows, P, n, levels=levels, **{a: b for a, b in sigmas().items() if a != "levels"})
    dev, xyz = gpu.denoise_developed_counts_kat(S, rows, P, n, levels=levels, **{a: b for a, b in sigmas().items() if a != "levels"})
    assert dev.dtype == F and dev.shape == (h, w, k)
    assert_same_floats(xyz, want_xyz, "%d x %d, K = %d XYZ" % (w, h, k))
    assert_same_floats(dev, want_dev, "%d x %d, K = %d payload" % (w, h, k))
    return S, rows, P, n, dev


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 5, 16])
def test_counts_kat_equals_the_restatement(gpu, k):
    S, rows, P, n, dev = check_counts_kat(gpu, 35, 67, k)
    # a scalar normalisation is another result
    scalar, _ = gpu.denoise_developed_kat(S, rows, P, int(n.max()), levels=5, **{a: b for a, b in sigmas().items() if a != "levels"})
    assert (bits(scalar) != bits(dev)).any()
    for w, h in ((1, 1), (1, 9), (9, 1), (3, 2)):
        check_counts_kat(gpu, h, w, k)
    check_counts_kat(gpu, 35, 67, k, levels=0)


@pytest.mark.gpu
def test_counts_kat_with_a_constant_map_is_the_scalar_kat(srt, gpu):
    S, rows, n0 = D.synthetic_case(35, 67)
    P = DD.random_payload(35, 67, 5)
    cfg = {a: b for a, b in sigmas().items() if a != "levels"}
    want_dev, want_xyz = gpu.denoise_developed_kat(S, rows, P, n0, levels=5, **cfg)
    dev, xyz = gpu.denoise_developed_counts_kat(S, rows, P, np.full((35, 67), n0, np.uint32), levels=5, **cfg)
    assert_same_floats(dev, want_dev, "constant map, payload")
    assert_same_floats(xyz, want_xyz, "constant map, XYZ")
    # the C entry point's own checks: those of srt_denoise_developed_kat, and srt_denoise_mv_kat's for the map
    L, fp = gpu_lib(), srt.binding.fptr
    good = srt.denoise_config()
    S, r8, _ = D.synthetic_case(3, 5)
    P = DD.random_payload(3, 5, 2)
    n = np.full((3, 5), 3, np.uint32)
    o_dev, o_xyz = np.zeros((3, 5, 2), F), np.zeros((3, 5, 3), F)

    def kat(cfg=good, s=S, r=r8, p=P, k=2, m=n, w=5, h=3, a=o_dev, b=o_xyz):
        f = lambda v: fp(v) if v is not None else None
        return L.srt_denoise_developed_counts_kat(gpu._h, C.byref(cfg), f(s), f(r), f(p), k, m.ctypes.data_as(C.POINTER(C.c_uint32)) if m is not None else None,
                                                  w, h, f(a), f(b))
    bad_levels = srt.denoise_config(); bad_levels.levels = 9
    zero = n.copy(); zero[2, 4] = 0
    flagged = n | np.uint32(0x80000000)          # bit 31 is a state word's converged flag: ignored
    assert kat() == 0 and kat(a=None) == 0 and kat(b=None) == 0 and kat(m=flagged) == 0
    assert kat(bad_levels) == ERR_INVALID and kat(s=None) == ERR_INVALID and kat(r=None) == ERR_INVALID and kat(p=None) == ERR_INVALID
    assert kat(m=None) == ERR_INVALID and kat(m=zero) == ERR_INVALID and kat(a=None, b=None) == ERR_INVALID
    assert kat(w=0) == ERR_INVALID and kat(h=0) == ERR_INVALID and kat(k=0) == ERR_INVALID and kat(k=17) == ERR_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random_spheres", "cornell"])
def test_denoise_developed_on_a_real_run_divides_each_pixel_by_its_own_count(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    run = adaptive_spectral_run(gpu, "featured", scene, cam, W, H, depth, 0.1)[-1]
    counts = run["stats"]["samples"].reshape(H, W)
    assert len(np.unique(counts)) >= 2
    S = xyz_sums_rowmajor(gpu, run["frame"], W, H)
    resp, scale = curves(5), 0.5
    planes = gpu.develop_spectral(W, H, resp, scale)
    want_dev, want_xyz = restated_counts(S, run["rows"], planes, counts, **D.DEFAULTS)
    got = gpu.denoise_developed(W, H, resp, scale)
    assert got["dev"].shape == (H, W, 5) and got["xyz"].shape == (H, W, 3)
    assert_same_floats(got["dev"], want_dev, name + " developed, denoised")
    assert_same_floats(got["xyz"], want_xyz, name + " XYZ")
    assert_same_floats(got["xyz"], gpu.denoise(W, H)["xyz"], name + " XYZ against denoise()")
    zero = gpu.denoise_developed(W, H, resp, scale, levels=0)["dev"]
    with np.errstate(all="ignore"):
        assert_same_floats(zero, ((F(1) / counts.astype(F)).astype(F)[..., None] * planes).astype(F), name + " levels = 0: inv_p * develop_spectral")
        assert (bits(zero) != bits(((F(1) / F(run["total"])) * planes).astype(F))).any()
    # the other denoisers take the featured kind as they take MODE 8's, and nothing changed the accumulation
    assert_same_floats(gpu.denoise(W, H)["xyz"], MV.denoise_counts(S, run["rows"], counts, **D.DEFAULTS), name + " denoise()")
    assert set(gpu.denoise_mv(W, H)) >= {"xyz", "var"} and set(gpu.denoise_vg(W, H)) >= {"xyz", "var"}
    assert_same_image(read_frame(gpu, W, H), run["frame"], name + " frame after the calls")
    assert_same_floats(gpu.read_spectral(W, H), run["film"], name + " film after the calls")


@pytest.mark.gpu
def test_render_adaptive_spectral_yields_what_the_manual_calls_give(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    kw = dict(min_spp=4, step=4, max_spp=12)
    plain = list(srt.render_adaptive(scene, cam, W, H, depth, 0.25, renderer=gpu, **kw))
    steps = list(srt.render_adaptive_spectral(scene, cam, W, H, depth, 0.25, renderer=gpu, **kw))
    full = list(srt.render_adaptive_spectral(scene, cam, W, H, depth, 0.25, renderer=gpu, features=True, levels=2, **kw))
    assert [s[0] for s in steps] == [s[0] for s in plain] == [s[0] for s in full] and len(steps[0]) == 4 and len(full[0]) == 6
    manual = adaptive_spectral_run(gpu, "featured", scene, cam, W, H, depth, 0.25, sched=[s[0] - (steps[k - 1][0] if k else 0) for k, s in enumerate(steps)], min_spp=4)
    for (t, act, res, rad), (t4, act4, res4), f, m in zip(steps, plain, full, manual):
        assert (t, act) == (t4, act4) == (f[0], f[1])
        assert_same_image(res, res4, "render_adaptive_spectral vs render_adaptive at %d" % t)
        assert np.array_equal(res["samples"], res4["samples"]) and np.array_equal(f[2]["samples"], res4["samples"])
        want = srt.spectral_radiance(m["film"], res["samples"].reshape(H, W))
        assert rad.shape == (H, W, 95) and np.array_equal(rad, want, equal_nan=True) and np.array_equal(f[3], want, equal_nan=True)
    assert len(np.unique(steps[-1][2]["samples"])) >= 2
    # the featured generator's last two items on the last pass: what the manual calls give on the same accumulation (still on the context)
    cie = srt.renderer.cie_response()
    assert_same_floats(full[-1][4], gpu.develop_spectral(W, H, cie, float(CIE_SCALE)), "generator's developed planes")
    den = gpu.denoise_developed(W, H, cie, float(CIE_SCALE), levels=2)
    for k in ("dev", "xyz"):
        assert_same_floats(full[-1][5][k], den[k], "generator's denoised " + k)


# ---- 10: refusals and neighbours ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_invalidation(srt, gpu, kind):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    fn = L.srt_accum_reset_adaptive_spectral_features if kind == "featured" else L.srt_accum_reset_adaptive_spectral
    reset = reset_of(gpu, kind)
    fresh_context(gpu, scene, cam, W, H, depth)
    reset(0.1, 0.0, 4)
    assert gpu.accum_active == 0
    expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read_spectral before the first pass")
    expect_error(srt, lambda: gpu.accum_stats(W, H), ERR_INVALID, "accum_stats before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first, film, active = read_frame(gpu, W, H), gpu.read_spectral(W, H), gpu.accum_active
    bad = [(0.0, 0.0, 4, 0), (-0.1, 0.0, 4, 0), (0.1, -1.0, 4, 0), (float("nan"), 0.0, 4, 0), (float("inf"), 0.0, 4, 0),
           (0.1, 0.0, 1, 0), (0.1, 0.0, 0, 0), (0.1, 0.0, 4, 1)]
    for rel, ab, mn, res in bad:        # straight through the C-ABI: the Python check would refuse most of them first
        cfg = srt.binding.Adaptive(rel, ab, mn, res)
        assert fn(gpu._h, C.byref(cfg)) == ERR_INVALID, (rel, ab, mn, res)
        assert gpu.accum_samples == 4 and gpu.accum_active == active, (rel, ab, mn, res)
    assert fn(gpu._h, None) == ERR_INVALID
    assert fn(None, C.byref(srt.binding.Adaptive(0.1, 0.0, 4, 0))) == ERR_INVALID
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: reset(0.1), ERR_UNSUPPORTED, "instrumented context")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_UNSUPPORTED, "instrumented pass")
    gpu.set_count_traversal(False)
    for k, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, first[k], "after the refusals " + k)
    assert_same_floats(gpu.read_spectral(W, H), film, "film after the refusals")
    gpu.render_chunk_accum(W, H, 4)         # the accumulation survived the refusals
    assert gpu.accum_samples == 8
    cont, cont_film = read_frame(gpu, W, H), gpu.read_spectral(W, H)
    again = adaptive_spectral_run(gpu, kind, scene, cam, W, H, depth, 0.1, sched=[4, 4], min_spp=4)[-1]
    assert_same_image(cont, again["frame"], "continued after the refusals")
    assert_same_floats(cont_film, again["film"], "film continued after the refusals")
    # a context without device parameters: refused
    r = srt.Renderer(0)
    try:
        expect_error(srt, lambda: reset_of(r, kind)(0.1), ERR_INVALID, "no device parameters")
    finally:
        r.close()
    # srt_set_gather_planes ends it, as it ends an adaptive accumulation; so do the other invalidations
    gpu.set_gather_planes(9)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, "pass after srt_set_gather_planes")
    expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active after srt_set_gather_planes")
    expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read_spectral after srt_set_gather_planes")
    for what, call in (("srt_set_camera", lambda: gpu.set_camera(cam)), ("srt_render_chunk", lambda: gpu.render_chunk(W, H)),
                       ("srt_upload_scene", lambda: gpu.upload_scene(scene)), ("srt_set_partition", lambda: gpu.set_partition(0, 1))):
        fresh_context(gpu, scene, cam, W, H, depth)
        reset(0.1, 0.0, 4)
        gpu.render_chunk_accum(W, H, 4)
        call()
        expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, what)
    # one accumulation per context and chunk, and the 65535-sample limit
    fresh_context(gpu, scene, cam, W, H, depth)
    reset(0.1, 0.0, 4)
    gpu.render_chunk_accum(W, H, 4)
    expect_error(srt, lambda: gpu.render_chunk_accum(W - 8, H, 4), ERR_INVALID, "another chunk")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 65535), ERR_INVALID, "more than 65535 samples")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 0), ERR_INVALID, "no samples")
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == 8


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_neighbouring_kinds(srt, gpu, kind):
    """what the new kinds' neighbours still refuse, what the unfeatured kind refuses, and every other reset makes the next accumulation
    that kind again"""
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
    resp = curves(2)
    resets = {"plain": gpu.accum_reset, "adaptive": lambda: gpu.accum_reset_adaptive(0.1, 0.0, 4), "features": gpu.accum_reset_features,
              "spectral": gpu.accum_reset_spectral, "streams": lambda: gpu.accum_reset_streams(2),
              "adaptive features": lambda: gpu.accum_reset_adaptive_features(0.1, 0.0, 4), "spectral features": gpu.accum_reset_spectral_features,
              "the other new kind": lambda: reset_of(gpu, KINDS[1 - KINDS.index(kind)])(0.1, 0.0, 4)}
    for other, reset in resets.items():
        fresh_context(gpu, scene, cam, W, H, depth)
        reset_of(gpu, kind)(0.1, 0.0, 4)
        gpu.render_chunk_accum(W, H, 4)
        assert gpu.accum_active >= 0 and bits(gpu.read_spectral(W, H)).any() and gpu.accum_stats(W, H)["samples"].max() == 4
        if kind == "featured":
            assert gpu.read_features(W, H)["hits"].max() > 0
            assert set(gpu.denoise_developed(W, H, resp)) == {"dev", "xyz"} and "var" in gpu.denoise_mv(W, H)
        else:
            expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features on the unfeatured kind")
            expect_error(srt, lambda: gpu.denoise(W, H), ERR_INVALID, "denoise on the unfeatured kind")
            expect_error(srt, lambda: gpu.denoise_mv(W, H), ERR_INVALID, "denoise_mv on the unfeatured kind")
            expect_error(srt, lambda: gpu.denoise_developed(W, H, resp), ERR_INVALID, "denoise_developed on the unfeatured kind")
        reset()
        gpu.render_chunk_accum(W, H, 4)
        adaptive = "adaptive" in other or other == "the other new kind"
        spectral = "spectral" in other or other == "the other new kind"
        featured = "features" in other or (other == "the other new kind" and kind == "unfeatured")
        if adaptive:
            assert gpu.accum_stats(W, H)["samples"].max() == 4 and gpu.accum_active >= 0
        else:
            expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active on a %s accumulation" % other)
            expect_error(srt, lambda: gpu.accum_stats(W, H), ERR_INVALID, "the sample map of a %s accumulation" % other)
        if spectral:
            assert bits(gpu.read_spectral(W, H)).any()
        else:
            expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read_spectral on a %s accumulation" % other)
            expect_error(srt, lambda: gpu.develop_spectral_srgb(W, H), ERR_INVALID, "develop on a %s accumulation" % other)
        if featured:
            assert gpu.read_features(W, H)["hits"].max() == 4
        else:
            expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features on a %s accumulation" % other)
        if not (spectral and featured):
            expect_error(srt, lambda: gpu.denoise_developed(W, H, resp), ERR_INVALID, "denoise_developed on a %s accumulation" % other)
        if not (adaptive and featured):
            expect_error(srt, lambda: gpu.denoise_mv(W, H), ERR_INVALID, "denoise_mv on a %s accumulation" % other)
    # a plain accumulation after the new kind behaves as before: passes of 5 + 7 are the one-shot 12-spp frame
    fresh_context(gpu, scene, cam, W, H, depth)
    reset_of(gpu, kind)(0.1, 0.0, 4)
    gpu.render_chunk_accum(W, H, 4)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset()
    for s in (5, 7):
        gpu.render_chunk_accum(W, H, s)
    got = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(got[k], one_shot[k], "plain accumulation after an adaptive spectral one " + k)
    # a spectral featured accumulation after the featured new kind has its rows where it always had them
    if kind == "featured":
        def sf_rows():
            fresh_context(gpu, scene, cam, W, H, depth)
            gpu.accum_reset_spectral_features()
            gpu.render_chunk_accum(W, H, 4)
            return stack_features(gpu.read_features(W, H)), gpu.read_spectral(W, H)
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, 4)
        want = stack_features(gpu.read_features(W, H))
        rows, film = sf_rows()
        assert_same_floats(rows, want, "rows of a spectral featured accumulation after the new kind")
        assert_same_floats(film, spectral_run(gpu, scene, cam, W, H, depth, [4])[1], "film of a spectral featured accumulation after the new kind")
    gpu.set_gather_planes(3)


# ---- 11: two ranks on one GPU over the mock transport ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    from accum_helpers import run_mock_transport_child
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth, rel = 80, 45, 16, 0.1
cam = scene.default_camera(W, H)
for features in (False, True):
    steps = list(srt.render_adaptive_spectral(scene, cam, W, H, depth, rel, min_spp=4, step=4, max_spp=12, features=features))
    total, active, ref, radiance = steps[-1][:4]
    assert total == 12 and active > 0 and len(np.unique(ref['samples'])) >= 2, (total, active)
    def reset(comm):
        (comm.accum_reset_adaptive_spectral_features if features else comm.accum_reset_adaptive_spectral)(rel, 0.0, 4)
        assert comm.accum_active == 0
    for _, comm in comm_accumulations(srt, 2, (9,), scene, cam, W, H, depth, 12, reset, (4, 4, 4)):
        assert comm.accum_active == active
        assert_planes_equal(comm.root.read_fb_aux(2), ref['xyz'], 'xyz')
        films = [r.read_spectral(W, H) for r in comm.renderers]
        owned = [(f.view(np.uint32) != 0).any(axis=-1) for f in films]
        assert not (owned[0] & owned[1]).any() and owned[0].any() and owned[1].any()
        got = srt.spectral_radiance(films[0] + films[1], ref['samples'].reshape(H, W))
        assert np.array_equal(got, radiance, equal_nan=True)
r = srt.Renderer(0)
c1 = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
c1.upload_scene(scene); c1.set_camera(cam); c1.init_device_params(W, H, 12, depth, 1984)
for reset in (c1.accum_reset_adaptive_spectral, c1.accum_reset_adaptive_spectral_features):
    try:
        reset(rel)
        raise SystemExit('process-per-GPU adaptive spectral reset was accepted')
    except srt.SrtError as e:
        assert e.code == -5, e
c1.close(); r.close()
print('adaptive spectral mock transport ok')
""", "adaptive spectral mock transport ok", timeout=300)
