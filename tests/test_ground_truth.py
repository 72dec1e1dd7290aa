"""The device against tests/ground_truth.py: ray hits (srt_trace_rays, both tree builders), radiometry (render_image, both kernel
builds and both tree builders), the spectral film (MODE 5) and the first-hit feature rows (MODE 7) held to an independent float64
truth.  No oracle call: the conditions, inputs and thresholds are those
the CPU suite (tests/test_ground_truth_reference.py) holds the oracle to, where every threshold is measured."""
import numpy as np
import pytest

import ground_truth as G
from accum_helpers import fresh_context
from ground_truth import BUILTINS, N_RAYS, POPULATIONS, builtin_report, cached, population

pytestmark = pytest.mark.gpu

MODES = ("BVH_REFERENCE", "BVH_SAH")


def device_hits(srt, gpu, sc, mode, rays):
    gpu.upload_scene(G.product_scene(srt, sc, getattr(srt, mode)))
    return gpu.trace_rays(rays)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(POPULATIONS))
def test_random_rays_hold(srt, gpu, name, mode):
    """20 000 rays into each soup (30 / 200 triangles, spread 0.5 / 2.0), the 12 x 12 sheet and the axis-aligned / sticky set: every ray at
    least EDGE_MARGIN from every edge agrees with the brute-force truth in hit / miss and triangle (the truth ignores the tree: a tree
    that loses a triangle fails here), |t - t_truth| <= C_T t_bound, front_face == sign(n.d), at most 0.5 % of the rays left out.
    The oracle on the same input: 0 rays differ, at most 2 of 20 000 inside the margin, largest |dt| / t_bound 3.44."""
    sc, rays = population(name)
    _, summary = G.assert_hits_hold(G.f64(sc["V"]), rays, device_hits(srt, gpu, sc, mode, rays), "%s %s" % (name, mode))
    print(name, mode, summary)
    assert len(rays) == N_RAYS and summary["hit_share"] > 0.04


@pytest.mark.parametrize("mode", MODES)
def test_edge_aimed_rays_hold(srt, gpu, mode):
    """10 712 rays aimed at interior vertices, edge midpoints and random edge points of the sheet: each hits a triangle adjacent to its
    target, within the t bound, or misses (a leak: the reference's per-triangle interior test is not watertight); none
    hits another triangle.  The leak share is printed, not asserted (the oracle's: 9.2 % with the reference tree, 9.3 % with the SAH tree)."""
    sc = G.bumpy_sheet()[0]
    rays, adjacent = cached("edge_rays", G.edge_aimed_rays)
    s = G.assert_edge_aimed_hold(G.f64(sc["V"]), rays, adjacent, device_hits(srt, gpu, sc, mode, rays), "edge-aimed %s" % mode)
    print("edge-aimed rays, %s: %d of %d leak (%.2f %%)" % (mode, s["leaks"], s["rays"], 100 * s["leak_share"]), s)


@pytest.mark.parametrize("scene_id", BUILTINS)
def test_builtin_scenes(srt, gpu, scene_id):
    """4 000 camera rays (pixel centres, 80 x 50) of CORNELL, PRISM and TRIS: every ray that differs from the truth is near an edge or
    involves a triangle whose projection is degenerate (listed in the printed report and in DESIGN section 2)."""
    def trace(scene, rays):
        gpu.upload_scene(scene)
        return gpu.trace_rays(rays)
    print(builtin_report(srt, scene_id, trace))


@pytest.mark.parametrize("name", list(G.RADIOMETRY))
def test_radiometry_holds(srt, gpu, name):
    """XYZ sums of small frames against the closed forms, all three channels, through the instrumented and the production kernel and both
    tree builders: |z_img| <= 5 (+ the float32 summation allowance spp 2^-24), and for the cosine law 0.8 <= rms per-pixel z <= 1.2.
    The five cases about where the light goes (wedge_dispersion, wedge_tir: refraction, Sellmeier's n and the critical angle;
    fuzz_absorbed, fuzz_directed: fuzzed metal; lens: the thin lens) are held per pixel too: the same range of the rms z in every
    channel over at least 300 pixels with spp P >= 10, and sums of exactly 0 wherever the truth and its neighbours are dark.
    The oracle's own values on these inputs stand in test_ground_truth_reference.test_oracle_radiometry_holds (|z_img| <= 2.2)."""
    sc, camera, W, H, spp, depth = G.RADIOMETRY[name]()
    cam = G.camera(srt, camera, W, H)
    exp = cached(("expectation", name), lambda: G.expectation(name, G.color_tables(srt), cam, sc, W, H, depth))
    for mode in MODES:
        scene = G.product_scene(srt, sc, getattr(srt, mode))
        for counted in (True, False):
            out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=counted)
            z = G.assert_radiometry_holds(name, out["xyz"], W, H, spp, exp, "%s counted=%s" % (mode, counted))
            print(name, mode, "instrumented" if counted else "production", z)
    if name == "floor_under_sky":                      # at depth 1 every path ends at the bounce limit: every sum is exactly 0
        out = srt.render_image(scene, cam, W, H, spp, 1, renderer=gpu)
        assert all(not p.any() for p in out["xyz"])


@pytest.mark.parametrize("name", list(G.FILM_CASES))
def test_film_holds(srt, gpu, name):
    """The spectral film (accum_reset_spectral, one render_chunk_accum of the case's film spp, read_spectral) against the film's float64
    truth, both tree builders: per bin over the image |z_bin| <= 5 (+ the float32 summation allowance); per entry (pixel, bin) the rms z
    in 0.8 .. 1.2 over at least 3 000 entries with spp Pdep >= 10 in at least 300 pixels (mirror: per bin only); entries dark in the
    truth with their 26 neighbours exactly 0, and so are bins dark in every pixel; for sky_only and sky_spikes the image mean of
    spectral_radiance is the hat average of the background at every bin.  Inputs, spp and thresholds are those the CPU suite holds
    the oracle to (test_ground_truth_reference.test_oracle_film_holds, where the oracle's figures stand)."""
    sc, cam, W, H, spp, depth, exp = G.film_case(srt, name)
    radiance = srt.spectral_radiance if name in ("sky_only", "sky_spikes") else None
    for mode in MODES:
        fresh_context(gpu, G.product_scene(srt, sc, getattr(srt, mode)), cam, W, H, depth)
        gpu.accum_reset_spectral()
        gpu.render_chunk_accum(W, H, spp)
        out = G.assert_film_holds(name, gpu.read_spectral(W, H), W, H, spp, exp, mode, radiance)
        print(name, mode, "truth's CPU time %.2f s" % exp["seconds"], out)


@pytest.mark.parametrize("name", G.FEATURE_CASES)
def test_features_hold(srt, gpu, name):
    """The first-hit feature rows (accum_reset_features, one render_chunk_accum of n samples, read_features) against the feature truth,
    both tree builders: hits binomial in the exact coverage (z_img, rms z over the edge pixels, hits == n where P == 1, all eight sums 0
    where the pixel and its neighbours are dark); normal sum / hits the unit normal turned towards the camera within NORMAL_TOL and
    albedo sum == hits col exactly wherever a pixel sees one triangle; for plates the mean distance of every full pixel against the
    footprint mean of |hit - eye| (rms z in 0.8 .. 1.2).  The oracle's figures stand in test_ground_truth_reference.test_oracle_features_hold."""
    sc, cam, W, H, n, depth, exp = G.feature_case(srt, name)
    for mode in MODES:
        fresh_context(gpu, G.product_scene(srt, sc, getattr(srt, mode)), cam, W, H, depth)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, n)
        f = gpu.read_features(W, H)
        rows = np.concatenate([f["normal"], f["albedo"], f["distance"][..., None], f["hits"][..., None]], axis=-1)
        print(name, mode, G.assert_features_hold(rows, n, exp, "%s %s" % (name, mode)))
