"""The direct-light pass's restatement (tests/direct_light_reference.py) held to published vectors and to the float64 truth, without a GPU.

Generator and tables: Philox4x32-10 against Random123's known answers; the T tables against ground_truth.exact_integral; the thresholds
exactly (sum 2^24, every light at least 1 wide, the pick frequencies over all 2^24 draws).  Truth scenes (tests/direct_light_cases.py): the
restatement runs with its two queries answered by ground_truth's float64 brute force, and its sums meet the closed forms.

Deliberate breaks of the restatement, each tried once on test_truth_scene (what turned red; z_img of channel 0, allowed 5):
  * the 1 / pi of the weight left out          cosine_law z_img = 542, split_light 543, occluded_light 442
  * r^2 in place of r^4                         cosine_law z_img = 1733, split_light 1733, occluded_light 884
  * one-sided lights (n_l . d clamped at 0)     keeping the face n_l points to: cosine_law, split_light (z_img = -129) and occluded_light,
                                                whose sums are then all 0 (no pixel has a variance); keeping the other face: split_light
                                                alone (z_img = -691), whose two halves are wound opposite ways
  * the pick not divided out (no area / p_l)    split_light z_img = -378; the scenes with one light stay green (p = 1)
  * n not face-forwarded                        cosine_law, split_light, occluded_light: every sum 0 (the floor's own normal points down,
                                                away from camera and light); sky_blocker z_img = 98.  floor_under_sky stays green:
                                                a sky ray leaves on either side of a floor with nothing around it.

Cases that reach what the five above cannot (each also runs on the device, tests/test_direct_light.py):
  many_lights        37 lights, eight pinned at width 1 (test_many_lights_table states the scene before anything is sampled): a binary
                     search of several unequal halves, thresholds by largest remainder with pinned entries, the weight area / p_l over
                     seven decades of area.  test_fixed_draw re-derives two committed draws with one Philox call each -- one equal to
                     thresholds[a] of a pinned light a, one equal to thresholds[m] of a wide light m, which must pick m and not m - 1 --
                     and holds the weight of that sample to its float64 value within a bound counted from the rounded operations.
  two_emitters       two emissive materials whose slot order is not their material order, over a floor of two materials: a swapped or
                     mis-strided t_light index.  Deliberate breaks of the expectation, each tried once (test_two_emitters_tells_its_
                     tables_apart keeps both red): the two emitters' T swapped, z_img = 196 (channel 0, allowed 5); the floor materials'
                     rows swapped, z_img = 35 (channel 0).
  emitters_in_view   EMITTED: T_emit[material] on each of two emitters and T_bg on the sky, to the rounding of S equal terms, at least
                     MIN_PIXELS pixels of each; the tables themselves against the exact integral (test_tables_hold_the_exact_integral).
  test_black_sky     SKY under a black background: no sky row, no occlusion query, sums 0; LIGHTS with SKY is LIGHTS alone.
  the lens           floor_under_sky_lens (every pixel still T_sky: every lens ray meets the floor) and cosine_law_lens (F averaged over
                     footprint and lens; test_lens_quadrature_is_converged: the two resolutions differ by 0.004 of the smallest per-pixel
                     standard error, the pinhole's expectation by 43 of them).
  lens rows          test_lens_rows_hold_to_geometry, float64 on the rows of samples 0 .. 3: origin - centre = a disk_u + b disk_v by
                     least squares with a residual within the four rounded operations' 4 x 2^-24 M per component (M the largest
                     coordinate of the centre plus the disk vectors'), a^2 + b^2 < 1 up to that; origin + d lies in the pixel's own
                     footprint [-0.5, 0.5)^2 in the (du, dv) basis to the nine rounded operations behind it (this fails where d is not
                     taken from the moved origin); over the N rows |mean a|, |mean b| <= 5 x 0.5 / sqrt(N) and
                     |mean (a^2 + b^2) - 0.5| <= 5 sqrt(1/12) / sqrt(N), a uniform disk's own moments; no row starts at the centre.
                     Two breaks of the rows, each tried once on both cameras: d taken from the centre puts origin + d up to 1.2 (1.4)
                     pixels off the centre of its pixel, allowed 0.5; a disk of 0.7 of the radius gives mean (a^2 + b^2) = 0.25.
Not reached, and not faked: the fallbacks after 16 disk tries and 32 sphere tries and the guard for n + ruv ~ 0 have a probability of about
1e-11 per row; no search finds them in a sitting.
"""
import numpy as np
import pytest

import direct_light_cases as DC
import direct_light_reference as R
import ground_truth as G
from helpers import bits


def test_philox_known_answers():
    for counter, key, want in R.PHILOX_KAT:
        got = R.philox(*[np.array([c], np.uint32) for c in counter], *key)
        assert [int(x[0]) for x in got] == list(want), (counter, key)
    # arrays of counters: each entry is the scalar call's
    c0 = np.arange(5, dtype=np.uint32)
    many = R.philox(c0, 7, 2, 0, 0x1234, 0xabcd)
    for k in range(5):
        one = R.philox(np.array([k], np.uint32), 7, 2, 0, 0x1234, 0xabcd)
        assert [int(x[k]) for x in many] == [int(x[0]) for x in one]


def test_uniforms_are_exact_dyadics():
    x = np.array([0, 255, 256, 0xffffffff, 0x80000000], np.uint32)
    u = R.u01(x)
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]
    assert R.pm1(x).tolist() == [-1.0, -1.0, -1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23, 0.0]
    assert R.seed_key(0x123456789abcdef0) == (0x9abcdef0, 0x12345678)


@pytest.mark.parametrize("name", ["cosine_law", "sky_blocker", "two_emitters", "emitters_in_view"])
def test_tables_hold_the_exact_integral(srt, name):
    """every T entry against three-point Gauss-Legendre in float64: one float32 rounding (2^-24 relative) plus the doubles' own (1e-12)"""
    c = DC.case(srt, name)
    cmf = G.color_tables(srt)[:3]
    tab, sp, bg = R.tables(c["desc"]), G.f64(c["desc"]["spectra"]), G.f64(c["desc"]["background"])
    close = lambda got, want: np.abs(got.astype(np.float64) - want) <= np.abs(want) * (2.0 ** -24 + 1e-12)
    assert close(tab["t_bg"], G.exact_integral(cmf, [bg])).all()
    for m in range(len(sp)):
        assert close(tab["t_emit"][m], G.exact_integral(cmf, [sp[m]])).all()
        assert close(tab["t_sky"][m], G.exact_integral(cmf, [sp[m], bg])).all()
        for e in set(tab["mat"].tolist()):
            assert close(tab["t_light"][m, e], G.exact_integral(cmf, [sp[m], sp[e]])).all()
    assert tab["bg_nonzero"] == bool(bg.any())


def _device_pick(th, k):
    """the binary search as the header states it"""
    a, b = 0, len(th) - 1
    while b - a > 1:
        m = (a + b) >> 1
        if th[m] <= k:
            a = m
        else:
            b = m
    return a


def test_thresholds_are_exact():
    rng = np.random.default_rng(5)
    g = np.exp(rng.normal(0.0, 3.0, 1000))
    g[::50] *= 1e-14                                   # lights too weak for one draw in 2^24: pinned at width 1
    th = R.thresholds(g)
    width = np.diff(th.astype(np.int64))
    assert th[0] == 0 and th[-1] == R.N_DRAWS and width.sum() == R.N_DRAWS and (width >= 1).all()
    assert (width[::50] == 1).all()
    free = width > 1
    ideal = g[free] / g[free].sum() * (R.N_DRAWS - (~free).sum())
    assert np.abs(width[free] - ideal).max() < 1.0 + 1e-6      # largest remainder: floor or floor + 1 of the free lights' share
    # the pick frequencies over all 2^24 draws
    picks = np.searchsorted(th, np.arange(R.N_DRAWS, dtype=np.uint32), side="right") - 1
    assert np.array_equal(np.bincount(picks, minlength=len(g)), width)
    for k in np.concatenate([th[:-1], th[1:] - 1, rng.integers(0, R.N_DRAWS, 64)]).tolist()[::7]:
        assert _device_pick(th, k) == picks[k]
    assert R.thresholds([3.0]).tolist() == [0, R.N_DRAWS] and R.thresholds([]).tolist() == [0]
    assert np.diff(R.thresholds([1.0, 1.0, 1.0]).astype(np.int64)).tolist() == [5592406, 5592405, 5592405]      # ties: the lower index first


def _restated(srt, name, **over):
    """the restatement's run of a truth scene under the float64 queries, computed once per set of arguments"""
    c = DC.case(srt, name)

    def make():
        intersect, occluded = R.truth_queries(c["desc"])
        kw = dict(samples=c["samples"], seed=11, parts=c["parts"])
        kw.update(over)
        return R.run(c["desc"], c["cam"], c["W"], c["H"], 0, 0, intersect, occluded, **kw)
    return c, G.cached(("direct light restated", name, tuple(sorted(over.items()))), make)


@pytest.mark.parametrize("name", DC.NAMES)
def test_truth_scene(srt, name):
    """the sampler with visibility from ground_truth.closest_hit's float64 brute force: tests/direct_light_cases.py's conditions"""
    c, out = _restated(srt, name)
    n = c["W"] * c["H"] * c["samples"]
    st = out["stats"]
    assert st["miss"] + st["emitted"] + st["specular"] + st["shaded"] == n
    if name in DC.EXACT + DC.ALL_HELD:          # under a lens too: every camera ray's first hit is the floor
        assert st["shaded"] == n, (name, st)
    if name in DC.ALL_HELD:                     # nothing stands between the floor and its lights
        assert st["light_rows"] == st["light_unoccluded"] == n, (name, st)
    if name == "emitters_in_view":
        assert st["shaded"] == 0 and st["emitted"] > 0 and st["miss"] > 0, st
    print(name, st, DC.assert_holds(name, DC.expectation(srt, name), out["sum"], out["m2"], c["samples"], c["W"], c["H"], "restatement"))


def test_many_lights_table(srt):
    """the many_lights scene is what tests/direct_light_cases.py says, before anything is sampled on it: 37 lights of positive float32
    area, exactly the eight at TINY pinned at width 1, the tiny triangles' float32 sides within 1 % of the sides asked for, the wide ones'
    areas over three decades, every pixel held; and the binary search as the header states it picks, at both ends of every light's
    interval of draws, the light the interval belongs to"""
    c = DC.case(srt, "many_lights")
    tab = R.tables(c["desc"])
    th = tab["thresholds"]
    width = np.diff(th.astype(np.int64))
    assert len(tab["area"]) == DC.N_MANY and tab["area"].dtype == np.float32 and (tab["area"] > 0).all()
    assert np.nonzero(width == 1)[0].tolist() == list(DC.TINY) and (width == 1).sum() == 8 and width.sum() == R.N_DRAWS
    wide = np.delete(tab["area"].astype(np.float64), DC.TINY)
    assert wide.max() / wide.min() >= 1e3, wide.max() / wide.min()
    V, e = G.f64(DC.many_lights()), np.linalg.norm(G.f64(G.LIGHT[1:] - G.LIGHT[0]), axis=1)
    for k in DC.TINY:
        for a, b, edge in ((1, 0, 0), (2, 0, 1)) if k % 3 != 1 else ((1, 2, 0), (0, 2, 1)):
            assert abs(np.linalg.norm(V[k, a] - V[k, b]) / (DC.TINY_SIDE * e[edge]) - 1.0) < 0.01, (k, a, b)
    normal = tab["normal"].astype(np.float64)
    assert (normal[:, 1] > 0).any() and (normal[:, 1] < 0).any(), "both windings"
    held = DC.expectation(srt, "many_lights")["held"]
    assert held.all() and held.sum() == c["W"] * c["H"]
    for a in range(DC.N_MANY):
        assert _device_pick(th, int(th[a])) == a and _device_pick(th, int(th[a + 1]) - 1) == a, a


@pytest.mark.parametrize("which", ["pinned", "edge"])
def test_fixed_draw(srt, which):
    """the two committed draws of many_lights (DC.DRAW_S, found once by DC.find_draw), re-derived with one Philox call: "pinned" equals
    thresholds[a] of a light of width 1, "edge" equals thresholds[m] of a light wider than 1 and must pick m, not m - 1.  The restatement
    of that one sample under the float64 queries then picks the light, traces the row and weighs it within the bound
    DC.assert_weight_holds derives."""
    c = DC.case(srt, "many_lights")
    tab = R.tables(c["desc"])
    th = tab["thresholds"]
    (x, y), s = DC.DRAW_PIXEL, DC.DRAW_S[which]
    k = int(R.philox(np.array([y * c["W"] + x], np.uint32), np.uint32(s), 2, 0, *R.seed_key(DC.DRAW_SEED))[0][0] >> np.uint32(8))
    a = int(np.nonzero(th == k)[0][0]) if (th == k).any() else -1
    assert a >= 0 and k in DC.draw_targets(th)[which].tolist(), (which, k)
    width = int(th[a + 1]) - int(th[a])
    assert (width == 1 and a in DC.TINY) if which == "pinned" else (width > 1 and a > 0), (which, a, width)
    assert _device_pick(th, k) == a
    assert DC.find_draw(DC.draw_targets(th)[which], y * c["W"] + x, DC.DRAW_SEED, start=s - 5, limit=s + 5) == (s, k)
    assert DC.expectation(srt, "many_lights")["held"][y * c["W"] + x]
    intersect, occluded = R.truth_queries(c["desc"])
    out = R.run(c["desc"], c["cam"], 1, 1, x, y, intersect, occluded, samples=1, first_sample=s, seed=DC.DRAW_SEED, parts=("lights",), keep=True)
    assert (c["desc"]["normal"][0:2] == np.array([0, 1, 0], np.float32)).all(1).all() or (c["desc"]["normal"][0:2] == np.array([0, -1, 0], np.float32)).all(1).all()
    rnd = out["rounds"][0]
    print(which, "light %d of width %d, draw %d; weight off by %.3g, allowed %.3g" % (
        (a, width, k) + DC.assert_weight_holds(tab, rnd["records"][0], rnd["light_rows"][0], a, which)))


def test_two_emitters_tells_its_tables_apart(srt):
    """both floor materials are in view, and each of the two deliberate breaks of the expectation (module docstring) turns it red"""
    c, out = _restated(srt, "two_emitters")
    tri = DC.first_hits(c, 0.0, 0.0)[0]
    assert min((tri == 0).sum(), (tri == 1).sum()) >= G.MIN_PIXELS, ((tri == 0).sum(), (tri == 1).sum())
    tab = out["tab"]
    assert tab["mat"].tolist() == [3, 1], "the red emitter (material 3) comes first: slot order is not material order"
    assert abs(float(tab["area"][0]) / float(tab["area"][1]) - 1.0) > 0.2, "unequal areas"
    exp = DC.expectation(srt, "two_emitters")
    for broken in ("emitters", "floors"):
        wrong = dict(exp, **DC.two_emitters_expectation(c, tab, broken))
        with pytest.raises(AssertionError) as e:
            DC.assert_holds("two_emitters", wrong, out["sum"], out["m2"], c["samples"], c["W"], c["H"], broken + " swapped")
        print(broken, "swapped:", e.value)


def test_black_sky(srt):
    """cosine_law has a black background.  SKY alone: no sky row is made, no occlusion query asked, every sum 0.  LIGHTS with SKY is
    LIGHTS alone in every bit and counter."""
    c = DC.case(srt, "cosine_law")
    intersect, occluded = R.truth_queries(c["desc"])
    calls = dict(intersect=0, occluded=0)

    def counted(fn, name):
        def call(rows):
            calls[name] += 1
            return fn(rows)
        return call
    run = lambda **kw: R.run(c["desc"], c["cam"], c["W"], c["H"], 0, 0, counted(intersect, "intersect"), counted(occluded, "occluded"), samples=3, seed=11, **kw)
    sky = run(parts=("sky",), keep=True)
    assert not R.tables(c["desc"])["bg_nonzero"]
    assert calls == dict(intersect=3, occluded=0)
    assert not sky["sum"].any() and not sky["m2"].any() and sky["stats"]["sky_rows"] == 0 and sky["stats"]["light_rows"] == 0
    assert sky["stats"]["shaded"] == 3 * c["W"] * c["H"]
    assert all(not r["sky_rows"].any() and not (r["records"][:, 3] & R.ROW_SKY).any() for r in sky["rounds"])
    both, lights = run(parts=("lights", "sky")), run(parts=("lights",))
    assert calls == dict(intersect=9, occluded=6)
    assert np.array_equal(bits(both["sum"]), bits(lights["sum"])) and np.array_equal(bits(both["m2"]), bits(lights["m2"]))
    assert both["stats"] == lights["stats"] and lights["stats"]["light_unoccluded"] > 0


def lens_camera(srt, name):
    """(cam, W, H): RANDOM_SPHERES' default camera at 64 x 48 (defocus angle 0.6 degrees) or a lens case's own"""
    if name == "random_spheres":
        return srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).default_camera(64, 48), 64, 48
    c = DC.case(srt, name)
    return c["cam"], c["W"], c["H"]


@pytest.mark.parametrize("name", DC.LENS_CAMERAS)
def test_lens_rows_hold_to_geometry(srt, name):
    """the restatement's camera rows of samples 0 .. 3 under a thin lens (module docstring, "lens rows")"""
    cam, W, H = lens_camera(srt, name)
    assert cam.defocus_angle > 0
    gx, gy, pid = R.pixels(cam, W, H, 0, 0)
    rows = np.stack([R.camera_rows(cam, gx, gy, pid, np.uint32(s), R.seed_key(11)) for s in range(4)])
    print(name, DC.assert_lens_rows_hold(cam, W, H, rows, name))


def test_lens_quadrature_is_converged(srt):
    """cosine_law_lens' expectation at LENS_COARSE and at LENS_FINE: the finer one is used, and the two differ by less than a tenth of the
    smallest per-pixel standard error of the test in every channel"""
    c, out = _restated(srt, "cosine_law_lens")
    S = c["samples"]
    coarse, fine = DC.lens_share(c, *DC.LENS_COARSE), DC.expectation(srt, "cosine_law_lens")["share"]
    T = out["tab"]["t_light"][0, 1].astype(np.float64)
    mean = out["sum"].reshape(-1, 3).astype(np.float64) / S
    se = np.sqrt(np.maximum(out["m2"].reshape(-1, 3).astype(np.float64) - S * mean * mean, 0.0) / (S - 1) / S)
    worst = (np.abs(fine - coarse).max() * T) / se.min(0)
    pinhole = np.abs(fine - DC.expectation(srt, "cosine_law")["share"]).max() * T / se.min(0)
    print("lens quadrature: max |fine - coarse| / min standard error per channel", worst, "; against the pinhole's expectation", pinhole)
    assert (se > 0).all() and (worst < 0.1).all(), worst


def test_occluded_truth_converges(srt):
    """the exact occluded form factor against a float64 midpoint quadrature of the light at n and 2 n nodes per axis.  The shadow's edge
    (at most 4 lines, each through at most 2 n cells, twice for the fold) meets at most 16 n of the n^2 cells, each wrong by at most its
    whole value: |q_n - exact| <= 16 / n x (max integrand x area).  Held at n and 2 n, and the two quadratures differ by no more than
    the sum of their bounds.  The geometry: asserted inside occluded_share (the blocker stays between every floor point and the light's plane)."""
    exp, c = DC.expectation(srt, "occluded_light"), DC.case(srt, "occluded_light")
    eye, d = G.pixel_rays(c["cam"], c["W"], c["H"])
    held = np.nonzero(exp["held"])[0][::29]
    x = DC.floor_hits(eye, d[held])
    exact, F_light, dark = DC.occluded_share(x, DC.OCC_LIGHT, DC.BLOCKER)
    assert dark.any() and (exact > 0).any() and ((exact > 0) & (exact < 0.99 * F_light)).any(), "umbra, light and penumbra are all sampled"
    n = 96
    q1, q2 = DC.occluded_share_quadrature(x, DC.OCC_LIGHT, DC.BLOCKER, n), DC.occluded_share_quadrature(x, DC.OCC_LIGHT, DC.BLOCKER, 2 * n)
    light = G.f64(DC.OCC_LIGHT)
    area = 0.5 * np.linalg.norm(np.cross(light[1] - light[0], light[2] - light[0]))
    fmax = 1.0 / (np.pi * (light[:, 1].min() ** 2))      # cos cos / (pi r^2) <= 1 / (pi h^2), h the light's lowest height above the floor
    b1, b2 = 16.0 / n * fmax * area, 16.0 / (2 * n) * fmax * area
    print("occluded truth: max |q_n - exact| %.3g (bound %.3g), max |q_2n - exact| %.3g (bound %.3g), max F %.3g" % (
        np.abs(q1 - exact).max(), b1, np.abs(q2 - exact).max(), b2, F_light.max()))
    assert np.abs(q1 - exact).max() <= b1 and np.abs(q2 - exact).max() <= b2 and np.abs(q2 - q1).max() <= b1 + b2
    assert np.abs(q2 - exact).max() <= np.abs(q1 - exact).max() + 1e-12 or np.abs(q2 - exact).max() <= 0.5 * b2
    assert (q2[dark] == 0).all() and (exact[dark] == 0).all()


def test_floor_seen_from_below(srt):
    """a camera under the floor sees its other face: every sample is shaded, every sky ray leaves, every pixel gets T_sky"""
    sc, _, W, H, _, _ = G.floor_under_sky()
    scene = G.product_scene(srt, sc, srt.BVH_SAH)
    desc = R.describe(srt, scene)
    cam = G.camera(srt, (30.0, (0, -3, 4), (0, 0, 0)), 16, 12)
    intersect, occluded = R.truth_queries(desc)
    out = R.run(desc, cam, 16, 12, 0, 0, intersect, occluded, samples=4, seed=3, parts=("sky",))
    assert out["stats"]["shaded"] == 16 * 12 * 4 == out["stats"]["sky_unoccluded"]
    mean = out["sum"].reshape(-1, 3) / 4
    assert (np.abs(mean - out["tab"]["t_sky"][0]) <= 3 * 2.0 ** -24 * out["tab"]["t_sky"][0]).all()


def test_samples_do_not_depend_on_rectangle_parts_or_split(srt):
    """counter-based numbers: a sub-rectangle, a single part and two halves of the samples reproduce the full call's values"""
    c = DC.case(srt, "occluded_light")
    intersect, occluded = R.truth_queries(c["desc"])
    run = lambda w, h, ox, oy, **kw: R.run(c["desc"], c["cam"], w, h, ox, oy, intersect, occluded, seed=5, **kw)
    full = run(c["W"], c["H"], 0, 0, samples=4)
    part = run(7, 5, 11, 9, samples=4)
    assert np.array_equal(part["sum"], full["sum"][9:14, 11:18]) and np.array_equal(part["m2"], full["m2"][9:14, 11:18])
    lights = run(c["W"], c["H"], 0, 0, samples=4, parts=("lights",))
    assert np.array_equal(lights["sum"], full["sum"])          # (no sky, nothing emissive in view: the lights' term is the whole sum)
    a, b = run(c["W"], c["H"], 0, 0, samples=2), run(c["W"], c["H"], 0, 0, samples=2, first_sample=2)
    assert np.array_equal(a["m2"] + b["m2"], full["m2"]) or np.allclose(a["m2"] + b["m2"], full["m2"], rtol=2.0 ** -22, atol=0)
    assert np.allclose(a["sum"] + b["sum"], full["sum"], rtol=2.0 ** -22, atol=0)
    assert a["stats"]["light_unoccluded"] + b["stats"]["light_unoccluded"] == full["stats"]["light_unoccluded"]
