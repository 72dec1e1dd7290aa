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
"""
import numpy as np
import pytest

import direct_light_cases as DC
import direct_light_reference as R
import ground_truth as G


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


@pytest.mark.parametrize("name", ["cosine_law", "sky_blocker"])
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
    c = DC.case(srt, name)
    intersect, occluded = R.truth_queries(c["desc"])
    kw = dict(samples=c["samples"], seed=11, parts=c["parts"])
    kw.update(over)
    return c, R.run(c["desc"], c["cam"], c["W"], c["H"], 0, 0, intersect, occluded, **kw)


@pytest.mark.parametrize("name", DC.NAMES)
def test_truth_scene(srt, name):
    """the sampler with visibility from ground_truth.closest_hit's float64 brute force: tests/direct_light_cases.py's conditions"""
    c, out = _restated(srt, name)
    n = c["W"] * c["H"] * c["samples"]
    st = out["stats"]
    assert st["miss"] + st["emitted"] + st["specular"] + st["shaded"] == n
    print(name, st, DC.assert_holds(name, DC.expectation(srt, name), out["sum"], out["m2"], c["samples"], c["W"], c["H"], "restatement"))


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
