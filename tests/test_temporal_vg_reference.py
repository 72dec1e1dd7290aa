"""tests/temporal_vg_reference.py, the numpy restatement of the variance measured across frames, held to independent arithmetic and to the
properties srt_c_api.h lists: fractions with one rounding per operation, the colour of the moment-less restatement, exact power-of-two
scaling, a statistical truth about what the moments measure, and the fallbacks to the spatial estimate.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import denoise_vg_reference as V
import temporal_reference as T
import temporal_vg_reference as TV
from helpers import bits

F = np.float32
INF = float("inf")
OFF = dict(sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)


def _rounded(x):
    """a Fraction rounded to the nearest float32 (ties to even, normal range), as a Fraction"""
    if x == 0:
        return Fraction(0)
    mag, e = abs(x), 0
    while mag >= Fraction(2) ** (e + 1):
        e += 1
    while mag < Fraction(2) ** e:
        e -= 1
    assert -126 <= e <= 127
    quantum = Fraction(2) ** (e - 23)
    n = mag / quantum
    lo = n.numerator // n.denominator
    rest = n - lo
    lo += 1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2) else 0
    return (lo * quantum) * (1 if x > 0 else -1)


def _fr(v):
    return Fraction(float(v))


def _static(srt, h=None, w=None):
    """the exact geometry with zero shift: one camera for both frames, every pixel reprojects onto itself"""
    prev, _, g = T.shift_case(srt.CameraData)
    return prev, (g if h is None else g[:h, :w])


def test_moment_blend_against_fractions(srt):
    """one pixel, one tap of weight 1: the moments' own length, the alpha_min floor, the b >= 1 select, each operation rounded once"""
    cam, g = _static(srt, 1, 1)
    rng = np.random.default_rng(11)
    for trial in range(80):
        max_len = float(rng.choice([1.0, 2.0, 5.0, 7.5, 32.0]))
        alpha_min = float(F(rng.choice([1.0, 0.5, 0.3, 0.1, 1e-3])))
        c = rng.uniform(0, 4, (1, 1, 3)).astype(F)
        hc = np.concatenate([rng.uniform(0, 4, 3), [rng.choice([1.0, 3.0, 31.0, 40.0])]]).astype(F).reshape(1, 1, 4)
        hm = np.array([rng.uniform(0, 4), rng.uniform(0, 16), rng.choice([0.5, 1.0, 2.0, 6.5, 31.0, 40.0]), 0.0], F).reshape(1, 1, 4)
        out = TV.temporal_moments(c, g, cam, dict(colour=hc, guides=g, cam=cam, moments=hm), alpha_min=alpha_min, max_len=max_len, **OFF)
        assert out["stats"]["blended"] == 1 and out["tap_taken"].sum() == 1 and out["tap_weight"][0, 0, 0] == 1
        Y = _fr(c[0, 0, 1])
        Q = _rounded(Y * Y)
        ml = _rounded(_fr(hm[0, 0, 2]) + 1)
        ml = ml if ml < Fraction(max_len) else Fraction(max_len)
        b = _rounded(1 / ml)
        b = b if b > Fraction(alpha_min) else Fraction(alpha_min)
        g1, g2 = _fr(hm[0, 0, 0]), _fr(hm[0, 0, 1])      # (s / sw with sw = 1 and one tap of weight 1: the stored values)
        m1 = Y if b >= 1 else _rounded(g1 + _rounded(b * _rounded(Y - g1)))
        m2 = Q if b >= 1 else _rounded(g2 + _rounded(b * _rounded(Q - g2)))
        got = out["moments"][0, 0]
        assert (_fr(got[0]), _fr(got[1]), _fr(got[2]), _fr(got[3])) == (m1, m2, ml, 0), trial
    # the moments' length is their own: a colour history of 31 frames joined by fresh moments counts 1, 2, 3 ..
    c = np.full((1, 1, 3), F(0.75))
    hist = dict(colour=np.array([0.75, 0.75, 0.75, 31.0], F).reshape(1, 1, 4), guides=g, cam=cam, moments=None)
    lens = []
    for _ in range(4):
        hist = TV.temporal_moments(c, g, cam, hist, alpha_min=0.01, max_len=32.0, **OFF)
        lens.append((float(hist["len"][0, 0]), float(hist["moments"][0, 0, 2])))
    assert lens == [(32.0, 1.0), (32.0, 2.0), (32.0, 3.0), (32.0, 4.0)]


def test_choice_against_fractions():
    rng = np.random.default_rng(12)
    n = 400
    m1 = rng.uniform(0, 4, n).astype(F)
    m2 = ((m1.astype(np.float64) ** 2) * rng.uniform(0.9, 1.3, n)).astype(F)      # (below m1^2 at some pixels: d is clamped to 0)
    mlen = rng.choice([0.0, 1.0, 3.0, 3.5, 4.0, 17.0], n).astype(F)
    ln = rng.choice([0.0, 1.0, 2.5, 4.0, 32.0], n).astype(F)
    vs = rng.uniform(0, 1, n).astype(F)
    Hm = np.stack([m1, m2, mlen, np.zeros(n, F)], axis=-1).reshape(20, 20, 4)
    v, count = TV.choose_variance(Hm, ln.reshape(20, 20), vs.reshape(20, 20), min_len=4)
    want_count, clamped = 0, 0
    for k in range(n):
        d = _rounded(_fr(m2[k]) - _rounded(_fr(m1[k]) * _fr(m1[k])))
        clamped += d <= 0
        d = d if d > 0 else Fraction(0)
        use = mlen[k] >= 4 and ln[k] > 0
        want = _rounded(d / _fr(ln[k])) if use else _fr(vs[k])
        want_count += bool(use)
        assert _fr(v.reshape(-1)[k]) == want, k
    assert count == want_count and 0 < count < n and clamped > 0
    # a non-finite vt is never used (an overflowed m2), nor 0 / 0 at len' = 0, which the len' > 0 clause refuses first; a NaN d fails
    # d > 0 and is clamped to 0 like a negative one, as the statement's select says
    Hm = np.array([[INF, INF, 8.0, 0.0], [1.0, INF, 8.0, 0.0], [0.0, 0.0, 8.0, 0.0], [np.nan, 1.0, 8.0, 0.0]], F).reshape(1, 4, 4)
    v, count = TV.choose_variance(Hm, np.array([[8.0, 8.0, 0.0, 8.0]], F), np.full((1, 4), F(0.125)), min_len=2)
    assert count == 2 and np.array_equal(bits(v), bits(np.array([[0.0, 0.125, 0.125, 0.0]], F)))


@pytest.mark.parametrize("w,h", [(5, 3), (33, 9), (67, 35)])
def test_the_moments_never_touch_the_colour(srt, w, h):
    prev = srt.camera_init(w + 7, h + 4, 40.0, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0))
    cur = srt.camera_init(w + 7, h + 4, 40.0, (0.2, 0.1, 6.0), (0.2, 0.1, 0.0))
    c, g, hc, hg = T.random_case(w, h, 3)
    rng = np.random.default_rng(w)
    hm = np.concatenate([rng.uniform(0, 2, (h, w, 1)), rng.uniform(0, 4, (h, w, 1)), rng.integers(1, 9, (h, w, 1)), np.zeros((h, w, 1))], axis=-1).astype(F)
    for cam in (prev, cur):
        for off in ((0, 0), (5, 3)):
            want = T.temporal(c, g, cam, dict(colour=hc, guides=hg, cam=prev), off[0], off[1], **T.DEFAULTS)
            for moments in (None, hm):
                got = TV.temporal_moments(c, g, cam, dict(colour=hc, guides=hg, cam=prev, moments=moments), off[0], off[1], **T.DEFAULTS)
                for key in ("colour", "guides", "motion", "xyz", "len"):
                    assert np.array_equal(bits(got[key]), bits(want[key])), key
                assert got["stats"] == want["stats"] and np.array_equal(got["tap_taken"], want["tap_taken"])
    first = TV.temporal_moments(c, g, cur, None, **T.DEFAULTS)
    assert np.array_equal(bits(first["colour"]), bits(T.temporal(c, g, cur, None, **T.DEFAULTS)["colour"]))
    assert want["stats"]["blended"] > 0 and want["stats"]["nonfinite"] > 0


def test_scaling_by_powers_of_two(srt):
    """the picture scaled by 2^k: m1 scales by 2^k, m2 and v by 4^k, exactly; with variance_floor scaled by 4^k the filtered picture by 2^k"""
    cam, g = _static(srt, 24, 32)
    g = g.copy()
    g[:, 16:, 0:3] = F([0.0, 0.6, 0.8])      # an edge for the guides to stop at
    rng = np.random.default_rng(13)
    frames = [rng.uniform(0.25, 2.0, (24, 32, 3)).astype(F) for _ in range(6)]
    for k in (-3, 5):
        s, s2 = F(2.0 ** k), F(4.0 ** k)
        hist_a = hist_b = None
        for c in frames:
            a = TV.chain(c, g, cam, hist_a, min_len=3, levels=2, variance_floor=1e-6)
            b = TV.chain((c * s).astype(F), g, cam, hist_b, min_len=3, levels=2, variance_floor=float(F(1e-6) * s2))
            hist_a, hist_b = a["stage"], b["stage"]
            ma, mb = a["stage"]["moments"], b["stage"]["moments"]
            assert np.array_equal(bits((ma[..., 0] * s).astype(F)), bits(mb[..., 0])) and np.array_equal(bits((ma[..., 1] * s2).astype(F)), bits(mb[..., 1]))
            assert np.array_equal(bits(ma[..., 2]), bits(mb[..., 2])) and a["n_temporal"] == b["n_temporal"]
            assert np.array_equal(bits((a["var"] * s2).astype(F)), bits(b["var"]))
            assert np.array_equal(bits((a["xyz"] * s).astype(F)), bits(b["xyz"]))
        assert a["n_temporal"] == 24 * 32 and (a["var"][..., 0] > 0).any() and (bits(a["xyz"]) != bits(a["stage"]["xyz"])).any()


def test_the_moments_measure_the_variance_of_the_frames(srt):
    """64 x 64 pixels, n = 32 frames of independent Gaussian luminance (mean 1, sigma 0.25) under a camera pair that reprojects exactly:
    a = 1 / len throughout (alpha_min 2^-10, max_len 64), so m1 and m2 are the running means of Y and Y^2 and m2 - m1^2 is the biased
    sample variance, whose expectation is sigma^2 (n - 1) / n.  One pixel's sample variance has relative standard deviation
    sqrt(2 / (n - 1)) = 0.254; the mean over 4096 independent pixels 0.254 / 64 = 0.004; the bound is six of those, 2.4 %."""
    cam, g48 = _static(srt)
    # shift_case's plane at depth 4 continued to 64 rows: z = 4 L with L the length of the pixel's centre ray, so that s = z / L is exactly 4
    ys, xs = np.mgrid[0:64, 0:64]
    d = np.stack([F(-0.5) + xs.astype(F) * F(2.0 ** -6), F(0.375) - ys.astype(F) * F(2.0 ** -6), np.full((64, 64), F(-1))], axis=-1).astype(F)
    g = np.tile(g48[:1, :1], (64, 64, 1))
    g[..., 3] = (F(4) * np.sqrt(T.dot(d, d)).astype(F)).astype(F)
    assert np.array_equal(bits(g[:48]), bits(g48))
    n, sigma = 32, 0.25
    rng = np.random.default_rng(20171)
    hist = None
    for k in range(n):
        Y = rng.normal(1.0, sigma, (64, 64)).astype(F)
        c = np.stack([Y, Y, Y], axis=-1)
        hist = TV.temporal_moments(c, g, cam, hist, alpha_min=2.0 ** -10, max_len=64.0)
        if k:
            assert (hist["tap_taken"].sum(axis=0) == 1).all() and (hist["tap_weight"][0] == 1).all() and hist["stats"]["blended"] == 64 * 64
    m = hist["moments"].astype(np.float64)
    d = m[..., 1] - m[..., 0] ** 2
    want = sigma * sigma * (n - 1) / n
    print("mean of m2 - m1^2: %.6f, sigma^2 (n - 1) / n: %.6f, ratio %.4f" % (d.mean(), want, d.mean() / want))
    assert abs(d.mean() / want - 1.0) <= 0.024
    assert (hist["moments"][..., 2] == n).all() and (hist["len"] == n).all()
    # at that point v * len' is the same number
    v, count = TV.choose_variance(hist["moments"], hist["len"], np.zeros((64, 64), F), min_len=4)
    assert count == 64 * 64
    vl = (v.astype(np.float64) * n).mean()
    assert abs(vl / want - 1.0) <= 0.024


def test_fallbacks(srt):
    cam, g = _static(srt, 12, 16)
    rng = np.random.default_rng(14)
    frames = [rng.uniform(0.25, 2.0, (12, 16, 3)).astype(F) for _ in range(8)]
    frames[5][3, 4, 1] = np.nan
    frames[5][7, 2, 0] = np.inf      # (non-finite in X alone: the class is the colour's, not the luminance's)
    cfg = dict(min_len=3, levels=1)
    # a first frame: mlen' = 1, the variance is the spatial one everywhere
    out = TV.chain(frames[0], g, cam, None, **cfg)
    assert (out["stage"]["moments"][..., 2] == 1).all() and out["n_temporal"] == 0
    assert np.array_equal(bits(out["var"][..., 0]), bits(out["spatial"])) and (out["spatial"] > 0).any()
    Y = frames[0][..., 1]
    assert np.array_equal(bits(out["stage"]["moments"][..., 0]), bits(Y)) and np.array_equal(bits(out["stage"]["moments"][..., 1]), bits((Y * Y).astype(F)))
    hist = out["stage"]
    for k in (1, 2, 3):
        out = TV.chain(frames[k], g, cam, hist, **cfg)
        hist = out["stage"]
        assert (hist["moments"][..., 2] == k + 1).all() and out["n_temporal"] == (12 * 16 if k + 1 >= 3 else 0)
    assert (bits(out["var"][..., 0]) != bits(out["spatial"])).any()
    # a moment-less call in between restarts mlen at 1 while len keeps growing
    plain = T.temporal(frames[4], g, cam, hist, **T.DEFAULTS)
    assert (plain["len"] == 5).all()
    out = TV.chain(frames[4], g, cam, TV.without_moments(plain), **cfg)
    assert (out["stage"]["len"] == 6).all() and (out["stage"]["moments"][..., 2] == 1).all() and out["n_temporal"] == 0
    assert np.array_equal(bits(out["stage"]["moments"][..., 0]), bits(frames[4][..., 1]))
    hist = out["stage"]
    # a non-finite pixel stores (0, 0, 0, 0) and takes the spatial variance; its neighbours go on
    out = TV.chain(frames[5], g, cam, hist, min_len=2, levels=1)
    for y, x in ((3, 4), (7, 2)):
        assert not out["stage"]["moments"][y, x].any() and out["stage"]["len"][y, x] == 0
        assert bits(out["var"][y, x, 0]) == bits(out["spatial"][y, x])
    assert out["n_temporal"] == 12 * 16 - 2 and out["stage"]["stats"]["nonfinite"] == 2
    # ... and the pixel starts again from a first frame of its own
    out = TV.chain(frames[6], g, cam, out["stage"], min_len=2, levels=1)
    assert out["stage"]["moments"][3, 4, 2] == 1 and out["stage"]["len"][3, 4] == 1 and out["stage"]["moments"][0, 0, 2] == 3
    # min_len > max_len: never the temporal variance
    hist = None
    for k in range(8):
        out = TV.chain(frames[k % 5], g, cam, hist, temporal=dict(max_len=4.0), min_len=5, levels=0)
        hist = out["stage"]
        assert out["n_temporal"] == 0 and np.array_equal(bits(out["var"][..., 0]), bits(out["spatial"]))
    assert (hist["moments"][..., 2] == 4).all()
