"""tests/expose_reference.py (the restatement of metering and tone mapping) against exact arithmetic, and srt_meter_decide of the built
library against the restatement, without a GPU: the decision in Python integers, the tone curve in fractions.Fraction with one rounding
to float32 per operation, every cfg refusal."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import expose_reference as R
from helpers import bits

F = np.float32
ERR_INVALID = -1


def round_f32(x):
    """the Fraction x rounded to the nearest float32, ties to even (finite results only), as a Fraction"""
    if x == 0:
        return Fraction(0)
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)                         # the spacing of float32 at a (the denormals' below 2^-126)
    m, rest = divmod(a, q)
    m = int(m)
    if rest * 2 > q or (rest * 2 == q and m % 2):
        m += 1
    out = m * q
    assert out < Fraction(2) ** 128
    return sign * out


def fr(v):
    return Fraction(float(v))


# ---- the tone curve and the luminance against exact arithmetic ---------------------------------------------------------------------
def _tone_exact(c, g, curve, white):
    kw = round_f32(fr(F(white)) * fr(F(white)))
    cp = [round_f32(fr(g) * fr(v)) for v in c]
    if curve == 0:
        return cp
    y = cp[1]
    t = round_f32(y / kw)
    num, den = round_f32(1 + t), round_f32(1 + y)
    s = round_f32(num / den) if y > 0 else Fraction(1)
    return [round_f32(s * v) for v in cp]


def test_round_f32_is_numpys_rounding():
    rng = np.random.default_rng(3)
    a = (rng.random(300) * 10.0 ** rng.integers(-44, 30, 300)).astype(F)
    b = (rng.random(300) * 10.0 ** rng.integers(-6, 6, 300) + 1e-3).astype(F)
    for x, y in zip(a, b):
        assert round_f32(fr(x) * fr(y)) == fr(F(x * y)) or not np.isfinite(F(x * y))
        assert round_f32(fr(x) / fr(y)) == fr(F(x / y))
    assert round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == 1 and round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == 1 + Fraction(1, 2 ** 22)


def test_tone_curve_equals_fraction_arithmetic_with_one_rounding_per_operation():
    rng = np.random.default_rng(4)
    c = ((rng.random((120, 3)) - 0.2) * 10.0 ** rng.integers(-6, 5, (120, 1))).astype(F)
    c[0] = 0
    c[1] = [0.5, -0.25, 0.125]          # a negative luminance keeps s = 1
    c[2] = [1e-41, 1e-40, 1e-42]        # denormals
    for curve in (0, 1):
        for g, white in ((F(1), 4.0), (F(0.37), 1.5), (F(37.5), 1000.0), (F(2.0 ** -9), 4.0)):
            got = R.tone(c, g, curve, white)
            assert got.dtype == F and got.shape == c.shape
            for p in range(c.shape[0]):
                want = _tone_exact(c[p], g, curve, white)
                assert [fr(v) for v in got[p]] == want, (curve, float(g), white, p)
    # white = +inf: t = 0 and the curve is plain Reinhard, s = 1 / (1 + y)
    got = R.tone(c, F(1), 1, np.inf)
    pos = c[:, 1] > 0
    want = (F(1) / (F(1) + c[pos, 1])).astype(F)[:, None] * c[pos]
    assert np.array_equal(bits(got[pos]), bits(want.astype(F))) and np.array_equal(bits(got[~pos]), bits(c[~pos]))
    # curve 0 at gain 1 is the identity, bit for bit, NaN and inf included
    odd = np.array([[np.nan, 1, 2], [np.inf, -np.inf, 0], [-0.0, 0.0, 1e-45]], F)
    assert np.array_equal(bits(R.tone(odd, 1.0, 0)), bits(odd))
    # a non-finite pixel stays in its own row
    mixed = np.concatenate([c[:4], odd, c[4:8]])
    out = R.tone(mixed, F(2), 1, 4.0)
    assert np.isfinite(out[:4]).all() and np.isfinite(out[7:]).all() and not np.isfinite(out[4:6]).all()


def test_luminance_is_one_reciprocal_and_one_product():
    s = np.array([3.0, 5.0, 7.0, 0.0, 1e-30], F)
    for n in (1, 3, 7, 4096, 65535):
        want = [round_f32(round_f32(Fraction(1, n)) * fr(v)) for v in s]
        assert [fr(v) for v in R.luminance(s, n)] == want
    # per-pixel counts: the converged flag is masked off, a pixel without a sample is normalised by 1
    n = np.array([3, 3 | R.CONVERGED, 0, R.CONVERGED, 7], np.uint32)
    got = R.luminance(s, n)
    want = [F(F(1) / F(3)) * s[0], F(F(1) / F(3)) * s[1], s[2], s[3], F(F(1) / F(7)) * s[4]]
    assert np.array_equal(bits(got), bits(np.array(want, F)))


# ---- classification and bins ---------------------------------------------------------------------------------------------------------
def test_classification_and_bins_on_the_bit_patterns():
    u = np.array([0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0x00800001, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000,
                  0xbf800000, 0x3f800000, 0x3f87ffff, 0x3f880000], np.uint32)
    nonfinite, dark, metered, b = R.classify(u.view(F))
    assert nonfinite.tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert dark.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert b[metered].tolist() == [16, 16, 4079, 2032, 2032, 2033]
    # 16 bins per octave: y and 2 y are 16 bins apart, and the midpoint of a bin lies in it
    y = np.array([0.18, 0.36, 0.72], F)
    bb = R.classify(y)[3]
    assert bb[1] - bb[0] == 16 and bb[2] - bb[1] == 16
    for k in (16, 17, 2032, 4079):
        mid = R.bin_midpoint(k)
        assert R.classify(np.array([mid], F))[3][0] == k and np.isfinite(mid)
    h = R.histogram(u.view(F))
    assert (h["metered"], h["dark"], h["nonfinite"]) == (6, 5, 3) and int(h["hist"].sum()) == 6
    m = np.zeros(u.size, bool)
    m[[0, 4, 7]] = True
    h = R.histogram(u.view(F), m)
    assert (h["metered"], h["dark"], h["nonfinite"]) == (1, 1, 1)


# ---- srt_meter_decide of the built library against the restatement ------------------------------------------------------------------
def _decide(srt, hist, **cfg):
    return srt.meter_decide(np.asarray(hist, np.uint32), srt.meter_config(**cfg))


def _same_decision(srt, hist, **cfg):
    got = _decide(srt, hist, **cfg)
    want = R.decide(hist, **dict(R.DEFAULTS, **cfg))
    assert got["metered"] == want["metered"] and got["bin_ref"] == want["bin_ref"], (got, want, cfg)
    assert bits(F(got["y_ref"])) == bits(want["y_ref"]) and bits(F(got["gain"])) == bits(want["gain"]), (got, want, cfg)
    return got


def _brute_bin(hist, ppm):
    """the definition, spelt out on the sorted list of the metered pixels' bins"""
    pixels = np.repeat(np.arange(R.BINS), np.asarray(hist, np.int64))
    target = max(1, -(-len(pixels) * ppm // 1000000))
    return int(pixels[target - 1])


def test_decide_on_random_histograms(srt):
    rng = np.random.default_rng(8)
    for trial in range(40):
        hist = np.zeros(R.BINS, np.uint32)
        k = int(rng.integers(1, 60))
        where = rng.integers(16, 4080, k)
        hist[where] = rng.integers(1, [3, 1000, 2 ** 31][trial % 3], k)
        for ppm in (1, 250000, 500000, 999999, 1000000, int(rng.integers(1, 1000001))):
            got = _same_decision(srt, hist, percentile_ppm=ppm, key=float(rng.choice([0.18, 1.0, 3e-5, 7e6])))
            if hist.sum(dtype=np.uint64) < 100000:
                assert got["bin_ref"] == _brute_bin(hist, ppm)
            assert hist[got["bin_ref"]] > 0


def test_decide_edge_histograms(srt):
    empty = np.zeros(R.BINS, np.uint32)
    got = _same_decision(srt, empty)
    assert (got["metered"], got["bin_ref"], got["y_ref"], got["gain"]) == (0, 0, 0.0, 1.0)
    # the empty histogram's gain of 1 is clamped like any other
    assert _same_decision(srt, empty, gain_min=2.0, gain_max=8.0)["gain"] == 2.0
    assert _same_decision(srt, empty, gain_min=0.125, gain_max=0.5)["gain"] == 0.5
    # counts outside [16, 4080) are not metered
    stray = empty.copy()
    stray[[0, 15, 4080, 4095]] = 9
    assert _same_decision(srt, stray)["metered"] == 0
    one = empty.copy()
    one[2000] = 1
    for ppm in (1, 500000, 1000000):
        assert _same_decision(srt, one, percentile_ppm=ppm)["bin_ref"] == 2000
    two = empty.copy()
    two[[100, 3000]] = [999999, 1]
    assert _same_decision(srt, two, percentile_ppm=1)["bin_ref"] == 100
    assert _same_decision(srt, two, percentile_ppm=999999)["bin_ref"] == 100
    assert _same_decision(srt, two, percentile_ppm=1000000)["bin_ref"] == 3000
    low, high = empty.copy(), empty.copy()
    low[16], high[4079] = 70000, 2 ** 32 - 1
    # all mass in the first bin: key / y_ref is about 1.5e37 and the clamp brings it back; in the last: a denormal 5e-40, clamped too
    got = _same_decision(srt, low)
    assert got["bin_ref"] == 16 and got["gain"] == 2.0 ** 24
    got = _same_decision(srt, high)
    assert got["bin_ref"] == 4079 and got["gain"] == 2.0 ** -24
    assert 2.0 ** 24 < _same_decision(srt, low, key=1e-30, gain_max=3e38)["gain"] < 3e38      # ... and unclamped under wider limits
    assert _same_decision(srt, low, key=3e38, gain_max=3e38)["gain"] == float(F(3e38))          # key / y_ref = inf, clamped
    assert 0 < _same_decision(srt, high, gain_min=1e-44)["gain"] < 1e-39
    # both clamps on an ordinary histogram
    mid = empty.copy()
    mid[2032] = 5          # y_ref = 1.03125
    assert _same_decision(srt, mid, key=0.18, gain_min=0.5, gain_max=2.0)["gain"] == 0.5
    assert _same_decision(srt, mid, key=18.0, gain_min=0.5, gain_max=2.0)["gain"] == 2.0
    assert _same_decision(srt, mid, key=1.03125, gain_min=0.5, gain_max=2.0)["gain"] == 1.0
    # dark and nonfinite pass through
    assert srt.meter_decide(mid, None, dark=7, nonfinite=9)["dark"] == 7


def test_scale_invariance_of_the_restatement():
    rng = np.random.default_rng(12)
    y = (rng.random(5000) * 10.0 ** rng.integers(-3, 3, 5000) + 1e-4).astype(F)
    base = R.meter(y)
    for k in (-7, 3, 20):
        m = R.meter((y * F(2.0 ** k)).astype(F))
        assert np.array_equal(np.roll(base["hist"], 16 * k), m["hist"]) and m["bin_ref"] == base["bin_ref"] + 16 * k
        assert float(m["gain"]) == float(base["gain"]) * 2.0 ** -k


def test_every_cfg_refusal(srt):
    L = srt.binding.lib()
    B = srt.binding
    hist = np.zeros(R.BINS, np.uint32)
    hist[2000] = 3
    hp = hist.ctypes.data_as(C.POINTER(C.c_uint32))
    res = B.MeterResult()

    def cfg(**kw):
        base = dict(x0=0, y0=0, w=0, h=0, percentile_ppm=500000, key=0.18, gain_min=0.5, gain_max=2.0)
        base.update(kw)
        m = B.Meter(base["x0"], base["y0"], base["w"], base["h"], base["percentile_ppm"], base["key"], base["gain_min"], base["gain_max"], (C.c_uint32 * 4)(*kw.get("reserved", (0, 0, 0, 0))))
        return m

    assert L.srt_meter_decide(hp, C.byref(cfg()), C.byref(res)) == 0 and res.metered == 3
    assert L.srt_meter_decide(hp, C.byref(cfg(x0=3, y0=4, w=5, h=6)), C.byref(res)) == 0
    inf, nan = float("inf"), float("nan")
    bad = [dict(percentile_ppm=0), dict(percentile_ppm=1000001), dict(key=0.0), dict(key=-1.0), dict(key=inf), dict(key=nan),
           dict(gain_min=0.0), dict(gain_min=-1.0), dict(gain_min=nan), dict(gain_min=3.0), dict(gain_max=inf), dict(gain_max=nan), dict(gain_min=inf, gain_max=inf),
           dict(reserved=(1, 0, 0, 0)), dict(reserved=(0, 0, 0, 1)), dict(w=5), dict(h=5), dict(x0=2), dict(x0=1, y0=1, w=0, h=3), dict(x0=1, y0=1, w=3, h=0)]
    for kw in bad:
        before = bytes(res)
        assert L.srt_meter_decide(hp, C.byref(cfg(**kw)), C.byref(res)) == ERR_INVALID, kw
        assert bytes(res) == before, kw
    assert L.srt_meter_decide(None, C.byref(cfg()), C.byref(res)) == ERR_INVALID
    assert L.srt_meter_decide(hp, None, C.byref(res)) == ERR_INVALID
    assert L.srt_meter_decide(hp, C.byref(cfg()), None) == ERR_INVALID
    assert b"srt_meter_decide" in L.srt_last_error(None)
    # the Python front door refuses the same before the library is asked
    for kw in (dict(percentile_ppm=0), dict(percentile_ppm=2.5), dict(key=0), dict(key="x"), dict(gain_min=4.0, gain_max=2.0), dict(gain_max=inf),
               dict(rect=(0, 0, 0, 4)), dict(rect=(1, 2, 3)), dict(rect=(-1, 0, 2, 2))):
        with pytest.raises(ValueError):
            srt.meter_config(**kw)
    for kw in (dict(gain=0.0), dict(gain=inf), dict(gain=nan), dict(curve=2), dict(curve="filmic"), dict(white=0.0), dict(white=nan), dict(white=-1.0)):
        with pytest.raises(ValueError):
            srt.tone_config(**kw)
    t = srt.tone_config(gain=2.0, curve="linear", white=inf)
    assert (t.curve, t.gain, t.white) == (0, 2.0, inf)
    with pytest.raises(ValueError):
        srt.meter_decide(np.zeros(100, np.uint32))
