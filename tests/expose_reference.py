"""Exposure metering and tone mapping (srt_meter_decide, srt_meter_accum, srt_expose_accum; include/srt_c_api.h) restated in numpy: the
luminance and the tone curve in float32, one rounded operation per line, vectorised over the pixels; the classification and the bins on
the bit patterns; the decision in Python integers.  tests/test_expose_reference.py holds this restatement to exact arithmetic;
tests/test_expose.py holds the device to it in every integer and every bit.  The conversion to sRGB behind the tone curve is not
restated here: it is the CPU oracle's orc_XYZ_to_sRGB, as in the other suites (accum_helpers.convert_xyz)."""
import numpy as np

F = np.float32
BINS = 4096
FLT_MIN = F(1.17549435e-38)
CONVERGED = 0x80000000      # the state word's flag; the low 31 bits are the samples the pixel holds
DEFAULTS = dict(percentile_ppm=500000, key=0.18, gain_min=2.0 ** -24, gain_max=2.0 ** 24)


def luminance(sum_y, n):
    """Y = inv * S_y, inv = 1.0f / (float)n; n a scalar total or the per-pixel counts (state words: the flag is masked off), 0 counts as 1"""
    n = np.asarray(n, np.int64) & (CONVERGED - 1)
    n = np.where(n == 0, 1, n)
    with np.errstate(all="ignore"):
        inv = (F(1) / n.astype(F)).astype(F)
        return (inv * np.asarray(sum_y, F)).astype(F)


def mean_xyz(sums, n):
    """the three components normalised like the luminance: sums (..., 3), n a scalar or an array of the leading shape"""
    n = np.asarray(n)
    return np.stack([luminance(np.asarray(sums, F)[..., c], n) for c in range(3)], axis=-1)


def classify(y):
    """(nonfinite, dark, metered, bin) of luminances y, the tests in the header's order"""
    y = np.asarray(y, F)
    with np.errstate(all="ignore"):
        finite = (y - y) == 0
        bright = y >= FLT_MIN
    nonfinite = ~finite
    dark = finite & ~bright
    metered = finite & bright
    return nonfinite, dark, metered, np.ascontiguousarray(y).view(np.uint32) >> 19


def histogram(y, mask=None):
    """dict(hist (4096 uint64), metered, dark, nonfinite) of the luminances y where mask (None: everywhere) holds"""
    y = np.asarray(y, F).reshape(-1)
    mask = np.ones(y.shape, bool) if mask is None else np.asarray(mask, bool).reshape(-1)
    nonfinite, dark, metered, b = classify(y)
    hist = np.bincount(b[metered & mask], minlength=BINS).astype(np.uint64)
    assert hist.size == BINS and not hist[:16].any() and not hist[4080:].any()
    return dict(hist=hist, metered=int((metered & mask).sum()), dark=int((dark & mask).sum()), nonfinite=int((nonfinite & mask).sum()))


def rect_mask(w, h, rect=None):
    """(h, w) bool: the pixels of rect = (x0, y0, rw, rh), None the whole image"""
    m = np.zeros((h, w), bool)
    if rect is None:
        m[:] = True
    else:
        x0, y0, rw, rh = rect
        m[y0:y0 + rh, x0:x0 + rw] = True
    return m


def owner_mask(w, h, tiles_x, rank, world):
    """(h, w) bool: the pixels whose 8 x 8 tile t = (j / 8) * tiles_x + i / 8 has t % world == rank"""
    j, i = np.mgrid[0:h, 0:w]
    return ((j // 8) * tiles_x + i // 8) % world == rank


def bin_midpoint(b):
    return np.array([(int(b) << 19) | (1 << 18)], np.uint32).view(F)[0]


def decide(hist, percentile_ppm=DEFAULTS["percentile_ppm"], key=DEFAULTS["key"], gain_min=DEFAULTS["gain_min"], gain_max=DEFAULTS["gain_max"]):
    """dict(metered, bin_ref, y_ref, gain): the counts in Python integers, the gain in float32"""
    counts = [int(v) for v in hist]
    n = sum(counts[16:4080])
    bin_ref, y_ref, g = 0, F(0), F(1)
    if n:
        target = max(1, (n * int(percentile_ppm) + 999999) // 1000000)
        run = 0
        for b in range(16, 4080):
            run += counts[b]
            if run >= target:
                bin_ref = b
                break
        y_ref = bin_midpoint(bin_ref)
        with np.errstate(all="ignore"):
            g = F(F(key) / y_ref)
    g = F(gain_min) if g < F(gain_min) else g
    g = F(gain_max) if g > F(gain_max) else g
    return dict(metered=n, bin_ref=bin_ref, y_ref=F(y_ref), gain=F(g))


def meter(y, mask=None, **cfg):
    """histogram and decision together: what srt_meter_accum / srt_meter_kat report"""
    out = histogram(y, mask)
    d = decide(out["hist"], **cfg)
    assert d["metered"] == out["metered"]
    out.update(d)
    return out


def tone(c, gain, curve=1, white=4.0):
    """the toned XYZ o of XYZ means c (..., 3): c' = g * c; curve 0: o = c'; curve 1: t = y / kw, num = 1 + t, den = 1 + y, s = num / den,
    s = y > 0 ? s : 1, o = s * c' -- kw = white * white formed once, every line one float32 operation"""
    c = np.asarray(c, F)
    g = F(gain)
    with np.errstate(all="ignore"):
        kw = F(F(white) * F(white))
        cp = (g * c).astype(F)
        if curve == 0:
            return cp
        y = cp[..., 1]
        t = (y / kw).astype(F)
        num = (F(1) + t).astype(F)
        den = (F(1) + y).astype(F)
        s = (num / den).astype(F)
        s = np.where(y > 0, s, F(1)).astype(F)
        return (s[..., None] * cp).astype(F)


def clip_counts(o, q, mask=None):
    """dict(blown, crushed, nonfinite) of toned XYZ o (..., 3) and its quantised sRGB q (..., 3), over mask (None: everywhere)"""
    o, q = np.asarray(o, F).reshape(-1, 3), np.asarray(q, F).reshape(-1, 3)
    mask = np.ones(o.shape[0], bool) if mask is None else np.asarray(mask, bool).reshape(-1)
    with np.errstate(all="ignore"):
        nonfinite = ~((o - o) == 0).all(axis=1)
    return dict(blown=int(((q == 255).any(axis=1) & mask).sum()), crushed=int(((q == 0).all(axis=1) & mask).sum()), nonfinite=int((nonfinite & mask).sum()))
