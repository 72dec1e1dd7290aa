"""The firefly filter (include/srt_c_api.h at srt_despeckle_accum, csrc/srt_despeckle.hip) restated in numpy float32, operation by
operation: stack the window, np.sort, take_along_axis.  tests/test_despeckle_reference.py holds it to a per-pixel brute force in exact
arithmetic; tests/test_despeckle.py holds the device to it in every bit and every integer.  Also the inputs the two suites share."""
import numpy as np

F = np.float32
INF = F(np.inf)
DEFAULTS = dict(radius=2, rank_ppm=875000, gain=4.0, floor=0.0)
RANKS = (0, 250000, 500000, 875000, 1000000)


def window_offsets(radius):
    """the (dy, dx) of the window in row-major order, the centre left out"""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def canonical_luminance(xyz):
    """v_q of every pixel, +inf where the pixel is no valid neighbour: (Y - Y) == 0 false"""
    Y = np.asarray(xyz, F)[..., 1]
    with np.errstate(all="ignore"):
        valid = (Y - Y) == F(0)
    v = np.where(Y > F(0), Y, F(0)).astype(F)
    return np.where(valid, v, INF).astype(F)


def despeckle(xyz, radius=2, rank_ppm=875000, gain=4.0, floor=0.0):
    """dict(xyz (h, w, 3), scale (h, w), clip = dict(clamped, nonfinite, alone), clamped / nonfinite / alone: the (h, w) class masks,
    m, ref) of the filter on XYZ means xyz (h, w, 3)"""
    c = np.ascontiguousarray(xyz, F)
    assert c.ndim == 3 and c.shape[2] == 3 and radius in (1, 2) and 0 <= rank_ppm <= 1000000, (c.shape, radius, rank_ppm)
    h, w, _ = c.shape
    r = radius
    pad = np.full((h + 2 * r, w + 2 * r), INF, F)
    pad[r:r + h, r:r + w] = canonical_luminance(c)
    win = np.stack([pad[r + dy:r + dy + h, r + dx:r + dx + w] for dy, dx in window_offsets(r)], axis=-1)
    m = (win < INF).sum(axis=-1)
    u = np.sort(win, axis=-1)
    k = (np.maximum(m, 1) - 1).astype(np.uint64) * np.uint64(rank_ppm) // np.uint64(1000000)
    ref = np.take_along_axis(u, k[..., None].astype(np.int64), axis=-1)[..., 0]
    Y = c[..., 1]
    with np.errstate(all="ignore"):
        limit = (F(gain) * ref).astype(F)
        limit = (limit + F(floor)).astype(F)
        finite = ((c - c) == F(0)).all(axis=-1)
        alone = finite & (m == 0)
        clamp = finite & (m != 0) & (Y > limit)
        s = np.where(clamp, (limit / Y).astype(F), F(1)).astype(F)
        o = np.where(clamp[..., None], (s[..., None] * c).astype(F), c).astype(F)
    return dict(xyz=o, scale=s, clip=dict(clamped=int(clamp.sum()), nonfinite=int((~finite).sum()), alone=int(alone.sum())),
                clamped=clamp, nonfinite=~finite, alone=alone, m=m, ref=ref)


def mean_xyz(sums, n):
    """c = inv * S, inv = 1.0f / (float)n; n the sample total or the (h, w) map of the pixels' own counts, where 0 counts as 1"""
    n = np.asarray(n)
    n = np.where(n == 0, 1, n)
    with np.errstate(all="ignore"):
        inv = np.asarray(F(1) / n.astype(F), F)
        return ((inv[..., None] if inv.ndim else inv) * np.asarray(sums, F)).astype(F)


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------
def recipe_image(w, h, seed=0, sprinkle=True):
    """the seeded recipe, (h, w, 3): log-normal noise (sigma 0.5, chromaticity varying), a fifth of the pixels x 64, and -- sprinkle --
    2 % each (at least one each where the image has nine pixels) of NaN, +inf, negated and denormal pixels"""
    rng = np.random.default_rng(9100 + 1000 * h + w + seed)
    n = w * h
    Y = np.exp(rng.normal(0.0, 0.5, n)).astype(F)
    Y[rng.random(n) < 0.2] *= F(64)
    img = np.empty((n, 3), F)
    img[:, 0] = Y * (rng.random(n) * 0.5 + 0.7).astype(F)
    img[:, 1] = Y
    img[:, 2] = Y * (rng.random(n) * 0.9 + 0.3).astype(F)
    if sprinkle and n >= 9:
        cnt = max(1, int(round(0.02 * n)))
        where = rng.permutation(n)[:4 * cnt].reshape(4, cnt)
        img[where[0], rng.integers(0, 3, cnt)] = np.nan
        img[where[1], 1] = np.inf
        img[where[2]] = -img[where[2]]
        img[where[3]] = (img[where[3]] * F(2.0 ** -130)).astype(F)
    elif sprinkle and n >= 2:
        img[n - 1, 1] = np.nan
    return img.reshape(h, w, 3)


def step_edge(h=12, w=14, lo=0.25, hi=40.0):
    """a straight vertical step edge in the middle of the image"""
    img = np.full((h, w, 3), F(lo), F)
    img[:, w // 2:] = F(hi)
    return img


def cluster(count=12, size=15, lo=0.5, hi=900.0):
    """`count` (<= 12) outliers inside the 5 x 5 window at the centre of a size x size constant image; returns (image, mask of the outliers)"""
    assert 1 <= count <= 12 and size >= 11
    img = np.full((size, size, 3), F(lo), F)
    mask = np.zeros((size, size), bool)
    c0 = size // 2 - 2
    for t in np.random.default_rng(31 + count).permutation(25)[:count]:
        mask[c0 + t // 5, c0 + t % 5] = True
    img[mask] = F(hi)
    return img, mask


def bright_line(size=13, lo=0.5, hi=900.0):
    """a one-pixel-wide bright line down the middle column of a size x size constant image; returns (image, mask of the line pixels whose
    5 x 5 window lies inside the image: size - 4 of them, which the line crosses from edge to edge)"""
    img = np.full((size, size, 3), F(lo), F)
    img[:, size // 2] = F(hi)
    inner = np.zeros((size, size), bool)
    inner[2:size - 2, size // 2] = True
    return img, inner
