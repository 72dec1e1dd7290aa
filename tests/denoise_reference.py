"""The a-trous denoiser (include/srt_c_api.h, srt_denoise_features) restated in numpy float32, operation by operation: every product,
sum, quotient and select in the order the header gives, each rounded once, selects as np.where (np.maximum's NaN rules differ).
Vectorised over the pixels with one loop over the 25 taps.  tests/test_denoise_reference.py holds this file to exact arithmetic;
tests/test_denoise.py holds the device to this file, bit for bit.  Also the synthetic inputs both suites share."""
import numpy as np

F = np.float32
TAPS = (F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16))      # B3 spline, exact in float32
DEFAULTS = dict(levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)


def edge_term(d2, k):
    """e(d2, k): t = 1 - d2 / k; t = t > 0 ? t : 0; t * t   (NaN gives 0, an infinite k gives 1)"""
    with np.errstate(all="ignore"):
        t = (F(1) - np.asarray(d2 / k, F)).astype(F)
        t = np.where(t > F(0), t, F(0)).astype(F)
        return (t * t).astype(F)


def dist2(a, b):
    """(a.x - b.x)^2 + (a.y - b.y)^2 + (a.z - b.z)^2, left to right"""
    d = (a - b).astype(F)
    sq = (d * d).astype(F)
    return ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)


def prepass(xyz_sums, features, samples):
    """(c, N, A, z) of the prepass: inv = 1 / n; c = inv * S; N = inv * F[0..2]; A = inv * F[3..5]; z = F[7] > 0 ? F[6] / F[7] : 0"""
    S = np.asarray(xyz_sums, F)
    R = np.asarray(features, F)
    assert S.ndim == 3 and S.shape[2] == 3 and R.shape == S.shape[:2] + (8,), (S.shape, R.shape)
    with np.errstate(all="ignore"):
        inv = F(1) / F(samples)
        c = (inv * S).astype(F)
        N = (inv * R[..., 0:3]).astype(F)
        A = (inv * R[..., 3:6]).astype(F)
        z = np.where(R[..., 7] > F(0), (R[..., 6] / R[..., 7]).astype(F), F(0)).astype(F)
    return c, N, A, z


def level_constants(i, sigma_color, sigma_normal, sigma_albedo, sigma_depth):
    """(kn, ka, kz, kc) of level i, computed in float32: kc from sigma_color * 2^-i"""
    with np.errstate(all="ignore"):
        sn, sa, sz = F(sigma_normal), F(sigma_albedo), F(sigma_depth)
        sc = np.ldexp(F(sigma_color), -i).astype(F)
        return F(sn * sn), F(sa * sa), F(sz * sz), F(sc * sc)


def tap_weights(c, N, A, z, i, dy, dx, consts):
    """For tap (dy, dx) of level i (step 1 << i) over the whole image: (inside, py, px, qy, qx, wt) -- wt the float32 weight of every
    pixel p = (py, px) whose tap q = (qy, qx) lies inside the rectangle, as flat index arrays."""
    h, w = z.shape
    s = 1 << i
    kn, ka, kz, kc = consts
    ys, xs = np.mgrid[0:h, 0:w]
    qy, qx = ys + dy * s, xs + dx * s
    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    py, px, qy, qx = ys[inside], xs[inside], qy[inside], qx[inside]
    with np.errstate(all="ignore"):
        dn = dist2(N[py, px], N[qy, qx])
        da = dist2(A[py, px], A[qy, qx])
        dc = dist2(c[py, px], c[qy, qx])
        zp, zq = z[py, px], z[qy, qx]
        m = np.where(zp > zq, zp, zq).astype(F)
        r = np.where(m > F(0), ((zp - zq).astype(F) / m).astype(F), F(0)).astype(F)
        dz = (r * r).astype(F)
        wt = np.full(py.shape, F(TAPS[dy + 2] * TAPS[dx + 2]), F)
        wt = (wt * edge_term(dn, kn)).astype(F)
        wt = (wt * edge_term(da, ka)).astype(F)
        wt = (wt * edge_term(dz, kz)).astype(F)
        wt = (wt * edge_term(dc, kc)).astype(F)
    return py, px, qy, qx, wt


def filter_level(c, N, A, z, i, consts, stats=None):
    """one level: the accumulation over the 25 taps, dy outer, dx inner.  stats (a dict): counts of the in-rectangle non-centre taps
    with wt > 0 / wt == 0 are added under "taken" / "skipped"."""
    h, w = z.shape
    sw = np.zeros((h, w), F)
    sc = np.zeros((h, w, 3), F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                py, px, qy, qx, wt = tap_weights(c, N, A, z, i, dy, dx, consts)
                take = wt > F(0)
                if stats is not None and (dy or dx):
                    stats["taken"] = stats.get("taken", 0) + int(take.sum())
                    stats["skipped"] = stats.get("skipped", 0) + int((wt == F(0)).sum())
                    stats["taps"] = stats.get("taps", 0) + int(wt.size)
                py, px, qy, qx, wt = py[take], px[take], qy[take], qx[take], wt[take]
                sw[py, px] = (sw[py, px] + wt).astype(F)          # (one tap per pixel per step: the indices are unique)
                sc[py, px] = (sc[py, px] + (wt[:, None] * c[qy, qx]).astype(F)).astype(F)
        out = np.where((sw > F(0))[..., None], (sc / sw[..., None]).astype(F), c).astype(F)
    return out


def denoise(xyz_sums, features, samples, levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1, stats=None):
    """the filtered XYZ mean (h, w, 3) float32.  stats: a list that receives one dict per level (filter_level)."""
    c, N, A, z = prepass(xyz_sums, features, samples)
    for i in range(levels):
        st = {} if stats is not None else None
        c = filter_level(c, N, A, z, i, level_constants(i, sigma_color, sigma_normal, sigma_albedo, sigma_depth), st)
        if stats is not None:
            stats.append(st)
    return c


# ---- inputs shared by the CPU and the GPU suite ----------------------------------------------------------------------------------
def flat_guides(h, w, samples=1, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.5, 0.5), distance=4.0):
    """feature sums of an image whose every sample hit one surface: all guides equal"""
    rows = np.zeros((h, w, 8), F)
    rows[..., 0:3] = F(samples) * np.asarray(normal, F)
    rows[..., 3:6] = F(samples) * np.asarray(albedo, F)
    rows[..., 6] = F(samples) * F(distance)
    rows[..., 7] = F(samples)
    return rows


def impulse_case(size=45):
    """(xyz_sums, features, samples): a single 1.0 (all three channels) at the centre of a size x size image of equal guides"""
    S = np.zeros((size, size, 3), F)
    S[size // 2, size // 2] = F(1)
    return S, flat_guides(size, size), 1


def impulse_expected(size, levels):
    """the impulse response in exact arithmetic: the convolution of the dilated B3 kernels [1, 4, 6, 4, 1] / 16 (separable), computed
    in integers over 2^(8 levels), as float32 (exact: every value is a multiple of 2^-24 below 1 for levels <= 3)"""
    img = np.zeros((size, size), object)
    img[size // 2, size // 2] = 1
    k = (1, 4, 6, 4, 1)
    for i in range(levels):
        s = 1 << i
        nxt = np.zeros((size, size), object)
        for y in range(size):
            for x in range(size):
                if img[y, x]:
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qy, qx = y + dy * s, x + dx * s
                            assert 0 <= qy < size and 0 <= qx < size, "the footprint left the image"
                            nxt[qy, qx] += img[y, x] * k[dy + 2] * k[dx + 2]
        img = nxt
    den = 1 << (8 * levels)
    assert den <= 1 << 24
    out = np.array([[F(int(v)) / F(den) for v in row] for row in img], F)
    assert int(sum(int(v) for v in img.ravel())) == den
    return out


EDGE_KINDS = ("normal", "albedo", "depth", "coverage")


def edge_case(kind, h=21, w=40):
    """(xyz_sums, features, samples, cfg, split): the left half [0, split) and the right half differ in one guide by more than its sigma
    allows (normal (0,0,1) | (1,0,0) at sigma_normal 0.5; albedo 0.5 | 1.0 at 0.25; distance 4 | 8, relative step 0.5, at 0.1; hit |
    miss), an impulse three pixels left of the edge, sigma_color = inf: the right half must stay exactly +0."""
    assert kind in EDGE_KINDS
    split = w // 2
    rows = flat_guides(h, w)
    right = rows[:, split:]
    if kind == "normal":
        right[..., 0:3] = np.asarray((1.0, 0.0, 0.0), F)
    elif kind == "albedo":
        right[..., 3:6] = F(1.0)
    elif kind == "depth":
        right[..., 6] = F(8.0)
    else:
        right[...] = F(0)      # every sample missed: zero normal, zero albedo, no distance
    S = np.zeros((h, w, 3), F)
    S[h // 2, split - 3] = F(1)
    return S, rows, 1, dict(DEFAULTS, levels=3, sigma_color=float("inf")), split


def synthetic_case(h, w, seed=0):
    """(xyz_sums, features, samples): random guides in patches (so that neighbours often agree and often do not), zero-hit pixels, partly
    covered pixels, one NaN pixel and one inf pixel (when the image has room for them)"""
    rng = np.random.default_rng(4200 + seed + 1000 * h + w)
    n = 8
    ph, pw = (h + 5) // 6, (w + 5) // 6
    def patches(vals):
        idx = rng.integers(0, len(vals), (ph, pw))
        return np.asarray(vals, F)[np.kron(idx, np.ones((6, 6), np.int64))[:h, :w]]
    normals = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0.6, 0, 0.8), (0, -0.6, 0.8)]
    albedos = [(0.73, 0.73, 0.73), (0.5, 0.5, 0.5), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15)]
    dist = patches([2.0, 2.1, 4.0, 7.5])
    hits = patches([0.0, 3.0, 8.0, 8.0, 8.0]) if h * w > 1 else np.full((h, w), 8.0, F)
    rows = np.zeros((h, w, 8), F)
    jitter = (1.0 + 0.02 * rng.standard_normal((h, w))).astype(F)
    rows[..., 0:3] = (hits[..., None] * patches(normals) * jitter[..., None]).astype(F)
    rows[..., 3:6] = (hits[..., None] * patches(albedos)).astype(F)
    rows[..., 6] = (hits * dist * jitter).astype(F)
    rows[..., 7] = hits
    S = (F(n) * rng.uniform(0.05, 0.6, (h, w, 3))).astype(F)
    if h * w >= 6:
        S[h // 3, w // 3, 1] = F("nan")
        S[(2 * h) // 3, (2 * w) // 3, 0] = F("inf")
    return S, rows, n


def pick_sigmas(S, rows, n):
    """sigmas for synthetic_case under which level 0 both takes and skips at least a quarter of its in-rectangle non-centre taps; picked
    on the restatement alone (the first of a fixed list that qualifies)"""
    for sc in (0.5, 0.35, 0.25, 0.7, 1.0):
        cfg = dict(sigma_color=sc, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
        st = []
        denoise(S, rows, n, levels=1, stats=st, **cfg)
        if 4 * st[0]["taken"] >= st[0]["taps"] and 4 * st[0]["skipped"] >= st[0]["taps"]:
            return cfg, st[0]
    raise AssertionError("no sigma set takes and skips a quarter of the taps each")
