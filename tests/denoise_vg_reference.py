"""The variance-guided a-trous denoiser (include/srt_c_api.h, srt_denoise_features_vg) restated in numpy float32, operation by
operation, in the order the header gives: the spatial variance estimator, the 3x3 blur of the variance, the level with its luminance
term and the variance it carries.  Edge term, distances, prepass and the shared inputs are those of tests/denoise_reference.py.
tests/test_denoise_vg_reference.py holds this file to exact arithmetic; tests/test_denoise_vg.py holds the device to this file."""
import numpy as np

from denoise_reference import F, TAPS, dist2, edge_term, prepass

VG_DEFAULTS = dict(levels=5, sigma_variance=2.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1, variance_floor=1e-8)
BLUR = (F(1) / F(4), F(1) / F(2), F(1) / F(4))      # the variance's 3x3 blur, exact in float32
SIGMA_VARIANCE_CANDIDATES = (1.0, 0.7, 1.5, 2.0, 0.5)


def vg_constants(sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor):
    """(kn, ka, kz, ks, floor), computed in float32: ks = sigma_variance * sigma_variance, formed once"""
    with np.errstate(all="ignore"):
        sn, sa, sz, sv = F(sigma_normal), F(sigma_albedo), F(sigma_depth), F(sigma_variance)
        return F(sn * sn), F(sa * sa), F(sz * sz), F(sv * sv), F(variance_floor)


def taps_inside(h, w, dy, dx):
    """(py, px, qy, qx): every pixel p whose tap q = p + (dy, dx) lies inside the rectangle"""
    ys, xs = np.mgrid[0:h, 0:w]
    qy, qx = ys + dy, xs + dx
    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    return ys[inside], xs[inside], qy[inside], qx[inside]


def guide_terms(N, A, z, py, px, qy, qx, kn, ka, kz):
    """(e(dn, kn), e(da, ka), e(dz, kz)) of the taps"""
    with np.errstate(all="ignore"):
        dn = dist2(N[py, px], N[qy, qx])
        da = dist2(A[py, px], A[qy, qx])
        zp, zq = z[py, px], z[qy, qx]
        m = np.where(zp > zq, zp, zq).astype(F)
        r = np.where(m > F(0), ((zp - zq).astype(F) / m).astype(F), F(0)).astype(F)
        dz = (r * r).astype(F)
        return edge_term(dn, kn), edge_term(da, ka), edge_term(dz, kz)


def estimate_variance(c, N, A, z, kn, ka, kz):
    """the estimator: the guide-weighted variance of Y over the 7x7 window, dy outer, dx inner; taps with a non-finite Y do not count"""
    h, w = z.shape
    s0, s1, s2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                py, px, qy, qx = taps_inside(h, w, dy, dx)
                en, ea, ez = guide_terms(N, A, z, py, px, qy, qx, kn, ka, kz)
                g = en
                g = (g * ea).astype(F)
                g = (g * ez).astype(F)
                Y = c[qy, qx, 1]
                take = (g > F(0)) & ((Y - Y).astype(F) == F(0))
                py, px, g, Y = py[take], px[take], g[take], Y[take]
                s0[py, px] = (s0[py, px] + g).astype(F)
                s1[py, px] = (s1[py, px] + (g * Y).astype(F)).astype(F)
                s2[py, px] = (s2[py, px] + (g * (Y * Y).astype(F)).astype(F)).astype(F)
        mu = (s1 / s0).astype(F)
        m2 = (s2 / s0).astype(F)
        v = (m2 - (mu * mu).astype(F)).astype(F)
        return np.where((s0 > F(0)) & (v > F(0)), v, F(0)).astype(F)


def blur_variance(v):
    """vb = sum k v_q / sum k over the 3x3 neighbours at distance 1 inside the rectangle, k = {1/4, 1/2, 1/4}^2, dy outer"""
    h, w = v.shape
    sk, sv = np.zeros((h, w), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                py, px, qy, qx = taps_inside(h, w, dy, dx)
                k = F(BLUR[dy + 1] * BLUR[dx + 1])
                sk[py, px] = (sk[py, px] + k).astype(F)
                sv[py, px] = (sv[py, px] + (k * v[qy, qx]).astype(F)).astype(F)
        return (sv / sk).astype(F)


def filter_level_vg(c, v, N, A, z, i, consts, stats=None):
    """one level at step 1 << i on (c, v) -> (c, v).  stats (a dict): over the in-rectangle non-centre taps whose three guide terms are
    > 0, the counts "accepted" / "rejected" by the luminance term e(dl, kc_p) and their total "taps"."""
    h, w = z.shape
    s = 1 << i
    kn, ka, kz, ks, floor = consts
    sw, sv = np.zeros((h, w), F), np.zeros((h, w), F)
    sc = np.zeros((h, w, 3), F)
    with np.errstate(all="ignore"):
        kc = ((ks * blur_variance(v)).astype(F) + floor).astype(F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                py, px, qy, qx = taps_inside(h, w, dy * s, dx * s)
                en, ea, ez = guide_terms(N, A, z, py, px, qy, qx, kn, ka, kz)
                d = (c[py, px, 1] - c[qy, qx, 1]).astype(F)
                el = edge_term((d * d).astype(F), kc[py, px])
                dc = dist2(c[py, px], c[qy, qx])
                wt = np.full(py.shape, F(TAPS[dy + 2] * TAPS[dx + 2]), F)
                wt = (wt * en).astype(F)
                wt = (wt * ea).astype(F)
                wt = (wt * ez).astype(F)
                wt = (wt * el).astype(F)
                if stats is not None and (dy or dx):
                    guided = (en > F(0)) & (ea > F(0)) & (ez > F(0))
                    stats["taps"] = stats.get("taps", 0) + int(guided.sum())
                    stats["accepted"] = stats.get("accepted", 0) + int((guided & (el > F(0))).sum())
                    stats["rejected"] = stats.get("rejected", 0) + int((guided & (el == F(0))).sum())
                take = (wt > F(0)) & ((dc - dc).astype(F) == F(0))
                py, px, qy, qx, wt = py[take], px[take], qy[take], qx[take], wt[take]
                sw[py, px] = (sw[py, px] + wt).astype(F)
                sc[py, px] = (sc[py, px] + (wt[:, None] * c[qy, qx]).astype(F)).astype(F)
                sv[py, px] = (sv[py, px] + ((wt * wt).astype(F) * v[qy, qx]).astype(F)).astype(F)
        ok = sw > F(0)
        out_c = np.where(ok[..., None], (sc / sw[..., None]).astype(F), c).astype(F)
        out_v = np.where(ok, (sv / (sw * sw).astype(F)).astype(F), v).astype(F)
    return out_c, out_v


def denoise_vg(xyz_sums, features, samples, levels=5, sigma_variance=2.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1,
               variance_floor=1e-8, stats=None, variance=None):
    """(xyz (h, w, 3), var (h, w, 2)) float32: the filtered XYZ mean; the estimator's variance and the variance after the last level.
    stats: a list that receives one dict per level (filter_level_vg).  variance: an (h, w) image that replaces the estimator's (the
    propagation test feeds a known one)."""
    consts = vg_constants(sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor)
    c, N, A, z = prepass(xyz_sums, features, samples)
    v0 = estimate_variance(c, N, A, z, *consts[:3]) if variance is None else np.asarray(variance, F)
    v = v0
    for i in range(levels):
        st = {} if stats is not None else None
        c, v = filter_level_vg(c, v, N, A, z, i, consts, st)
        if stats is not None:
            stats.append(st)
    return c, np.stack([v0, v], axis=-1)


def pick_sigma_variance(S, rows, n):
    """(sigma_variance, level-0 stats): the first of SIGMA_VARIANCE_CANDIDATES under which, at variance_floor 1e-8, level 0's luminance
    term both accepts and rejects at least a quarter of the in-rectangle non-centre taps whose guide terms are > 0"""
    for sv in SIGMA_VARIANCE_CANDIDATES:
        st = []
        denoise_vg(S, rows, n, **dict(VG_DEFAULTS, levels=1, sigma_variance=sv), stats=st)
        if 4 * st[0]["accepted"] >= st[0]["taps"] and 4 * st[0]["rejected"] >= st[0]["taps"]:
            return sv, st[0]
    raise AssertionError("no sigma_variance accepts and rejects a quarter of the guided taps each")


def finite_synthetic_case(h, w, seed=0):
    """synthetic_case with its NaN and its inf pixel replaced by finite values"""
    from denoise_reference import synthetic_case
    S, rows, n = synthetic_case(h, w, seed)
    S = np.where(np.isfinite(S), S, F(1.5)).astype(F)
    return S, rows, n


def integer_variance_case():
    """(xyz_sums, features, samples, Y, variance): a 4 x 4 image of small integer Y with flat guides -- every pixel's 7x7 window is the
    whole image, every g is 1 and s0 = 16 -- and its population variance, exact in float32"""
    from denoise_reference import flat_guides
    Y = np.array([[1, 2, 3, 4], [2, 5, 1, 0], [7, 3, 3, 2], [0, 1, 6, 4]], np.int64)
    S = np.zeros((4, 4, 3), F)
    S[..., 0] = F(0.5)
    S[..., 1] = Y.astype(F)
    S[..., 2] = F(0.25)
    s1, s2 = int(Y.sum()), int((Y * Y).sum())
    var = F(s2) / F(16) - (F(s1) / F(16)) * (F(s1) / F(16))      # every step exact: multiples of 2^-8 far below 2^24
    assert float(var) == (16 * s2 - s1 * s1) / 256.0
    return S, flat_guides(4, 4), 1, Y, F(var)


def non_finite_case(h=9, w=11):
    """(xyz_sums, features, samples, bad): small integer Y on flat guides (every g is 1, every sum exact), X = 0.5, Z = 0.25, and three
    non-finite pixels `bad`: a NaN in Y, an inf in Y, and an inf in X next to a finite Y (which only the level's (dc - dc) clause sees)"""
    from denoise_reference import flat_guides
    ys, xs = np.mgrid[0:h, 0:w]
    S = np.zeros((h, w, 3), F)
    S[..., 0] = F(0.5)
    S[..., 1] = ((3 * ys + 5 * xs + (xs * ys) % 4) % 8 + 1).astype(F)
    S[..., 2] = F(0.25)
    S[2, 2, 1] = F("nan")
    S[7, 2, 1] = F("inf")
    S[6, 7, 0] = F("inf")
    return S, flat_guides(h, w), 1, ((2, 2), (7, 2), (6, 7))


def non_finite_case_variance(S):
    """the estimator's result on non_finite_case from integer sums over the finite Y of every 7x7 window: three exact float32 operands
    and the estimator's four last operations"""
    h, w = S.shape[:2]
    Y = S[..., 1]
    out = np.zeros((h, w), F)
    for y in range(h):
        for x in range(w):
            win = [int(Y[qy, qx]) for qy in range(max(0, y - 3), min(h, y + 4)) for qx in range(max(0, x - 3), min(w, x + 4)) if np.isfinite(Y[qy, qx])]
            s0, s1, s2 = F(len(win)), F(sum(win)), F(sum(v * v for v in win))
            mu, m2 = F(s1 / s0), F(s2 / s0)
            v = F(m2 - F(mu * mu))
            out[y, x] = v if v > 0 else F(0)
    return out
