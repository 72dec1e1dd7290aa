"""The a-trous filter with a K-channel payload (include/srt_c_api.h, srt_denoise_developed) restated in numpy float32 on top of
tests/denoise_reference.py: its prepass, its level constants and its tap_weights, unchanged -- the weights never see the payload --
plus the payload's prepass (d = inv * D), the payload's accumulation inside the same `wt > 0` and its output `sw > 0 ? sd / sw : d_p`.
The develop step itself is tests/develop_reference.py's.  tests/test_denoise_developed_reference.py holds this file to exact
arithmetic; tests/test_denoise_developed.py holds the device to this file, bit for bit."""
import numpy as np

import denoise_reference as D

F = np.float32


def payload_prepass(developed, samples):
    """d = inv * D with the prepass's inv = 1 / n, (h, w, K) float32"""
    P = np.asarray(developed, F)
    assert P.ndim == 3 and P.shape[2] >= 1, P.shape
    with np.errstate(all="ignore"):
        inv = F(1) / F(samples)
        return (inv * P).astype(F)


def filter_level(c, d, N, A, z, i, consts):
    """one level on (colour, payload): the 25 taps, dy outer, dx inner; a tap whose weight is not > 0 multiplies neither"""
    h, w = z.shape
    sw = np.zeros((h, w), F)
    sc = np.zeros((h, w, 3), F)
    sd = np.zeros(d.shape, F)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                py, px, qy, qx, wt = D.tap_weights(c, N, A, z, i, dy, dx, consts)
                take = wt > F(0)
                py, px, qy, qx, wt = py[take], px[take], qy[take], qx[take], wt[take]
                sw[py, px] = (sw[py, px] + wt).astype(F)          # (one tap per pixel per step: the indices are unique)
                sc[py, px] = (sc[py, px] + (wt[:, None] * c[qy, qx]).astype(F)).astype(F)
                sd[py, px] = (sd[py, px] + (wt[:, None] * d[qy, qx]).astype(F)).astype(F)
        live = (sw > F(0))[..., None]
        out_c = np.where(live, (sc / sw[..., None]).astype(F), c).astype(F)
        out_d = np.where(live, (sd / sw[..., None]).astype(F), d).astype(F)
    return out_c, out_d


def denoise_developed(xyz_sums, features, developed, samples, levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1):
    """(the filtered developed mean (h, w, K), the filtered XYZ mean (h, w, 3)), float32"""
    c, N, A, z = D.prepass(xyz_sums, features, samples)
    d = payload_prepass(developed, samples)
    assert d.shape[:2] == z.shape, (d.shape, z.shape)
    for i in range(levels):
        c, d = filter_level(c, d, N, A, z, i, D.level_constants(i, sigma_color, sigma_normal, sigma_albedo, sigma_depth))
    return d, c


def random_payload(h, w, k, seed=0):
    """developed sums for synthetic_case(h, w): K channels of different magnitude, some negative, one -0"""
    rng = np.random.default_rng(9100 + seed + 1000 * h + 10 * w + k)
    P = (rng.uniform(-2.0, 6.0, (h, w, k)) * (1.0 + np.arange(k))).astype(F)
    P[0, 0, k - 1] = F(-0.0)
    return P
