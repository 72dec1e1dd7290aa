"""The denoisers on an accumulation whose pixels hold different sample counts (include/srt_c_api.h: the prepass note at
srt_denoise_features, and srt_denoise_features_mv) restated in numpy float32, operation by operation: the per-pixel-count prepass, the
measured estimator -- the variance of the pixel's mean luminance from its own count, Y sum and S2 -- and the three filters driven from
them.  Levels, edge terms and the variance blur are those of tests/denoise_reference.py and tests/denoise_vg_reference.py, reused as they
are.  tests/test_denoise_mv_reference.py holds this file to exact arithmetic; tests/test_denoise_mv.py holds the device to this file."""
from fractions import Fraction

import numpy as np

import denoise_reference as D
import denoise_vg_reference as V

F = np.float32


def prepass_counts(xyz_sums, features, samples):
    """(c, N, A, z) of the prepass with the pixel's own count: inv = 1 / (float)n_p; c = inv * S; N = inv * F[0..2]; A = inv * F[3..5];
    z = F[7] > 0 ? F[6] / F[7] : 0.  samples: (h, w) whole numbers >= 1"""
    S = np.asarray(xyz_sums, F)
    R = np.asarray(features, F)
    n = np.asarray(samples)
    assert S.ndim == 3 and S.shape[2] == 3 and R.shape == S.shape[:2] + (8,) and n.shape == S.shape[:2], (S.shape, R.shape, n.shape)
    assert n.dtype.kind in "iu" and (n >= 1).all()
    with np.errstate(all="ignore"):
        inv = (F(1) / n.astype(F)).astype(F)[..., None]
        c = (inv * S).astype(F)
        N = (inv * R[..., 0:3]).astype(F)
        A = (inv * R[..., 3:6]).astype(F)
        z = np.where(R[..., 7] > F(0), (R[..., 6] / R[..., 7]).astype(F), F(0)).astype(F)
    return c, N, A, z


def measured_variance(sum_y, sum_y2, samples):
    """the measured estimator: mean = S1 / n; v = S2 / n - mean * mean; v = v > 0 ? v : 0; vm = v / (n - 1);
    v_p = (n_p >= 2 && (vm - vm) == 0) ? vm : 0 -- the first four operations of the stopping rule (accum_helpers.converged_f32)"""
    s1, s2, n_i = np.asarray(sum_y, F), np.asarray(sum_y2, F), np.asarray(samples)
    with np.errstate(all="ignore"):
        n = n_i.astype(F)
        mean = (s1 / n).astype(F)
        mm = (mean * mean).astype(F)
        v = ((s2 / n).astype(F) - mm).astype(F)
        v = np.where(v > F(0), v, F(0)).astype(F)
        vm = (v / (n - F(1)).astype(F)).astype(F)
        return np.where((n_i >= 2) & ((vm - vm).astype(F) == F(0)), vm, F(0)).astype(F)


def denoise_counts(xyz_sums, features, samples, levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1):
    """srt_denoise_features on per-pixel counts: the filtered XYZ mean (h, w, 3)"""
    c, N, A, z = prepass_counts(xyz_sums, features, samples)
    for i in range(levels):
        c = D.filter_level(c, N, A, z, i, D.level_constants(i, sigma_color, sigma_normal, sigma_albedo, sigma_depth))
    return c


def _vg_levels(c, N, A, z, v0, levels, consts):
    v = v0
    for i in range(levels):
        c, v = V.filter_level_vg(c, v, N, A, z, i, consts)
    return c, np.stack([v0, v], axis=-1)


def denoise_vg_counts(xyz_sums, features, samples, levels=5, sigma_variance=2.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1,
                      variance_floor=1e-8):
    """srt_denoise_features_vg on per-pixel counts: (xyz (h, w, 3), var (h, w, 2)), the spatial estimator"""
    consts = V.vg_constants(sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor)
    c, N, A, z = prepass_counts(xyz_sums, features, samples)
    return _vg_levels(c, N, A, z, V.estimate_variance(c, N, A, z, *consts[:3]), levels, consts)


def denoise_mv(xyz_sums, features, samples, sum_y2, levels=5, sigma_variance=2.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1,
               variance_floor=1e-8):
    """srt_denoise_features_mv / srt_denoise_mv_kat: (xyz (h, w, 3), var (h, w, 2)), the measured estimator; S1 is xyz_sums[..., 1]"""
    consts = V.vg_constants(sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor)
    c, N, A, z = prepass_counts(xyz_sums, features, samples)
    v0 = measured_variance(np.asarray(xyz_sums, F)[..., 1], sum_y2, samples)
    return _vg_levels(c, N, A, z, v0, levels, consts)


# ---- inputs shared by the CPU and the GPU suite ----------------------------------------------------------------------------------
def nearest_float32(q):
    """the float32 nearest to the Fraction q (q has no tie here: asserted)"""
    with np.errstate(all="ignore"):
        f = F(float(q))
        cands = [f, np.nextafter(f, F(np.inf)), np.nextafter(f, F(-np.inf))]
    err = sorted((abs(Fraction(float(c)) - q), k) for k, c in enumerate(cands) if np.isfinite(c))
    assert len(err) == 1 or err[0][0] < err[1][0], "a tie"
    return cands[err[0][1]]


def integer_measured_case():
    """(xyz_sums, features, samples, sum_y2, per-sample Y lists, variance): a 3 x 4 image of flat guides whose pixel p holds n_p in {1, 2,
    4, 8, 16} small integer samples of Y.  S1 and S2 are integers, n_p is a power of two: mean, mean * mean, S2 / n and their difference
    are exact in float32, so the estimate is ONE rounding of the rational max(S2 / n - (S1 / n)^2, 0) / (n - 1) -- computed here in
    exact rational arithmetic; +0 at n_p = 1."""
    counts = np.array([[2, 4, 8, 16], [16, 2, 1, 4], [8, 8, 2, 16]], np.int64)
    rng = np.random.default_rng(77)
    h, w = counts.shape
    ys = [[[int(v) for v in rng.integers(0, 12, counts[y, x])] for x in range(w)] for y in range(h)]
    ys[2][1] = [5] * 8                      # a constant pixel: variance +0
    S = np.zeros((h, w, 3), F)
    s2 = np.zeros((h, w), F)
    var = np.zeros((h, w), F)
    for y in range(h):
        for x in range(w):
            n, a, b = int(counts[y, x]), sum(ys[y][x]), sum(v * v for v in ys[y][x])
            S[y, x] = (F(0.5 * n), F(a), F(0.25 * n))
            s2[y, x] = F(b)
            v = Fraction(b, n) - Fraction(a, n) ** 2
            assert v >= 0 and v.denominator <= 256 and v.numerator < 1 << 16      # exact in float32, like every step before it
            var[y, x] = nearest_float32(v / (n - 1)) if n >= 2 else F(0)
    return S, D.flat_guides(h, w) * counts.astype(F)[..., None], counts.astype(np.uint32), s2, ys, var


def varying_case(h, w, seed=0, finite=False):
    """(xyz_sums, features, samples, sum_y2): D.synthetic_case (its NaN and its inf pixel included unless `finite`) re-dressed as an
    adaptive accumulation -- a per-pixel count in 1 .. 24 with n_p = 1 and n_p = 2 present when there is room, sums and rows scaled to the
    pixel's count, and an S2 that leaves a variance of every size: zero (S2 = S1^2 / n, rounded down), small and large"""
    S, rows, n0 = V.finite_synthetic_case(h, w, seed) if finite else D.synthetic_case(h, w, seed)
    rng = np.random.default_rng(9100 + seed + 1000 * h + w)
    n = rng.integers(2, 25, (h, w)).astype(np.uint32)
    flat = n.reshape(-1)
    flat[rng.integers(0, flat.size)] = 2
    if flat.size >= 3:
        flat[0], flat[-1] = 2, 1
    scale = (n.astype(F) / F(n0)).astype(F)[..., None]
    S = (S * scale).astype(F)
    rows = (rows * scale).astype(F)
    with np.errstate(all="ignore"):
        mean_sq = (S[..., 1] * S[..., 1] / n.astype(F)).astype(F)
        s2 = (mean_sq * rng.choice(np.array([0.999, 1.0, 1.05, 1.5, 4.0], F), (h, w))).astype(F)
    if not finite and flat.size >= 12:
        s2[h // 2, w // 2] = F("inf")       # an S2 that overflowed: the estimate there is +0
    return S, rows, n, s2
