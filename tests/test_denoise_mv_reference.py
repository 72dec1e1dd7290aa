"""tests/denoise_mv_reference.py held to exact arithmetic and to the restatements it extends, without a GPU: the measured estimator on
integer samples against exact rational arithmetic, its guards, its identity with the stopping rule's first four operations, the +inf
floor identity, and a uniform sample map giving what the scalar-count restatements give."""
from fractions import Fraction

import numpy as np

import denoise_mv_reference as M
import denoise_reference as D
import denoise_vg_reference as V
from accum_helpers import converged_f32
from helpers import bits

F = np.float32
INF = float("inf")


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def test_estimator_equals_exact_rational_arithmetic():
    S, rows, n, s2, ys, var = M.integer_measured_case()
    got = M.measured_variance(S[..., 1], s2, n)
    assert same(got, var), (got, var)
    assert set(np.unique(n)) >= {1, 2, 4, 8, 16}
    assert not bits(got[n == 1]).any() and not bits(got[2, 1]).any() and (got[(n >= 2)] > 0).sum() >= 8
    # ... and the rational value is the unbiased sample variance over n: the variance of the mean
    for y in range(n.shape[0]):
        for x in range(n.shape[1]):
            k = int(n[y, x])
            if k >= 2:
                mean = Fraction(sum(ys[y][x]), k)
                exact = sum((Fraction(v) - mean) ** 2 for v in ys[y][x]) / (k - 1) / k
                assert abs(Fraction(float(got[y, x])) - exact) <= abs(exact) * Fraction(1, 1 << 23), (y, x)
    # levels 0 returns the per-pixel mean and the estimate in both channels
    xyz, v = M.denoise_mv(S, rows, n, s2, levels=0)
    assert same(xyz[..., 1], (S[..., 1] / n.astype(F)).astype(F)) and same(xyz[..., 0], np.full(n.shape, F(0.5)))
    assert same(v[..., 0], var) and same(v[..., 1], var)


def test_estimator_guards():
    n = np.array([1, 2, 3, 4, 5, 6], np.uint32)
    s1 = np.array([3, F("nan"), 3, F("inf"), 2, 4], F)
    s2 = np.array([9, 1, F("inf"), 1, 0.5, F("nan")], F)
    got = M.measured_variance(s1, s2, n)
    assert not bits(got[[0, 1, 2, 3, 5]]).any(), got           # one sample; NaN and inf sums: +0, never NaN
    assert got[4] == 0 and not np.signbit(got[4])               # S2 / n < mean^2 (rounding): clamped to +0
    assert np.isfinite(M.measured_variance(F(3e38), F(3e38), np.uint32(2)))
    assert M.measured_variance(F(2), F(3e38), np.uint32(2)) > 0


def test_estimator_is_the_stopping_rules_var_mean():
    """converged(S1, S2, n, tol) with rel_tol = 0 is var_mean <= abs_tol^2: bracketing the estimate between two float32 thresholds shows
    that it is the number the sampler compares"""
    rng = np.random.default_rng(5)
    n = rng.integers(2, 40, 500)
    s1 = (rng.uniform(0.1, 3.0, 500) * n).astype(F)
    s2 = (s1 * s1 / n.astype(F) * rng.uniform(1.0, 3.0, 500)).astype(F)
    vm = M.measured_variance(s1, s2, n)
    assert (vm > 0).sum() > 400
    for k in np.flatnonzero(vm > F(1e-12))[:200]:
        tol = F(np.sqrt(np.float64(vm[k])))
        lo, hi = tol, tol
        while F(lo * lo) > vm[k]:
            lo = np.nextafter(lo, F(0))
        while F(hi * hi) < vm[k]:
            hi = np.nextafter(hi, F(np.inf))
        if F(lo * lo) < vm[k]:
            assert not converged_f32(s1[k], s2[k], n[k], 2, 0.0, lo), k
        assert converged_f32(s1[k], s2[k], n[k], 2, 0.0, hi), k


def test_a_uniform_sample_map_gives_the_scalar_restatements():
    for h, w in ((9, 33), (3, 2), (1, 1)):
        S, rows, n = D.synthetic_case(h, w)
        full = np.full((h, w), n, np.uint32)
        for a, b in zip(M.prepass_counts(S, rows, full), D.prepass(S, rows, n)):
            assert same(a, b)
        assert same(M.denoise_counts(S, rows, full, levels=3), D.denoise(S, rows, n, levels=3))
        got, want = M.denoise_vg_counts(S, rows, full, levels=3), V.denoise_vg(S, rows, n, levels=3)
        assert same(got[0], want[0]) and same(got[1], want[1])
    # ... and a varying one does not: the per-pixel count is read
    S, rows, n, s2 = M.varying_case(9, 33)
    assert len(np.unique(n)) > 5 and (n == 1).any() and (n == 2).any()
    assert not same(M.prepass_counts(S, rows, n)[0], D.prepass(S, rows, 8)[0])


def test_an_infinite_floor_gives_the_plain_filter():
    for h, w in ((35, 67), (9, 33), (2, 3)):
        S, rows, n, s2 = M.varying_case(h, w)
        cfg = dict(levels=4, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
        got, var = M.denoise_mv(S, rows, n, s2, variance_floor=INF, **cfg)
        assert same(got, M.denoise_counts(S, rows, n, sigma_color=INF, **cfg)), (h, w)
        assert np.isfinite(var).all()


def test_exposure_invariance_of_the_restatement():
    S, rows, n, s2 = M.varying_case(9, 33, finite=True)
    cfg = dict(V.VG_DEFAULTS, sigma_variance=1.0)
    xyz, var = M.denoise_mv(S, rows, n, s2, **cfg)
    xyz4, var16 = M.denoise_mv((F(4) * S).astype(F), rows, n, (F(16) * s2).astype(F), **dict(cfg, variance_floor=float(F(16) * F(cfg["variance_floor"]))))
    assert same(xyz4, (F(4) * xyz).astype(F)) and same(var16, (F(16) * var).astype(F))
    assert (var[..., 0] > 0).any() and (bits(var[..., 0]) != bits(var[..., 1])).any()
    # the measured estimate steers the filter: another S2, another picture
    other, _ = M.denoise_mv(S, rows, n, (F(9) * s2).astype(F), **cfg)
    assert not same(other, xyz)
