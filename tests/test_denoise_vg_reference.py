"""The numpy float32 restatement of the variance-guided denoiser (tests/denoise_vg_reference.py) held to exact arithmetic, without a
GPU: so that product and restatement cannot drift together.  The same cases run on the device in tests/test_denoise_vg.py."""
import numpy as np
import pytest

import denoise_reference as D
import denoise_vg_reference as V
from helpers import bits

F = np.float32
INF = float("inf")


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(np.ascontiguousarray(a, F)), bits(np.ascontiguousarray(b, F)))


# ---- 1. exact variance ----------------------------------------------------------------------------------------------------------------
def test_the_estimator_gives_the_population_variance_exactly():
    S, rows, n, Y, var = V.integer_variance_case()
    assert var == F(3.9375) and float(np.var(Y.astype(np.float64))) == 3.9375
    xyz, v = V.denoise_vg(S, rows, n, **dict(V.VG_DEFAULTS, levels=0))
    assert same_bits(v[..., 0], np.full((4, 4), var, F)), v[..., 0]
    flat = S.copy()
    flat[..., 1] = F(3)
    _, v = V.denoise_vg(flat, rows, n, **dict(V.VG_DEFAULTS, levels=0))
    assert (bits(v) == 0).all(), "a constant image has variance +0"


# ---- 2. the plain filter is a special case ----------------------------------------------------------------------------------------------
def plain_special_cases():
    for levels in (1, 2, 3):
        S, rows, n = D.impulse_case(45)
        yield "impulse-%d" % levels, S, rows, n, dict(levels=levels, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    for kind in D.EDGE_KINDS:
        S, rows, n, cfg, _ = D.edge_case(kind)
        yield "edge-" + kind, S, rows, n, {k: v for k, v in cfg.items() if k != "sigma_color"}
    for h, w in ((35, 67), (9, 33), (2, 3), (4, 4)):
        S, rows, n = D.synthetic_case(h, w)
        yield "synthetic-%dx%d" % (w, h), S, rows, n, dict(levels=5, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)


PLAIN_SPECIAL_CASES = list(plain_special_cases())


@pytest.mark.parametrize("case", PLAIN_SPECIAL_CASES, ids=[c[0] for c in PLAIN_SPECIAL_CASES])
def test_an_infinite_floor_gives_the_plain_filter(case):
    name, S, rows, n, cfg = case
    want = D.denoise(S, rows, n, sigma_color=INF, **cfg)
    got, _ = V.denoise_vg(S, rows, n, sigma_variance=2.0, variance_floor=INF, **cfg)
    assert same_bits(got, want), (name, int((bits(got) != bits(want)).sum()))
    if name.startswith("impulse"):      # ... so the integer proof of the plain filter's impulse response carries over
        exact = D.impulse_expected(45, cfg["levels"])
        assert all(same_bits(got[..., c], exact) for c in range(3))


# ---- 3. exposure invariance ---------------------------------------------------------------------------------------------------------------
def test_exposure_scales_the_result_exactly_and_the_plain_filter_lacks_that():
    S, rows, n = V.finite_synthetic_case(35, 67)
    cfg = dict(V.VG_DEFAULTS, sigma_variance=1.0)
    floor16 = float(F(16) * F(cfg["variance_floor"]))
    xyz, var = V.denoise_vg(S, rows, n, **cfg)
    xyz4, var16 = V.denoise_vg((F(4) * S).astype(F), rows, n, **dict(cfg, variance_floor=floor16))
    assert np.isfinite(xyz).all() and (var[..., 0] > 0).any() and (bits(xyz) != bits(D.denoise(S, rows, n, levels=0))).any()
    assert same_bits(xyz4, (F(4) * xyz).astype(F)) and same_bits(var16, (F(16) * var).astype(F))
    # the plain filter at a fixed sigma_color filters the brighter picture differently
    pcfg, _ = D.pick_sigmas(*D.synthetic_case(35, 67))
    plain = D.denoise(S, rows, n, levels=5, **pcfg)
    plain4 = D.denoise((F(4) * S).astype(F), rows, n, levels=5, **pcfg)
    assert not same_bits(plain4, (F(4) * plain).astype(F))


# ---- 4. variance propagation ----------------------------------------------------------------------------------------------------------------
def test_one_level_propagates_the_variance_as_the_integer_sums_say():
    S, rows, n, Y, var = V.integer_variance_case()
    assert var == F(63) / F(16)
    _, v = V.denoise_vg(S, rows, n, **dict(V.VG_DEFAULTS, levels=1, variance_floor=INF))
    k = (1, 4, 6, 4, 1)
    want = np.zeros((4, 4), F)
    for y in range(4):
        for x in range(4):
            taps = [k[dy + 2] * k[dx + 2] for dy in range(-2, 3) for dx in range(-2, 3) if 0 <= y + dy < 4 and 0 <= x + dx < 4]
            num, den = 63 * sum(t * t for t in taps), 16 * sum(taps) ** 2      # sum wt^2 v / (sum wt)^2 with wt = t / 256, v = 63 / 16
            assert num < 1 << 24 and den <= 1 << 24
            want[y, x] = F(num) / F(den)      # one correctly rounded division of two exact operands, as in the filter
    assert same_bits(v[..., 0], np.full((4, 4), var, F)) and same_bits(v[..., 1], want), (v[..., 1], want)
    assert (want < var).all()      # averaging lowers the variance


# ---- 5. non-finite pixels -------------------------------------------------------------------------------------------------------------------
def test_non_finite_pixels_keep_their_colour_and_stay_out_of_their_neighbours():
    S, rows, n, bad = V.non_finite_case()
    xyz, var = V.denoise_vg(S, rows, n, **V.VG_DEFAULTS)
    mean = D.denoise(S, rows, n, levels=0)
    good = np.ones(S.shape[:2], bool)
    for y, x in bad:
        good[y, x] = False
        assert same_bits(xyz[y, x], mean[y, x]), "the pixel at %r changed" % ((y, x),)
    assert np.isfinite(xyz[good]).all() and np.isfinite(var).all(), "a neighbour took a non-finite pixel in"
    assert same_bits(var[..., 0], V.non_finite_case_variance(S)), "the estimate is not that of the finite pixels of each window"
    assert (var[..., 0][good] > 0).all()      # ... and in particular not zeroed by a NaN in the window


# ---- 6. levels = 0 ----------------------------------------------------------------------------------------------------------------------------
def test_zero_levels_return_the_mean_and_the_estimate_twice():
    S, rows, n = D.synthetic_case(9, 7)
    xyz, var = V.denoise_vg(S, rows, n, **dict(V.VG_DEFAULTS, levels=0))
    c, N, A, z = D.prepass(S, rows, n)
    with np.errstate(all="ignore"):
        assert same_bits(xyz, ((F(1) / F(n)) * S).astype(F))
    assert same_bits(var[..., 0], var[..., 1]) and same_bits(var[..., 0], V.estimate_variance(c, N, A, z, *V.vg_constants(2.0, 0.5, 0.25, 0.1, 1e-8)[:3]))
    assert (var[..., 0] > 0).any()


# ---- the condition on the synthetic inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(35, 67), (9, 33)])
def test_the_luminance_term_accepts_and_rejects_a_quarter_of_the_guided_taps(h, w):
    S, rows, n = D.synthetic_case(h, w)
    sv, st = V.pick_sigma_variance(S, rows, n)
    print(sv, st)
    assert sv == V.SIGMA_VARIANCE_CANDIDATES[0] == 1.0
    assert st["accepted"] + st["rejected"] == st["taps"] and 4 * st["accepted"] >= st["taps"] and 4 * st["rejected"] >= st["taps"]


def test_the_constants_are_float32():
    kn, ka, kz, ks, vf = V.vg_constants(0.7, 0.5, 0.25, 0.1, 1e-8)
    assert ks == F(F(0.7) * F(0.7)) and vf == F(1e-8) and kn == F(0.25) and ka == F(0.0625) and kz == F(F(0.1) * F(0.1))
    assert V.BLUR == (F(0.25), F(0.5), F(0.25))
    v = np.arange(12, dtype=F).reshape(3, 4)
    b = V.blur_variance(v)
    assert b[1, 1] == F((0 + 2 * 1 + 2 + 2 * 4 + 4 * 5 + 2 * 6 + 8 + 2 * 9 + 10) / 16.0) and b[0, 0] == F((4 * 0 + 2 * 1 + 2 * 4 + 5) / 9.0)
