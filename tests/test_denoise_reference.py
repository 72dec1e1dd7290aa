"""The numpy float32 restatement of the denoiser (tests/denoise_reference.py) held to exact arithmetic, without a GPU: so that product
and restatement cannot drift together.  The same cases run on the device in tests/test_denoise.py."""
import numpy as np
import pytest

import denoise_reference as D
from helpers import bits

F = np.float32


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_impulse_response_is_the_integer_convolution(levels):
    S, rows, n = D.impulse_case(45)
    want = D.impulse_expected(45, levels)
    # every value is a multiple of 2^-24 below 1: float32 holds it exactly
    assert (want * F(1 << 24) == np.round(want * F(1 << 24))).all() and want.max() < 1 and (want > 0).sum() == (2 * (2 ** (levels + 1) - 2) + 1) ** 2
    got = D.denoise(S, rows, n, levels=levels, sigma_color=float("inf"), sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    for c in range(3):
        assert np.array_equal(bits(got[..., c]), bits(want)), (levels, c, int((bits(got[..., c]) != bits(want)).sum()))


@pytest.mark.parametrize("kind", D.EDGE_KINDS)
def test_an_edge_in_one_guide_stops_the_impulse(kind):
    S, rows, n, cfg, split = D.edge_case(kind)
    got = D.denoise(S, rows, n, **cfg)
    assert (bits(got[:, split:]) == 0).all(), "%s edge: %d values of the right half are not +0" % (kind, int((bits(got[:, split:]) != 0).sum()))
    left = got[:, :split]
    assert (left > 0).sum() > 3 * 50 and (left[:, split - 1] > 0).any(), "the impulse did not spread up to the edge"
    # ... and without the edge it crosses: the case tests the guide, not the geometry
    flat = D.denoise(S, D.flat_guides(*S.shape[:2]), n, **cfg)
    assert (flat[:, split:] > 0).any()


def test_a_nan_pixel_keeps_its_nan_and_contaminates_no_neighbour():
    S, rows, n = D.impulse_case(21)
    S[...] = F(0.25)
    S[10, 10, 1] = F("nan")
    got = D.denoise(S, rows, n, **D.DEFAULTS)
    nan = np.isnan(got)
    assert nan[10, 10, 1] and nan.sum() == 1, np.argwhere(nan)
    # the pixel's finite channels are its own (every tap of a NaN pixel weighs 0), every other pixel averages equal values
    assert got[10, 10, 0] == F(0.25) and got[10, 10, 2] == F(0.25)
    others = np.ones((21, 21), bool); others[10, 10] = False
    assert (got[others] == F(0.25)).all()
    # ... and so with an infinite colour term (the NaN then comes through dc of the pixel itself only)
    S[10, 10, 1] = F("inf")
    got = D.denoise(S, rows, n, **D.DEFAULTS)
    assert np.isinf(got[10, 10, 1]) and np.isfinite(got[others]).all() and (got[others] == F(0.25)).all()


def test_zero_levels_return_the_mean():
    S, rows, n = D.synthetic_case(9, 7)
    got = D.denoise(S, rows, n, levels=0)
    with np.errstate(all="ignore"):
        want = ((F(1) / F(n)) * S).astype(F)
    assert np.array_equal(bits(got), bits(want))


def test_the_synthetic_input_takes_and_skips_a_quarter_of_its_taps():
    S, rows, n = D.synthetic_case(35, 67)
    hits = rows[..., 7]
    assert (hits == 0).any() and ((hits > 0) & (hits < n)).any() and (hits == n).any()
    assert np.isnan(S).sum() == 1 and np.isinf(S).sum() == 1
    cfg, st = D.pick_sigmas(S, rows, n)
    print(cfg, st)
    assert 4 * st["taken"] >= st["taps"] and 4 * st["skipped"] >= st["taps"]
    # step-16 taps land inside in x only: 2 * 16 < 35 is false for y, true for x
    assert 16 < 35 <= 2 * 16 + 16 and 2 * 16 < 67


def test_the_level_constants_are_float32():
    kn, ka, kz, kc = D.level_constants(3, 1.0, 0.5, 0.25, 0.1)
    assert kn == F(0.25) and ka == F(0.0625) and kz == F(F(0.1) * F(0.1)) and kc == F(1 / 64)
    assert D.level_constants(0, float("inf"), 1, 1, 1)[3] == F("inf")
    assert D.edge_term(F(3), F("inf")) == F(1) and D.edge_term(F("nan"), F(1)) == F(0) and D.edge_term(F("inf"), F("inf")) == F(0)
    assert D.edge_term(F(0.5), F(1)) == F(0.25) and D.edge_term(F(2), F(1)) == F(0)
