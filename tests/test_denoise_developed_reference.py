"""The numpy float32 restatement of the payload filter (tests/denoise_developed_reference.py) held to the plain restatement, to exact
rational arithmetic and to the consequences the header draws, without a GPU.  The same cases run on the device in
tests/test_denoise_developed.py."""
from fractions import Fraction

import numpy as np
import pytest

import denoise_developed_reference as DD
import denoise_reference as D
from helpers import bits

F = np.float32
INF = float("inf")


def same_bits(a, b):
    """same bits, or both NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def nearest_f32(q):
    """the float32 nearest to the Fraction q (what one correctly rounded float32 division of exact operands returns); no tie occurs here"""
    f = F(float(q))
    cands = [f, np.nextafter(f, F(-INF)), np.nextafter(f, F(INF))]
    err = [abs(Fraction(float(c)) - q) for c in cands]
    best = min(err)
    assert err.count(best) == 1, "a tie: pick other inputs"
    return cands[err.index(best)]


@pytest.mark.parametrize("levels", [0, 1, 3, 5])
def test_the_xyz_output_is_the_plain_restatement(levels):
    S, rows, n = D.synthetic_case(35, 67)
    cfg, _ = D.pick_sigmas(S, rows, n)
    dev, xyz = DD.denoise_developed(S, rows, DD.random_payload(35, 67, 5), n, levels=levels, **cfg)
    assert dev.shape == (35, 67, 5) and dev.dtype == F
    assert same_bits(xyz, D.denoise(S, rows, n, levels=levels, **cfg))


@pytest.mark.parametrize("k", [3, 7])
def test_a_payload_of_copied_xyz_sums_comes_out_as_the_xyz_output(k):
    S, rows, n = D.synthetic_case(35, 67)
    cfg, _ = D.pick_sigmas(S, rows, n)
    P = np.ascontiguousarray(S[..., [c % 3 for c in range(k)]])
    dev, xyz = DD.denoise_developed(S, rows, P, n, levels=5, **cfg)
    for c in range(k):
        assert same_bits(dev[..., c], xyz[..., c % 3]), c
    assert np.isnan(xyz).sum() == 1 and np.isinf(xyz).sum() == 1


def dyadic_case(h, w, edge):
    """(S, rows, payload (h, w, 2) of whole numbers 0 .. 15, side): equal colour, and with `edge` an albedo step at w // 2 that no tap crosses"""
    rng = np.random.default_rng(77)
    rows = D.flat_guides(h, w)
    side = np.zeros((h, w), np.int64)
    if edge:
        rows[:, w // 2:, 3:6] = F(1.0)
        side[:, w // 2:] = 1
    S = np.full((h, w, 3), F(0.25), F)
    P = rng.integers(0, 16, (h, w, 2)).astype(F)
    return S, rows, P, side


def exact_level(d, side, step):
    """one level in Fractions over a list-of-lists image of Fractions: weights h[dy] h[dx] where tap and pixel lie on one side, else 0;
    returns (sd, sw) per pixel"""
    taps = [Fraction(1, 16), Fraction(1, 4), Fraction(3, 8), Fraction(1, 4), Fraction(1, 16)]
    h, w = side.shape
    out = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            sw, sd = Fraction(0), [Fraction(0)] * len(d[y][x])
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + dy * step, x + dx * step
                    if 0 <= qy < h and 0 <= qx < w and side[qy, qx] == side[y, x]:
                        wt = taps[dy + 2] * taps[dx + 2]
                        sw += wt
                        sd = [a + wt * b for a, b in zip(sd, d[qy][qx])]
            out[y][x] = (sd, sw)
    return out


def test_one_level_equals_exact_arithmetic_on_dyadic_inputs():
    """every product and every sum of the level is exact (weights are multiples of 2^-8, the payload whole numbers below 16): the only
    rounding is the final division, once, which nearest_f32 reproduces from the exact quotient"""
    h, w = 11, 14
    S, rows, P, side = dyadic_case(h, w, edge=True)
    dev, xyz = DD.denoise_developed(S, rows, P, 1, levels=1, sigma_color=INF, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    exact = exact_level([[[Fraction(int(v)) for v in P[y, x]] for x in range(w)] for y in range(h)], side, 1)
    partial = 0
    for y in range(h):
        for x in range(w):
            sd, sw = exact[y][x]
            partial += sw != 1
            for c in range(2):
                assert bits(dev[y, x, c]) == bits(nearest_f32(sd[c] / sw)), (y, x, c)
    assert partial > h * w // 2      # borders and the edge: most pixels divide by a sum that is not 1
    assert (xyz == F(0.25)).all()


def test_two_levels_equal_exact_arithmetic_where_every_operation_is_exact():
    """flat guides, 21 x 21: a pixel at least 6 from the border has sw == 1 in both levels and reads level-1 results that had sw == 1
    too -- multiples of 2^-8 below 16, whose products with the weights are multiples of 2^-16: float32 holds every intermediate"""
    h = w = 21
    S, rows, P, side = dyadic_case(h, w, edge=False)
    dev, _ = DD.denoise_developed(S, rows, P, 1, levels=2, sigma_color=INF, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    l1 = exact_level([[[Fraction(int(v)) for v in P[y, x]] for x in range(w)] for y in range(h)], side, 1)
    l1 = [[[a / sw for a in sd] for sd, sw in row] for row in l1]
    l2 = exact_level(l1, side, 2)
    for y in range(6, h - 6):
        for x in range(6, w - 6):
            sd, sw = l2[y][x]
            assert sw == 1
            for c in range(2):
                assert Fraction(float(dev[y, x, c])) == sd[c], (y, x, c)


def test_an_infinite_payload_at_a_tap_of_zero_weight_does_not_enter():
    S, rows, n, cfg, split = D.edge_case("albedo")
    h, w = S.shape[:2]
    P = np.ones((h, w, 3), F)
    P[:, split:] = F("inf")          # the whole right half: every tap across the edge weighs 0
    P[h // 2, split + 2, 1] = F("nan")
    dev, xyz = DD.denoise_developed(S, rows, P, n, **cfg)
    assert np.isfinite(dev[:, :split]).all() and (dev[:, :split] == F(1)).all()
    assert not np.isfinite(dev[:, split:]).any()
    # 0 * inf would have been NaN: nothing on the left is, and the XYZ output is the plain filter's
    assert same_bits(xyz, D.denoise(S, rows, n, **cfg))


def test_a_nan_colour_pixel_keeps_its_payload_and_contaminates_no_neighbour():
    S, rows, n = D.impulse_case(21)
    S[...] = F(0.25)
    S[10, 10, 1] = F("nan")
    P = np.full((21, 21, 4), F(2.0), F)
    P[10, 10] = (F(7.0), F("nan"), F("inf"), F(-3.0))
    dev, xyz = DD.denoise_developed(S, rows, P, n, **D.DEFAULTS)
    assert same_bits(dev[10, 10], P[10, 10])          # every tap of the pixel weighs 0: it keeps d_p (n = 1: inv * D is D)
    others = np.ones((21, 21), bool); others[10, 10] = False
    assert (dev[others] == F(2.0)).all()
    assert np.isnan(xyz).sum() == 1
    # a payload NaN at a tap that does count propagates as the arithmetic says
    S[10, 10, 1] = F(0.25)
    dev, _ = DD.denoise_developed(S, rows, P, n, levels=1, **{k: v for k, v in D.DEFAULTS.items() if k != "levels"})
    assert np.isnan(dev[8:13, 8:13, 1]).all() and np.isnan(dev[..., 1]).sum() == 25 and np.isfinite(dev[..., 0]).all()


def test_zero_levels_return_inv_times_the_developed_sums():
    S, rows, n = D.synthetic_case(9, 7)
    P = DD.random_payload(9, 7, 5)
    dev, xyz = DD.denoise_developed(S, rows, P, n, levels=0)
    with np.errstate(all="ignore"):
        inv = F(1) / F(n)
        assert same_bits(dev, (inv * P).astype(F)) and same_bits(xyz, (inv * S).astype(F))
    assert bits(dev[0, 0, 4]) == 0x80000000      # -0 stays -0
