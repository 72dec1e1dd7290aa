"""tests/develop_reference.py (the float32 restatement of srt_develop_spectral) against exact arithmetic, without a GPU: exact where every
operation is exact, within the a-priori rounding bound of a float64 contraction elsewhere, and sensitive to the order of the sum."""
from fractions import Fraction

import numpy as np

from develop_reference import CIE_SCALE, N_GRID, develop, normalise, one_hot
from helpers import bits

F = np.float32


def _exact(film, resp, scale):
    out = []
    for row in film:
        out.append([sum((Fraction(float(row[j])) * Fraction(float(r[j])) for j in range(N_GRID)), Fraction(0)) * Fraction(float(scale)) for r in resp])
    return out


def test_equals_exact_rational_arithmetic_where_every_operation_is_exact():
    """small integers: products below 2^9 and sums below 2^16; scaled powers of two: every term a multiple of 2^-4 below 2^8, every sum
    below 2^15 -- 19 significant bits at most, so no fp32 operation rounds"""
    rng = np.random.default_rng(5)
    cases = [(rng.integers(0, 64, (7, N_GRID)).astype(F), rng.integers(-8, 9, (5, N_GRID)).astype(F), F(1)),
             (rng.integers(0, 64, (7, N_GRID)).astype(F), rng.integers(-8, 9, (16, N_GRID)).astype(F), F(-0.25)),
             ((rng.integers(0, 16, (6, N_GRID)) * 2.0 ** rng.integers(-2, 3, (6, N_GRID))).astype(F),
              (rng.choice([-1.0, 1.0], (3, N_GRID)) * 2.0 ** rng.integers(-2, 3, (3, N_GRID))).astype(F), F(8))]
    for film, resp, scale in cases:
        got = develop(film, resp, scale)
        want = _exact(film, resp, scale)
        assert got.shape == (film.shape[0], resp.shape[0]) and got.dtype == F
        for p in range(film.shape[0]):
            for k in range(resp.shape[0]):
                assert Fraction(float(got[p, k])) == want[p][k], (p, k)
    # a (95,) response is one channel, and a 96th word of the row never enters
    film96 = np.concatenate([cases[0][0], np.full((7, 1), np.nan, F)], axis=1)
    assert np.array_equal(bits(develop(film96, cases[0][1][0])), bits(develop(cases[0][0], cases[0][1][:1])))


def test_one_hot_responses_return_the_film():
    rng = np.random.default_rng(6)
    film = (rng.random((9, N_GRID)) * 10.0 ** rng.integers(-30, 30, (9, N_GRID))).astype(F)
    film[0, 3] = 0.0
    for first, count in ((0, 16), (80, 15), (94, 1)):
        assert np.array_equal(bits(develop(film, one_hot(first, count))), bits(film[:, first:first + count]))


def test_within_the_a_priori_bound_of_a_float64_contraction():
    """non-negative terms: one rounding for the product, at most 94 for the sums that follow the first (0 + t is exact), one for the
    scale -- 96 factors (1 + d), |d| <= u = 2^-24, on every term: a relative error of at most 96 u / (1 - 96 u) = 5.73e-6 < 6e-6"""
    u = 2.0 ** -24
    bound = 96 * u / (1 - 96 * u)
    assert bound < 6e-6
    rng = np.random.default_rng(7)
    film = (rng.random((200, N_GRID)) * 10.0 ** rng.integers(-3, 4, (200, 1))).astype(F)
    resp = rng.random((16, N_GRID)).astype(F)
    for scale in (F(1), CIE_SCALE, F(0.37)):
        got = develop(film, resp, scale).astype(np.float64)
        want = (film.astype(np.float64) @ resp.astype(np.float64).T) * float(scale)
        assert (want > 0).all()
        rel = np.abs(got - want) / want
        print("scale %r: largest relative error %.3g (bound %.3g)" % (float(scale), rel.max(), bound))
        assert rel.max() <= bound


def test_the_order_of_the_sum_is_pinned():
    """2^24 + 1 + 1 in fp32: ascending, each 1 is lost to the tie (2^24); descending, 1 + 1 = 2 survives (2^24 + 2)"""
    film = np.zeros((1, N_GRID), F)
    film[0, :3] = [2.0 ** 24, 1.0, 1.0]
    resp = np.ones((1, N_GRID), F)
    up = develop(film, resp)
    down = develop(film, resp, order=range(N_GRID - 1, -1, -1))
    assert float(up[0, 0]) == 2.0 ** 24 and float(down[0, 0]) == 2.0 ** 24 + 2
    assert bits(up)[0, 0] != bits(down)[0, 0]


def test_normalising_step_is_one_reciprocal_and_one_product():
    s = np.array([[3.0, 5.0, 7.0]], F)
    for n in (1, 3, 7, 4096):
        inv = F(1) / F(n)
        assert np.array_equal(bits(normalise(s, n)), bits((inv * s).astype(F)))
    assert float(CIE_SCALE) == float(F(470.0) / F(7.0))
