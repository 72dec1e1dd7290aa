"""tests/despeckle_reference.py -- the numpy restatement of the firefly filter the device is held to -- against a per-pixel brute force
that follows the text of include/srt_c_api.h with Python's sorted() and exact rationals, one rounding to float32 per operation; then the
consequences that text names: power-of-two scaling, flips and transposes, a step edge, a cluster of outliers, a bright line, the
switched-off filter.  Also the compare-exchange network of csrc/srt_despeckle.hip, restated, under the zero-one principle.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import despeckle_reference as R
from helpers import bits

F = np.float32


# ---- exact float32 arithmetic on Python floats that hold float32 values -----------------------------------------------------------------
def round32(q):
    """the float32 nearest to the rational q (ties to even; denormals; overflow to inf), as a Python float"""
    if q == 0:
        return 0.0
    sign, a = (-1.0, -q) if q < 0 else (1.0, q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                      # 2^e <= a < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(a, quantum)
    n = int(n)
    if rem * 2 > quantum or (rem * 2 == quantum and n % 2 == 1):
        n += 1
    v = n * quantum
    return sign * (float("inf") if v >= Fraction(2) ** 128 else float(v))


def op32(a, b, what):
    """a (what) b rounded once to float32; non-finite operands follow IEEE through Python's own arithmetic"""
    if all(np.isfinite(v) for v in (a, b)) and not (what == "/" and b == 0):
        fa, fb = Fraction(a), Fraction(b)
        r = round32(fa * fb if what == "*" else fa + fb if what == "+" else fa / fb)
        if r == 0.0:      # the sign of a zero result, which a rational does not carry (an underflow to zero included)
            neg_a, neg_b = np.signbit(a), np.signbit(b)
            if what == "+":
                exact = fa + fb
                return -0.0 if (exact < 0 or (exact == 0 and neg_a and neg_b)) else 0.0
            return -0.0 if neg_a != neg_b else 0.0
        return r
    with np.errstate(all="ignore"):
        return float(F(a) * F(b) if what == "*" else F(a) + F(b) if what == "+" else F(a) / F(b))


def test_round32_is_float32_rounding():
    rng = np.random.default_rng(3)
    a = rng.random(400).astype(F) * F(10.0) ** rng.integers(-44, 38, 400).astype(F)
    b = rng.random(400).astype(F) * F(10.0) ** rng.integers(-20, 20, 400).astype(F) + F(1e-30)
    with np.errstate(all="ignore"):
        for x, y in zip(a, b):
            assert bits(F(op32(float(x), float(y), "*"))) == bits(x * y)
            assert bits(F(op32(float(x), float(y), "+"))) == bits(x + y)
            assert bits(F(op32(float(x), float(y), "/"))) == bits(x / y)
    assert round32(Fraction(2) ** -150) == 0.0 and round32(Fraction(3, 2) * Fraction(2) ** -149) == 2.0 ** -148      # ties to even, both ways
    assert round32(Fraction(2) ** 128) == float("inf") and round32(-(Fraction(2) ** 128 - Fraction(2) ** 103)) == -float("inf")


def brute_force(img, radius, rank_ppm, gain, floor):
    """(o, s, class) per pixel, by the header's text"""
    h, w, _ = img.shape
    gain, floor = float(F(gain)), float(F(floor))
    out = np.empty_like(img)
    scale = np.empty((h, w), F)
    cls = np.empty((h, w), object)
    for y in range(h):
        for x in range(w):
            vals = []
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    qy, qx = y + dy, x + dx
                    if (dy, dx) == (0, 0) or not (0 <= qy < h and 0 <= qx < w):
                        continue
                    Yq = float(img[qy, qx, 1])
                    if not np.isfinite(Yq):
                        continue
                    vals.append(Yq if Yq > 0 else 0.0)
            u, m = sorted(vals), len(vals)
            c = [float(v) for v in img[y, x]]
            out[y, x], scale[y, x] = img[y, x], F(1)
            if not all(np.isfinite(v) for v in c):
                cls[y, x] = "nonfinite"
                continue
            if m == 0:
                cls[y, x] = "alone"
                continue
            ref = u[(m - 1) * rank_ppm // 1000000]
            limit = op32(op32(gain, ref, "*"), floor, "+")
            if c[1] > limit:
                s = op32(limit, c[1], "/")
                out[y, x] = [F(op32(s, v, "*")) for v in c]
                scale[y, x] = F(s)
                cls[y, x] = "clamped"
            else:
                cls[y, x] = "kept"
    return out, scale, cls


def special_image(h, w, seed):
    """values over many decades with NaN, +-inf, negatives, -0, +0, denormals and huge values among them"""
    rng = np.random.default_rng(500 + seed)
    img = (rng.random((h, w, 3)) * 10.0 ** rng.integers(-3, 4, (h, w, 1))).astype(F)
    specials = [np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0, 1e-41, 3e-39, 3e38, 1e38, 2.0 ** -126]
    flat = img.reshape(-1, 3)
    where = rng.permutation(h * w)
    for i, v in enumerate(specials[:max(0, h * w - 2)]):
        flat[where[i % (h * w)], 1 if i % 3 else rng.integers(0, 3)] = F(v)
    return img


@pytest.mark.parametrize("h,w", [(1, 1), (1, 4), (5, 1), (2, 3), (6, 7), (5, 5)])
def test_the_restatement_equals_the_brute_force(h, w):
    seen = set()
    for seed in range(3):
        img = special_image(h, w, seed)
        for radius in (1, 2):
            for rank_ppm in R.RANKS + (333333,):
                for gain, floor in ((4.0, 0.0), (1.0, 0.003), (0.0, 0.5), (3e38, 1e-40), (2.5, np.inf)):
                    got = R.despeckle(img, radius, rank_ppm, gain, floor)
                    o, s, cls = brute_force(img, radius, rank_ppm, gain, floor)
                    what = (h, w, seed, radius, rank_ppm, gain, floor)
                    assert np.array_equal(bits(got["xyz"]), bits(o)), what
                    assert np.array_equal(bits(got["scale"]), bits(s)), what
                    for name in ("clamped", "nonfinite", "alone"):
                        assert np.array_equal(got[name], cls == name), (what, name)
                        assert got["clip"][name] == int((cls == name).sum())
                    seen |= set(cls.reshape(-1))
    if h * w > 12:
        assert seen == {"clamped", "kept", "nonfinite"} or seen == {"clamped", "kept", "nonfinite", "alone"}
    if h * w == 1:
        assert "alone" in seen or "nonfinite" in seen


def test_ranks_of_a_full_window():
    """with 24 neighbours 875000 is the 4th largest (k = 20), 500000 the lower median (k = 11), 1000000 the largest; with 8: k = 6, 3, 7"""
    assert [23 * r // 1000000 for r in R.RANKS] == [0, 5, 11, 20, 23]
    assert [7 * r // 1000000 for r in R.RANKS] == [0, 1, 3, 6, 7]
    img = np.zeros((5, 5, 3), F)
    img[..., 1] = np.arange(25, dtype=F).reshape(5, 5) + F(1)
    img[2, 2, 1] = F(1000)
    for rank, k in zip(R.RANKS, (0, 5, 11, 20, 23)):
        want = sorted(v for v in range(1, 26) if v != 13)[k]
        assert R.despeckle(img, 2, rank, 1.0, 0.0)["ref"][2, 2] == want


# ---- the consequences the header names ---------------------------------------------------------------------------------------------------
def test_power_of_two_scaling():
    img = R.recipe_image(23, 17, sprinkle=False)
    for radius in (1, 2):
        for rank in (250000, 500000, 875000):
            base = R.despeckle(img, radius, rank, 4.0, 0.125)
            assert base["clip"]["clamped"] > 10
            for k in (-60, -7, 3, 40):
                sc = F(2.0 ** k)
                got = R.despeckle((img * sc).astype(F), radius, rank, 4.0, float(F(0.125) * sc))
                assert np.array_equal(got["clamped"], base["clamped"]), (radius, rank, k)
                assert np.array_equal(bits(got["xyz"]), bits((base["xyz"] * sc).astype(F))), (radius, rank, k)
                assert np.array_equal(bits(got["scale"]), bits(base["scale"])), (radius, rank, k)


def test_flips_and_transposes_commute():
    img = R.recipe_image(19, 11, seed=2)
    for radius in (1, 2):
        for rank in R.RANKS:
            base = R.despeckle(img, radius, rank, 4.0, 0.01)
            for name, f in (("flip x", lambda a: a[:, ::-1]), ("flip y", lambda a: a[::-1]), ("transpose", lambda a: np.swapaxes(a, 0, 1))):
                got = R.despeckle(np.ascontiguousarray(f(img)), radius, rank, 4.0, 0.01)
                assert np.array_equal(bits(got["xyz"]), bits(np.ascontiguousarray(f(base["xyz"])))), (name, radius, rank)
                assert np.array_equal(bits(got["scale"]), bits(np.ascontiguousarray(f(base["scale"])))), (name, radius, rank)
                assert got["clip"] == base["clip"]


def test_a_step_edge_is_kept():
    for img in (R.step_edge(), np.ascontiguousarray(np.swapaxes(R.step_edge(), 0, 1))):
        for radius in (1, 2):
            for rank in (500000, 625000, 875000, 1000000):
                for gain in (1.0, 4.0):
                    got = R.despeckle(img, radius, rank, gain, 0.0)
                    assert got["clip"] == dict(clamped=0, nonfinite=0, alone=0), (radius, rank, gain)
                    assert np.array_equal(bits(got["xyz"]), bits(img))
    assert R.despeckle(R.step_edge(), 2, 250000, 4.0, 0.0)["clip"]["clamped"] > 0      # (below the median the edge's bright side is an outlier)


@pytest.mark.parametrize("count", [1, 5, 12])
def test_a_cluster_of_outliers_is_clamped_whole_at_the_median(count):
    img, mask = R.cluster(count)
    got = R.despeckle(img, 2, 500000, 4.0, 0.0)
    assert np.array_equal(got["clamped"], mask) and got["clip"]["clamped"] == count
    assert np.array_equal(bits(got["xyz"][~mask]), bits(img[~mask]))
    assert (got["xyz"][mask] == F(2.0)).all()          # limit = 4 * 0.5


def test_a_bright_line_is_clamped_at_the_median_and_kept_at_the_default_rank():
    """The nine pixels of a line that crosses their 5 x 5 windows from edge to edge: four of a pixel's 24 neighbours are line pixels, so
    the 4th largest (rank 875000, k = 20) is one of them and the lower median is not.  (A line's END has only two line neighbours and is
    clamped at either rank: the rank protects a line, not its tip.)"""
    img, inner = R.bright_line(13)
    assert inner.sum() == 9
    at_median = R.despeckle(img, 2, 500000, 4.0, 0.0)
    assert at_median["clamped"][inner].sum() == 9
    default = R.despeckle(img, 2, 875000, 4.0, 0.0)
    assert default["clamped"][inner].sum() == 0 and np.array_equal(bits(default["xyz"][inner]), bits(img[inner]))
    assert default["clamped"][:, :6].sum() == 0 and default["clamped"][:, 7:].sum() == 0      # the background is kept either way
    assert at_median["clamped"][:, :6].sum() == 0 and at_median["clamped"][:, 7:].sum() == 0


def test_an_infinite_floor_switches_the_filter_off():
    img = R.recipe_image(19, 11, seed=5)
    for radius in (1, 2):
        got = R.despeckle(img, radius, 500000, 0.0, np.inf)
        assert np.array_equal(bits(got["xyz"]), bits(img)) and (got["scale"] == 1).all() and got["clip"]["clamped"] == 0
    assert R.despeckle(img, 2, 500000, 0.0, 0.0)["clip"]["clamped"] > 100


def test_clamp_and_keep_shares_of_the_recipe():
    """the seeded recipe exercises both classes: at least a tenth of the pixels clamped and at least half kept"""
    img = R.recipe_image(67, 35)
    for radius in (1, 2):
        for rank in (250000, 500000):
            got = R.despeckle(img, radius, rank, 4.0, 0.0)
            n = 67 * 35
            kept = n - sum(got["clip"].values())
            print("radius %d rank %d: clamped %.3f kept %.3f" % (radius, rank, got["clip"]["clamped"] / n, kept / n))
            assert got["clip"]["clamped"] * 10 >= n and kept * 2 >= n


def test_mean_xyz():
    S = np.arange(24, dtype=F).reshape(2, 4, 3) + F(0.3)
    assert np.array_equal(bits(R.mean_xyz(S, 5)), bits((F(1) / F(5)) * S))
    n = np.array([[0, 1, 3, 7], [2, 2, 0, 9]])
    want = (F(1) / np.where(n == 0, 1, n).astype(F))[..., None] * S
    assert np.array_equal(bits(R.mean_xyz(S, n)), bits(want.astype(F)))


# ---- the kernel's sorting network -----------------------------------------------------------------------------------------------------
def network(n):
    """the comparators of sort_network<N> (csrc/srt_despeckle.hip), in its loop order"""
    out = []
    p = 1
    while p < n:
        k = p
        while k >= 1:
            for j in range(k % p, n - k, 2 * k):
                for i in range(0, min(k - 1, n - j - k - 1) + 1):
                    if (i + j) // (2 * p) == (i + j + k) // (2 * p):
                        out.append((i + j, i + j + k))
            k //= 2
        p *= 2
    return out


@pytest.mark.parametrize("n", [8, 24])
def test_the_compare_exchange_network_sorts(n):
    """zero-one principle: a network that sorts every 0/1 input sorts every input.  All 2^n inputs at once, one bit per input."""
    comps = network(n)
    assert all(a < b < n for a, b in comps)
    idx = np.arange(1 << n, dtype=np.uint32)
    wires = [np.packbits(((idx >> i) & 1).astype(np.uint8)) for i in range(n)]
    for a, b in comps:
        wires[a], wires[b] = wires[a] & wires[b], wires[a] | wires[b]      # min to the lower wire, max to the upper
    for i in range(n - 1):
        assert not (wires[i] & ~wires[i + 1]).any(), "wires %d, %d out of order for some input" % (i, i + 1)
    print("N = %d: %d comparators" % (n, len(comps)))
