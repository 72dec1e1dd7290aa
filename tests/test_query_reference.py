"""CPU: the interval truth of tests/query_reference.py against closed cases, and the share of rays its margin leaves out of every population
the GPU tests use (tests/test_query.py)."""
import numpy as np
import pytest

import ground_truth as G
import query_reference as Q


def _plane(z):
    """two triangles covering [-10, 10]^2 at height z"""
    return np.array(G.quad([-10, -10, z], [10, -10, z], [10, 10, z], [-10, 10, z]), np.float64)


def test_single_plane():
    """rays straight down from z = 5 onto the plane z = 1 cross it at t = 4 (|d| = 1): inside [tmin, tmax] a hit at exactly 4, outside a
    miss; the ray is held unless a bound lies within C_T t_bound + 2^-20 t of 4"""
    V = _plane(1.0)
    o = np.array([[0.25, 0.375, 5.0]] * 6, np.float32)
    d = np.array([[0.0, 0.0, -1.0]] * 6, np.float32)
    tmin = np.array([0.0, 0.0, 4.5, 0.0, 3.0, 4.0], np.float32)
    tmax = np.array([Q.FLT_MAX, 3.5, 9.0, 4.0, np.inf, 4.0], np.float32)
    t = Q.interval_truth(V, Q.rows(o, d, tmin, tmax))
    assert t["hit"].tolist() == [True, False, False, True, True, True]
    assert (t["t"][t["hit"]] == 4.0).all() and (t["tri"][t["hit"]] >= 0).all() and (t["tri"][~t["hit"]] == -1).all()
    assert t["held"].tolist() == [True, True, True, False, True, False]


def test_coplanar_tie():
    """a triangle lying on the plane (scene 0's tall box stands on its floor this way): a ray through both has two truth triangles at one t,
    a ray through the plane alone one"""
    V = np.concatenate([_plane(1.0), np.array([[[0, 0, 1], [2, 0, 1], [0, 2, 1]]], np.float64)])
    o = np.array([[0.5, 0.25, 5.0], [-3.0, -2.0, 5.0]], np.float32)
    d = np.array([[0.0, 0.0, -1.0]] * 2, np.float32)
    t = Q.interval_truth(V, Q.rows(o, d, 0.0, Q.FLT_MAX))
    assert t["hit"].all() and (t["t"] == 4.0).all() and t["held"].all()
    assert t["tie"][:, 0].sum() == 2 and t["tie"][2, 0] and t["tie"][t["tri"][0], 0]
    assert t["tie"][:, 1].sum() == 1 and t["tie"][t["tri"][1], 1]


def test_stack_of_plates():
    """parallel plates at z = 0, 1, .., 7 and a ray down from z = 10 (t_i = 10 - z): the answer is the first plate at or after tmin, if it
    is not after tmax; plates at a bound make the ray not held"""
    V = np.concatenate([_plane(float(z)) for z in range(8)])
    n = 200
    rng = np.random.default_rng(5)
    o = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), np.full(n, 10.0)]).astype(np.float32)
    d = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (n, 1))
    tmax = rng.uniform(0, 14, n).astype(np.float32)
    tmin = (rng.uniform(0, 1, n) * tmax).astype(np.float32)
    tmin[:20] = np.floor(tmin[:20]); tmax[20:40] = np.floor(tmax[20:40])       # bounds on a plate
    tmin[20:40] = np.minimum(tmin[20:40], tmax[20:40])
    t = Q.interval_truth(V, Q.rows(o, d, tmin, tmax))
    plates = 10.0 - np.arange(8)[::-1]        # t of the plates: 3 .. 10
    for k in range(n):
        inside = plates[(plates >= tmin[k]) & (plates <= tmax[k])]
        assert t["hit"][k] == (len(inside) > 0)
        if len(inside):
            assert t["t"][k] == inside.min()
            assert V[t["tri"][k], 0, 2] == 10.0 - inside.min()
        on_bound = np.isin(plates, [tmin[k], tmax[k]]).any()
        assert not (on_bound and t["held"][k]), k
    assert t["held"].sum() >= n - 40 - 5


@pytest.mark.parametrize("name", Q.POPULATIONS)
def test_population_leaves_out_few_rays(srt, name):
    """every population of the GPU tests: at most MAX_EXCLUDED of its rays lie inside the edge margin or have a crossing inside the interval
    margin -- on the truth alone; the population is not trivial (it has hits and misses inside its intervals)"""
    p = Q.population(name, srt)
    t = p["truth"]
    excluded = (~t["held"]).mean()
    print("%-18s %d rays, %.1f %% hit in their interval, %.2f crossings per ray, %d left out (%.3f %%)" % (
        name, len(p["rays"]), 100 * t["hit"].mean(), t["crossings"].mean(), (~t["held"]).sum(), 100 * excluded))
    assert excluded <= G.MAX_EXCLUDED
    assert 0.05 < t["hit"].mean() < 0.95
    # the intervals cut crossings off on both sides: some rays cross a triangle before tmin or after tmax
    r = p["rays"]
    assert (r[:, 3] > 0).mean() > 0.3 and (r[:, 7] < Q.far_crossing(np.where(t["hit"], t["t"], np.inf)[None, :])).mean() > 0.3
