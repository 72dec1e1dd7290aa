"""The float64 truth of the ray queries (srt_intersect_rays / srt_occluded_rays, include/srt_c_api.h "Ray queries") and the ray populations
the tests hold them to.

Built on ground_truth._scan: for rows (n, 8) = ox oy oz tmin dx dy dz tmax it gives every crossing t_i >= 0 of every triangle, from which the
truth's interval answer is the closest crossing with tmin <= t_i <= tmax (a hit when one exists).

A ray is HELD -- its float32 answer must agree with the truth -- when
  * its near >= EDGE_MARGIN (it passes no edge of any triangle closer than the margin of the closest-hit populations), and
  * every crossing t_i lies farther than C_T t_bound_i + 2^-20 t_i from both tmin and tmax.
C_T t_bound_i covers the float32 t of the triangle, as in the closest-hit conditions.  The product compares that t against tmin and against
c <= tmax in a triangle test, and a slab entry (b - o) (1 / d) against tmin in a box test: three roundings, about 3 u t.  2^-20 = 16 u gives
that term fourfold headroom, the project's usual factor.  A crossing inside the margin may fall on either side of a bound in float32, so its
ray is left out; the populations are made so that at most MAX_EXCLUDED of their rays are (tests/test_query_reference.py).

The intervals only use tmin >= 0: the truth scans crossings at t >= 0."""
import numpy as np

import ground_truth as G

FLT_MAX = float(np.finfo(np.float32).max)
INTERVAL_MARGIN = 2.0 ** -20
N_RAYS = 4096
SIZES = (1, 63, 64, 65, 4096)


def rows(o, d, tmin, tmax):
    """(n, 8) float32 rows ox oy oz tmin dx dy dz tmax"""
    d = np.asarray(d, np.float32)
    out = np.empty((len(d), 8), np.float32)
    out[:, 0:3] = o; out[:, 3] = tmin; out[:, 4:7] = d; out[:, 7] = tmax
    return out


def six(r):
    """the (n, 6) origin / direction rows of srt_trace_rays"""
    return np.ascontiguousarray(np.concatenate([r[:, 0:3], r[:, 4:7]], axis=1))


def scan(V, r):
    """(near, all_t (n_tris, m)) of ground_truth._scan for the rays' origins and directions"""
    _, _, _, near, all_t = G._scan(np.asarray(V, np.float64), G.f64(r[:, 0:3]), G.f64(r[:, 4:7]))
    return near, all_t


def interval_truth(V, r, scanned=None):
    """dict(t, tri, hit, held, near, crossings, tie) of the rows r: the truth's closest crossing in [tmin, tmax] (t inf, tri -1 when there
    is none), whether the ray is held (module docstring), and tie (n_tris, m): the triangles whose crossing in the interval lies within
    C_T (t_bound_i + t_bound_closest) of the closest -- tri among them; more than one only where triangles overlap in a plane"""
    r = np.asarray(r, np.float32)
    V = np.asarray(V, np.float64)
    near, all_t = scanned if scanned is not None else scan(V, r)
    o, d = G.f64(r[:, 0:3]), G.f64(r[:, 4:7])
    tmin, tmax = G.f64(r[:, 3]), G.f64(r[:, 7])
    assert (tmin >= 0).all() and (tmin <= tmax).all(), "the truth's intervals: 0 <= tmin <= tmax"
    inside = np.isfinite(all_t) & (all_t >= tmin[None, :]) & (all_t <= tmax[None, :])
    t_in = np.where(inside, all_t, np.inf)
    tri = np.argmin(t_in, axis=0)
    t = t_in[tri, np.arange(len(r))]
    hit = np.isfinite(t)
    held = near >= G.EDGE_MARGIN
    _, nu = G.normals(V)
    t_err = np.zeros_like(all_t)      # C_T t_bound of every crossing
    with np.errstate(all="ignore"):
        for k in range(len(V)):
            tk = all_t[k]
            fin = np.isfinite(tk)
            if not fin.any():
                continue
            t_err[k] = G.C_T * G.t_bound(np.broadcast_to(nu[k], o.shape), np.broadcast_to(V[k, 0], o.shape), o, d, np.where(fin, tk, 0.0))
            bound = t_err[k] + INTERVAL_MARGIN * tk
            close = fin & ((np.abs(tk - tmin) <= bound) | (np.abs(tk - tmax) <= bound) | ~np.isfinite(bound))
            held &= ~close
        # Ties: crossings in the interval that float32 cannot order against the closest one -- within the sum of their C_T t_bound (coplanar
        # overlapping triangles, like the floor of scene 0 under its tall box, cross at the same t).  Any of them is the truth's triangle.
        m = np.arange(len(r))
        tie = inside & hit[None, :] & (np.abs(all_t - t[None, :]) <= t_err + t_err[tri, m][None, :])
    return dict(t=t, tri=np.where(hit, tri, -1), hit=hit, held=held, near=near, crossings=np.isfinite(all_t).sum(0), tie=tie, all_t=all_t)


def random_intervals(base, seed, t_far):
    """the base rays' origins and directions with tmax uniform in [0, 2 t_far]; half of them tmin = 0, the other half tmin uniform in
    [0, tmax)"""
    rng = np.random.default_rng(seed)
    m = len(base)
    tmax = rng.uniform(0.0, 2.0 * t_far, m)
    tmin = np.where(rng.random(m) < 0.5, 0.0, rng.uniform(0.0, 1.0, m) * tmax)
    return rows(base[:, 0:3], base[:, 3:6], tmin.astype(np.float32), tmax.astype(np.float32))


def far_crossing(all_t):
    """the largest finite crossing of a population (1 when it has none): the scale of its intervals"""
    fin = np.isfinite(all_t)
    return float(all_t[fin].max()) if fin.any() else 1.0


# name -> (ground_truth scene, seed of the base rays); "scene0" (the built-in scene 0, CORNELL) is made from the library: scene0_population
SYNTHETIC = {
    "soup": (lambda: G.soup(104, 200, 2.0), 501),
    "bumpy_sheet": (lambda: G.bumpy_sheet()[0], 502),
    "axis_aligned_set": (G.axis_aligned_set, 503),
    "degenerate_walls": (G.degenerate_walls, 504),
}
POPULATIONS = tuple(SYNTHETIC) + ("scene0",)
# degenerate_walls: vertical walls projected onto XY, where they are segments -- the product (like the reference) answers them by its
# projected interior test and differs from the truth by design (tests/test_ground_truth_reference.py).  That population
# is held to the exact contracts (interval, occlusion, srt_trace_rays) only; the truth conditions hold on the four others.
TRUTH_POPULATIONS = ("soup", "bumpy_sheet", "axis_aligned_set", "scene0")
# 4 000 camera rays: the 80 x 50 view of ground_truth.builtin_report.  (A 64 x 64 view puts 0.61 % of its pixel centres inside the edge
# margin of CORNELL's quads -- the population must leave out at most MAX_EXCLUDED.)
SCENE0_W, SCENE0_H = 80, 50


def scene0_population(srt):
    """(product scene, V (n, 3, 3) float32, base rays (4 000, 6)): CORNELL (built-in scene 0, the reference builder) and the pixel-centre
    rays of its default 80 x 50 view"""
    scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    T = scene.triangles()
    V = np.array([[t.v0[:], t.v1[:], t.v2[:]] for t in T], np.float32)
    cam = scene.default_camera(SCENE0_W, SCENE0_H)
    eye, d = G.pixel_rays(cam, SCENE0_W, SCENE0_H)
    base = np.concatenate([np.broadcast_to(eye, d.shape), d], 1).astype(np.float32)
    return scene, V, base


def population(name, srt=None):
    """dict(V, base, rays, truth, scene_source) of a population: rays are its 4 096 interval rows (random_intervals, seed 600 + i), truth
    their interval_truth.  Built once per session (ground_truth.cached)."""
    def make():
        if name == "scene0":
            scene, V, base = scene0_population(srt)
            source = ("builtin", scene)
        else:
            build, seed = SYNTHETIC[name]
            sc = build()
            V, base = np.asarray(sc["V"], np.float32), G.random_rays(seed, N_RAYS)
            source = ("synthetic", sc)
        near, all_t = scan(V, rows(base[:, 0:3], base[:, 3:6], 0.0, FLT_MAX))      # (the crossings do not depend on the interval)
        r = random_intervals(base, 600 + POPULATIONS.index(name), far_crossing(all_t))
        return dict(V=V, base=base, rays=r, truth=interval_truth(V, r, (near, all_t)), source=source)
    return G.cached(("query population", name), make)
