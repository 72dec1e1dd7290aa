"""Independent float64 ground truth for ray hits and radiometry.  TEST INFRASTRUCTURE ONLY.

numpy float64 and nothing else: this module imports neither the product nor the oracle, restates no random number generator and
walks no tree.  Its inputs are the float32 values the renderer is given (vertices, rays, 95-sample spectra, the four CIE / D65 rows
of srt_color_tables, the camera struct), widened to float64; its outputs are what geometry and radiometry say about them:

  closest_hit    brute-force two-sided Moeller-Trumbore over all triangles
  t_bound        a-priori float32 error bound of t = (D - n.o) / (n.d)
  path_moments   mean and variance of one path's XYZ contribution for a given end spectrum (7 stratified wavelengths, or the hero alone)
  form_factor    Lambert's closed form for the cosine-weighted form factor of a polygon seen from a point
  glass_paths    the probability that a path through flat glass faces ends on the emitter, by enumeration (refraction, total reflection)
  fuzz_share, fuzz_light_share, lens_coverage
                 where a fuzzed metal and a thin lens send the light (the *_sampled twins state the same quantities as plain counts)
  lane_index, footprint_average, project_points, polygon_area, coverage_map     pixel helpers
  soup, bumpy_sheet, axis_aligned_set, ... , to_structs                          scene builders on raw arrays
  hat, film_integrals, hero_film_moments, film_expectation
                 one path's deposit into every bin of the spectral film: tents on the 5 nm grid, integrated exactly per cell
  plates, feature_expectation
                 the first-hit features: exact coverage of each triangle, the normal turned towards the camera, col, the distance
  assert_hits_hold, assert_edge_aimed_hold, builtin_report, assert_radiometry_holds, assert_film_holds, assert_features_hold
                 the conditions both suites apply: tests/test_ground_truth_reference.py to the oracle (CPU), tests/test_ground_truth.py
                 to the device (GPU), on the same inputs and with the same thresholds

The scene builders return plain dicts of numpy arrays; to_structs() fills the caller's ctypes classes (the product's or the oracle's:
they are byte-compatible), so a scene reaches either implementation without this module knowing it.  Where a helper needs the package
(its raw-array boundary, its colour tables, its built-in scenes) the caller passes it in.  One material per triangle, so that mat_index
names the triangle hit; spectra and the background are set DIRECTLY to non-flat tables (a ramp, a bump): the reference's baked greys
are nearly flat (0.73 bakes to a spectrum of about 1) and would hide an indexing error."""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of float32
N_GRID = 95                       # samples of the 5 nm grid, 360 .. 830 nm
LAMBDA_MIN, LAMBDA_MAX = 360.0, 830.0
N_WAVELENGTHS = 7
STEP = (LAMBDA_MAX - LAMBDA_MIN) / N_WAVELENGTHS          # distance of a path's wavelengths, and the weight of each in the XYZ sum
TX, TY = 28, 16                   # the block of the frame buffer's block-linear layout

MAT_LAMBERTIAN, MAT_METALLIC, MAT_DIELECTRIC, MAT_EMISSIVE = 0, 1, 2, 4      # materials/material.cuh
AAP_NONE, AAP_XY, AAP_YZ, AAP_XZ = 0, 1, 2, 3                                # primitives/tri.cuh
PROJECTED_AXIS = {AAP_NONE: 2, AAP_XY: 2, AAP_YZ: 0, AAP_XZ: 1}              # the axis the interior test drops (Q12)
MIN_PROJECTED_NORMAL = 0.05       # below this component of the unit normal a triangle's projection counts as degenerate

BK7_B = (1.03961212, 0.231792344, 1.01046945)             # Schott N-BK7, Sellmeier coefficients (C in um^2)
BK7_C = (0.00600069867, 0.0200179144, 103.560653)


# ---- hits ---------------------------------------------------------------------------------------------------------------------
def f64(a):
    """float32 values widened to float64 (the inputs are what the renderer gets, not what a float64 builder meant)"""
    return np.asarray(a, np.float32).astype(np.float64)


def unit(d):
    """rows of d (m, 3) scaled to length 1"""
    return d / np.linalg.norm(d, axis=1)[:, None]


def normals(V):
    """unnormalised and unit normals (v1 - v0) x (v2 - v0) of triangles V (n, 3, 3)"""
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    with np.errstate(all="ignore"):
        return n, n / np.linalg.norm(n, axis=1)[:, None]


BARY_ROUNDING = 1e-12   # the truth's own float64 rounding: a point this close to an edge belongs to the triangles on both sides of it


def _scan(V, o, d):
    V, o, d = np.asarray(V, np.float64), np.asarray(o, np.float64), np.asarray(d, np.float64)
    m = o.shape[0]
    best_t, best_i, best_b, near = np.full(m, np.inf), np.full(m, -1, np.int64), np.full(m, np.nan), np.full(m, np.inf)
    all_t = np.full((V.shape[0], m), np.inf)
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    with np.errstate(all="ignore"):
        for k in range(V.shape[0]):
            p = np.cross(d, e2[k])
            det = p @ e1[k]
            inv = 1.0 / det
            tv = o - V[k, 0]
            u = (tv * p).sum(1) * inv
            q = np.cross(tv, e1[k])
            v = (d * q).sum(1) * inv
            t = (q @ e2[k]) * inv
            mb = np.minimum(np.minimum(u, v), 1.0 - u - v)
            ok = (det != 0) & np.isfinite(t) & (t >= 0)
            near = np.where(ok & (np.abs(mb) < near), np.abs(mb), near)
            inside = ok & (mb >= -BARY_ROUNDING)
            all_t[k] = np.where(inside, t, np.inf)
            hit = inside & (t < best_t)
            best_t = np.where(hit, t, best_t); best_i = np.where(hit, k, best_i); best_b = np.where(hit, mb, best_b)
    return best_t, best_i, best_b, near, all_t


def closest_hit(V, o, d):
    """Two-sided Moeller-Trumbore of rays (o, d) (m, 3) against ALL triangles V (n, 3, 3), t >= 0, brute force.
    Returns t (inf on a miss), tri (-1 on a miss), bary = the smallest barycentric coordinate at the hit (NaN on a miss) and
    near = the smallest |min barycentric| over every triangle PLANE the ray meets at t >= 0: how close the ray passes to any edge
    of any triangle, hit or not (inf when it meets no plane)."""
    return _scan(V, o, d)[:4]


def later_crossings(V, o, d):
    """per ray, the number of triangles it passes through clearly BEHIND its closest hit (t > t_closest + 1e-3 (1 + t_closest))"""
    t, _, _, _, all_t = _scan(V, o, d)
    with np.errstate(all="ignore"):
        return (np.isfinite(all_t) & (all_t > (t + 1e-3 * (1 + t))[None, :])).sum(0)


def plane_t(V, k, o, d):
    """t at which rays (o, d) meet the plane of triangle k[i] of V, float64"""
    V = np.asarray(V, np.float64)
    n, _ = normals(V)
    nk = n[k]
    with np.errstate(all="ignore"):
        return ((V[k, 0] - o) * nk).sum(1) / (nk * d).sum(1)


def t_bound(n, v0, o, d, t):
    """A-priori float32 error bound of t = (D - n.o) / (n.d), D = n.v0, up to its constant factor c (measured on the oracle, fixed at
    twice the measurement: tests/test_ground_truth_reference.py): u (sum|n_k v0_k| + sum|n_k o_k| + t sum|n_k d_k|) / |n.d|.
    Every rounding in D, in n.o and in their difference is bounded by u times the first two sums; those of n.d and of the quotient by
    u t times the third.  n: unit normals, one per ray."""
    n, v0, o, d, t = (np.asarray(a, np.float64) for a in (n, v0, o, d, t))
    num = np.abs(n * v0).sum(-1) + np.abs(n * o).sum(-1) + t * np.abs(n * d).sum(-1)
    return U * num / np.abs((n * d).sum(-1))


def front_face(V, tri, d):
    """front_face of the reference's hit record: the ray runs against the triangle's normal (v1 - v0) x (v2 - v0)"""
    n, _ = normals(np.asarray(V, np.float64))
    return (n[tri] * d).sum(1) < 0


def effective_aa_plane(V, aa_plane):
    """the projection plane tri::init leaves a triangle with (Q12): the plane of an axis-aligned normal, else the value it came with"""
    _, nu = normals(np.asarray(V, np.float64))
    perp = np.abs(nu) < 1e-8
    out = np.array(aa_plane, np.int64).copy()
    out[perp[:, 1] & perp[:, 2]] = AAP_YZ
    out[perp[:, 0] & perp[:, 2] & ~(perp[:, 1] & perp[:, 2])] = AAP_XZ
    out[perp[:, 0] & perp[:, 1] & ~perp[:, 2]] = AAP_XY
    return out


def projected_normal(V, aa_plane):
    """|component of the unit normal along the axis the interior test drops|: 0 means the projected triangle is a segment"""
    _, nu = normals(np.asarray(V, np.float64))
    ax = np.array([PROJECTED_AXIS[int(a)] for a in effective_aa_plane(V, aa_plane)])
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(nu).all(1), np.abs(nu[np.arange(len(ax)), ax]), 0.0)


def compare_hits(V, rays, got, mat_of_tri=None):
    """An implementation's closest hits `got` (m, 4: t, -1 on a miss, front_face, mat_index -- the layout of srt_trace_rays) against the
    truth for the same float32 rays (m, 6).  mat_of_tri: the material of every triangle (default: its own number, the builders' rule).
    Returns a dict of per-ray arrays: want_hit, got_hit, same (hit / miss and the material of the triangle hit agree), both (both hit the
    same material), ratio = |t - t_truth| / t_bound and front_ok where `both`, near, tri (the truth's)."""
    V = np.asarray(V, np.float64)
    o, d = f64(rays[:, :3]), f64(rays[:, 3:])
    t, tri, _, near = closest_hit(V, o, d)
    mat_of_tri = np.arange(len(V)) if mat_of_tri is None else np.asarray(mat_of_tri)
    want_hit, got_hit = tri >= 0, got[:, 1] >= 0
    both = want_hit & got_hit & (got[:, 3].astype(np.int64) == mat_of_tri[np.maximum(tri, 0)])
    same = both | (~want_hit & ~got_hit)
    _, nu = normals(V)
    k = np.maximum(tri, 0)
    with np.errstate(all="ignore"):
        ratio = np.where(both, np.abs(got[:, 0].astype(np.float64) - t) / t_bound(nu[k], V[k, 0], o, d, t), 0.0)
    front_ok = ~both | ((got[:, 2] != 0) == front_face(V, k, d))
    return dict(want_hit=want_hit, got_hit=got_hit, same=same, both=both, ratio=ratio, front_ok=front_ok, near=near, tri=tri, t=t)


# Measured on the oracle by tests/test_ground_truth_reference.py (the numbers stand in its docstrings and in DESIGN section 2):
C_T = 6.9               # twice the largest |t - t_truth| / t_bound over all agreeing hits (measured 3.44, on a sliver triangle)
EDGE_MARGIN = 1.7e-6    # four times the largest `near` of a ray on which oracle and truth disagree (measured 4.23e-7, edge-aimed rays)
MAX_EXCLUDED = 0.005    # at most this share of a random population may lie inside the margin


def assert_hits_hold(V, rays, got, what, mat_of_tri=None):
    """the conditions of the random populations: every ray at least EDGE_MARGIN from every edge agrees with the truth in hit / miss and in
    the triangle; every agreeing hit has |t - t_truth| <= C_T t_bound and the truth's front_face; at most MAX_EXCLUDED of the rays are
    left out.  Returns the comparison and a summary for the test's printed line."""
    r = compare_hits(V, rays, got, mat_of_tri)
    held = r["near"] >= EDGE_MARGIN
    bad = held & ~r["same"]
    assert not bad.any(), "%s: %d rays away from every edge differ from the truth, first %d" % (what, bad.sum(), np.nonzero(bad)[0][0])
    assert r["ratio"].max() <= C_T, "%s: |dt| / t_bound = %.3g at ray %d" % (what, r["ratio"].max(), r["ratio"].argmax())
    assert r["front_ok"].all(), "%s: front_face differs from sign(n.d) at ray %d" % (what, np.nonzero(~r["front_ok"])[0][0])
    assert (~held).mean() <= MAX_EXCLUDED, "%s: %.3g of the rays lie inside the edge margin" % (what, (~held).mean())
    summary = dict(rays=len(rays), hit_share=float(r["want_hit"].mean()), excluded=int((~held).sum()), differ=int((~r["same"]).sum()),
                   max_ratio=float(r["ratio"].max()), max_near_differ=float(r["near"][~r["same"]].max()) if (~r["same"]).any() else 0.0)
    return r, summary


def assert_edge_aimed_hold(V, rays, adjacent, got, what):
    """the conditions of the edge-aimed rays: a ray hits a triangle adjacent to its target, within the t bound, or it misses (a leak);
    it never hits another triangle.  Returns the leak share."""
    r = compare_hits(V, rays, got)
    hit = got[:, 1] >= 0
    tri = got[:, 3].astype(np.int64)
    ok = ~hit | adjacent[np.arange(len(rays)), np.clip(tri, 0, adjacent.shape[1] - 1)]
    assert ok.all(), "%s: ray %d hits triangle %d, not adjacent to its target" % (what, np.nonzero(~ok)[0][0], tri[np.nonzero(~ok)[0][0]])
    # t against the plane of the triangle actually hit (the truth may have picked the neighbour across the edge)
    o, d = f64(rays[:, :3]), f64(rays[:, 3:])
    Vd = np.asarray(V, np.float64)
    k = np.where(hit, tri, 0)
    tp = plane_t(Vd, k, o, d)
    _, nu = normals(Vd)
    with np.errstate(all="ignore"):
        ratio = np.where(hit, np.abs(got[:, 0].astype(np.float64) - tp) / t_bound(nu[k], Vd[k, 0], o, d, tp), 0.0)
    assert ratio.max() <= C_T, "%s: |dt| / t_bound = %.3g at ray %d" % (what, ratio.max(), ratio.argmax())
    assert r["want_hit"].all()
    return dict(rays=len(rays), leaks=int((~hit).sum()), leak_share=float((~hit).mean()), max_ratio=float(ratio.max()),
                max_near_leak=float(r["near"][~hit].max()) if (~hit).any() else 0.0)


# ---- radiometry ---------------------------------------------------------------------------------------------------------------
def interp(table, lam):
    """linear interpolation of a 95-sample table on the 5 nm grid"""
    x = (np.asarray(lam, np.float64) - LAMBDA_MIN) / 5.0
    i = np.clip(np.floor(x).astype(np.int64), 0, N_GRID - 2)
    w = x - i
    return (1.0 - w) * table[i] + w * table[i + 1]


def path_wavelengths(h):
    """the seven wavelengths of a path with hero wavelength h: h + i 470/7 wrapped into [360, 830]"""
    lam = np.asarray(h, np.float64)[None, :] + np.arange(N_WAVELENGTHS)[:, None] * STEP
    return np.where(lam > LAMBDA_MAX, LAMBDA_MIN + (lam - LAMBDA_MAX), lam)


def path_moments(cmf, factors, hero_only=False, prob=None, nodes=200000):
    """E and Var (3,) of ONE path's XYZ contribution when every contributing path ends with the power spectrum p = product of the
    linear interpolants of `factors` (95-sample tables).  The hero wavelength h is uniform on [360, 830]; each of the path's seven
    wavelengths adds cmf(l) p(l) 470/7, so E = integral of cmf p over the grid.  hero_only: the path carries h alone (after a
    refraction) and adds cmf(h) p(h) 470/7.  prob: a function of h, the probability that the path contributes at all (it adds 0
    otherwise).  Midpoint quadrature over h with `nodes` nodes; cmf: rows x, y, z of the colour tables, (3, 95) float64."""
    h = LAMBDA_MIN + (np.arange(nodes) + 0.5) * (LAMBDA_MAX - LAMBDA_MIN) / nodes
    lam = h[None, :] if hero_only else path_wavelengths(h)
    p = np.ones_like(lam)
    for tab in factors:
        p = p * interp(np.asarray(tab, np.float64), lam)
    f = np.stack([(interp(cmf[c], lam) * p).sum(0) * STEP for c in range(3)])
    w = np.ones_like(h) if prob is None else prob(h)
    E = (f * w).mean(1)
    return E, (f * f * w).mean(1) - E * E


def exact_integral(cmf, factors):
    """integral over [360, 830] of cmf times the interpolants of `factors`, (3,): three-point Gauss-Legendre in every 5 nm cell, exact
    for the piecewise polynomial of degree 1 + len(factors) <= 5 the integrand is"""
    assert 1 + len(factors) <= 5
    x = np.array([-np.sqrt(0.6), 0.0, np.sqrt(0.6)]) * 0.5 + 0.5
    wq = np.array([5.0, 8.0, 5.0]) / 18.0
    out = np.zeros(3)
    for s, w in zip(x, wq):
        p = np.ones(N_GRID - 1)
        for tab in factors:
            tab = np.asarray(tab, np.float64)
            p = p * ((1 - s) * tab[:-1] + s * tab[1:])
        out += w * 5.0 * (((1 - s) * cmf[:3, :-1] + s * cmf[:3, 1:]) * p).sum(1)
    return out


def sellmeier_index(B, C, lam_nm):
    """n(lambda) of the Sellmeier formula, lambda in nm, C in um^2"""
    l2 = (np.asarray(lam_nm, np.float64) * 1e-3) ** 2
    return np.sqrt(1.0 + sum(b * l2 / (l2 - c) for b, c in zip(B, C)))


def schlick(cosine, ref_idx):
    """Schlick's term as the reference documents it (materials/material.cu:39-53): ref_idx is the refraction RATIO of the interface,
    the cosine is taken on the incoming side"""
    r0 = ((1.0 - ref_idx) / (1.0 + ref_idx)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cosine) ** 5


def slab_transmission(n, cos_in, bounce_limit):
    """Probability that a path entering a plane-parallel slab of index n at cos_in leaves through the far face and reaches an emitter
    behind it within the bounce limit: (1 - R1)(1 - R2) sum_{k <= K} R2^(2k).  R1 = Schlick(cos_in, 1/n) entering; inside, every
    interface is met at the refracted angle with ratio n, R2 = Schlick(cos_t, n).  A path with k internal round trips needs 3 + 2k hits."""
    sin_t = np.sqrt(1.0 - cos_in ** 2) / n
    cos_t = np.sqrt(1.0 - sin_t ** 2)
    R1, R2 = schlick(cos_in, 1.0 / n), schlick(cos_t, n)
    K = (bounce_limit - 3) // 2
    assert K >= 0 and np.all(n * sin_t <= 1.0)
    return (1.0 - R1) * (1.0 - R2) * sum(R2 ** (2 * k) for k in range(K + 1))


GLASS, EMITTER = 0, 1               # kinds of the polygons of glass_paths
EDGE_ROUNDING = 1e-9                # a point this close to a polygon's edge (scene units) counts as inside it


def polygon_planes(polys):
    """per planar convex polygon (k, 3): the unit normal N of its winding ((v1 - v0) x (v2 - v0)), c = N . v0, and the inward edge
    normals G (3, k) with their offsets h (k,): a point p of the plane lies inside when p @ G - h >= 0"""
    out = []
    for v in polys:
        v = np.asarray(v, np.float64)
        N = np.cross(v[1] - v[0], v[2] - v[0]); N = N / np.linalg.norm(N)
        G = np.stack([np.cross(N, np.roll(v, -1, 0)[i] - v[i]) for i in range(len(v))], 1)
        G = G / np.linalg.norm(G, axis=0)[None, :]
        out.append((N, N @ v[0], G, (G * v.T).sum(0)))
    return out


def nearest_polygon(planes, o, d, last):
    """the nearest polygon rays (o, d) (m, 3) meet at t > 0, brute force over ALL of them but the one each ray starts on (last (m,),
    -1: none; a straight ray cannot meet the planar polygon it leaves again): every ray takes its plane crossings in the order of t
    until one lies inside its polygon.  Returns t (inf on a miss) and the polygon (-1)."""
    m = o.shape[0]
    N, c = np.stack([p[0] for p in planes], 1), np.array([p[1] for p in planes])
    dn = d @ N
    with np.errstate(all="ignore"):
        t = (c[None, :] - o @ N) / dn
    t[~((dn != 0) & (t > 0))] = np.inf
    t[np.nonzero(last >= 0)[0], last[last >= 0]] = np.inf
    best_t, best_i = np.full(m, np.inf), np.full(m, -1, np.int64)
    todo = np.arange(m)
    while len(todo):
        i = t[todo].argmin(1)
        ti = t[todo, i]
        todo, i, ti = todo[np.isfinite(ti)], i[np.isfinite(ti)], ti[np.isfinite(ti)]
        p = o[todo] + ti[:, None] * d[todo]
        inside = np.zeros(len(todo), bool)
        for k in np.unique(i):
            inside[i == k] = ((p[i == k] @ planes[k][2] - planes[k][3]) >= -EDGE_ROUNDING).all(1)
        best_t[todo[inside]], best_i[todo[inside]] = ti[inside], i[inside]
        t[todo[~inside], i[~inside]] = np.inf
        todo = todo[~inside]
    return best_t, best_i


def snell(d, nrm, cos, ratio):
    """the refracted unit direction of Snell's law: the tangential part of d scaled by the ratio of the indices, the rest along -nrm
    (nrm: the unit normal against the ray, cos = -d . nrm; the caller has excluded total reflection)"""
    tang = ratio[:, None] * (d + cos[:, None] * nrm)
    return tang - np.sqrt(1.0 - (tang * tang).sum(1))[:, None] * nrm


def outside_convex(glass, polygon):
    """True when the convex planar polygon (k, 3) shares no point with the closed convex body bounded by the polygons `glass` (outward
    windings): clipping it against every face's inner half space (Sutherland-Hodgman) leaves nothing"""
    pts = [np.asarray(p, np.float64) for p in polygon]
    for N, c, _, _ in polygon_planes(glass):
        nxt = []
        for a, b in zip(pts, pts[1:] + pts[:1]):
            sa, sb = N @ a - c, N @ b - c
            if sa <= 0:
                nxt.append(a)
            if (sa <= 0) != (sb <= 0):
                nxt.append(a + (b - a) * sa / (sa - sb))
        pts = nxt
        if not pts:
            return True
    return False


CHUNK = 1 << 14


def glass_paths(polys, kinds, o, d, n, bounce_limit, record=None):
    """The probability that a camera path ends on the emitter, by enumeration, for scenes of flat faces: planar convex polygons `polys`,
    kinds[i] GLASS (one body of glass, windings outward) or EMITTER, black background.  o, d (m, 3): origins and UNIT directions, n (m,):
    the refractive index of each ray's hero wavelength (rays x wavelengths, flattened by the caller).  Float64, numpy only.
    Every step takes the nearest hit over all polygons.  At a glass face, as the reference documents its dielectric (the model
    slab_transmission restates): the cosine on the incoming side, the ratio 1 / n entering and n leaving; ratio sin > 1 reflects with
    probability 1, otherwise the ray reflects with probability R = schlick(cos, ratio) and refracts by Snell with 1 - R.  The path that
    stays inside the glass is followed on (its weight is the product of its R); every refracted branch that leaves is scored at once: it
    runs straight to the emitter, whose hit must be hit number <= bounce_limit, or to nothing.  ASSERTED, not assumed: a camera ray meets
    glass first or nothing; the branch reflected off the outside meets nothing (such a path would carry seven wavelengths: not this
    function's case); a ray inside the glass meets glass, from inside (the body is closed and holds no emitter); a ray that has left the
    glass does not enter it again.  The 1e-4 offset along the normal that the renderer gives every scattered origin is IGNORED: it moves
    a path sideways by at most 1e-4 tan(angle) per hit, far below a pixel's footprint on any face here.
    record: a list that receives (hit number of the exit, rows of the input, exit point, exit direction, weight) per scored branch."""
    if len(o) > CHUNK and record is None:               # (arrays that stay in the cache: the work is bound by memory)
        return np.concatenate([glass_paths(polys, kinds, o[a:a + CHUNK], d[a:a + CHUNK], n[a:a + CHUNK], bounce_limit)
                               for a in range(0, len(o), CHUNK)])
    planes = polygon_planes(polys)
    kinds = np.asarray(kinds)
    normal = np.stack([p[0] for p in planes])
    o, d, n = np.array(o, np.float64), np.array(d, np.float64), np.array(n, np.float64)
    P = np.zeros(o.shape[0])
    t, i = nearest_polygon(planes, o, d, np.full(o.shape[0], -1))
    rows = np.nonzero(i >= 0)[0]
    if bounce_limit < 3 or not len(rows):
        return P
    o, d, n, t, i = o[rows], d[rows], n[rows], t[rows], i[rows]
    assert (kinds[i] == GLASS).all(), "glass_paths: a camera ray meets the emitter directly"
    N = normal[i]
    cos = np.minimum(-(d * N).sum(1), 1.0)
    assert (cos > 0).all(), "glass_paths: a camera ray meets the glass from inside"
    ratio = 1.0 / n
    assert (ratio * np.sqrt(1.0 - cos * cos) <= 1.0).all()
    w = 1.0 - schlick(cos, ratio)
    o = o + t[:, None] * d
    assert (nearest_polygon(planes, o, d + 2.0 * cos[:, None] * N, i)[1] < 0).all(), "glass_paths: a reflection off the outside meets something"
    d, last = snell(d, N, cos, ratio), i
    for hit in range(2, bounce_limit):                   # the exit is hit number `hit`, the emitter's hit + 1 <= bounce_limit
        t, i = nearest_polygon(planes, o, d, last)
        assert (i >= 0).all(), "glass_paths: a ray inside the glass meets nothing (the body is open)"
        assert (kinds[i] == GLASS).all(), "glass_paths: the emitter is met from inside the glass"
        N = normal[i]
        cos = np.minimum((d * N).sum(1), 1.0)
        assert (cos > 0).all(), "glass_paths: a ray inside the glass meets a face from outside"
        o = o + t[:, None] * d
        goes = n * np.sqrt(1.0 - cos * cos) <= 1.0       # the reference reflects when ratio sin > 1
        R = np.where(goes, schlick(cos, n), 1.0)
        k = np.nonzero(goes)[0]
        if len(k):
            out = snell(d[k], -N[k], cos[k], n[k])
            j = nearest_polygon(planes, o[k], out, i[k])[1]
            assert (kinds[j[j >= 0]] == EMITTER).all(), "glass_paths: a ray that has left the glass enters it again"
            P[rows[k]] += w[k] * (1.0 - R[k]) * (j >= 0)
            if record is not None:
                record.append((hit, rows[k], o[k], out, w[k] * (1.0 - R[k])))
        d, last, w = d - 2.0 * cos[:, None] * N, i, w * R
    return P


JUMP = 0.02       # a change of P between neighbouring hero nodes above this counts as a jump (smooth changes are far below it)


def hero_moments(cmf, factors, prob, rays, nodes, refine):
    """E and the raw second moment (3, rays) of one path's XYZ contribution, and P (rays,) that it contributes, for paths that carry the
    hero wavelength alone (path_moments(hero_only=True)) and contribute with probability prob(ray numbers, hero wavelengths), which is
    piecewise smooth in the wavelength and JUMPS where a path changes its faces (total reflection, an emitter's edge).  Midpoint
    quadrature over hero_nodes(nodes); every cell next to a pair of nodes between which prob changes by more than JUMP is evaluated
    again on `refine` midpoints of its own, so that a jump is located to 470 / (nodes refine) nm."""
    def f(h):
        p = np.ones_like(h)
        for tab in factors:
            p = p * interp(np.asarray(tab, np.float64), h)
        return np.stack([interp(cmf[c], h) * p * STEP for c in range(3)])
    h0 = hero_nodes(nodes)
    P0 = prob(np.repeat(np.arange(rays), nodes), np.tile(h0, rays)).reshape(rays, nodes)
    jump = np.abs(np.diff(P0, axis=1)) > JUMP
    fine = np.zeros((rays, nodes), bool)
    fine[:, :-1] |= jump; fine[:, 1:] |= jump
    f0 = f(h0)
    coarse = np.where(fine, 0.0, P0)
    E, M2, P = f0 @ coarse.T / nodes, (f0 * f0) @ coarse.T / nodes, coarse.mean(1)
    r, k = np.nonzero(fine)
    if len(r) and refine > 1:
        h1 = LAMBDA_MIN + (k[:, None] + (np.arange(refine)[None, :] + 0.5) / refine) * (LAMBDA_MAX - LAMBDA_MIN) / nodes
        P1 = prob(np.repeat(r, refine), h1.ravel()).reshape(len(r), refine)
        f1 = f(h1.ravel()).reshape(3, len(r), refine)
        for c in range(3):
            E[c] += np.bincount(r, (f1[c] * P1).sum(1), rays) / (nodes * refine)
            M2[c] += np.bincount(r, (f1[c] ** 2 * P1).sum(1), rays) / (nodes * refine)
        P += np.bincount(r, P1.sum(1), rays) / (nodes * refine)
    else:
        E, M2, P = f0 @ P0.T / nodes, (f0 * f0) @ P0.T / nodes, P0.mean(1)
    return E, M2, P


def hero_nodes(nodes):
    """the midpoint nodes of path_moments over the hero wavelength"""
    return LAMBDA_MIN + (np.arange(nodes) + 0.5) * (LAMBDA_MAX - LAMBDA_MIN) / nodes


def fuzz_share(cos, fuzz):
    """the share of a fuzzed metal's reflections that scatter: reflected + fuzz u, u uniform on the unit sphere, is absorbed when it
    points into the surface.  u . n is uniform on [-1, 1] (Archimedes), reflected . n = cos: 1 - max(0, (1 - cos / fuzz) / 2)"""
    return 1.0 - np.maximum(0.0, (1.0 - np.asarray(cos, np.float64) / fuzz) / 2.0)


def sphere_nodes(nh, na):
    """nh x na unit vectors, midpoints of a grid uniform in the height along y and in the azimuth: equal areas of the unit sphere"""
    c = -1.0 + (np.arange(nh) + 0.5) * 2.0 / nh
    a = (np.arange(na) + 0.5) * 2.0 * np.pi / na
    s = np.sqrt(1.0 - c * c)
    return np.stack([np.outer(s, np.cos(a)), np.outer(c, np.ones(na)), np.outer(s, np.sin(a))], -1).reshape(-1, 3)


def light_in_reach(x, r, fuzz, light):
    """False for the points x whose cone of directions r + fuzz u (within asin(fuzz) of r) cannot reach the cap that holds the triangle"""
    v = light[None, :, :] - x[:, None, :]
    vu = v / np.linalg.norm(v, axis=2)[:, :, None]
    cu = unit(vu.mean(1))
    cap = np.arccos(np.clip((vu * cu[:, None, :]).sum(2), -1, 1)).max(1)      # the spherical triangle lies in this cap about cu
    return np.arccos(np.clip((r * cu).sum(1), -1, 1)) <= np.arcsin(fuzz) + cap + 1e-9


def fuzz_light_share_sampled(x, r, fuzz, light, nh, na):
    """per floor point x (m, 3) (normal +y) with unit reflected direction r: the share of the unit sphere of u for which r + fuzz u points
    above the floor and meets the triangle `light` (3, 3), wholly above it, by counting sphere_nodes(nh, na): the plain statement of the
    quantity, which fuzz_light_share is checked against (its error falls only like 1 / sqrt(nh na): too slow for the cases).  A point
    whose cone of directions (within asin(fuzz) of r) cannot reach the cap that holds the light has share exactly 0 and is skipped."""
    assert fuzz < 1.0 and (light[:, 1] > 0).all()
    v = light[None, :, :] - x[:, None, :]                                     # (m, 3, 3) the corners as seen from x
    share = np.zeros(x.shape[0])
    k = np.nonzero(light_in_reach(x, r, fuzz, light))[0]
    if not len(k):
        return share
    # a direction D from x meets the triangle when it lies in the cone of its corners: D . (v_i x v_i+1) all have the sign of det(v)
    edge = np.cross(v[k], np.roll(v[k], -1, axis=1))                          # (m', 3, 3)
    det = (edge[:, 0] * v[k][:, 2]).sum(1)
    edge = edge * np.sign(det)[:, None, None]
    u = fuzz * sphere_nodes(nh, na)
    for a in range(0, len(k), 256):
        D = r[k[a:a + 256], None, :] + u[None, :, :]                          # (b, K, 3)
        s = np.einsum("bkc,bec->bke", D, edge[a:a + 256])
        share[k[a:a + 256]] = ((s >= 0).all(2) & (D[:, :, 1] > 0)).mean(1)
    return share


def fuzz_light_share(x, r, fuzz, light, na):
    """the same share, exact along one variable.  With u = cos(psi) r + sin(psi) e, e the unit vector across r at the azimuth phi and psi
    in [0, pi], the sphere's area element is sin(psi) dpsi dphi, and r + fuzz u stays in the half plane of r and e, at the angle
    theta = atan2(fuzz sin psi, 1 + fuzz cos psi) from r.  That half plane cuts the triangle in a segment, which spans an interval of
    theta; every theta in it below asin(fuzz) is reached by two psi, fuzz sin(psi - theta) = sin(theta), and the integral of sin(psi)
    over both pre-images is elementary.  Midpoint quadrature over na azimuths of the arc the triangle spans about r (all of them when
    r points into the triangle); the integrand is continuous in phi."""
    assert fuzz < 1.0 and (light[:, 1] > 0).all() and (np.abs(r[:, 1]) < 0.999).all()
    reach = light_in_reach(x, r, fuzz, light)
    if not reach.all():                                                         # (the others' share is exactly 0)
        out = np.zeros(x.shape[0])
        if reach.any():
            out[reach] = fuzz_light_share(x[reach], r[reach], fuzz, light, na)
        return out
    v = light[None, :, :] - x[:, None, :]                                       # (m, 3, 3) the corners as seen from x
    assert (v[:, :, 1] > 0).all()                                               # (the light is above the floor: so is every direction to it)
    e1 = unit(np.cross(r, np.array([0.0, 1.0, 0.0]))); e2 = np.cross(r, e1)
    az = np.arctan2(np.einsum("mkc,mc->mk", v, e2), np.einsum("mkc,mc->mk", v, e1))
    rel = (az - az[:, :1] + np.pi) % (2.0 * np.pi) - np.pi                      # the corners' azimuths about r, from the first one's
    side = np.einsum("mkc,mc->mk", np.cross(v, np.roll(v, -1, axis=1)), r)
    within = (side >= 0).all(1) | (side <= 0).all(1)                            # r points into the triangle
    start = np.where(within, 0.0, az[:, 0] + rel.min(1))
    width = np.where(within, 2.0 * np.pi, rel.max(1) - rel.min(1))
    tmax = np.arcsin(fuzz)
    near = lambda t: t + np.arcsin(np.clip(np.sin(t) / fuzz, -1, 1))
    far = lambda t: t + np.pi - np.arcsin(np.clip(np.sin(t) / fuzz, -1, 1))
    share = np.zeros(x.shape[0])
    for q in range(na):
        phi = start + (q + 0.5) / na * width
        e = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
        w = np.einsum("mkc,mc->mk", v, np.cross(r, e))                          # the corners' distances from the plane of r and e
        cut = np.zeros(v.shape[:1] + (2, 3)); found = np.zeros(v.shape[0], np.int64)
        for i, j in ((0, 1), (1, 2), (2, 0)):
            k = np.nonzero(((w[:, i] <= 0) != (w[:, j] <= 0)) & (found < 2))[0]
            s = w[k, i] / (w[k, i] - w[k, j])
            cut[k, found[k]] = v[k, i] + s[:, None] * (v[k, j] - v[k, i]); found[k] += 1
        k = np.nonzero(found == 2)[0]
        a, b = np.einsum("kpc,kc->kp", cut[k], r[k]), np.einsum("kpc,kc->kp", cut[k], e[k])
        k, a, b = k[(b > 0).any(1)], a[(b > 0).any(1)], b[(b > 0).any(1)]
        # the part of the segment in the half plane b >= 0: an end behind it moves to the crossing of the axis, theta = 0
        s = np.where(b < 0, b / (b - b[:, ::-1]), 0.0)
        a, b = a + s * (a[:, ::-1] - a), np.where(b < 0, 0.0, b)
        th = np.clip(np.arctan2(b, a), 0.0, tmax)
        lo, hi = th.min(1), th.max(1)
        share[k] += ((np.cos(near(lo)) - np.cos(near(hi))) + (np.cos(far(hi)) - np.cos(far(lo)))) * width[k] / na
    return share / (4.0 * np.pi)


def disk_polygon_area(Q):
    """area of the intersection of the unit disk about the origin with polygons Q (m, k, 2): per edge A -> B the signed area between the
    origin and the edge clipped to the disk, a triangle where the edge runs inside and a sector where it runs outside"""
    total = np.zeros(Q.shape[0])
    cross = lambda a, b: a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    sector = lambda a, b: 0.5 * np.arctan2(cross(a, b), (a * b).sum(1))
    for i in range(Q.shape[1]):
        A, B = Q[:, i], Q[:, (i + 1) % Q.shape[1]]
        d = B - A
        a, b, c = (d * d).sum(1), 2.0 * (A * d).sum(1), (A * A).sum(1) - 1.0
        disc = b * b - 4.0 * a * c
        root = np.sqrt(np.maximum(disc, 0.0))
        t1 = np.where(disc > 0, np.clip((-b - root) / (2.0 * a), 0.0, 1.0), 0.0)
        t2 = np.where(disc > 0, np.clip((-b + root) / (2.0 * a), 0.0, 1.0), 0.0)
        P1, P2 = A + t1[:, None] * d, A + t2[:, None] * d
        total += sector(A, P1) + 0.5 * cross(P1, P2) + sector(P2, B)
    return np.where(np.abs(total) < 1e-12, 0.0, np.abs(total))              # (sectors alone: a rounding residue of the winding number 0)


def lens_coverage(cam, tri, W, H, k):
    """the same P, exact over the lens: from a point p of the pixel grid the triangle `tri`, between lens and grid, projects onto the lens
    plane as a triangle, and the share of the lens disk from which the ray to p meets it is the area the two have in common / pi.
    Averaged over k x k midpoint sub-samples of every pixel's square."""
    g = lambda name: np.array(getattr(cam, name)[:], np.float64)
    C, U, V = g("camera_center"), g("defocus_disk_u"), g("defocus_disk_v")
    _, p00, du, dv = camera_arrays(cam)
    j, i = np.mgrid[0:H, 0:W]
    acc = np.zeros(W * H)
    for a in range(k):
        for b in range(k):
            p = p00[None, :] + (i.ravel()[:, None] + (a + 0.5) / k - 0.5) * du[None, :] + (j.ravel()[:, None] + (b + 0.5) / k - 0.5) * dv[None, :]
            Q = np.zeros((W * H, 3, 2))
            for c in range(3):                             # C + a U + b V = p + s (corner - p)
                M = np.stack([np.broadcast_to(U, p.shape), np.broadcast_to(V, p.shape), p - tri[c][None, :]], axis=2)
                sol = np.linalg.solve(M, (p - C[None, :])[:, :, None])[:, :, 0]
                assert (sol[:, 2] > 1).all(), "lens: the triangle must lie between the lens and the pixel grid"
                Q[:, c] = sol[:, :2]
            acc += disk_polygon_area(Q) / np.pi
    return acc / (k * k)


def lens_points(cam, nr, na):
    """nr x na points of the thin lens, midpoints of a polar grid of equal areas: camera_center + p_x defocus_disk_u + p_y defocus_disk_v
    with p uniform on the unit disk (the reference's documented disk sample)"""
    g = lambda name: np.array(getattr(cam, name)[:], np.float64)
    rad = np.sqrt((np.arange(nr) + 0.5) / nr)
    a = (np.arange(na) + 0.5) * 2.0 * np.pi / na
    px, py = np.outer(rad, np.cos(a)).ravel(), np.outer(rad, np.sin(a)).ravel()
    return g("camera_center")[None, :] + px[:, None] * g("defocus_disk_u")[None, :] + py[:, None] * g("defocus_disk_v")[None, :]


def lens_coverage_sampled(cam, tri, W, H, nr, na, k):
    """P (H * W,) that a camera ray of each pixel meets the triangle `tri` (3, 3), nothing else in its way, through the thin lens: the ray
    runs from a lens point L to the pixel sample ON THE PIXEL GRID, which lies in the focus plane, so that from L the triangle covers
    its central projection from L onto the grid.  The mean of coverage_map of that projection over lens_points(nr, na): the plain
    statement of the quantity, which lens_coverage is checked against.  Also returns the image total, the mean of polygon_area: the
    projection is affine in L, the area quadratic, and the polar midpoint grid integrates a quadratic exactly (nr >= 1, na >= 3)."""
    cov, area = np.zeros(W * H), 0.0
    L = lens_points(cam, nr, na)
    for eye in L:
        Q, depth = project_points(cam, tri, eye)
        assert (depth > 0).all() and (Q.min(0) > -0.5).all() and (Q[:, 0].max() < W - 0.5) and (Q[:, 1].max() < H - 0.5), "lens: out of view"
        cov += coverage_map(Q, W, H, k); area += polygon_area(Q)
    return cov / len(L), area / len(L)


def form_factor(x, n, polygon):
    """Lambert's closed form for the cosine-weighted form factor of a planar polygon (k, 3) seen from points x (m, 3) with unit normal n:
    F = |sum_i gamma_i (r_i x r_i+1) . n / |r_i x r_i+1|| / (2 pi), gamma_i the angle the edge subtends.  F is the probability that a
    cosine-distributed direction about n hits the polygon.  The polygon must lie wholly above the receiver's horizon."""
    x, n, polygon = np.asarray(x, np.float64), np.asarray(n, np.float64), np.asarray(polygon, np.float64)
    r = polygon[None, :, :] - x[:, None, :]
    assert ((r @ n) > 0).all(), "form_factor: polygon below the horizon"
    r = r / np.linalg.norm(r, axis=2)[:, :, None]
    F = np.zeros(x.shape[0])
    k = polygon.shape[0]
    for i in range(k):
        a, b = r[:, i], r[:, (i + 1) % k]
        cr = np.cross(a, b)
        nc = np.linalg.norm(cr, axis=1)
        F += np.arctan2(nc, (a * b).sum(1)) * (cr @ n) / nc
    return np.abs(F) / (2.0 * np.pi)


# ---- pixels -------------------------------------------------------------------------------------------------------------------
def lane_index(W, H, tx=TX, ty=TY):
    """index of pixel (x, y) in the block-linear planes of a W x H frame (blocks of tx x ty, W // tx + 1 blocks per row), shape (H, W)"""
    bx = W // tx + 1
    y, x = np.mgrid[0:H, 0:W]
    return ((y // ty) * bx + x // tx) * tx * ty + (y % ty) * tx + x % tx


def camera_arrays(cam):
    """eye, pixel00, delta_u, delta_v of a camera struct, float64"""
    g = lambda name: np.array(getattr(cam, name)[:], np.float64)
    return g("camera_center"), g("pixel00_loc"), g("pixel_delta_u"), g("pixel_delta_v")


def pixel_rays(cam, W, H, fx=0.0, fy=0.0):
    """origin (3,) and directions (H * W, 3) of the rays through pixel (i + fx, j + fy), row-major; (0, 0) is the pixel centre"""
    eye, p00, du, dv = camera_arrays(cam)
    j, i = np.mgrid[0:H, 0:W]
    px = p00[None, :] + (i.ravel()[:, None] + fx) * du[None, :] + (j.ravel()[:, None] + fy) * dv[None, :]
    return eye, px - eye[None, :]


def footprint_average(fn, cam, W, H, k):
    """average of fn(eye, directions) -> (H * W,) over every pixel's jitter square, k x k midpoint sub-samples"""
    acc = np.zeros(W * H)
    for a in range(k):
        for b in range(k):
            eye, d = pixel_rays(cam, W, H, (a + 0.5) / k - 0.5, (b + 0.5) / k - 0.5)
            acc += fn(eye, d)
    return acc / (k * k)


def project_points(cam, P, eye=None):
    """perspective projection of points P (k, 3) into continuous pixel coordinates (i, j): pixel (x, y) is the square
    [x - 0.5, x + 0.5] x [y - 0.5, y + 0.5].  Also returns the depth s (eye + s (P - eye) lies on the image plane; s > 0 in front).
    eye: the centre of projection (default: the camera's centre; a lens point projects onto the same pixel grid)."""
    centre, p00, du, dv = camera_arrays(cam)
    eye = centre if eye is None else np.asarray(eye, np.float64)
    out = np.zeros((len(P), 2)); depth = np.zeros(len(P))
    for k, p in enumerate(np.asarray(P, np.float64)):
        i, j, s = np.linalg.solve(np.stack([du, dv, -(p - eye)], axis=1), eye - p00)
        out[k] = (i, j); depth[k] = s
    return out, depth


def polygon_area(Q):
    """area of a planar polygon (k, 2), shoelace formula"""
    x, y = Q[:, 0], Q[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def coverage_map(Q, W, H, k):
    """share of every pixel's square inside the triangle Q (3, 2) of pixel coordinates, k x k midpoint sub-samples, shape (H * W,)"""
    j, i = np.mgrid[0:H, 0:W]
    acc = np.zeros(W * H)
    e = lambda a, b, px, py: (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
    for a in range(k):
        for b in range(k):
            px, py = i.ravel() + (a + 0.5) / k - 0.5, j.ravel() + (b + 0.5) / k - 0.5
            s = [e(Q[0], Q[1], px, py), e(Q[1], Q[2], px, py), e(Q[2], Q[0], px, py)]
            acc += (((s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)) | ((s[0] <= 0) & (s[1] <= 0) & (s[2] <= 0)))
    return acc / (k * k)


def coverage_exact(Q, W, H):
    """share of every pixel's square inside the convex polygon Q (k, 2) of pixel coordinates, exact: the polygon clipped to the square
    (Sutherland-Hodgman), shape (H * W,).  Where a pixel's variance hangs on 1 - P, sub-samples are too coarse."""
    out = np.zeros((H, W))
    Q = np.asarray(Q, np.float64)
    for y in range(max(0, int(np.floor(Q[:, 1].min() + 0.5))), min(H, int(np.ceil(Q[:, 1].max() + 0.5)))):
        for x in range(max(0, int(np.floor(Q[:, 0].min() + 0.5))), min(W, int(np.ceil(Q[:, 0].max() + 0.5)))):
            pts = [q for q in Q]
            for axis, bound, sign in ((0, x - 0.5, 1.0), (0, x + 0.5, -1.0), (1, y - 0.5, 1.0), (1, y + 0.5, -1.0)):
                nxt = []
                for a, b in zip(pts, pts[1:] + pts[:1]):
                    sa, sb = sign * (a[axis] - bound), sign * (b[axis] - bound)
                    if sa >= 0:
                        nxt.append(a)
                    if (sa >= 0) != (sb >= 0):
                        nxt.append(a + (b - a) * sa / (sa - sb))
                pts = nxt
                if not pts:
                    break
            if len(pts) >= 3:
                out[y, x] = polygon_area(np.array(pts))
    return out.ravel()


def mirror_y(P):
    """points mirrored in the plane y = 0"""
    return np.asarray(P, np.float64) * np.array([1.0, -1.0, 1.0])


def z_scores(xyz_planes, W, H, spp, E, Var, min_expected=None, p_contribute=None, E_sum=None):
    """z_img (3,) = (sum measured - sum E) / sqrt(sum Var / spp) of the per-pixel means, the allowance sum E spp 2^-24 of the float32
    sums in the same units, the per-pixel z (3, n) over the pixels with spp P(contribute) >= min_expected (all if None).
    xyz_planes: the three block-linear planes of XYZ sums; E, Var: (3,) or (3, H * W) per path; E_sum: the image total of E where a
    closed form knows it better than the sum of the sub-sampled per-pixel values (the mirror's projected area)."""
    ln = lane_index(W, H).ravel()
    E = np.broadcast_to(np.asarray(E, np.float64).reshape(3, -1), (3, W * H))
    Var = np.broadcast_to(np.asarray(Var, np.float64).reshape(3, -1), (3, W * H))
    m = np.stack([np.asarray(xyz_planes[c], np.float64)[ln] / spp for c in range(3)])
    sigma = np.sqrt(Var.sum(1) / spp)
    total = E.sum(1) if E_sum is None else np.asarray(E_sum, np.float64)
    z_img = (m.sum(1) - total) / sigma
    allowance = spp * U * np.abs(total) / sigma
    sel = np.ones(W * H, bool) if min_expected is None else spp * np.asarray(p_contribute) >= min_expected
    with np.errstate(all="ignore"):
        z_px = (m[:, sel] - E[:, sel]) / np.sqrt(Var[:, sel] / spp)
    return z_img, allowance, z_px


# ---- spectra ------------------------------------------------------------------------------------------------------------------
def ramp(lo=0.2, hi=0.9):
    return np.linspace(lo, hi, N_GRID).astype(np.float32)


def bump(base=0.3, height=0.6, centre=560.0, width=60.0):
    lam = LAMBDA_MIN + 5.0 * np.arange(N_GRID)
    return (base + height * np.exp(-0.5 * ((lam - centre) / width) ** 2)).astype(np.float32)


def baked_emission(d65n, power):
    """what the reference bakes for a white emitter of the given power: power^2 D65n, sampled at 360 + i 470/95 (Q4: the bake steps by
    470/95 while the grid it is read back on steps by 470/94), float64"""
    lam = LAMBDA_MIN + np.arange(N_GRID) * (LAMBDA_MAX - LAMBDA_MIN) / N_GRID
    return float(power) ** 2 * interp(np.asarray(d65n, np.float64), lam)


# ---- scenes on raw arrays -----------------------------------------------------------------------------------------------------
def material(mtype, spectrum, fuzz=0.0, power=0.0, B=BK7_B, C=BK7_C, bake=False, col=(1.0, 1.0, 1.0)):
    """one material; spectrum: 95 floats set DIRECTLY into spectral_distribution (bake=True: left to the implementation's own bake of
    `col` / `power`, for the test of that bake)"""
    return dict(type=int(mtype), spectrum=None if bake else np.asarray(spectrum, np.float32), fuzz=float(fuzz), power=float(power),
                B=tuple(B), C=tuple(C), bake=bool(bake), col=tuple(col))


def scene(V, mats, mat_index=None, aa_plane=None, background=None):
    """a scene as plain arrays: V (n, 3, 3) float32; mat_index defaults to one material per triangle (mat_index then NAMES the triangle
    hit: mats may be one material, repeated); background: 95 floats, default black"""
    V = np.asarray(V, np.float32).reshape(-1, 3, 3)
    n = V.shape[0]
    if mat_index is None:
        mat_index = np.arange(n)
        if len(mats) == 1:
            mats = list(mats) * n
    assert len(mat_index) == n and max(mat_index) < len(mats)
    return dict(V=V, mats=list(mats), mat_index=np.asarray(mat_index, np.int64),
                aa_plane=np.zeros(n, np.int64) if aa_plane is None else np.asarray(aa_plane, np.int64),
                background=np.zeros(N_GRID, np.float32) if background is None else np.asarray(background, np.float32))


def to_structs(sc, TriIn, Material, bake):
    """ctypes arrays (TriIn * n, Material * m) and the background of a scene, in the caller's struct classes; bake(byref-able Material)
    is called for the materials that ask for the implementation's own bake"""
    T = (TriIn * len(sc["V"]))()
    for k, v in enumerate(sc["V"]):
        T[k].v0[:] = [float(x) for x in v[0]]; T[k].v1[:] = [float(x) for x in v[1]]; T[k].v2[:] = [float(x) for x in v[2]]
        T[k].mat_index = int(sc["mat_index"][k]); T[k].aa_plane = int(sc["aa_plane"][k])
    M = (Material * len(sc["mats"]))()
    for k, m in enumerate(sc["mats"]):
        M[k].col[:] = m["col"]; M[k].reflection_fuzz = m["fuzz"]; M[k].material_type = m["type"]; M[k].emission_power = m["power"]
        M[k].sellmeier_B[:] = m["B"]; M[k].sellmeier_C[:] = m["C"]
        if m["bake"]:
            bake(M[k])
        else:
            M[k].spectral_distribution[:] = [float(x) for x in m["spectrum"]]
    return T, M, sc["background"]


def product_scene(srt, sc, mode, seed=1984):
    """the scene handed to the package `srt` (passed in: nothing is imported here) through its raw-array boundary, tree built by `mode`"""
    import ctypes as C
    B = srt.binding
    T, M, bg = to_structs(sc, B.TriIn, B.Material, lambda m: B.check(B.lib().srt_material_bake(C.byref(m))))
    return srt.Scene.from_arrays(T, M, bg).build_bvh(mode, seed)


def color_tables(srt):
    """rows x, y, z, normalised D65 of srt_color_tables, (4, 95) float64"""
    B = srt.binding
    cmf, m = np.zeros(N_GRID * 4, np.float32), np.zeros(9, np.float32)
    B.check(B.lib().srt_color_tables(B.fptr(cmf), B.fptr(m)))
    return cmf.reshape(N_GRID, 4).T.astype(np.float64)


GREY = material(MAT_LAMBERTIAN, ramp())


def quad(a, b, c, d):
    """two triangles a b c, a c d"""
    return [[a, b, c], [a, c, d]]


def soup(seed, n, spread):
    """n random triangles: vertices normally spread about centres in [-5, 5]^3; triangles whose projection (XY: aa_plane NONE) is
    degenerate (|n_z| < 0.05) are drawn again"""
    rng = np.random.default_rng(seed)
    V = np.zeros((n, 3, 3), np.float32)
    k = 0
    while k < n:
        v = (rng.uniform(-5, 5, 3)[None, :] + rng.normal(0, spread, (3, 3))).astype(np.float32)
        if projected_normal(v[None], [AAP_NONE])[0] >= MIN_PROJECTED_NORMAL:
            V[k] = v; k += 1
    return scene(V, [GREY])


SHEET_N = 12


def sheet_vertices(seed=7, n=SHEET_N):
    """(n + 1)^2 vertices of a bumpy sheet over [-5, 5]^2: grid points moved by +-0.15 in x and y, z = bumps of +-0.25 (a height
    field: every |n_z| is far above 0.05, and a ray steeper than its slopes crosses it once)"""
    rng = np.random.default_rng(seed)
    g = np.linspace(-5, 5, n + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    x = x + np.where((np.abs(x) < 5), rng.uniform(-0.15, 0.15, x.shape), 0)
    y = y + np.where((np.abs(y) < 5), rng.uniform(-0.15, 0.15, y.shape), 0)
    return np.stack([x, y, rng.uniform(-0.25, 0.25, x.shape)], axis=-1).astype(np.float32)


def bumpy_sheet(seed=7, n=SHEET_N):
    """closed n x n sheet of 2 n^2 triangles sharing the grid's vertices bit for bit.  Returns the scene and idx (2 n^2, 3), the grid
    vertex numbers (a * (n + 1) + b) of every triangle."""
    P = sheet_vertices(seed, n)
    vid = lambda a, b: a * (n + 1) + b
    idx = []
    for a in range(n):
        for b in range(n):
            idx += [(vid(a, b), vid(a + 1, b), vid(a + 1, b + 1)), (vid(a, b), vid(a + 1, b + 1), vid(a, b + 1))]
    idx = np.array(idx)
    return scene(P.reshape(-1, 3)[idx], [GREY]), idx


def random_rays(seed, m):
    """m rays from origins in [-12, 12]^3 aimed at points of [-5, 5]^3, float32 (m, 6)"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-12, 12, (m, 3)).astype(np.float32)
    tgt = rng.uniform(-5, 5, (m, 3)).astype(np.float32)
    return np.concatenate([o, tgt - o], axis=1).astype(np.float32)


def edge_aimed_rays(seed=17, reps=8):
    """rays aimed EXACTLY (up to the float32 rounding of the direction) at interior vertices, interior edge midpoints and random points
    of interior edges of the bumpy sheet, `reps` origins per target, from either side and steeper than the sheet's slopes (one
    crossing).  Returns rays (m, 6) and, per ray, the boolean row of the triangles adjacent to its target: those that share the
    vertex, or both ends of the edge -- every triangle that contains the target point."""
    sc, idx = bumpy_sheet()
    n = SHEET_N
    P = sheet_vertices().reshape(-1, 3).astype(np.float64)
    rng = np.random.default_rng(seed)
    interior = lambda v: 0 < v // (n + 1) < n and 0 < v % (n + 1) < n
    edges = set()
    for tri in idx:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            e = (min(tri[a], tri[b]), max(tri[a], tri[b]))
            if interior(e[0]) or interior(e[1]):
                edges.add(e)
    edges = sorted(edges)
    targets, adjacent = [], []
    for v in range((n + 1) ** 2):
        if interior(v):
            targets.append(P[v]); adjacent.append((idx == v).any(1))
    for a, b in edges:
        both = (idx == a).any(1) & (idx == b).any(1)
        # a ray aimed at an edge point can, after rounding, pass either side of it, and so through any triangle at the edge
        for s in [0.5] + list(rng.uniform(0.02, 0.98, 2)):
            targets.append((1 - s) * P[a] + s * P[b]); adjacent.append(both)
    targets, adjacent = np.array(targets), np.array(adjacent)
    targets, adjacent = np.repeat(targets, reps, axis=0), np.repeat(adjacent, reps, axis=0)
    m = len(targets)
    o = np.concatenate([targets[:, :2] + rng.uniform(-2.5, 2.5, (m, 2)), rng.choice([-1.0, 1.0], m)[:, None] * rng.uniform(4, 12, (m, 1))], axis=1)
    o = o.astype(np.float32)
    d = (targets.astype(np.float32) - o).astype(np.float32)
    return np.concatenate([o, d], axis=1), adjacent


def axis_aligned_set(seed=11):
    """explicit axis-aligned triangles in the planes XY / YZ / XZ (flagged as such, and flagged NONE: tri::init finds the plane
    itself), and STICKY ones: rotated about an axis so that the normal is no longer axis aligned while the flag keeps YZ or XZ, as the
    side quads of PRISM do (Q12).  Every projection is non-degenerate (component >= 0.05)."""
    rng = np.random.default_rng(seed)
    V, aa = [], []
    for plane, axis in ((AAP_XY, 2), (AAP_YZ, 0), (AAP_XZ, 1)):
        for flag in (plane, AAP_NONE, plane):
            v = rng.uniform(-4, 4, (3, 3))
            v[:, axis] = np.float32(rng.uniform(-4, 4))
            V.append(v); aa.append(flag)
    for plane, axis in ((AAP_YZ, 0), (AAP_XZ, 1)):
        for angle in (10.0, 35.0, 60.0, 80.0):
            v = rng.uniform(-4, 4, (3, 3))
            v[:, axis] = rng.uniform(-4, 4)
            c, s = np.cos(np.radians(angle)), np.sin(np.radians(angle))
            other = 2 if axis == 0 else 0                        # rotate about the remaining axis: the normal tilts from `axis` to `other`
            a, b = v[:, axis].copy(), v[:, other].copy()
            v[:, axis], v[:, other] = c * a - s * b, s * a + c * b
            V.append(v); aa.append(plane)
    sc = scene(np.array(V), [GREY], aa_plane=aa)
    assert (projected_normal(sc["V"], sc["aa_plane"]) >= MIN_PROJECTED_NORMAL).all()
    return sc


def degenerate_walls(seed=13, n=60):
    """n vertical walls (n_z = 0) that are NOT axis aligned: flagged NONE they are projected onto XY, where they are segments"""
    rng = np.random.default_rng(seed)
    V = []
    for _ in range(n):
        c = rng.uniform(-5, 5, 3); a = rng.uniform(0.3, np.pi / 2 - 0.3) + rng.integers(0, 4) * np.pi / 2
        e = np.array([np.cos(a), np.sin(a), 0.0]) * rng.uniform(1, 3)
        V.append([c - e, c + e, c + np.array([0, 0, rng.uniform(1, 3)])])
    return scene(np.array(V), [GREY])


# the random populations of both suites: name -> (scene builder, seed of the N_RAYS rays)
POPULATIONS = {
    "soup_30_spread_0.5": (lambda: soup(101, 30, 0.5), 201),
    "soup_30_spread_2.0": (lambda: soup(102, 30, 2.0), 202),
    "soup_200_spread_0.5": (lambda: soup(103, 200, 0.5), 203),
    "soup_200_spread_2.0": (lambda: soup(104, 200, 2.0), 204),
    "sheet_12x12": (lambda: bumpy_sheet()[0], 205),
    "axis_aligned_and_sticky": (axis_aligned_set, 206),      # explicit XY / YZ / XZ triangles and rotated ones that keep YZ / XZ (Q12)
}
N_RAYS = 20000
BUILTINS = ("CORNELL", "PRISM", "TRIS")
_cache = {}


def cached(key, make):
    """scenes, rays and their truth inputs are built once per session and shared (nothing mutates them)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def population(name):
    build, seed = POPULATIONS[name]
    return cached(("pop", name), lambda: (build(), random_rays(seed, N_RAYS)))


def builtin_report(srt, scene_id, trace):
    """4 000 camera rays (pixel centres of the 80 x 50 default view) of a built-in scene of the package `srt` against the truth;
    trace(scene, rays) -> (m, 4) is the implementation.  A ray DIFFERS when hit / miss or the material differs or t is off by more
    than C_T t_bound.  Returns the listed triangles (degenerate projection), the number of differing rays and {truth's triangle: count};
    asserts that every differing ray is near an edge or involves a listed triangle."""
    scene = srt.Scene.builtin(getattr(srt, "SCENE_" + scene_id)).build_bvh(srt.BVH_REFERENCE, 1984)
    T = scene.triangles()
    V = np.array([[t.v0[:], t.v1[:], t.v2[:]] for t in T], np.float32)
    aa = np.array([t.aa_plane for t in T]); mat = np.array([t.mat_index for t in T])
    listed = np.nonzero(projected_normal(V, aa) < MIN_PROJECTED_NORMAL)[0]
    cam = scene.default_camera(80, 50)
    eye, d = pixel_rays(cam, 80, 50)
    rays = np.concatenate([np.broadcast_to(eye, d.shape), d], 1).astype(np.float32)
    got = trace(scene, rays)
    Vd = f64(V)
    r = compare_hits(Vd, rays, got, mat)
    differ = ~r["same"] | (r["ratio"] > C_T)
    o, dd = f64(rays[:, :3]), f64(rays[:, 3:])
    involved = np.isin(r["tri"], listed)
    for k in listed:                 # the implementation hit a listed triangle: its t lies on that plane and its material is that one's
        tp = plane_t(Vd, np.full(len(rays), k), o, dd)
        with np.errstate(all="ignore"):
            involved |= r["got_hit"] & (got[:, 3] == mat[k]) & (np.abs(got[:, 0] - tp) <= 1e-4 * np.abs(tp))
    unexplained = differ & ~involved & (r["near"] >= EDGE_MARGIN)
    assert not unexplained.any(), (scene_id, np.nonzero(unexplained)[0][:5], r["tri"][unexplained][:5])
    by_tri = {}
    for k in r["tri"][differ]:
        by_tri[int(k)] = by_tri.get(int(k), 0) + 1
    return dict(scene=scene_id, triangles=len(V), hit_share=round(float(r["want_hit"].mean()), 3), listed=listed.tolist(),
                differ=int(differ.sum()), near_edge=int((differ & ~involved).sum()), by_truth_triangle=by_tri)


# radiometry scenes: (scene, camera arguments (vfov, eye, look-at), W, H, spp, depth)
FAR_TRIANGLE = [[[100, 100, 100], [101, 100, 100], [100, 101, 100]]]
FLOOR = quad([-50, 0, -40], [50, 0, -40], [50, 0, 60], [-50, 0, 60])     # y = 0; its diagonal passes x = 0 at z = 10, outside every view


def sky_only():
    bg = bump(0.2, 0.8, 520.0, 70.0)
    return scene(FAR_TRIANGLE, [GREY], background=bg), (40.0, (0, 1, 5), (0, 0, 0)), 48, 32, 64, 4


SPIKES = {0: 0.875, 37: 0.625, 60: 0.3125, 61: 0.75, 94: 0.4375}      # grid sample -> value: isolated tents, one pair of neighbours


def sky_spikes():
    """sky_only under a background that is 0 but at five grid samples: its interpolant is a few tents, so the film is non-zero in bins
    0, 1, 36 .. 38, 59 .. 62, 93 and 94 only, in fixed ratios -- the test of the bin geometry, the clamped last cell and the end bins"""
    bg = np.zeros(N_GRID, np.float32)
    for j, v in SPIKES.items():
        bg[j] = v
    sc, camera, W, H, spp, depth = sky_only()
    sc["background"] = bg
    return sc, camera, W, H, spp, depth


def floor_under_sky():
    return scene(FLOOR, [material(MAT_LAMBERTIAN, ramp())], mat_index=[0, 0], background=bump()), (30.0, (0, 3, 4), (0, 0, 0)), 48, 32, 64, 2


WALL_POWER = 2.0


def emissive_wall():
    wall = quad([-50, -40, 0], [50, -40, 0], [50, 60, 0], [-50, 60, 0])
    return (scene(wall, [material(MAT_EMISSIVE, None, power=WALL_POWER, bake=True)], mat_index=[0, 0]), (30.0, (0, 0, 5), (0, 0, 0)),
            48, 32, 64, 4)


LIGHT = np.array([(-1.0, 2.0, -0.5), (1.5, 2.5, 0.0), (0.0, 1.5, 1.5)], np.float32)


def cosine_law():
    V = FLOOR + [LIGHT]
    mats = [material(MAT_LAMBERTIAN, ramp()), material(MAT_EMISSIVE, bump(0.5, 6.0, 600.0, 80.0))]
    return scene(V, mats, mat_index=[0, 0, 1]), (25.0, (0, 1.5, 6), (0, 0, 1.5)), 40, 24, 256, 2


MIRROR_LIGHT = np.array([(-0.8, 2.2, -4.6), (0.9, 2.0, -4.2), (0.1, 2.8, -3.4)], np.float32)


def mirror():
    """a perfect mirror floor; the light is outside the view, its mirror image (y -> -y) wholly inside"""
    V = FLOOR + [MIRROR_LIGHT]
    mats = [material(MAT_METALLIC, ramp(0.9, 0.3)), material(MAT_EMISSIVE, bump(0.5, 4.0, 480.0, 50.0))]
    return scene(V, mats, mat_index=[0, 0, 1]), (30.0, (0, 2, 6), (0, 0, 0)), 48, 32, 64, 2


SLAB_DEPTH = 16      # the bounce limit: K = 6 internal round trips


def slab(incidence_deg, spp):
    """BK7 slab 0 >= z >= -1 (true Sellmeier C, spectrum 1, outward normals) in front of an emissive wall at z = -5, black background,
    a 2 degree view onto the origin at the given angle of incidence.  At 55 degrees Schlick's fifth power moves the transmission by
    2 % against a fourth power: 1 024 samples per pixel put the image's standard error at 0.12 % (64 would leave that at 4 sigma)."""
    front = quad([-50, -40, 0], [50, -40, 0], [50, 60, 0], [-50, 60, 0])              # normal +z
    back = quad([-50, -40, -1], [-50, 60, -1], [50, 60, -1], [50, -40, -1])           # normal -z
    wall = quad([-200, -190, -5], [200, -190, -5], [200, 210, -5], [-200, 210, -5])
    glass = material(MAT_DIELECTRIC, np.ones(N_GRID, np.float32), B=BK7_B, C=BK7_C)
    a = np.radians(incidence_deg)
    eye = (6.0 * np.sin(a), 0.0, 6.0 * np.cos(a))
    return (scene(front + back + wall, [glass, material(MAT_EMISSIVE, bump(0.5, 3.0, 540.0, 90.0))], mat_index=[0, 0, 0, 0, 1, 1]),
            (2.0, eye, (0, 0, 0)), 48, 32, spp, SLAB_DEPTH)


def prism_polygons(apex_deg, a=2.0, b=2.0, h=10.0):
    """a closed prism as five convex polygons wound outwards, float32 corners: the front face in z = 0 (normal +z) from the refracting
    edge x = -a to the base x = b, the back face falling from that edge at the apex angle, the base x = b, and the caps y = -+h"""
    zb = -(a + b) * np.tan(np.radians(apex_deg))
    e0, e1, f0, f1, k0, k1 = (-a, -h, 0), (-a, h, 0), (b, -h, 0), (b, h, 0), (b, -h, zb), (b, h, zb)
    polys = [[e0, f0, f1, e1], [e0, e1, k1, k0], [f0, k0, k1, f1], [e0, k0, f0], [e1, f1, k1]]
    return [f64(p) for p in polys]


def polygon_scene(polys, kinds, glass, emitter):
    """the triangles of planar polygons (a fan from the first corner), material 0 = glass, 1 = emitter; keeps the polygons for the truth"""
    V, idx = [], []
    for p, k in zip(polys, kinds):
        for j in range(1, len(p) - 1):
            V.append([p[0], p[j], p[j + 1]]); idx.append(int(k))
    sc = scene(V, [glass, emitter], mat_index=idx)
    sc["polys"], sc["kinds"] = polys, list(kinds)
    assert (f64(sc["V"]) == np.array(V)).all()            # the truth's corners are the float32 corners the renderer gets
    return sc


def wedge(apex_deg, emitter_polygon, camera, W, H, spp):
    """a closed BK7 prism (true Sellmeier C, spectrum 1), its front face normal to the view, and one emissive polygon beyond its back
    face, black background; the eye stands off the principal plane y = 0, so that every ray is skew"""
    glass = material(MAT_DIELECTRIC, np.ones(N_GRID, np.float32), B=BK7_B, C=BK7_C)
    polys = prism_polygons(apex_deg) + [f64(emitter_polygon)]
    return (polygon_scene(polys, [GLASS] * 5 + [EMITTER], glass, material(MAT_EMISSIVE, bump(0.5, 3.0, 540.0, 90.0))),
            camera, W, H, spp, WEDGE_DEPTH)


WEDGE_DEPTH = 8
STRIPE = [(6.66, -30, -20), (6.78, -30, -20), (6.78, 30, -20), (6.66, 30, -20)]        # 0.12 wide, 20 behind the front face
TIR_WALL = [(5, -50, -25), (60, -50, -25), (60, 50, -25), (5, 50, -25)]               # below the back face; the base's exits pass above it


def wedge_dispersion():
    """apex 30 degrees: the deviation runs from 19.03 (830 nm) to 20.23 degrees (360 nm), 0.44 wide on the stripe's plane: the stripe
    is a quarter of that, so every pixel column sees its own band of wavelengths"""
    return wedge(30.0, STRIPE, (0.25, (0, 0.4, 6), (-0.005, 0, 0)), 44, 10, 256)


def wedge_tir():
    """apex 41 degrees: BK7's critical angle is 40.58 (360 nm) to 41.47 degrees (830 nm), and the view sweeps the internal angle of
    incidence across that range: from black through red to white"""
    return wedge(41.0, TIR_WALL, (0.7875, (0, 0.4, 6), (-0.012, 0, 0)), 32, 14, 128)


FUZZ_ABSORBED, FUZZ_DIRECTED = 0.8, 0.3
FUZZ_DEPTH = 4       # at 2 a reflection INTO the floor would meet it again and end at the bounce limit, absorbed or not: the absorption would go untested


def fuzz_absorbed():
    """a fuzzed metal floor under the sky, seen at 11 degrees above grazing: 32 to 44 % of the reflections point into the floor"""
    return (scene(FLOOR, [material(MAT_METALLIC, ramp(0.9, 0.3), fuzz=FUZZ_ABSORBED)], mat_index=[0, 0], background=bump()),
            (12.0, (0, 1.2, 6), (0, 0, 0)), 48, 32, 64, FUZZ_DEPTH)


def fuzz_directed():
    """the mirror case with fuzz 0.3 and 256 samples: the light's mirror image is smeared over the floor"""
    sc, camera, W, H, _, _ = mirror()
    sc["mats"][0] = material(MAT_METALLIC, ramp(0.9, 0.3), fuzz=FUZZ_DIRECTED)
    return sc, camera, W, H, 256, FUZZ_DEPTH


LENS_NEAR = np.array([(-0.825, -0.45, 5.0), (0.375, -0.3375, 5.3), (-0.3, 0.45, 4.8)], np.float32)     # 3 in front of the lens: blurred
LENS_FOCUS = np.array([(1.7, -1.4, 0.0), (2.5, -1.2, 0.0), (2.0, -0.4, 0.0)], np.float32)             # in the focus plane: sharp


def lens():
    """two emissive triangles through a thin lens (defocus angle 4 degrees, focus distance 8: radius 0.28), black background"""
    mats = [material(MAT_EMISSIVE, bump(0.5, 4.0, 480.0, 50.0)), material(MAT_EMISSIVE, bump(0.5, 3.0, 600.0, 80.0))]
    return scene([LENS_NEAR, LENS_FOCUS], mats), (24.0, (0, 0, 8), (0, 0, 0), 4.0, 8.0), 64, 40, 64, 2


RADIOMETRY = {"sky_only": sky_only, "floor_under_sky": floor_under_sky, "emissive_wall": emissive_wall, "cosine_law": cosine_law,
              "mirror": mirror, "slab_0": lambda: slab(0.0, 64), "slab_55": lambda: slab(55.0, 1024),
              "wedge_dispersion": wedge_dispersion, "wedge_tir": wedge_tir, "fuzz_absorbed": fuzz_absorbed, "fuzz_directed": fuzz_directed,
              "lens": lens}
# the cases held per pixel as well (rms z, at least MIN_PIXELS pixels, dark pixels exactly 0), and their quadratures: the smallest
# for which halving any one resolution moves no held pixel's E by 0.1 of its standard error (test_quadratures_are_converged)
PER_PIXEL = ("wedge_dispersion", "wedge_tir", "fuzz_absorbed", "fuzz_directed", "lens")
# The film's wedges (film_expectation) have resolutions of their own (film_*: hero intervals per 5 nm cell, bisections that place a
# jump, sub-pixels across and down), held to the same rule for the film's entries (test_film_quadratures_are_converged); the film
# shares the other cases' resolutions with the XYZ sums.
QUADRATURE = {"wedge_dispersion": dict(nodes=128, refine=16, sub_x=8, sub_y=1, film_cell=1, film_bisect=8, film_sub_x=16, film_sub_y=1),
              "wedge_tir": dict(nodes=64, refine=32, sub_x=16, sub_y=1, film_cell=1, film_bisect=8, film_sub_x=8, film_sub_y=1),
              "fuzz_absorbed": dict(sub=2), "fuzz_directed": dict(na=64, sub=8), "lens": dict(sub=4)}
XYZ_ONLY, FILM_ONLY = ("nodes", "refine", "sub_x", "sub_y"), ("film_cell", "film_bisect", "film_sub_x", "film_sub_y")
Z_IMG_MAX = 5.0                      # statistical constants, not measurements
RMS_Z_RANGE = (0.8, 1.2)
MIN_EXPECTED = 10.0                  # per-pixel z only where spp P(contribute) >= 10
MIN_PIXELS = 300                     # of them: the rms of correct code then scatters by 1 / sqrt(2 x 300) = 0.04


def camera(srt, args, W, H):
    """the camera of a radiometry case: (vfov, eye, look-at) and, for a thin lens, (defocus_angle, focus_dist) after them"""
    vfov, eye, at = args[:3]
    lens_args = dict(zip(("defocus_angle", "focus_dist"), args[3:]))
    return srt.camera_init(W, H, vfov, eye, at, **lens_args)


def floor_points(eye, d):
    """where rays from eye meet the plane y = 0; every ray must run downwards onto FLOOR"""
    assert (d[:, 1] < 0).all()
    x = eye[None, :] - (eye[1] / d[:, 1])[:, None] * d
    assert (np.abs(x[:, 0]) < 50).all() and (x[:, 2] > -40).all() and (x[:, 2] < 60).all()
    return x


def bernoulli(E1, V1, P):
    """E, Var (3, m) of a path that contributes, with moments E1, V1 (3,), with probability P (m,) and adds 0 otherwise"""
    E = E1[:, None] * P[None, :]
    return E, (V1 + E1 ** 2)[:, None] * P[None, :] - E ** 2


def expectation(name, cmf, cam, sc, W, H, depth, res=None):
    """closed-form E and Var per path of every pixel ((3,) when all pixels are alike, else (3, H * W)), P = the probability that a path
    of the pixel contributes (None: 1), E_sum = the exact image total where it is known better than the sum of the per-pixel values.
    res: the resolutions of the case's quadrature (default QUADRATURE[name])"""
    spec = lambda k: f64(sc["mats"][k]["spectrum"])
    bg = f64(sc["background"])
    q = res or QUADRATURE.get(name)
    if name.startswith("wedge_"):
        # every contributing path has crossed the glass and carries the hero wavelength alone; P per pixel and hero wavelength by
        # enumeration, averaged over the pixel's footprint
        polys, kinds = sc["polys"], sc["kinds"]
        glass = [p for p, k in zip(polys, kinds) if k == GLASS]
        assert all(outside_convex(glass, p) for p, k in zip(polys, kinds) if k == EMITTER), "the emitter must lie wholly outside the glass"
        assert (spec(0) == 1).all() and not bg.any()
        B, C = f64(sc["mats"][0]["B"]), f64(sc["mats"][0]["C"])
        sub = [((a + 0.5) / q["sub_x"] - 0.5, (b + 0.5) / q["sub_y"] - 0.5) for a in range(q["sub_x"]) for b in range(q["sub_y"])]
        d = np.concatenate([unit(pixel_rays(cam, W, H, fx, fy)[1]) for fx, fy in sub])              # (sub-samples x pixels, 3)
        eye = camera_arrays(cam)[0]
        prob = lambda r, h: glass_paths(polys, kinds, np.broadcast_to(eye, (len(r), 3)), d[r], sellmeier_index(B, C, h), depth)
        E, M2, P = (m.reshape(m.shape[:-1] + (len(sub), W * H)).mean(-2)
                    for m in hero_moments(cmf, [spec(1)], prob, len(d), q["nodes"], q["refine"]))
        Var = M2 - E * E
        return dict(E=E, Var=Var, P=P, E_sum=None)
    if name == "fuzz_absorbed":
        assert sc["mats"][0]["fuzz"] == FUZZ_ABSORBED
        def share(eye, d):
            floor_points(eye, d)                                      # (asserts: every ray lands on the floor)
            return fuzz_share(-unit(d)[:, 1], FUZZ_ABSORBED)
        P = footprint_average(share, cam, W, H, q["sub"])
        E, Var = bernoulli(*path_moments(cmf, [spec(0), bg]), P)
        return dict(E=E, Var=Var, P=P, E_sum=None)
    if name == "fuzz_directed":
        assert sc["mats"][0]["fuzz"] == FUZZ_DIRECTED and not bg.any()
        P = footprint_average(lambda eye, d: fuzz_light_share(floor_points(eye, d), unit(d) * np.array([1.0, -1.0, 1.0]), FUZZ_DIRECTED,
                                                               f64(MIRROR_LIGHT), q["na"]), cam, W, H, q["sub"])
        E, Var = bernoulli(*path_moments(cmf, [spec(0), spec(1)]), P)
        return dict(E=E, Var=Var, P=P, E_sum=None)
    if name == "lens":
        assert not bg.any() and cam.defocus_angle > 0
        Pa = lens_coverage(cam, f64(LENS_NEAR), W, H, q["sub"])
        area_a = lens_coverage_sampled(cam, f64(LENS_NEAR), W, H, 2, 8, 1)[1]             # (exact: see there; also asserts "in view")
        Qb, depth_b = project_points(cam, f64(LENS_FOCUS))
        assert np.abs(depth_b - 1.0).max() < 1e-6, "lens: the second triangle must lie in the focus plane, which holds the pixel grid"
        Pb = coverage_exact(Qb, W, H)
        assert not ((Pa > 0) & (Pb > 0)).any(), "lens: the two images must not overlap (no ray can then meet both triangles)"
        (Ea, Va), (Eb, Vb) = bernoulli(*path_moments(cmf, [spec(0)]), Pa), bernoulli(*path_moments(cmf, [spec(1)]), Pb)
        E = Ea + Eb
        Var = (Va + Ea ** 2) + (Vb + Eb ** 2) - E ** 2
        return dict(E=E, Var=Var, P=Pa + Pb, E_sum=path_moments(cmf, [spec(0)])[0] * area_a + path_moments(cmf, [spec(1)])[0] * polygon_area(Qb),
                    near=Pa, focus=Pb)
    if name in ("sky_only", "sky_spikes"):
        E, V = path_moments(cmf, [bg])
        return dict(E=E, Var=V, P=None, E_sum=None)
    if name == "floor_under_sky":
        footprint_average(lambda eye, d: floor_points(eye, d)[:, 0], cam, W, H, 2)          # (asserts: every ray lands on the floor)
        E, V = path_moments(cmf, [spec(0), bg])
        return dict(E=E, Var=V, P=None, E_sum=None)
    if name == "emissive_wall":
        E, V = path_moments(cmf, [baked_emission(cmf[3], sc["mats"][0]["power"])])
        return dict(E=E, Var=V, P=None, E_sum=None)
    if name == "cosine_law":
        E1, V1 = path_moments(cmf, [spec(0), spec(1)])
        F = footprint_average(lambda eye, d: form_factor(floor_points(eye, d), (0.0, 1.0, 0.0), f64(LIGHT)), cam, W, H, 6)
        E = E1[:, None] * F[None, :]
        return dict(E=E, Var=(V1 + E1 ** 2)[:, None] * F[None, :] - E ** 2, P=F, E_sum=None)
    if name == "mirror":
        E1, V1 = path_moments(cmf, [spec(0), spec(1)])
        real, depth_real = project_points(cam, f64(MIRROR_LIGHT))
        Q, depth_q = project_points(cam, mirror_y(f64(MIRROR_LIGHT)))
        inside = lambda q: (q[:, 0] > -0.5) & (q[:, 0] < W - 0.5) & (q[:, 1] > -0.5) & (q[:, 1] < H - 0.5)
        assert (depth_q > 0).all() and inside(Q).all(), "mirror: the virtual triangle must lie wholly inside the view"
        assert (depth_real > 0).all() and ((real[:, 1] < -0.5).all() or (real[:, 1] > H - 0.5).all()), "mirror: the light itself must be out of view"
        cov = coverage_map(Q, W, H, 8)
        E = E1[:, None] * cov[None, :]
        return dict(E=E, Var=(V1 + E1 ** 2)[:, None] * cov[None, :] - E ** 2, P=cov, E_sum=E1 * polygon_area(Q), area=polygon_area(Q), cov=cov)
    assert name.startswith("slab_"), name
    # only transmitted paths contribute, and they carry the hero wavelength alone; the angle of incidence varies a little over the
    # 2 degree view: moments on 9 cosines spanning the view, interpolated to every pixel's centre ray
    eye, d = pixel_rays(cam, W, H)
    cos_px = np.abs(d[:, 2]) / np.linalg.norm(d, axis=1)
    eye, dc = pixel_rays(cam, W, H, 0.5, 0.5)
    corners = np.concatenate([np.abs(dc[:, 2]) / np.linalg.norm(dc, axis=1), cos_px])
    grid = np.linspace(min(corners.min(), cos_px.min()) - 1e-4, min(1.0, corners.max() + 1e-4), 9)
    em, glass = spec(1), sc["mats"][0]
    B, C = f64(glass["B"]), f64(glass["C"])
    mom = [path_moments(cmf, [em], hero_only=True, nodes=50000,
                        prob=lambda h, c=c: slab_transmission(sellmeier_index(B, C, h), c, depth)) for c in grid]
    E = np.stack([np.interp(cos_px, grid, [m[0][ch] for m in mom]) for ch in range(3)])
    Var = np.stack([np.interp(cos_px, grid, [m[1][ch] for m in mom]) for ch in range(3)])
    return dict(E=E, Var=Var, P=None, E_sum=None)


def assert_radiometry_holds(name, xyz_planes, W, H, spp, exp, what):
    """|z_img| <= 5 + the float32 summation allowance in all three channels, and for the cosine law 0.8 <= rms per-pixel z <= 1.2 over
    the pixels with spp P >= 10.  For every case of PER_PIXEL -- the cases about WHERE the light goes, to which z_img is blind -- the same
    range holds in all three channels over the pixels with spp P >= 10, of which there must be at least MIN_PIXELS, and a pixel whose P
    is 0, like that of its eight neighbours, has all three XYZ sums exactly 0.  Returns the z values for the test's printed line."""
    z_img, allowance, z_px = z_scores(xyz_planes, W, H, spp, exp["E"], exp["Var"], MIN_EXPECTED if exp["P"] is not None else None,
                                      exp["P"], exp["E_sum"])
    held = ~np.isnan(z_px)               # 0 / 0: a channel the truth gives this pixel nothing in, and that got nothing, has no z (x / 0 has)
    out = dict(z_img=[round(float(z), 2) for z in z_img], max_z_px=round(float(np.abs(z_px[held]).max()), 2), pixels=int(z_px.shape[1]),
               rms_z=[round(float(np.sqrt((z_px[c][held[c]] ** 2).mean())), 3) for c in range(3)])
    assert (np.abs(z_img) <= Z_IMG_MAX + allowance).all(), "%s %s: z_img %s" % (what, name, out)
    if name == "cosine_law":
        assert z_px.shape[1] >= 100, (what, name, z_px.shape)
        assert all(RMS_Z_RANGE[0] <= r <= RMS_Z_RANGE[1] for r in out["rms_z"]), "%s %s: rms z %s" % (what, name, out)
    if name in PER_PIXEL:
        assert held.sum(1).min() >= MIN_PIXELS, (what, name, held.sum(1))
        assert all(RMS_Z_RANGE[0] <= r <= RMS_Z_RANGE[1] for r in out["rms_z"]), "%s %s: rms z %s" % (what, name, out)
        lit = np.pad(np.asarray(exp["P"]).reshape(H, W) > 0, 1)
        dark = ~np.any([lit[a:a + H, b:b + W] for a in range(3) for b in range(3)], axis=0)
        out["dark"] = int(dark.sum())
        sums = np.stack([np.asarray(xyz_planes[c])[lane_index(W, H)] for c in range(3)])
        assert not sums[:, dark].any(), "%s %s: %d dark pixels are lit" % (what, name, (sums[:, dark] != 0).any(0).sum())
    return out


# ---- the spectral film ------------------------------------------------------------------------------------------------------------
GRID = LAMBDA_MIN + 5.0 * np.arange(N_GRID)          # lambda_j = 360 + 5 j: the tent of film bin j peaks there
FILM_GL = 4                   # Gauss-Legendre nodes per 5 nm cell: exact to degree 7 (hat^2 p^2 with two linear factors has degree 6)
FILM_JUMP = 0.005             # hero_film_moments' JUMP: a film entry sees 10 nm of the hero, so smaller steps of P must be placed too
FILM_MIN_ENTRIES = 3000      # entries (pixel, bin) with spp Pdep >= MIN_EXPECTED a per-entry hold needs, in at least MIN_PIXELS pixels
PER_BIN_ONLY = ("mirror",)    # 33 lit pixels: held per bin over the image alone
FILM_CASES = dict(RADIOMETRY, sky_spikes=sky_spikes)


def hat(j, lam):
    """the tent of film bin j: 1 at lambda_j, 0 from 5 nm away; the grid's ends cut the tents of bins 0 and 94 in half"""
    lam = np.asarray(lam, np.float64)
    inside = (lam >= LAMBDA_MIN) & (lam <= LAMBDA_MAX)
    return np.where(inside, np.maximum(0.0, 1.0 - np.abs(lam - GRID[j]) / 5.0), 0.0)


def film_integrals(factors, prob=None):
    """per bin j (3, 95): the integrals over lambda of hat_j P p, of hat_j^2 P p^2 and of P over the part of hat_j's support where p > 0,
    p the product of the linear interpolants of `factors` (non-negative 95-sample tables) and P = prob(lambda) (default 1).  In a 5 nm
    cell the two tents that meet there and every factor are linear: FILM_GL-point Gauss-Legendre per cell is exact for P = 1.  A linear
    factor is > 0 on a whole open cell unless both its ends are 0, so the length where p > 0 is exact as well."""
    x, wq = np.polynomial.legendre.leggauss(FILM_GL)
    s, wq = 0.5 * (x + 1.0), 2.5 * wq                                        # nodes in [0, 1] across a cell, weights in nm
    p, pos = np.ones((FILM_GL, N_GRID - 1)), np.ones(N_GRID - 1, bool)
    for tab in factors:
        tab = np.asarray(tab, np.float64)
        assert (tab >= 0).all()
        p = p * ((1.0 - s)[:, None] * tab[None, :-1] + s[:, None] * tab[None, 1:])
        pos &= np.maximum(tab[:-1], tab[1:]) > 0
    P = np.ones_like(p) if prob is None else prob(GRID[None, :-1] + 5.0 * s[:, None])
    out = np.zeros((3, N_GRID))
    for k, tent in ((0, 1.0 - s), (1, s)):                                  # the cell's left bin (k = 0) and right bin (k = 1)
        w = (wq * tent)[:, None] * P
        out[0, k:N_GRID - 1 + k] += (w * p).sum(0)
        out[1, k:N_GRID - 1 + k] += (w * tent[:, None] * p * p).sum(0)
        out[2, k:N_GRID - 1 + k] += (wq[:, None] * P).sum(0) * pos
    return out


def hero_film_moments(factors, prob, rays, cell, bisect):
    """E, M2 and Pdep (rays, 95) of one hero-only path's deposit into every bin when it contributes with probability prob(ray numbers,
    hero wavelengths) (hero_moments' setting): (1 / 470) times the integrals of film_integrals.  The hero's range is cut into `cell`
    equal intervals per 5 nm cell, so that each lies inside one cell and meets the two tents of that cell; prob is taken at an
    interval's midpoint and held there, while the tents and the spectrum are integrated over it exactly (film_integrals' Gauss-Legendre
    rule).  Where prob changes by more than FILM_JUMP between neighbouring midpoints (or between an end of the range and its
    midpoint), the jump is placed by `bisect` bisections, and the interval that holds it is split there into two, each with prob at its
    own midpoint.  ASSERTED: no interval holds two jumps."""
    N = (N_GRID - 1) * cell
    x, wq = np.polynomial.legendre.leggauss(FILM_GL)

    def weights(lo, width):
        """per interval [lo, lo + width] inside one cell: the cell and the integrals of tent x p, (tent x p)^2 and [p > 0] for the
        cell's left and right bin, (2, 3, m)"""
        off = np.minimum(np.floor((lo - LAMBDA_MIN) / 5.0 + 1e-9).astype(np.int64), N_GRID - 2)
        out = np.zeros((2, 3, len(lo)))
        for xq, wt in zip(0.5 * (x + 1.0), 0.5 * wq):
            lam = lo + xq * width
            s = (lam - GRID[off]) / 5.0
            p = np.ones_like(lam)
            for tab in factors:
                p = p * interp(np.asarray(tab, np.float64), lam)
            for side, tent in ((0, 1.0 - s), (1, s)):
                out[side] += wt * width * np.stack([tent * p, (tent * p) ** 2, (tent > 0) * (p > 0)])
        return off, out

    width = (LAMBDA_MAX - LAMBDA_MIN) / N
    h0 = hero_nodes(N)
    P0 = prob(np.repeat(np.arange(rays), N), np.tile(h0, rays)).reshape(rays, N)
    ends = prob(np.repeat(np.arange(rays), 2), np.tile([LAMBDA_MIN, LAMBDA_MAX], rays)).reshape(rays, 2)
    Pe, he = np.concatenate([ends[:, :1], P0, ends[:, 1:]], 1), np.concatenate([[LAMBDA_MIN], h0, [LAMBDA_MAX]])
    r, i = np.nonzero(np.abs(np.diff(Pe, axis=1)) > FILM_JUMP)
    lo, hi, plo, phi = he[i], he[i + 1], Pe[r, i], Pe[r, i + 1]
    for _ in range(bisect):
        mid = 0.5 * (lo + hi)
        pm = prob(r, mid)
        left = np.abs(pm - plo) > np.abs(pm - phi)               # the jump lies below mid
        lo, hi = np.where(left, lo, mid), np.where(left, mid, hi)
    at = 0.5 * (lo + hi)
    k = np.clip(np.floor((at - LAMBDA_MIN) / width).astype(np.int64), 0, N - 1)
    assert len(set(zip(r.tolist(), k.tolist()))) == len(r), "hero_film_moments: two jumps in one interval (raise the cells' nodes)"
    split = np.zeros((rays, N), bool)
    split[r, k] = True
    coarse = np.where(split, 0.0, P0) / (LAMBDA_MAX - LAMBDA_MIN)
    off, w = weights(h0 - 0.5 * width, np.full(N, width))
    A = np.zeros((3, N, N_GRID))
    for side in (0, 1):
        A[:, np.arange(N), off + side] = w[side]
    E, M2, D = (coarse @ A[q] for q in range(3))
    a = LAMBDA_MIN + k * width
    for start, part in ((a, at - a), (at, a + width - at)):
        Pp = prob(r, start + 0.5 * part) / (LAMBDA_MAX - LAMBDA_MIN)
        off, w = weights(start, part)
        for q, out in enumerate((E, M2, D)):
            for side in (0, 1):
                np.add.at(out, (r, off + side), Pp * w[side, q])
    return E, M2, D


def _share(name, cam, sc, W, H, q):
    """(H * W,) the probability that a path of each pixel contributes, for the cases whose paths keep all seven wavelengths and whose
    P does not depend on the wavelength: the quantities expectation() computes, with exact coverages for the two projected triangles"""
    bg = f64(sc["background"])
    if name in ("sky_only", "sky_spikes", "emissive_wall"):
        return np.ones(W * H)
    if name == "floor_under_sky":
        footprint_average(lambda eye, d: floor_points(eye, d)[:, 0], cam, W, H, 2)          # (asserts: every ray lands on the floor)
        return np.ones(W * H)
    if name == "cosine_law":
        return footprint_average(lambda eye, d: form_factor(floor_points(eye, d), (0.0, 1.0, 0.0), f64(LIGHT)), cam, W, H, 6)
    if name == "mirror":
        return coverage_exact(project_points(cam, mirror_y(f64(MIRROR_LIGHT)))[0], W, H)
    if name == "fuzz_absorbed":
        def share(eye, d):
            floor_points(eye, d)                                      # (asserts: every ray lands on the floor)
            return fuzz_share(-unit(d)[:, 1], FUZZ_ABSORBED)
        return footprint_average(share, cam, W, H, q["sub"])
    assert name == "fuzz_directed" and not bg.any(), name
    return footprint_average(lambda eye, d: fuzz_light_share(floor_points(eye, d), unit(d) * np.array([1.0, -1.0, 1.0]), FUZZ_DIRECTED,
                                                              f64(MIRROR_LIGHT), q["na"]), cam, W, H, q["sub"])


def film_expectation(name, cam, sc, W, H, depth, res=None, d65n=None):
    """E, Var and Pdep (H * W, 95) of ONE path's deposit into every film bin of every pixel of a case of FILM_CASES (Pdep: the
    probability that the deposit is non-zero), and all_seven (the paths keep their seven wavelengths; P does not depend on them).
    A path deposits hat_j(l) p(l) at each of its m valid wavelengths l, each marginally uniform on [360, 830], at most one of them in a
    tent's support (they lie 470/7 apart): E_j = (m / 470) int hat_j P p, M2_j = (m / 470) int hat_j^2 P p^2, Pdep_j = (m / 470)
    int over supp hat_j of P [p > 0]; m = 7, or 1 for a path that refracted (slab_*, wedge_*: the hero alone).  res: the resolutions
    of the case's quadrature (default QUADRATURE[name]); d65n: the normalised D65 row of the colour tables (emissive_wall's bake)."""
    spec = lambda k: f64(sc["mats"][k]["spectrum"])
    bg = f64(sc["background"])
    q = res or QUADRATURE.get(name)
    if name.startswith("wedge_"):
        polys, kinds = sc["polys"], sc["kinds"]
        glass = [p for p, k in zip(polys, kinds) if k == GLASS]
        assert all(outside_convex(glass, p) for p, k in zip(polys, kinds) if k == EMITTER), "the emitter must lie wholly outside the glass"
        assert (spec(0) == 1).all() and not bg.any()
        B, C = f64(sc["mats"][0]["B"]), f64(sc["mats"][0]["C"])
        nx, ny = q["film_sub_x"], q["film_sub_y"]
        sub = [((a + 0.5) / nx - 0.5, (b + 0.5) / ny - 0.5) for a in range(nx) for b in range(ny)]
        d = np.concatenate([unit(pixel_rays(cam, W, H, fx, fy)[1]) for fx, fy in sub])
        eye = camera_arrays(cam)[0]
        prob = lambda r, h: glass_paths(polys, kinds, np.broadcast_to(eye, (len(r), 3)), d[r], sellmeier_index(B, C, h), depth)
        E, M2, D = (m.reshape(len(sub), W * H, N_GRID).mean(0)
                    for m in hero_film_moments([spec(1)], prob, len(d), q["film_cell"], q["film_bisect"]))
        return dict(E=E, Var=M2 - E * E, Pdep=D, all_seven=False)
    if name.startswith("slab_"):
        # the slab_ case of expectation(): moments on 9 cosines spanning the view, interpolated to every pixel's centre ray
        eye, d = pixel_rays(cam, W, H)
        cos_px = np.abs(d[:, 2]) / np.linalg.norm(d, axis=1)
        eye, dc = pixel_rays(cam, W, H, 0.5, 0.5)
        corners = np.concatenate([np.abs(dc[:, 2]) / np.linalg.norm(dc, axis=1), cos_px])
        grid = np.linspace(min(corners.min(), cos_px.min()) - 1e-4, min(1.0, corners.max() + 1e-4), 9)
        B, C = f64(sc["mats"][0]["B"]), f64(sc["mats"][0]["C"])
        mom = np.stack([film_integrals([spec(1)], lambda l, c=c: slab_transmission(sellmeier_index(B, C, l), c, depth)) for c in grid])
        E, M2, D = (np.stack([np.interp(cos_px, grid, mom[:, i, j]) for j in range(N_GRID)], 1) / (LAMBDA_MAX - LAMBDA_MIN) for i in range(3))
        return dict(E=E, Var=M2 - E * E, Pdep=D, all_seven=False)
    scale = N_WAVELENGTHS / (LAMBDA_MAX - LAMBDA_MIN)
    if name == "lens":
        assert not bg.any() and cam.defocus_angle > 0
        Qb, depth_b = project_points(cam, f64(LENS_FOCUS))
        assert np.abs(depth_b - 1.0).max() < 1e-6
        terms = [(lens_coverage(cam, f64(LENS_NEAR), W, H, q["sub"]), [spec(0)]), (coverage_exact(Qb, W, H), [spec(1)])]
        assert not ((terms[0][0] > 0) & (terms[1][0] > 0)).any(), "lens: the two images must not overlap"
    elif name == "emissive_wall":
        assert d65n is not None, "emissive_wall: the bake needs the D65 row"
        terms = [(_share(name, cam, sc, W, H, q), [baked_emission(d65n, sc["mats"][0]["power"])])]
    else:
        ends = {"sky_only": ("bg",), "sky_spikes": ("bg",), "floor_under_sky": (0, "bg"), "cosine_law": (0, 1), "mirror": (0, 1),
                "fuzz_absorbed": (0, "bg"), "fuzz_directed": (0, 1)}[name]              # the tables a contributing path's power multiplies
        terms = [(_share(name, cam, sc, W, H, q), [bg if k == "bg" else spec(k) for k in ends])]
    E, M2, D = (np.zeros((W * H, N_GRID)) for _ in range(3))
    for P, factors in terms:                     # the terms are exclusive: a path ends on one of the triangles, or on none
        I = film_integrals(factors) * scale
        E += P[:, None] * I[0]; M2 += P[:, None] * I[1]; D += P[:, None] * I[2]
    return dict(E=E, Var=M2 - E * E, Pdep=D, all_seven=True)


def film_spp(name, spp, fexp):
    """the film run's samples per pixel: the case's spp, raised to the smallest power of two at which the entries with spp Pdep >=
    MIN_EXPECTED number at least FILM_MIN_ENTRIES in at least MIN_PIXELS pixels (the case's own for PER_BIN_ONLY)"""
    if name in PER_BIN_ONLY:
        return spp
    for k in range(6):
        held = spp * 2 ** k * fexp["Pdep"] >= MIN_EXPECTED
        if held.sum() >= FILM_MIN_ENTRIES and held.any(1).sum() >= MIN_PIXELS:
            return spp * 2 ** k
    raise AssertionError("%s: no spp up to %d meets the per-entry counts" % (name, spp * 32))


def film_case(srt, name, res=None):
    """scene, camera, frame, the film run's spp, depth and film_expectation (with its CPU time in `seconds`) of a case of FILM_CASES,
    computed once per session and shared by both builders (res: other resolutions of the quadrature)"""
    import time
    sc, args, W, H, spp, depth = FILM_CASES[name]()
    cam = camera(srt, args, W, H)

    def make():
        t = time.process_time()
        exp = film_expectation(name, cam, sc, W, H, depth, res, color_tables(srt)[3])
        exp["seconds"] = round(time.process_time() - t, 2)
        return exp
    exp = cached(("film", name) if res is None else ("film", name, tuple(sorted(res.items()))), make)
    return sc, cam, W, H, film_spp(name, spp, exp), depth, exp


def neighbourhood_lit(lit):
    """lit (a, b, c) -> whether any of the 3 x 3 x 3 entries around each is lit"""
    a, b, c = lit.shape
    pad = np.pad(lit, 1)
    return np.any([pad[i:i + a, j:j + b, k:k + c] for i in range(3) for j in range(3) for k in range(3)], axis=0)


def assert_film_holds(name, film, W, H, spp, exp, what, radiance=None):
    """The conditions on a film (H, W, 95) of raw sums after spp samples of every pixel, against film_expectation `exp`:
      per bin over the image   |z_bin| <= Z_IMG_MAX + the float32 summation allowance (spp 2^-24 of the expected total) for every bin
                               with Var > 0, z_bin = (sum F_j - spp sum E_j) / sqrt(spp sum Var_j);
      per entry (pixel, bin)   RMS_Z_RANGE holds the rms z over the entries with spp Pdep >= MIN_EXPECTED, of which there are at least
                               FILM_MIN_ENTRIES in at least MIN_PIXELS pixels (not for PER_BIN_ONLY);
      dark entries             a sum is exactly 0 where E is 0 at the entry and at its 26 neighbours (3 x 3 pixels x bin -+ 1); where
                               P does not depend on the wavelength, every bin whose E is 0 in every pixel holds 0 everywhere;
      estimator                radiance (srt.spectral_radiance, for sky_only and sky_spikes): the image mean at bin j is the hat average
                               of the background, int hat_j b / int hat_j (5 nm, 2.5 at the ends), within the same bound.
    Returns the figures for the test's printed line."""
    F = np.asarray(film, np.float64).reshape(H * W, N_GRID)
    E, Var, Pdep = exp["E"], exp["Var"], exp["Pdep"]
    sE, sV = E.sum(0), Var.sum(0)
    bins = sV > 0
    sd = np.sqrt(spp * sV[bins])
    z_bin = (F.sum(0)[bins] - spp * sE[bins]) / sd
    allowance = spp * U * spp * sE[bins] / sd
    out = dict(spp=spp, max_z_bin=round(float(np.abs(z_bin).max()), 2), rms_z_bin=round(float(np.sqrt((z_bin ** 2).mean())), 3))
    assert (np.abs(z_bin) <= Z_IMG_MAX + allowance).all(), "%s %s: z_bin %s at bin %d" % (what, name, out, np.nonzero(bins)[0][np.abs(z_bin).argmax()])
    if name not in PER_BIN_ONLY:
        held = spp * Pdep >= MIN_EXPECTED
        z = (F[held] - spp * E[held]) / np.sqrt(spp * Var[held])
        out.update(entries=int(held.sum()), pixels=int(held.any(1).sum()), rms_z=round(float(np.sqrt((z ** 2).mean())), 3),
                   max_z=round(float(np.abs(z).max()), 2))
        assert held.sum() >= FILM_MIN_ENTRIES and held.any(1).sum() >= MIN_PIXELS, (what, name, out)
        assert RMS_Z_RANGE[0] <= out["rms_z"] <= RMS_Z_RANGE[1], "%s %s: rms z %s" % (what, name, out)
    dark = ~neighbourhood_lit((E > 0).reshape(H, W, N_GRID)).reshape(H * W, N_GRID)
    out["dark"] = int(dark.sum())
    assert not F[dark].any(), "%s %s: %d dark entries are non-zero" % (what, name, (F[dark] != 0).sum())
    if exp["all_seven"]:
        unlit = ~(E > 0).any(0)
        out["unlit_bins"] = int(unlit.sum())
        assert not F[:, unlit].any(), "%s %s: unlit bins %s hold deposits" % (what, name, np.nonzero(unlit & (F != 0).any(0))[0])
    if radiance is not None:
        assert name in ("sky_only", "sky_spikes")
        width = np.where((np.arange(N_GRID) == 0) | (np.arange(N_GRID) == N_GRID - 1), 2.5, 5.0)
        want = film_integrals([f64(FILM_CASES[name]()[0]["background"])])[0] / width
        scale = (LAMBDA_MAX - LAMBDA_MIN) / 35.0 * 5.0 / width / (W * H * spp)      # image mean of the estimator per raw sum
        got = np.asarray(radiance(film, spp), np.float64).reshape(H * W, N_GRID).mean(0)
        z_est = (got[bins] - want[bins]) / (scale[bins] * sd)
        out["max_z_estimator"] = round(float(np.abs(z_est).max()), 2)
        assert (np.abs(z_est) <= Z_IMG_MAX + allowance).all(), "%s %s: estimator z %s at bin %d" % (what, name, out, np.nonzero(bins)[0][np.abs(z_est).argmax()])
        assert not got[~bins].any(), (what, name, "estimator non-zero in an unlit bin")
    return out


# ---- first-hit features ------------------------------------------------------------------------------------------------------------
PLATE_IMAGES = np.array([[(2.0, 2.0), (29.0, 3.0), (6.0, 17.0)], [(34.0, 2.0), (61.0, 5.0), (50.0, 18.0)],        # pixel coordinates
                         [(3.0, 21.0), (28.0, 23.0), (14.0, 37.0)], [(36.0, 22.0), (61.0, 21.0), (45.0, 37.0)]])
PLATE_PLANES = [((0.0, 0.0, 0.0), (0.3, 0.2, 1.0)), ((0.0, 0.0, -1.5), (-0.4, 0.1, 1.0)),                             # point, normal
                ((0.0, 0.0, 1.0), (0.2, -0.5, 1.0)), ((0.0, 0.0, -3.0), (0.1, 0.35, 1.0))]
PLATE_COLS = [(0.5, 0.25, 0.75), (0.125, 0.625, 0.375), (0.875, 0.0625, 0.5625), (0.3125, 0.9375, 0.1875)]     # dyadic: n col is exact
PLATE_CAMERA = (30.0, (0.0, 0.0, 10.0), (0.0, 0.0, 0.0))
FEATURE_SUB = 16              # k x k sub-samples of the distance truth (test_feature_distance_is_converged)
MIN_EDGE_PIXELS = 100         # pixels with n P >= MIN_EXPECTED and n (1 - P) >= MIN_EXPECTED that hold the binomial rms
NORMAL_TOL = 1.15e-6            # twice the largest |normal sum / hits - unit normal| the oracle's prediction shows (tests/test_ground_truth_reference.py)


def plates(srt):
    """four triangles seen by a pinhole camera under a bumped sky, 64 x 40 pixels x 64 samples: each the camera's central projection of
    the pixel triangle PLATE_IMAGES[k] onto a tilted plane PLATE_PLANES[k] at its own depth, so that the images are known and pairwise
    disjoint; the last is wound away from the camera.  Materials Lambertian, metallic, dielectric, emissive, their col distinct dyadic
    fractions.  Needs the package's camera (srt) to place the corners."""
    W, H = 64, 40
    cam = camera(srt, PLATE_CAMERA, W, H)
    eye, p00, du, dv = camera_arrays(cam)
    V = []
    for img, (pt, nrm) in zip(PLATE_IMAGES, PLATE_PLANES):
        pt, nrm = np.array(pt), np.array(nrm)
        d = p00[None, :] + img[:, :1] * du[None, :] + img[:, 1:] * dv[None, :] - eye[None, :]
        V.append(eye[None, :] + (((pt - eye) @ nrm) / (d @ nrm))[:, None] * d)
    V = np.array([v[::-1] for v in V[:3]] + V[3:])                 # (the image's y runs down: the corners as listed are wound away)
    toward = (np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]) * (eye[None, :] - V[:, 0])).sum(1) > 0
    assert toward.tolist() == [True, True, True, False], toward
    mats = [material(MAT_LAMBERTIAN, ramp(), col=PLATE_COLS[0]), material(MAT_METALLIC, ramp(0.9, 0.3), col=PLATE_COLS[1]),
            material(MAT_DIELECTRIC, np.ones(N_GRID, np.float32), col=PLATE_COLS[2]),
            material(MAT_EMISSIVE, bump(0.5, 3.0, 540.0, 90.0), col=PLATE_COLS[3])]
    return scene(V, mats, background=bump()), PLATE_CAMERA, W, H, 64, 4


def feature_expectation(name, cam, sc, W, H, sub=FEATURE_SUB, lens_sub=None):
    """per triangle k: P (K, H * W) that a camera ray of the pixel meets it first, the unit normal turned towards the camera (K, 3) and
    the material's col as float32 (K, 3); for the pinhole case (plates) also the footprint mean and variance of |hit - eye| over
    sub x sub sub-samples (dist, dist_var: (H * W,), NaN where a sub-sample misses), with the hits from closest_hit"""
    Vd = f64(sc["V"])
    _, nu = normals(Vd)
    eye = camera_arrays(cam)[0]
    toward = np.sign(((eye[None, :] - Vd[:, 0]) * nu).sum(1))
    # a thin lens moves the origin by its radius at most: every lens point must lie on the same side of every plane
    radius = np.linalg.norm(np.array(cam.defocus_disk_u[:], np.float64)) if cam.defocus_angle > 0 else 0.0
    assert (np.abs(((eye[None, :] - Vd[:, 0]) * nu).sum(1)) > radius).all()
    col = np.array([sc["mats"][m]["col"] for m in sc["mat_index"]], np.float32)
    out = dict(normal=nu * toward[:, None], col=col, facing=toward)
    if name == "lens":
        out["P"] = np.stack([lens_coverage(cam, Vd[0], W, H, lens_sub or QUADRATURE["lens"]["sub"]),
                             coverage_exact(project_points(cam, Vd[1])[0], W, H)])
        return out
    assert name == "plates" and cam.defocus_angle == 0
    out["P"] = np.stack([coverage_exact(project_points(cam, v)[0], W, H) for v in Vd])
    m1, m2 = np.zeros(W * H), np.zeros(W * H)
    for a in range(sub):
        for b in range(sub):
            e, d = pixel_rays(cam, W, H, (a + 0.5) / sub - 0.5, (b + 0.5) / sub - 0.5)
            t, tri, _, _ = closest_hit(Vd, np.broadcast_to(e, d.shape), d)
            r = np.where(tri >= 0, t * np.linalg.norm(d, axis=1), np.nan)
            m1 += r; m2 += r * r
    m1, m2 = m1 / sub ** 2, m2 / sub ** 2
    out["dist"], out["dist_var"] = m1, m2 - m1 * m1
    return out


FEATURE_CASES = ("plates", "lens")


def feature_case(srt, name, sub=FEATURE_SUB):
    """scene, camera, frame, samples, depth and feature_expectation of plates or lens, computed once per session"""
    sc, args, W, H, n, depth = plates(srt) if name == "plates" else lens()
    cam = camera(srt, args, W, H)
    return sc, cam, W, H, n, depth, cached(("features", name, sub), lambda: feature_expectation(name, cam, sc, W, H, sub))


def assert_features_hold(rows, n, exp, what):
    """The conditions on feature rows (H, W, 8) of raw sums after n samples of every pixel, against feature_expectation `exp`:
      hits     |z_img| <= Z_IMG_MAX against the sum of P; the rms of the binomial z in RMS_Z_RANGE over the pixels with n P >= 10 and
               n (1 - P) >= 10, of which there are at least MIN_EDGE_PIXELS; hits == n where P == 1; all eight sums exactly 0 where P
               is 0 at the pixel and its eight neighbours;
      normal   normal sum / hits within NORMAL_TOL of the unit normal turned towards the camera, at every pixel that sees one triangle;
      albedo   albedo sum == hits col exactly at those pixels;
      distance (when exp holds one) at every pixel wholly inside one triangle, of which there are at least MIN_PIXELS, the rms of
               (distance sum / n - mean) / sqrt(variance / n) in RMS_Z_RANGE.
    Returns the figures for the test's printed line."""
    Hh, Ww = rows.shape[:2]
    R = np.asarray(rows, np.float64).reshape(-1, 8)
    hits, Pk = R[:, 7], exp["P"]
    P = Pk.sum(0)
    assert P.max() <= 1.0 + 1e-9
    z_img = (hits.sum() - n * P.sum()) / np.sqrt(n * (P * (1 - P)).sum())
    edge = (n * P >= MIN_EXPECTED) & (n * (1 - P) >= MIN_EXPECTED)
    z = (hits[edge] - n * P[edge]) / np.sqrt(n * P[edge] * (1 - P[edge]))
    full = P >= 1.0 - 1e-12
    lit = np.pad((P > 0).reshape(Hh, Ww), 1)
    dark = ~np.any([lit[a:a + Hh, b:b + Ww] for a in range(3) for b in range(3)], axis=0).ravel()
    out = dict(z_img=round(float(z_img), 2), edge_pixels=int(edge.sum()), rms_z_hits=round(float(np.sqrt((z ** 2).mean())), 3),
               full=int(full.sum()), dark=int(dark.sum()))
    assert abs(z_img) <= Z_IMG_MAX, "%s: hits z_img %s" % (what, out)
    assert edge.sum() >= MIN_EDGE_PIXELS and RMS_Z_RANGE[0] <= out["rms_z_hits"] <= RMS_Z_RANGE[1], "%s: hits %s" % (what, out)
    assert (hits[full] == n).all(), "%s: %d full pixels missed" % (what, (hits[full] != n).sum())
    assert not R[dark].any(), "%s: %d dark pixels hold sums" % (what, R[dark].any(1).sum())
    one = ((Pk > 0).sum(0) == 1) & (hits > 0)
    k = Pk.argmax(0)[one]
    dev = np.abs(R[one, 0:3] / hits[one, None] - exp["normal"][k]).max()
    out.update(one_triangle=int(one.sum()), normal_dev=float("%.3g" % dev))
    assert dev <= NORMAL_TOL, "%s: normal off by %.3g" % (what, dev)
    albedo = R[one, 3:6] != hits[one, None] * exp["col"][k].astype(np.float64)
    assert not albedo.any(), "%s: %d albedo sums differ from hits x col" % (what, albedo.any(1).sum())
    if "dist" in exp:
        inside = (Pk >= 1.0 - 1e-12).any(0)
        zd = (R[inside, 6] / n - exp["dist"][inside]) / np.sqrt(exp["dist_var"][inside] / n)
        out.update(inside=int(inside.sum()), rms_z_distance=round(float(np.sqrt((zd ** 2).mean())), 3))
        assert inside.sum() >= MIN_PIXELS and RMS_Z_RANGE[0] <= out["rms_z_distance"] <= RMS_Z_RANGE[1], "%s: distance %s" % (what, out)
    return out
