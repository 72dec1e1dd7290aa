"""The truth scenes of the direct-light pass and what they are held to, shared by the CPU suite (restatement under the float64 queries) and
the GPU suite (the device's output, no restatement in between).

  floor_under_sky   ground_truth's floor under its sky: SKY gives every floor pixel T_sky exactly (every sky ray leaves).
  cosine_law        ground_truth's floor + LIGHT: LIGHTS gives T_light F, F = Lambert's form factor of the light averaged over the pixel.
  split_light       cosine_law with its light cut into two triangles of unequal area (0.3 : 0.7) and opposite winding: the same expectation,
                    a pick that must be divided out, and one light facing the floor with either face.
  sky_blocker       cosine_law with the light's triangle made Lambertian under a grey sky: SKY gives T_sky (1 - F(blocker)).
  occluded_light    the floor, a light above it (OCC_LIGHT) and a convex Lambertian quad between them: LIGHTS gives T_light (F(light) - F(light n shadow)),
                    the shadow being the blocker projected from the floor point onto the light's plane, clipped convex against convex.
  many_lights       the floor under 37 disjoint triangles of one emissive material in LIGHT's plane, mixed windings, areas over seven decades,
                    eight of them too small for one of the 2^24 draws (pinned at width 1): LIGHTS gives T_light sum_l F_l.  The pick among an
                    odd number of lights, the largest-remainder thresholds and the weight area / p_l.  DRAW_S names two samples of one pixel
                    whose draw lands on a pinned light's single value and on a wide light's first value (find_draw).
  two_emitters      a floor of two materials (its diagonal crosses the view) under a red and a blue emitter, the red one -- the material
                    with the higher index -- first in scene order, so that slot order is not material order: LIGHTS gives, on floor
                    triangle f, sum_e T_light[mat(f), e] F_e.  The [material][slot] layout of t_light and the slot read from the light record.
  emitters_in_view  two_emitters under a grey sky seen from below: EMITTED gives T_emit[material] on each emitter and T_bg on the sky,
                    exactly (S equal terms).  Held where the whole footprint shows one of the three (view_classes).
  floor_under_sky_lens, cosine_law_lens
                    the two scenes through a thin lens (LENS) focused in front of the floor: every lens ray still meets the floor, so SKY
                    gives T_sky exactly, and LIGHTS gives T_light F averaged over footprint and lens (lens_share, a quadrature taken at
                    two resolutions).  The lens branch of the camera rows; assert_lens_rows_hold holds the rows themselves to geometry.
Pixels are held where every sub-sample of the footprint (K x K midpoints) has the floor as its first hit in the float64 truth, from every
point of a coarse grid on the lens where there is one.

Statistics (ground_truth's constants, not measurements): the per-pixel variance of the mean comes from m2, v = (m2 - S mean^2) / (S - 1) / S;
z = (mean - E) / sqrt(v) over the held pixels with v > 0, of which there must be MIN_PIXELS; rms z within RMS_Z_RANGE, and for the image
|sum mean - sum E| <= Z_IMG_MAX sqrt(sum v) + sum E S 2^-24 (the float32 summation of S terms)."""
import numpy as np

import direct_light_reference as R
import ground_truth as G

K = 4                      # footprint sub-samples per axis
BLOCKER = np.array([(-1.2, 0.8, -0.6), (1.6, 0.8, -0.8), (1.8, 0.8, 1.6), (-1.0, 0.8, 1.8)], np.float32)
OCC_LIGHT = np.array([(-1.0, 3.0, -0.5), (1.5, 3.2, 0.0), (0.0, 2.9, 1.5)], np.float32)      # high above the blocker: every floor point sees the blocker below the light's plane
GREY_SKY = np.full(G.N_GRID, 0.75, np.float32)
EMITTER = lambda: G.material(G.MAT_EMISSIVE, G.bump(0.5, 6.0, 600.0, 80.0))
CAMERA = (25.0, (0, 1.5, 6), (0, 0, 1.5))
LENS = (2.0, 3.0)           # defocus angle in degrees and focus distance: a disk of radius 3 tan 1 deg = 0.052, focused well in front of the floor (4.7 .. 5 away)
LENS_COARSE, LENS_FINE = (4, 3, 8), (6, 4, 12)      # quadratures of cosine_law_lens: footprint nodes per axis, lens radii, lens angles
N_MANY, TINY = 37, (0, 5, 6, 13, 20, 27, 31, 36)     # many_lights: the tiny triangles' places in scene order (first, last, two neighbours)
BIG_SIDE, SIDE_RANGE, TINY_SIDE = 0.18, 0.03, 0.18 * 2e-4      # sides in units of LIGHT's edges: 29 from 0.18 down to 0.03 of it, 8 of 3.6e-5
FLOOR_AB = G.quad([-50, 0, -48.5], [50, 0, -48.5], [50, 0, 51.5], [-50, 0, 51.5])      # its diagonal z = x + 1.5 runs through CAMERA's look-at point
# two emitters in the one plane y = 2.25 + x / 8 + z / 16, on dyadic coordinates (the float32 vertices lie in it exactly): no segment from
# the floor to one of them can cross the other, so every shadow ray is free and the expectation is the plain sum of form factors
_in_plane = lambda xz: np.array([(x, 2.25 + x / 8.0 + z / 16.0, z) for x, z in xz], np.float32)
RED_LIGHT = _in_plane([(-1.75, 0.25), (-0.125, 0.5), (-0.875, 2.0)])
BLUE_LIGHT = _in_plane([(0.125, 0.5), (1.5, 0.75), (0.75, 2.0)])
UP_CAMERA = (34.0, (0.0, 0.1, 2.6), (0.0, 2.3, 1.1))      # under the two emitters, looking up at them
# two draws of the light pick found by find_draw (test_direct_light_reference.py re-derives both): sample DRAW_S[which] of pixel DRAW_PIXEL
# under DRAW_SEED draws k = thresholds[a] of a pinned light a (width 1) / k = thresholds[m] of a light m wider than 1
DRAW_SEED, DRAW_PIXEL = 0x5eed0123456789ab, (17, 9)
DRAW_S = {"pinned": 2356909, "edge": 143164}
NAMES = ("floor_under_sky", "cosine_law", "split_light", "sky_blocker", "occluded_light", "many_lights", "two_emitters", "emitters_in_view",
         "floor_under_sky_lens", "cosine_law_lens")
PARTS = {"floor_under_sky": ("sky",), "cosine_law": ("lights",), "split_light": ("lights",), "sky_blocker": ("sky",), "occluded_light": ("lights",),
         "many_lights": ("lights",), "two_emitters": ("lights",), "emitters_in_view": ("emitted",), "floor_under_sky_lens": ("sky",),
         "cosine_law_lens": ("lights",)}
SAMPLES = {"floor_under_sky": 8, "cosine_law": 256, "split_light": 256, "sky_blocker": 256, "occluded_light": 256, "many_lights": 256,
           "two_emitters": 256, "emitters_in_view": 8, "floor_under_sky_lens": 8, "cosine_law_lens": 256}
LENS_CAMERAS = ("random_spheres", "floor_under_sky_lens", "cosine_law_lens")      # RANDOM_SPHERES' default camera at 64 x 48 (0.6 degrees) and the lens cases' own
EXACT = ("floor_under_sky", "floor_under_sky_lens")                                              # every pixel T_sky to rounding
ALL_HELD = ("cosine_law", "split_light", "many_lights", "two_emitters", "cosine_law_lens")      # every pixel is a floor pixel with a variance


def many_lights():
    """(37, 3, 3) float32: disjoint triangles in LIGHT's plane, one per 0.2 x 0.2 cell of the plane's (e1, e2) coordinates, every third
    wound the other way; the sides of the 29 wide ones fall geometrically from BIG_SIDE to SIDE_RANGE of it in a scattered order (areas
    over three decades), the 8 at TINY have TINY_SIDE (an area 4e-8 of the largest's: less than one of the 2^24 draws)"""
    v0, e1, e2 = G.f64(G.LIGHT[0]), G.f64(G.LIGHT[1] - G.LIGHT[0]), G.f64(G.LIGHT[2] - G.LIGHT[0])
    sides = iter(BIG_SIDE * SIDE_RANGE ** (((np.arange(N_MANY - len(TINY)) * 11) % (N_MANY - len(TINY))) / (N_MANY - len(TINY) - 1.0)))
    out = []
    for k in range(N_MANY):
        a, b = 0.2 * (k % 7) + 0.01, 0.2 * (k // 7) + 0.01
        side = TINY_SIDE if k in TINY else next(sides)
        p = [v0 + a * e1 + b * e2, v0 + (a + side) * e1 + b * e2, v0 + a * e1 + (b + side) * e2]
        out.append(p[::-1] if k % 3 == 1 else p)
    return np.array(out, np.float32)


def two_emitter_materials():
    """[floor A, emitter blue, floor B, emitter red]: the floors' reflectances fall and rise with the wavelength, the emitters peak far apart"""
    return [G.material(G.MAT_LAMBERTIAN, G.ramp(0.9, 0.1)), G.material(G.MAT_EMISSIVE, G.bump(0.05, 6.0, 450.0, 30.0)), G.GREY,
            G.material(G.MAT_EMISSIVE, G.bump(0.05, 6.0, 620.0, 30.0))]


def _scene(name):
    if name == "floor_under_sky":
        sc, camera, W, H, _, _ = G.floor_under_sky()
        return sc, camera, W, H
    if name == "cosine_law":
        sc, camera, W, H, _, _ = G.cosine_law()
        return sc, camera, W, H
    if name == "split_light":
        mid = (G.LIGHT[1] + np.float32(0.3) * (G.LIGHT[2] - G.LIGHT[1])).astype(np.float32)
        V = G.FLOOR + [np.array([G.LIGHT[0], G.LIGHT[1], mid]), np.array([G.LIGHT[0], G.LIGHT[2], mid])]      # (the second one wound the other way: its normal is the first one's, negated)
        sc = G.cosine_law()[0]
        return G.scene(V, sc["mats"], mat_index=[0, 0, 1, 1]), CAMERA, 40, 24
    if name == "sky_blocker":
        V = G.FLOOR + [G.LIGHT]
        return G.scene(V, [G.material(G.MAT_LAMBERTIAN, G.ramp()), G.GREY], mat_index=[0, 0, 1], background=GREY_SKY), CAMERA, 40, 24
    if name == "many_lights":
        V = G.FLOOR + list(many_lights())
        return G.scene(V, G.cosine_law()[0]["mats"], mat_index=[0, 0] + [1] * N_MANY), CAMERA, 40, 24
    if name in ("two_emitters", "emitters_in_view"):      # the red light (material 3) first: slot 0 is material 3, slot 1 material 1
        V = FLOOR_AB + [RED_LIGHT, BLUE_LIGHT]
        if name == "two_emitters":
            return G.scene(V, two_emitter_materials(), mat_index=[0, 2, 3, 1]), CAMERA, 40, 24
        return G.scene(V, two_emitter_materials(), mat_index=[0, 2, 3, 1], background=GREY_SKY), UP_CAMERA, 64, 48
    if name in ("floor_under_sky_lens", "cosine_law_lens"):
        sc, camera, W, H = _scene(name[:-5])
        return sc, tuple(camera) + LENS, W, H
    assert name == "occluded_light", name
    V = G.FLOOR + [OCC_LIGHT] + G.quad(*BLOCKER.tolist())
    return G.scene(V, [G.material(G.MAT_LAMBERTIAN, G.ramp()), EMITTER(), G.GREY], mat_index=[0, 0, 1, 2, 2]), CAMERA, 40, 24


def case(srt, name):
    """dict(sc, scene, desc, cam, W, H, parts, samples) of a truth scene, built once per session"""
    def make():
        sc, camera, W, H = _scene(name)
        scene = G.product_scene(srt, sc, srt.BVH_SAH)
        return dict(sc=sc, scene=scene, desc=R.describe(srt, scene), cam=G.camera(srt, camera, W, H), W=W, H=H, parts=PARTS[name],
                    samples=SAMPLES[name])
    return G.cached(("direct light case", name), make)


# ---- the occluded light's exact truth ---------------------------------------------------------------------------------------------
def _plane_basis(poly):
    n = np.cross(poly[1] - poly[0], poly[2] - poly[0])
    n = n / np.linalg.norm(n)
    u = poly[1] - poly[0]
    u = u / np.linalg.norm(u)
    return poly[0], n, u, np.cross(n, u)


def _clip(subject, clip):
    """Sutherland-Hodgman: the convex polygon `subject` (k, 2) clipped against the convex polygon `clip` (either winding)"""
    area2 = np.dot(clip[:, 0], np.roll(clip[:, 1], -1)) - np.dot(clip[:, 1], np.roll(clip[:, 0], -1))
    if area2 < 0:
        clip = clip[::-1]
    pts = [p for p in subject]
    for a, b in zip(clip, np.roll(clip, -1, axis=0)):
        side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        nxt = []
        for p, q in zip(pts, pts[1:] + pts[:1]):
            sp, sq = side(p), side(q)
            if sp >= 0:
                nxt.append(p)
            if (sp >= 0) != (sq >= 0):
                nxt.append(p + (q - p) * sp / (sp - sq))
        pts = nxt
        if not pts:
            break
    return np.array(pts) if len(pts) >= 3 else np.zeros((0, 2))


def occluded_share(x, light, blocker):
    """(F_visible, F_light, dark) at floor points x (m, 3), normal +y: F_light - F(light n projected blocker), exactly; dark where the shadow
    covers the whole light (F_visible is then 0 exactly).  Asserts that the blocker lies strictly on one side of the light's plane."""
    light, blocker = G.f64(light), G.f64(blocker)
    o, n, u, v = _plane_basis(light)
    sb = (blocker - o) @ n
    assert (sb > 1e-6).all() or (sb < -1e-6).all(), "the blocker crosses the light's plane"
    nrm = np.array([0.0, 1.0, 0.0])
    F_light = G.form_factor(x, nrm, light)
    vis, dark = F_light.copy(), np.zeros(len(x), bool)
    l2 = np.stack([(light - o) @ u, (light - o) @ v], 1)
    light_area = G.polygon_area(l2)
    for k, p in enumerate(x):
        sx = (p - o) @ n
        if sx * sb[0] <= 0:          # the blocker is beyond the light's plane as seen from p: no segment to the light meets it
            continue
        s = -sx / ((blocker - p) @ n)          # p + s (b - p) lies in the plane; s > 1: the blocker is between
        assert (s > 1.0).all(), "a blocker vertex is not between the floor point and the light's plane"
        proj = p[None, :] + s[:, None] * (blocker - p[None, :])
        shadow = _clip(l2, np.stack([(proj - o) @ u, (proj - o) @ v], 1))
        if len(shadow) == 0:
            continue
        if abs(G.polygon_area(shadow) - light_area) <= 1e-12 * light_area:
            vis[k], dark[k] = 0.0, True
            continue
        poly3 = o[None, :] + shadow[:, 0:1] * u[None, :] + shadow[:, 1:2] * v[None, :]
        vis[k] = F_light[k] - G.form_factor(p[None, :], nrm, poly3)[0]
    return vis, F_light, dark


def occluded_share_quadrature(x, light, blocker, nodes):
    """F_visible by float64 midpoint quadrature of the light (nodes^2 barycentric cells), visibility by segment against the blocker's plane
    and its convex interior"""
    light, blocker = G.f64(light), G.f64(blocker)
    e1, e2 = light[1] - light[0], light[2] - light[0]
    nl = np.cross(e1, e2)
    area = 0.5 * np.linalg.norm(nl)
    nl = nl / np.linalg.norm(nl)
    i, j = np.mgrid[0:nodes, 0:nodes]
    a, b = (i.ravel() + 0.5) / nodes, (j.ravel() + 0.5) / nodes
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    q = light[0][None, :] + a[:, None] * e1[None, :] + b[:, None] * e2[None, :]
    bo, bn, bu, bv = _plane_basis(blocker)
    b2 = np.stack([(blocker - bo) @ bu, (blocker - bo) @ bv], 1)
    if np.dot(b2[:, 0], np.roll(b2[:, 1], -1)) - np.dot(b2[:, 1], np.roll(b2[:, 0], -1)) < 0:
        b2 = b2[::-1]
    out = np.zeros(len(x))
    for k, p in enumerate(x):
        d = q - p[None, :]
        r2 = (d * d).sum(1)
        f = np.maximum(d[:, 1], 0) * np.abs(d @ nl) / (np.pi * r2 * r2)
        s = ((bo - p) @ bn) / (d @ bn)
        hitp = p[None, :] + s[:, None] * d
        h2 = np.stack([(hitp - bo) @ bu, (hitp - bo) @ bv], 1)
        inside = (s > 0) & (s < 1)
        for c0, c1 in zip(b2, np.roll(b2, -1, axis=0)):
            inside &= (c1[0] - c0[0]) * (h2[:, 1] - c0[1]) - (c1[1] - c0[1]) * (h2[:, 0] - c0[0]) >= 0
        out[k] = (f * ~inside).mean() * area
    return out


# ---- expectations -----------------------------------------------------------------------------------------------------------------
def lens_rays(cam, W, H, fx, fy, nr, na):
    """[(eye, d)] of the rays to the pixel samples (i + fx, j + fy) of the grid: from the camera's centre, or, under a thin lens, from each
    of G.lens_points(cam, nr, na) -- the grid lies in the focus plane, so every lens point aims at the same sample"""
    centre, d = G.pixel_rays(cam, W, H, fx, fy)
    if not cam.defocus_angle > 0:
        return [(centre, d)]
    sample = centre[None, :] + d
    return [(eye, sample - eye[None, :]) for eye in G.lens_points(cam, nr, na)]


def lens_footprint_average(fn, cam, W, H, k, nr, na):
    """G.footprint_average over the lens as well: k x k Gauss-Legendre nodes of the footprint (the rows near the horizon see metres of
    floor through one pixel, and midpoints converge as 1 / k^2 only) times the nr x na polar midpoint grid of the lens"""
    x, w = np.polynomial.legendre.leggauss(k)
    acc = np.zeros(W * H)
    for a in range(k):
        for b in range(k):
            rays = lens_rays(cam, W, H, 0.5 * x[a], 0.5 * x[b], nr, na)
            for eye, d in rays:
                acc += (0.25 * w[a] * w[b] / len(rays)) * fn(eye, d)
    return acc


def first_hits(c, fx, fy):
    """[(H * W,) triangle index] of the float64 truth's first hit through the pixel samples (i + fx, j + fy), one per lens point"""
    V = G.f64(c["sc"]["V"])
    return [G.closest_hit(V, np.broadcast_to(eye, d.shape), d)[1] for eye, d in lens_rays(c["cam"], c["W"], c["H"], fx, fy, *LENS_COARSE[1:])]


def held_pixels(c):
    """(H * W,) bool: every footprint sub-sample's first hit is the floor (triangles 0 and 1) in the float64 truth, from every lens point"""
    held = np.ones(c["W"] * c["H"], bool)
    for a in range(K):
        for b in range(K):
            for tri in first_hits(c, (a + 0.5) / K - 0.5, (b + 0.5) / K - 0.5):
                held &= (tri == 0) | (tri == 1)
    return held


RED, BLUE, SKY, MIXED = 0, 1, 2, 3          # what a pixel of emitters_in_view shows


def view_classes(c):
    """(H * W,) class of every pixel of emitters_in_view: RED / BLUE where the K x K footprint sub-samples and the footprint's four corners
    all have that emitter (triangle 2 / 3) as their first hit in the float64 truth -- the corners make it the whole square, the emitter's
    image being convex --, SKY where they all miss and so do all of the eight neighbours' (no tip of a triangle reaches in between the
    sub-samples), MIXED otherwise"""
    W, H = c["W"], c["H"]
    offsets = [((a + 0.5) / K - 0.5, (b + 0.5) / K - 0.5) for a in range(K) for b in range(K)] + [(-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), (0.5, 0.5)]
    tris = np.stack([first_hits(c, fx, fy)[0] for fx, fy in offsets])
    cls = np.full(W * H, MIXED)
    cls[(tris == 2).all(0)], cls[(tris == 3).all(0)] = RED, BLUE
    empty = np.pad((tris < 0).all(0).reshape(H, W), 1, constant_values=True)
    cls[np.all([empty[a:a + H, b:b + W] for a in range(3) for b in range(3)], axis=0).ravel()] = SKY
    return cls


def floor_hits(eye, d):
    """where rays from eye meet the plane y = 0 (rays that do not run downwards get a far point: their pixels are not held)"""
    s = np.where(d[:, 1] < 0, -eye[1] / np.where(d[:, 1] < 0, d[:, 1], -1.0), 1e3)
    return eye[None, :] + s[:, None] * d


def lens_share(c, k, nr, na):
    """cosine_law's F averaged over footprint and lens (lens_footprint_average), float64"""
    return lens_footprint_average(lambda eye, d: G.form_factor(floor_hits(eye, d), (0.0, 1.0, 0.0), G.f64(G.LIGHT)), c["cam"], c["W"], c["H"], k, nr, na)


def two_emitters_expectation(c, tab, break_=None):
    """dict(E (3, H * W)): per sub-sample on floor triangle f, sum over the emitters e of T_light[mat(f), e] F_e, footprint-averaged.
    break_: None, or one of the deliberate breaks the tests try -- "emitters" swaps the two emitters' T, "floors" the floor materials' rows"""
    V, mi = G.f64(c["sc"]["V"]), c["sc"]["mat_index"]
    W, H = c["W"], c["H"]
    E = np.zeros((3, W * H))
    for f in (0, 1):
        for e in (2, 3):
            def part(eye, d):
                tri = G.closest_hit(V, np.broadcast_to(eye, d.shape), d)[1]
                return np.where(tri == f, G.form_factor(floor_hits(eye, d), (0.0, 1.0, 0.0), V[e]), 0.0)
            surface, emitter = mi[1 - f if break_ == "floors" else f], mi[5 - e if break_ == "emitters" else e]
            E += tab["t_light"][surface, emitter].astype(np.float64)[:, None] * G.footprint_average(part, c["cam"], W, H, K)[None, :]
    return dict(E=E)


def expectation(srt, name):
    """dict(E (3, H * W), held, dark) of a truth scene for its part: the expected per-sample contribution of every pixel"""
    def make():
        c = case(srt, name)
        tab = R.tables(c["desc"])
        held = held_pixels(c)
        W, H = c["W"], c["H"]
        dark = np.zeros(W * H, bool)
        if name == "floor_under_sky":
            share, T = np.ones(W * H), tab["t_sky"][0]
        elif name in ("cosine_law", "split_light"):
            share = G.footprint_average(lambda eye, d: G.form_factor(floor_hits(eye, d), (0.0, 1.0, 0.0), G.f64(G.LIGHT)), c["cam"], W, H, K)
            T = tab["t_light"][0, 1]
        elif name == "sky_blocker":
            share = 1.0 - G.footprint_average(lambda eye, d: G.form_factor(floor_hits(eye, d), (0.0, 1.0, 0.0), G.f64(G.LIGHT)), c["cam"], W, H, K)
            T = tab["t_sky"][0]
        elif name == "many_lights":
            lights = G.f64(c["sc"]["V"][2:])          # the float32 vertices the device has
            share = G.footprint_average(lambda eye, d: sum(G.form_factor(floor_hits(eye, d), (0.0, 1.0, 0.0), l) for l in lights), c["cam"], W, H, K)
            T = tab["t_light"][0, 1]
        elif name == "two_emitters":
            return dict(two_emitters_expectation(c, tab, break_=None), held=held, dark=dark)
        elif name == "emitters_in_view":
            cls = view_classes(c)
            T = np.stack([tab["t_emit"][3], tab["t_emit"][1], tab["t_bg"], np.zeros(3, np.float32)]).astype(np.float64)
            return dict(E=T[cls].T, held=cls != MIXED, dark=dark, cls=cls)
        elif name == "floor_under_sky_lens":
            share, T = np.ones(W * H), tab["t_sky"][0]
        elif name == "cosine_law_lens":
            share, T = lens_share(c, *LENS_FINE), tab["t_light"][0, 1]
        else:
            all_dark = np.ones(W * H, bool)

            def vis(eye, d):
                v, _, dk = occluded_share(floor_hits(eye, d), OCC_LIGHT, BLOCKER)
                all_dark[:] &= dk
                return v
            share = G.footprint_average(vis, c["cam"], W, H, K)
            T = tab["t_light"][0, 1]
            dark = all_dark & held
            share = np.where(dark, 0.0, share)
        return dict(E=T.astype(np.float64)[:, None] * share[None, :], held=held, dark=dark, share=share, T=T)
    return G.cached(("direct light expectation", name), make)


def dark_neighbourhood(exp, W, H):
    """pixels that are dark and held, with their eight neighbours (off-image neighbours do not count against them)"""
    ok = np.pad((exp["dark"] & exp["held"]).reshape(H, W), 1, constant_values=True)
    return np.all([ok[a:a + H, b:b + W] for a in range(3) for b in range(3)], axis=0).ravel() & exp["dark"]


def assert_holds(name, exp, out_sum, out_m2, S, W, H, what):
    """the module docstring's conditions on sums (H, W, 3); returns the figures for the test's printed line"""
    s, m2 = out_sum.reshape(-1, 3).astype(np.float64), out_m2.reshape(-1, 3).astype(np.float64)
    held = exp["held"]
    mean = s / S
    figures = dict(pixels=int(held.sum()))
    if name in EXACT:
        assert held.all(), "%s: every pixel shows the floor" % name
        rel = np.abs(mean - exp["E"].T) / exp["E"].T
        figures["max_rel"] = float(rel.max())
        assert rel.max() <= (S - 1) * 2.0 ** -24, (what, figures)
        return figures
    if name == "emitters_in_view":      # S equal terms T_emit[material] or T_bg: the float32 sum of S of them is (S - 1) roundings off at most
        figures["classes"] = [int((exp["cls"] == k).sum()) for k in (RED, BLUE, SKY)]
        assert min(figures["classes"]) >= G.MIN_PIXELS, (what, figures)
        rel = np.abs(mean[held] - exp["E"].T[held]) / exp["E"].T[held]
        figures["max_rel"] = float(rel.max())
        assert rel.max() <= (S - 1) * 2.0 ** -24, (what, figures, "worst pixel %d" % np.nonzero(held)[0][rel.max(1).argmax()])
        return figures
    var = np.maximum(m2 - S * mean * mean, 0.0) / (S - 1) / S
    dark = dark_neighbourhood(exp, W, H)
    figures["dark"] = int(dark.sum())
    assert not s[dark].any(), "%s: %d dark pixels are lit" % (what, (s[dark] != 0).any(1).sum())
    rms, zimg = [], []
    for ch in range(3):
        E = exp["E"][ch]
        use = held & (var[:, ch] > 0) & ~exp["dark"]
        if name == "sky_blocker":      # a Bernoulli term T x [the sky ray leaves]: its exact variance, where both outcomes are expected MIN_EXPECTED times
            p = exp["share"]
            var[:, ch] = float(exp["T"][ch]) ** 2 * p * (1.0 - p) / S
            use = held & (S * p >= G.MIN_EXPECTED) & (S * (1 - p) >= G.MIN_EXPECTED)
        z = (mean[use, ch] - E[use]) / np.sqrt(var[use, ch])
        figures.setdefault("z_pixels", []).append(int(use.sum()))
        assert use.sum() >= G.MIN_PIXELS, (what, ch, int(use.sum()))
        if name in ALL_HELD:
            assert use.sum() == held.sum() == W * H, (what, "every floor pixel is held", int(use.sum()))
        rms.append(float(np.sqrt((z * z).mean())))
        zimg.append(float((mean[held, ch].sum() - E[held].sum()) / np.sqrt(var[held, ch].sum())))
        allowance = E[held].sum() * S * 2.0 ** -24 / np.sqrt(var[held, ch].sum())
        assert abs(zimg[-1]) <= G.Z_IMG_MAX + allowance, (what, ch, zimg, allowance)
    figures.update(rms_z=[round(r, 3) for r in rms], z_img=[round(z, 2) for z in zimg])
    assert all(G.RMS_Z_RANGE[0] <= r <= G.RMS_Z_RANGE[1] for r in rms), (what, figures)
    return figures


# ---- single draws of the light pick -----------------------------------------------------------------------------------------------
def find_draw(values, pid, seed, start=0, block=1 << 20, limit=1 << 28):
    """(s, k): the first sample index s >= start of pixel id pid whose light draw k = philox(pid, s, 2, 0, key)[0] >> 8 is one of `values`.
    How DRAW_S was found: Philox is counter-based, so the search costs one vector call per 2^20 indices; a width-1 light is drawn once in
    2^24 / 8 = 2 M indices when 8 are pinned."""
    key, values = R.seed_key(seed), np.asarray(values, np.uint32)
    for s0 in range(start, limit, block):
        s = np.arange(s0, min(s0 + block, limit), dtype=np.uint32)
        k = R.philox(pid, s, 2, 0, *key)[0] >> np.uint32(8)
        at = np.nonzero(np.isin(k, values))[0]
        if len(at):
            return int(s[at[0]]), int(k[at[0]])
    return None


def draw_targets(th):
    """dict(pinned, edge): the draws k that find_draw looked for among the thresholds th -- thresholds[a] of the lights of width 1, and
    thresholds[m] of the lights wider than 1 (m > 0: the draw 0 is no edge between two lights)"""
    width = np.diff(th.astype(np.int64))
    return dict(pinned=th[:-1][width == 1], edge=th[1:-1][width[1:] > 1])


def assert_weight_holds(tab, rec, light_row, a, what):
    """the record and light row of one shaded floor sample whose draw picked light a: the pick, the traced row, and the weight against the
    float64 value of (n . d) |n_l . d| / (pi r^4) x area / p_l on the row's own float32 d.  The bound counts the rounded float32 operations
    (each within 2^-24 relative; n = (0, 1, 0), so n . d = d.y exactly):
        |n_l . d|: three products and two sums, 3 roundings on sum |n_l,i d_i|, that is 3 c on the result, c = sum |n_l,i d_i| / |n_l . d|
        (n . d) x that: 1          r^2 = d . d, all terms positive: 3          r^2 r^2: 2 x 3 + 1          x pi: 1, and 1 for the float32 pi itself
        the quotient: 1            area / p_l: 1 (0 where p_l is a power of two: the width -> float and x 2^-24 are exact)          the product: 1
    n = 3 c + 12 + [p_l is no power of two], and |w / w64 - 1| <= (1 + 2^-24)^n - 1.  Returns (relative error, bound)."""
    assert int(rec[2]) == a, (what, "picked light %d, the draw belongs to %d" % (int(rec[2]), a))
    assert (int(rec[3]) & 3) == R.SHADED and (int(rec[3]) & R.ROW_LIGHT), (what, "the light row is not traced", int(rec[3]))
    assert light_row[3] == 0.0 and light_row[7] == R.SHADOW_END, (what, light_row)
    d, nl = G.f64(light_row[4:7]), G.f64(tab["normal"][a])
    width = int(tab["thresholds"][a + 1]) - int(tab["thresholds"][a])
    terms = nl * d
    c = np.abs(terms).sum() / abs(terms.sum())
    r2 = (d * d).sum()
    want = d[1] * abs(terms.sum()) / (np.pi * r2 * r2) * float(tab["area"][a]) / (width * 2.0 ** -24)
    n = 3.0 * c + 12.0 + (width & (width - 1) != 0)
    got = float(np.asarray(rec[0], np.uint32).view(np.float32))
    rel, bound = abs(got / want - 1.0), (1.0 + G.U) ** n - 1.0
    assert d[1] > 0 and want > 0 and rel <= bound, (what, got, want, rel, bound)
    return rel, bound


# ---- the lens rows' geometry ------------------------------------------------------------------------------------------------------
def assert_lens_rows_hold(cam, W, H, rows, what):
    """camera rows (n_samples, H * W, 8) of a thin-lens camera held to geometry in float64 (module docstring of
    test_direct_light_reference.py, "lens rows"); returns the figures"""
    g = lambda name: np.array(getattr(cam, name)[:], np.float64)
    centre, p00, du, dv = G.camera_arrays(cam)
    U, V = g("defocus_disk_u"), g("defocus_disk_v")
    rows = G.f64(rows)
    n_samples = rows.shape[0]
    o, d = rows[:, :, 0:3].reshape(-1, 3), rows[:, :, 4:7].reshape(-1, 3)
    N = len(o)
    assert not (o == centre[None, :]).all(1).any(), (what, "a row starts at the lens centre")
    # origin = (centre + a U) + b V: two products and two sums, each component within 4 roundings of magnitude M
    M = np.abs(centre).max() + np.abs(U).max() + np.abs(V).max()
    err = np.sqrt(3.0) * 4.0 * G.U * M
    A = np.stack([U, V], 1)
    ab = np.linalg.lstsq(A, (o - centre[None, :]).T, rcond=None)[0]
    res = np.linalg.norm((o - centre[None, :]).T - A @ ab, axis=0)
    rad = np.sqrt((ab * ab).sum(0))
    slack = err / np.linalg.svd(A, compute_uv=False).min()
    figures = dict(rows=N, residual=float(res.max()), residual_bound=float(err), max_radius=float(rad.max()))
    assert res.max() <= err and rad.max() < 1.0 + slack, (what, figures)
    # origin + d is the pixel sample: p00 + (x + fx) du + (y + fy) dv with fx, fy in [-0.5, 0.5).  The sample took 8 rounded operations
    # from p00, d one more, all on magnitudes below Mp
    j, i = np.mgrid[0:H, 0:W]
    pc = p00[None, :] + i.ravel()[:, None] * du[None, :] + j.ravel()[:, None] * dv[None, :]
    off = (o + d) - np.tile(pc, (n_samples, 1))
    B = np.stack([du, dv], 1)
    f = np.linalg.lstsq(B, off.T, rcond=None)[0]
    Mp = np.abs(p00).max() + W * np.abs(du).max() + H * np.abs(dv).max() + np.abs(d).max()
    errp = np.sqrt(3.0) * 9.0 * G.U * Mp
    tol = errp / np.linalg.svd(B, compute_uv=False).min()
    out_of_plane = np.linalg.norm(off.T - B @ f, axis=0)
    figures.update(footprint=[float(f.min()), float(f.max())], footprint_tol=float(tol), out_of_plane=float(out_of_plane.max()))
    assert f.min() >= -0.5 - tol and f.max() <= 0.5 + tol and out_of_plane.max() <= errp, (what, figures)
    # a uniform disk's own moments at five standard deviations: a, b have mean 0 and variance 1/4, a^2 + b^2 mean 1/2 and variance 1/12
    m_a, m_b, m_r = float(ab[0].mean()), float(ab[1].mean()), float((rad * rad).mean())
    figures.update(mean_a=m_a, mean_b=m_b, mean_r2=m_r, mean_bound=2.5 / np.sqrt(N), r2_bound=5.0 * np.sqrt(1.0 / 12.0) / np.sqrt(N))
    assert abs(m_a) <= 2.5 / np.sqrt(N) and abs(m_b) <= 2.5 / np.sqrt(N) and abs(m_r - 0.5) <= 5.0 * np.sqrt(1.0 / 12.0) / np.sqrt(N), (what, figures)
    return figures
