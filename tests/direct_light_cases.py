"""The truth scenes of the direct-light pass and what they are held to, shared by the CPU suite (restatement under the float64 queries) and
the GPU suite (the device's output, no restatement in between).

  floor_under_sky   ground_truth's floor under its sky: SKY gives every floor pixel T_sky exactly (every sky ray leaves).
  cosine_law        ground_truth's floor + LIGHT: LIGHTS gives T_light F, F = Lambert's form factor of the light averaged over the pixel.
  split_light       cosine_law with its light cut into two triangles of unequal area (0.3 : 0.7) and opposite winding: the same expectation,
                    a pick that must be divided out, and one light facing the floor with either face.
  sky_blocker       cosine_law with the light's triangle made Lambertian under a grey sky: SKY gives T_sky (1 - F(blocker)).
  occluded_light    the floor, a light above it (OCC_LIGHT) and a convex Lambertian quad between them: LIGHTS gives T_light (F(light) - F(light n shadow)),
                    the shadow being the blocker projected from the floor point onto the light's plane, clipped convex against convex.
Pixels are held where every sub-sample of the footprint (K x K midpoints) has the floor as its first hit in the float64 truth.

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
NAMES = ("floor_under_sky", "cosine_law", "split_light", "sky_blocker", "occluded_light")
PARTS = {"floor_under_sky": ("sky",), "cosine_law": ("lights",), "split_light": ("lights",), "sky_blocker": ("sky",), "occluded_light": ("lights",)}
SAMPLES = {"floor_under_sky": 8, "cosine_law": 256, "split_light": 256, "sky_blocker": 256, "occluded_light": 256}


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
def held_pixels(c):
    """(H * W,) bool: every footprint sub-sample's first hit is the floor (triangles 0 and 1) in the float64 truth"""
    V = G.f64(c["sc"]["V"])
    held = np.ones(c["W"] * c["H"], bool)
    for a in range(K):
        for b in range(K):
            eye, d = G.pixel_rays(c["cam"], c["W"], c["H"], (a + 0.5) / K - 0.5, (b + 0.5) / K - 0.5)
            _, tri, _, _ = G.closest_hit(V, np.broadcast_to(eye, d.shape), d)
            held &= (tri == 0) | (tri == 1)
    return held


def floor_hits(eye, d):
    """where rays from eye meet the plane y = 0 (rays that do not run downwards get a far point: their pixels are not held)"""
    s = np.where(d[:, 1] < 0, -eye[1] / np.where(d[:, 1] < 0, d[:, 1], -1.0), 1e3)
    return eye[None, :] + s[:, None] * d


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
    if name == "floor_under_sky":
        assert held.all(), "floor_under_sky: every pixel shows the floor"
        rel = np.abs(mean - exp["E"].T) / exp["E"].T
        figures["max_rel"] = float(rel.max())
        assert rel.max() <= (S - 1) * 2.0 ** -24, (what, figures)
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
        if name in ("cosine_law", "split_light"):
            assert use.sum() == held.sum() == W * H, (what, "every floor pixel is held", int(use.sum()))
        rms.append(float(np.sqrt((z * z).mean())))
        zimg.append(float((mean[held, ch].sum() - E[held].sum()) / np.sqrt(var[held, ch].sum())))
        allowance = E[held].sum() * S * 2.0 ** -24 / np.sqrt(var[held, ch].sum())
        assert abs(zimg[-1]) <= G.Z_IMG_MAX + allowance, (what, ch, zimg, allowance)
    figures.update(rms_z=[round(r, 3) for r in rms], z_img=[round(z, 2) for z in zimg])
    assert all(G.RMS_Z_RANGE[0] <= r <= G.RMS_Z_RANGE[1] for r in rms), (what, figures)
    return figures
