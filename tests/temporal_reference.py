"""Temporal reprojection (include/srt_c_api.h, srt_temporal_accum) restated in numpy float32, operation by operation: every product, sum,
quotient, root and select in the order the header gives, each rounded once, selects as np.where.  Vectorised over the pixels with one loop
over the four taps.  It uses nothing of the product but the camera struct.  tests/test_temporal_reference.py holds this file to independent
arithmetic; tests/test_temporal.py holds the device to this file, bit for bit.  Also the synthetic inputs both suites share."""
import copy

import numpy as np

F = np.float32
DEFAULTS = dict(alpha_min=0.1, max_len=32.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
INF = float("inf")


def dot(a, b):
    """(a.x * b.x + a.y * b.y) + a.z * b.z"""
    with np.errstate(all="ignore"):
        return (((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)).astype(F)


def cross(a, b):
    """(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x)"""
    m = lambda p, q: F(F(p) * F(q))
    return np.array([F(m(a[1], b[2]) - m(a[2], b[1])), F(m(a[2], b[0]) - m(a[0], b[2])), F(m(a[0], b[1]) - m(a[1], b[0]))], F)


def camera_vectors(cam):
    """(du, dv, p00, center) of a camera struct as float32 vectors"""
    return tuple(np.array(list(v), F) for v in (cam.pixel_delta_u, cam.pixel_delta_v, cam.pixel00_loc, cam.camera_center))


def previous_constants(cam):
    """(n', e', k', bu', bv', center') of the previous camera: the header's host constants"""
    du, dv, p00, center = camera_vectors(cam)
    with np.errstate(all="ignore"):
        n = cross(du, dv)
        e = (p00 - center).astype(F)
        k = dot(e, n)
        cu, cv = cross(dv, n), cross(n, du)
        bu = (cu / dot(du, cu)).astype(F)
        bv = (cv / dot(dv, cv)).astype(F)
    return n, e, k, bu, bv, center


def finite3(v):
    with np.errstate(all="ignore"):
        return (((v - v) == F(0))[..., :3]).all(axis=-1)


def _inverse_count(samples):
    """inv = 1 / (float)n as (per pixel, per channel) factors: n the sample total or a per-pixel map (h, w)"""
    with np.errstate(all="ignore"):
        inv = (F(1) / np.asarray(samples).astype(F)).astype(F)
    return (inv, inv[..., None]) if inv.ndim == 2 else (inv, inv)


def guides_of(features, samples):
    """the prepass's guides (h, w, 8) = (N, z, A, cov) from raw feature sums (h, w, 8) and the sample total, or a per-pixel map (h, w)"""
    R = np.asarray(features, F)
    inv, inv3 = _inverse_count(samples)
    g = np.zeros(R.shape, F)
    with np.errstate(all="ignore"):
        g[..., 0:3] = (inv3 * R[..., 0:3]).astype(F)
        g[..., 3] = np.where(R[..., 7] > F(0), (R[..., 6] / R[..., 7]).astype(F), F(0))
        g[..., 4:7] = (inv3 * R[..., 3:6]).astype(F)
        g[..., 7] = (inv * R[..., 7]).astype(F)
    return g


def mean_of(sums, samples):
    """the prepass's colour: inv * S with inv = 1 / (float)n, n the total or a per-pixel map"""
    inv, inv3 = _inverse_count(samples)
    with np.errstate(all="ignore"):
        return (inv3 * np.asarray(sums, F)).astype(F)


def project(guides, cam, prev_cam, ox=0, oy=0):
    """steps 1 - 4 for every pixel of the (h, w) rectangle at (ox, oy): dict(hit, P -- the fp32 point of a hit pixel, the direction d of a
    sky pixel --, v, zexp, ok -- step 4 succeeded --, u, w)"""
    g = np.asarray(guides, F)
    h, w = g.shape[:2]
    du, dv, p00, center = camera_vectors(cam)
    n, e, k, bu, bv, pcenter = previous_constants(prev_cam)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        hit = g[..., 7] >= F(0.5)
        fi, fj = (ox + xs).astype(F)[..., None], (oy + ys).astype(F)[..., None]
        pc = ((p00 + (fi * du).astype(F)).astype(F) + (fj * dv).astype(F)).astype(F)
        d = (pc - center).astype(F)
        L = np.sqrt(dot(d, d)).astype(F)
        s = (g[..., 3] / L).astype(F)
        P = (center + (s[..., None] * d).astype(F)).astype(F)
        vh = (P - pcenter).astype(F)
        v = np.where(hit[..., None], vh, d).astype(F)
        zexp = np.where(hit, np.sqrt(dot(vh, vh)).astype(F), F(0)).astype(F)
        den = dot(v, n)
        t = (k / den).astype(F)
        ok = t > F(0)
        q = ((t[..., None] * v).astype(F) - e).astype(F)
        u = (dot(q, bu) - F(ox)).astype(F)
        ww = (dot(q, bv) - F(oy)).astype(F)
    return dict(hit=hit, P=np.where(hit[..., None], P, d).astype(F), v=v, zexp=zexp, ok=ok, u=u, w=ww)


def temporal(c, guides, cam, hist=None, ox=0, oy=0, alpha_min=0.1, max_len=32.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1):
    """the stage on the picture c (h, w, 3) with guides (h, w, 8) under the camera cam; hist: None or dict(colour (h, w, 4), guides
    (h, w, 8), cam) as a previous call returned it.  dict(colour (h, w, 4) = (o, len'), guides, cam -- the new history --, xyz, len,
    motion (h, w, 2), stats, and the masks blended / fresh / offscreen / rejected / nonfinite, tap_inside and tap_taken (4, h, w))."""
    c, g = np.asarray(c, F), np.asarray(guides, F)
    h, w = c.shape[:2]
    assert c.shape == (h, w, 3) and g.shape == (h, w, 8), (c.shape, g.shape)
    ys, xs = np.mgrid[0:h, 0:w]
    finite = finite3(c)
    motion = np.full((h, w, 2), np.nan, F)
    sw, sl, sc = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
    tap_inside, tap_taken = np.zeros((4, h, w), bool), np.zeros((4, h, w), bool)
    ok = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        if hist is not None:
            sn, sa, sz = F(sigma_normal), F(sigma_albedo), F(sigma_depth)
            kn, ka, kz = F(sn * sn), F(sa * sa), F(sz * sz)
            Hc, Hg = np.asarray(hist["colour"], F), np.asarray(hist["guides"], F)
            assert Hc.shape == (h, w, 4) and Hg.shape == (h, w, 8)
            pr = project(g, cam, hist["cam"], ox, oy)
            hit, zexp, ok, u, ww = pr["hit"], pr["zexp"], pr["ok"], pr["u"], pr["w"]
            mu, mv = (u - xs.astype(F)).astype(F), (ww - ys.astype(F)).astype(F)
            motion[..., 0] = np.where(ok, mu, F(np.nan))
            motion[..., 1] = np.where(ok, mv, F(np.nan))
            x0, y0 = np.floor(u).astype(F), np.floor(ww).astype(F)
            fx, fy = (u - x0).astype(F), (ww - y0).astype(F)
            for tap in range(4):
                a, b = tap & 1, tap >> 1
                tx = (x0 + F(1)).astype(F) if a else x0
                ty = (y0 + F(1)).astype(F) if b else y0
                wx = fx if a else (F(1) - fx).astype(F)
                wy = fy if b else (F(1) - fy).astype(F)
                wt = (wx * wy).astype(F)
                inside = ok & (tx >= F(0)) & (tx < F(w)) & (ty >= F(0)) & (ty < F(h))
                tap_inside[tap] = inside
                qx = np.where(inside, tx, F(0)).astype(np.int64)
                qy = np.where(inside, ty, F(0)).astype(np.int64)
                hc, hg = Hc[qy, qx], Hg[qy, qx]
                acc = (hc[..., 3] > F(0)) & finite3(hc) & ((hg[..., 7] >= F(0.5)) == hit)
                dn3 = (g[..., 0:3] - hg[..., 0:3]).astype(F)
                dn3 = (dn3 * dn3).astype(F)
                dn = ((dn3[..., 0] + dn3[..., 1]).astype(F) + dn3[..., 2]).astype(F)
                da3 = (g[..., 4:7] - hg[..., 4:7]).astype(F)
                da3 = (da3 * da3).astype(F)
                da = ((da3[..., 0] + da3[..., 1]).astype(F) + da3[..., 2]).astype(F)
                zq = hg[..., 3]
                m = np.where(zexp > zq, zexp, zq).astype(F)
                r = np.where(m > F(0), ((zexp - zq).astype(F) / m).astype(F), F(0)).astype(F)
                geo = (dn <= kn) & (da <= ka) & ((r * r).astype(F) <= kz)
                acc = acc & (geo | ~hit)
                take = inside & acc & (wt > F(0))
                tap_taken[tap] = take
                sw = np.where(take, (sw + wt).astype(F), sw).astype(F)
                sc = np.where(take[..., None], (sc + (wt[..., None] * hc[..., :3]).astype(F)).astype(F), sc).astype(F)
                sl = np.where(take, (sl + (wt * hc[..., 3]).astype(F)).astype(F), sl).astype(F)
        has = sw > F(0)
        nonfinite = ~finite
        fresh = finite & ~has
        blended = finite & has
        hh = (sc / sw[..., None]).astype(F)
        lh = (sl / sw).astype(F)
        ln = (lh + F(1)).astype(F)
        ln = np.where(ln < F(max_len), ln, F(max_len)).astype(F)
        al = (F(1) / ln).astype(F)
        al = np.where(al > F(alpha_min), al, F(alpha_min)).astype(F)
        mix = (hh + (al[..., None] * (c - hh).astype(F)).astype(F)).astype(F)
        o = np.where((blended & ~(al >= F(1)))[..., None], mix, c).astype(F)
        length = np.where(nonfinite, F(0), np.where(blended, ln, F(1))).astype(F)
    offscreen = np.zeros((h, w), bool)
    if hist is not None:
        offscreen = fresh & (~ok | ~tap_inside.any(axis=0))
    rejected = fresh & ~offscreen if hist is not None else np.zeros((h, w), bool)
    stats = dict(blended=int(blended.sum()), fresh=int(fresh.sum()), offscreen=int(offscreen.sum()), rejected=int(rejected.sum()),
                 nonfinite=int(nonfinite.sum()))
    colour = np.concatenate([o, length[..., None]], axis=-1).astype(F)
    return dict(colour=colour, guides=g.copy(), cam=cam, xyz=o, len=length, motion=motion, stats=stats, blended=blended, fresh=fresh,
                offscreen=offscreen, rejected=rejected, nonfinite=nonfinite, tap_inside=tap_inside, tap_taken=tap_taken)


# ---- cameras and inputs shared by the CPU and the GPU suite ----------------------------------------------------------------------------
def plain_camera(cam_type, width, height, du, dv, p00, center):
    """a camera struct from explicit vectors (no lens)"""
    cam = cam_type()
    cam.width, cam.height = width, height
    for name, v in (("pixel_delta_u", du), ("pixel_delta_v", dv), ("pixel00_loc", p00), ("camera_center", center)):
        for k in range(3):
            getattr(cam, name)[k] = float(v[k])
    return cam


def move_camera(cam, translate=(0.0, 0.0, 0.0), yaw_deg=0.0, pitch_deg=0.0):
    """cam moved rigidly: rotated about its own centre (yaw about y, then pitch about x; float64, rounded to float32 once) and translated"""
    out = copy.deepcopy(cam)
    ya, pa = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Ry = np.array([[np.cos(ya), 0, np.sin(ya)], [0, 1, 0], [-np.sin(ya), 0, np.cos(ya)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(pa), -np.sin(pa)], [0, np.sin(pa), np.cos(pa)]])
    Rm = Rx @ Ry
    du, dv, p00, center = (np.asarray(v, np.float64) for v in camera_vectors(cam))
    nc = center + np.asarray(translate, np.float64)
    for name, v in (("pixel_delta_u", Rm @ du), ("pixel_delta_v", Rm @ dv), ("pixel00_loc", nc + Rm @ (p00 - center)), ("camera_center", nc)):
        for k in range(3):
            getattr(out, name)[k] = float(F(v[k]))
    return out


def shift_case(cam_type):
    """the exact-shift geometry: 64 x 48, the previous camera at the origin, du = (2^-6, 0, 0), dv = (0, -2^-6, 0), p00 = (-0.5, 0.375, -1),
    the current one moved by 3 * 2^-4 along x, a fronto-parallel plane at depth 4: u - x is exactly 3 and w - y exactly 0.
    (prev_cam, cur_cam, guides (48, 64, 8))"""
    W, H = 64, 48
    du, dv, p00 = (2.0 ** -6, 0, 0), (0, -2.0 ** -6, 0), (-0.5, 0.375, -1.0)
    prev = plain_camera(cam_type, W, H, du, dv, p00, (0, 0, 0))
    cur = plain_camera(cam_type, W, H, du, dv, (p00[0] + 0.1875, p00[1], p00[2]), (0.1875, 0, 0))
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([F(-0.5) + xs.astype(F) * F(2.0 ** -6), F(0.375) - ys.astype(F) * F(2.0 ** -6), np.full((H, W), F(-1))], axis=-1).astype(F)
    L = np.sqrt(dot(d, d)).astype(F)
    g = np.zeros((H, W, 8), F)
    g[..., 2] = 1.0
    g[..., 3] = (F(4) * L).astype(F)          # (exact: s = z / L is 4)
    g[..., 4:7] = 0.5
    g[..., 7] = 1.0
    return prev, cur, g


def random_case(w, h, seed=0, holes=True, specials=True):
    """a random picture, guides and history of a w x h rectangle: both classes, guides of the history equal to the current ones at most
    pixels (so that taps are accepted) and different at others, len = 0 holes and non-finite values in picture and history.
    (c (h, w, 3), guides (h, w, 8), hist_colour (h, w, 4), hist_guides (h, w, 8))"""
    rng = np.random.default_rng(1000 * w + h + 7919 * seed)
    c = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    g = np.zeros((h, w, 8), F)
    g[..., 0:3] = np.where((np.arange(w) < (w + 1) // 2)[None, :, None], F([0.0, 0.0, 1.0]), F([0.0, 0.6, 0.8]))
    g[..., 3] = rng.uniform(4.9, 5.1, (h, w)).astype(F)
    g[..., 4:7] = rng.choice([0.25, 0.5, 0.75], (h, w, 1)).astype(F)
    g[..., 7] = rng.choice([0.0, 0.25, 0.75, 1.0], (h, w), p=[0.2, 0.1, 0.1, 0.6]).astype(F)
    sky = g[..., 7] < F(0.5)
    g[sky, 3] = rng.choice([0.0, 3.0], int(sky.sum())).astype(F)
    hg = g.copy()
    other = rng.random((h, w)) < 0.3
    hg[other, 0:3] = -hg[other, 0:3]
    far = rng.random((h, w)) < 0.2
    hg[far, 3] = (hg[far, 3] * F(1.5)).astype(F)
    flip = rng.random((h, w)) < 0.1
    hg[flip, 7] = F(1) - hg[flip, 7]
    hc = np.concatenate([rng.uniform(0.0, 2.0, (h, w, 3)), rng.integers(1, 40, (h, w, 1))], axis=-1).astype(F)
    if holes:
        hc[rng.random((h, w)) < 0.15, 3] = 0.0
    if specials and w * h >= 4:
        for val in (np.nan, np.inf, -np.inf):
            c[rng.integers(h), rng.integers(w), rng.integers(3)] = val
            hc[rng.integers(h), rng.integers(w), rng.integers(3)] = val
    return c, g, hc, hg
