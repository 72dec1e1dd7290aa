"""The surface-motion pass (include/srt_c_api.h, srt_surface_motion: step 4, and steps 1 and 3 around it) and the moving step 3 of the
temporal stage (srt_temporal_moving_kat) restated in numpy float32, operation by operation: every product, sum and quotient in the order the
header gives, each rounded once, selects as np.where.  The closest hit (t, k) of step 2 is an INPUT: the GPU suite takes it from
srt_trace_rays, the CPU suite from a brute-force float64 intersection.  tests/test_surface_motion_reference.py holds this file to
independent arithmetic; tests/test_surface_motion.py and tests/test_temporal_moving.py hold the device to this file, bit for bit."""
import numpy as np

import temporal_reference as T

F = np.float32


def centre_rays(cam, w, h, ox=0, oy=0):
    """step 1: (center (3,), d (h, w, 3)) of the w x h rectangle at (ox, oy)"""
    du, dv, p00, center = T.camera_vectors(cam)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        fi, fj = (ox + xs).astype(F)[..., None], (oy + ys).astype(F)[..., None]
        pc = ((p00 + (fi * du).astype(F)).astype(F) + (fj * dv).astype(F)).astype(F)
        d = (pc - center).astype(F)
    return center, d


def _finite(v):
    with np.errstate(all="ignore"):
        return (v - v) == F(0)


def move_points(center, d, t, k, v_cur, v_prev=None):
    """steps 3 and 4 for the rays (center, d (.., 3)) with the closest hits t (..) float32 and k (..) int (-1: a miss); v_cur, v_prev
    (n_tris, 3, 3) float32, v_prev None: nothing moved.  dict(point (.., 4), tri (..) int32, bary (.., 3), stats, and the intermediate
    P, beta, gamma, den, moved, valid, hit)"""
    center, d, t, k = np.asarray(center, F), np.asarray(d, F), np.asarray(t, F), np.asarray(k, np.int64)
    v_cur = np.asarray(v_cur, F)
    v_prev = v_cur if v_prev is None else np.asarray(v_prev, F)
    assert v_cur.shape == v_prev.shape and v_cur.shape[1:] == (3, 3) and d.shape == k.shape + (3,) and t.shape == k.shape
    hit = k >= 0
    kk = np.where(hit, k, 0)      # (no vertex row is read for a miss: a stand-in row, masked out below)
    m = lambda p, q: (p * q).astype(F)
    s = lambda p, q: (p - q).astype(F)
    with np.errstate(all="ignore"):
        P = (center + (t[..., None] * d).astype(F)).astype(F)
        a, b, c = v_cur[kk, 0], v_cur[kk, 1], v_cur[kk, 2]
        e1, e2, r = s(b, a), s(c, a), s(P, a)
        d11, d12, d22, r1, r2 = T.dot(e1, e1), T.dot(e1, e2), T.dot(e2, e2), T.dot(r, e1), T.dot(r, e2)
        den = s(m(d11, d22), m(d12, d12))
        beta = (s(m(d22, r1), m(d12, r2)) / den).astype(F)
        gamma = (s(m(d11, r2), m(d12, r1)) / den).astype(F)
        Da, Db, Dc = s(v_prev[kk, 0], a), s(v_prev[kk, 1], b), s(v_prev[kk, 2], c)
        moved = hit & ((Da != F(0)).any(axis=-1) | (Db != F(0)).any(axis=-1) | (Dc != F(0)).any(axis=-1))
        disp = ((Da + (beta[..., None] * s(Db, Da)).astype(F)).astype(F) + (gamma[..., None] * s(Dc, Da)).astype(F)).astype(F)
        Pm = (P + disp).astype(F)
        Pprev = np.where(moved[..., None], Pm, P).astype(F)
        ok = (den > F(0)) & _finite(beta) & _finite(gamma) & _finite(Pm).all(axis=-1)
        valid = hit & np.where(moved, ok, True)
    point = np.zeros(k.shape + (4,), F)
    point[..., :3] = np.where(valid[..., None], Pprev, F(0))
    point[..., 3] = np.where(valid, F(1), F(0))
    bary = np.zeros(k.shape + (3,), F)
    bary[..., 0] = np.where(hit, t, F(0))
    bary[..., 1] = np.where(hit, beta, F(0))
    bary[..., 2] = np.where(hit, gamma, F(0))
    stats = dict(hit=int(hit.sum()), miss=int((~hit).sum()), moved=int(moved.sum()), degenerate=int((moved & ~valid).sum()))
    return dict(point=point, tri=np.where(hit, k, -1).astype(np.int32), bary=bary, stats=stats, P=P, beta=beta, gamma=gamma, den=den,
                d11=d11, d22=d22, moved=moved, valid=valid, hit=hit)


def surface_motion(cam, t, k, v_cur, v_prev=None, ox=0, oy=0):
    """the pass over the (h, w) rectangle at (ox, oy) with the closest hits t, k (h, w) of its centre rays: move_points' dict"""
    h, w = np.asarray(k).shape
    center, d = centre_rays(cam, w, h, ox, oy)
    return move_points(center, d, t, k, v_cur, v_prev)


def trace_inputs(cam, w, h, ox=0, oy=0):
    """the centre rays of the rectangle as srt_trace_rays takes them: (w * h, 6) float32 = (origin, direction), row-major pixels"""
    center, d = centre_rays(cam, w, h, ox, oy)
    rays = np.zeros((h * w, 6), F)
    rays[:, :3] = center
    rays[:, 3:] = d.reshape(-1, 3)
    return rays


def hits_of_trace(out, w, h):
    """(t (h, w) float32, k (h, w) int) of srt_trace_rays' answer (n, 4) = (t or 0, triangle or -1, ..)"""
    out = np.asarray(out, F).reshape(h, w, 4)
    return out[..., 0].copy(), out[..., 1].astype(np.int64)


def project_moving(guides, cam, prev_cam, prev_point, ox=0, oy=0):
    """temporal_reference.project with the moving step 3: a hit pixel takes v = M.xyz - center' when M.w == 1 and fails step 4 otherwise"""
    g, M = np.asarray(guides, F), np.asarray(prev_point, F)
    h, w = g.shape[:2]
    assert M.shape == (h, w, 4)
    n, e, k, bu, bv, pcenter = T.previous_constants(prev_cam)
    _, d = centre_rays(cam, w, h, ox, oy)
    with np.errstate(all="ignore"):
        hit = g[..., 7] >= F(0.5)
        tracked = M[..., 3] == F(1)
        vh = (M[..., :3] - pcenter).astype(F)
        v = np.where(hit[..., None], vh, d).astype(F)
        zexp = np.where(hit, np.sqrt(T.dot(vh, vh)).astype(F), F(0)).astype(F)
        den = T.dot(v, n)
        t = (k / den).astype(F)
        ok = (t > F(0)) & (tracked | ~hit)
        q = ((t[..., None] * v).astype(F) - e).astype(F)
        u = (T.dot(q, bu) - F(ox)).astype(F)
        ww = (T.dot(q, bv) - F(oy)).astype(F)
    return dict(hit=hit, P=np.where(hit[..., None], M[..., :3], d).astype(F), v=v, zexp=zexp, ok=ok, u=u, w=ww)


def temporal_moving(c, guides, cam, prev_point, hist=None, ox=0, oy=0, **cfg):
    """the moving stage: temporal_reference.temporal, every operation of it, with project_moving in the place of its steps 1 - 4"""
    saved = T.project
    T.project = lambda g, cam_, prev_cam, ox_=0, oy_=0: project_moving(g, cam_, prev_cam, prev_point, ox_, oy_)
    try:
        return T.temporal(c, guides, cam, hist, ox, oy, **cfg)
    finally:
        T.project = saved


def static_points(guides, cam, ox=0, oy=0):
    """the point the static stage reconstructs from the distance guide, as prev_point: (center + (z_p / L) * d, 1) for every pixel"""
    g = np.asarray(guides, F)
    h, w = g.shape[:2]
    center, d = centre_rays(cam, w, h, ox, oy)
    with np.errstate(all="ignore"):
        L = np.sqrt(T.dot(d, d)).astype(F)
        s = (g[..., 3] / L).astype(F)
        P = (center + (s[..., None] * d).astype(F)).astype(F)
    return np.concatenate([P, np.ones((h, w, 1), F)], axis=-1).astype(F)


def brute_force_hits(center, d, verts):
    """closest hits of the rays (center, d (.., 3)) on the triangles verts (n, 3, 3), float64 Moeller-Trumbore, both faces: (t (..)
    float32 in units of d, k (..) int, -1 for a miss).  Independent of the product: it only supplies (t, k) to the restatement."""
    o = np.asarray(center, np.float64)
    D = np.asarray(d, np.float64).reshape(-1, 3)
    V = np.asarray(verts, np.float64)
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    best_t, best_k = np.full(D.shape[0], np.inf), np.full(D.shape[0], -1, np.int64)
    with np.errstate(all="ignore"):
        for k in range(V.shape[0]):
            p = np.cross(D, e2[k])
            det = p @ e1[k]
            s = o - V[k, 0]
            u = (p @ s) / det
            q = np.cross(s, e1[k])
            v = (D @ q) / det
            t = (q @ e2[k]) / det
            ok = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-6) & (t < best_t)
            best_t, best_k = np.where(ok, t, best_t), np.where(ok, k, best_k)
    shape = np.asarray(d).shape[:-1]
    return np.where(best_k >= 0, best_t, 0.0).astype(F).reshape(shape), best_k.reshape(shape)
