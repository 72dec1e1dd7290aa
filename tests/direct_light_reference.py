"""The numpy float32 restatement of the deferred direct-light pass (srt_direct_light; include/srt_c_api.h "Direct lighting").

Everything but the two ray queries is restated here, operation by operation in the order the header gives: Philox4x32-10, the host tables
(float64, rounded to float32 once), the light table with its integer thresholds, the camera rows, the shade rows with their records and the
gather.  The queries are arguments: run() takes intersect(rows (n, 8)) -> (n, 4) hit rows and occluded(rows) -> (n,) bool, which the GPU
suite binds to Renderer.intersect / occluded and the CPU suite to the float64 truth (truth_queries).

A scene is described by plain arrays (describe): V (n, 3, 3), normal (n, 3) -- the unit normals of srt_scene_get_tri_records --, mat_index
(n,), mat_type (m,), spectra (m, 95), background (95,), cmf (95, 3), all float32 where they are numbers the device computes with."""
import numpy as np

import ground_truth as G
import query_reference as Q

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
N_DRAWS = 1 << 24
MAX_LIGHTS = 1 << 20
EPSILON = F(0.0001)
PI = F(3.14159265358979)
SHADOW_END = F(1.0 - 2.0 ** -10)
DISK_TRIES, SPHERE_TRIES = 16, 32
PARTS = {"emitted": 1, "lights": 2, "sky": 4}
MISS, EMITTED, SPECULAR, SHADED, ROW_LIGHT, ROW_SKY = 0, 1, 2, 3, 4, 8
MAT_METALLIC, MAT_DIELECTRIC, MAT_EMISSIVE = 1, 2, 4
COUNTERS = ("miss", "emitted", "specular", "shaded", "light_rows", "light_unoccluded", "sky_rows", "sky_unoccluded")

# Philox4x32-10 known answers (Random123's kat_vectors): counter, key -> output
PHILOX_KAT = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ---- random numbers ---------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (broadcast against each other) under one key: four uint32 arrays"""
    c = [np.asarray(x, np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return [x.astype(np.uint32) for x in c]


def u01(x):
    return (x >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def pm1(x):
    return F(2.0) * u01(x) - F(1.0)


def seed_key(seed):
    return int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff


# ---- host tables ------------------------------------------------------------------------------------------------------------------
def integral(cmf, a=None, b=None):
    """(3,) float32: the integral of cmf a b over the grid, Simpson's rule per 5 nm cell in float64, cells added in ascending order"""
    c = np.asarray(cmf, F).astype(np.float64)
    one = np.ones(len(c))
    A = one if a is None else np.asarray(a, F).astype(np.float64)
    Bf = one if b is None else np.asarray(b, F).astype(np.float64)
    fa = (c[:-1] * A[:-1, None]) * Bf[:-1, None]
    fb = (c[1:] * A[1:, None]) * Bf[1:, None]
    fm = (((c[:-1] + c[1:]) * 0.5) * ((A[:-1] + A[1:]) * 0.5)[:, None]) * ((Bf[:-1] + Bf[1:]) * 0.5)[:, None]
    cell = ((fa + 4.0 * fm) + fb) * (5.0 / 6.0)
    return np.add.accumulate(cell, axis=0)[-1].astype(F)


def thresholds(g):
    """the integer thresholds (L + 1,) uint32 of the weights g (float64): largest remainder over 2^24 draws, every light at least 1 wide"""
    g = np.asarray(g, np.float64)
    L = len(g)
    if L == 0:
        return np.zeros(1, np.uint32)
    assert L <= MAX_LIGHTS
    pinned = np.zeros(L, bool)
    while True:
        G_ = np.add.accumulate(g[~pinned])[-1]
        B_ = float(N_DRAWS - pinned.sum())
        small = ~pinned & (g / G_ * B_ < 1.0)
        if not small.any():
            break
        pinned |= small
    ideal = g / G_ * B_
    width = np.where(pinned, 1, np.floor(ideal)).astype(np.int64)
    rem = np.where(pinned, -1.0, ideal - np.floor(ideal))
    free = np.nonzero(~pinned)[0]
    order = free[np.argsort(-rem[free], kind="stable")]
    left = N_DRAWS - int(width.sum())
    assert 0 <= left <= len(order)
    width[order[:left]] += 1
    return np.concatenate([[0], np.cumsum(width)]).astype(np.uint32)


def tables(desc):
    """dict of the host tables of a described scene: t_light (m, m, 3), t_sky (m, 3), t_emit (m, 3), t_bg (3,), bg_nonzero, and the light
    table: thresholds, v0, e1, e2, normal, area, mat, tri (per light, in scene order)"""
    cmf, sp, bg = desc["cmf"], desc["spectra"], desc["background"]
    m = len(sp)
    t_emit = np.stack([integral(cmf, sp[k]) for k in range(m)])
    t_sky = np.stack([integral(cmf, sp[k], bg) for k in range(m)])
    V = np.asarray(desc["V"], F)
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    a, b = e1.astype(np.float64), e2.astype(np.float64)
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = (0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)).astype(F)
    mi = np.asarray(desc["mat_index"], np.int64)
    keep = (np.asarray(desc["mat_type"])[mi] == MAT_EMISSIVE) & (area > 0) & (t_emit[mi, 1] > 0)
    k = np.nonzero(keep)[0]
    g = area[k].astype(np.float64) * t_emit[mi[k], 1].astype(np.float64)
    emissive = sorted(set(mi[k].tolist()))
    t_light = np.zeros((m, m, 3), F)
    for s in range(m):
        for e in emissive:
            t_light[s, e] = integral(cmf, sp[s], sp[e])
    return dict(t_light=t_light, t_sky=t_sky, t_emit=t_emit, t_bg=integral(cmf, bg), bg_nonzero=bool(np.any(np.asarray(bg) != 0)),
                thresholds=thresholds(g), v0=V[k, 0], e1=e1[k], e2=e2[k], normal=np.asarray(desc["normal"], F)[k], area=area[k],
                mat=mi[k].astype(np.uint32), tri=k.astype(np.uint32))


def describe(srt, scene):
    """the plain arrays of a product scene (module docstring)"""
    T, M = scene.triangles(), scene.materials()
    return dict(V=np.array([[t.v0[:], t.v1[:], t.v2[:]] for t in T], F), normal=scene.tri_records()[:, 0:3].copy(),
                mat_index=np.array([t.mat_index for t in T], np.int64), mat_type=np.array([m.material_type for m in M], np.int64),
                spectra=np.array([m.spectral_distribution[:] for m in M], F), background=scene.background(),
                cmf=G.color_tables(srt)[:3].T.astype(F))


# ---- one sample -------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def pixels(cam, w, h, ox, oy):
    """global x, y and the pixel id of the rectangle's pixels, row-major"""
    y, x = np.mgrid[0:h, 0:w]
    gx, gy = (x.ravel() + ox).astype(np.uint32), (y.ravel() + oy).astype(np.uint32)
    return gx, gy, gy * np.uint32(cam.width) + gx


def camera_rows(cam, gx, gy, pid, si, key):
    g = lambda name: np.array(getattr(cam, name)[:], F)
    du, dv, p00, centre, disk_u, disk_v = (g(n) for n in ("pixel_delta_u", "pixel_delta_v", "pixel00_loc", "camera_center", "defocus_disk_u",
                                                          "defocus_disk_v"))
    j = philox(pid, si, 0, 0, *key)
    px, py = F(-0.5) + u01(j[0]), F(-0.5) + u01(j[1])
    pc = (p00[None, :] + gx.astype(F)[:, None] * du[None, :]) + gy.astype(F)[:, None] * dv[None, :]
    ps = pc + (px[:, None] * du[None, :] + py[:, None] * dv[None, :])
    n = len(pid)
    origin = np.broadcast_to(centre, (n, 3)).astype(F)
    if not (F(cam.defocus_angle) <= F(0.0)):
        dx, dy, done = np.zeros(n, F), np.zeros(n, F), np.zeros(n, bool)
        for t in range(DISK_TRIES):
            idx = np.nonzero(~done)[0]
            if not len(idx):
                break
            q = philox(pid[idx], si, 1, t, *key)
            a, b = pm1(q[0]), pm1(q[1])
            acc = a * a + b * b < F(1.0)
            dx[idx[acc]], dy[idx[acc]] = a[acc], b[acc]
            done[idx[acc]] = True
        origin = (centre[None, :] + dx[:, None] * disk_u[None, :]) + dy[:, None] * disk_v[None, :]
    rows = np.zeros((n, 8), F)
    rows[:, 0:3] = origin; rows[:, 4:7] = ps - origin; rows[:, 7] = FLT_MAX
    return rows


def shade_rows(desc, tab, parts, cam, hits, pid, si, key):
    """(light_rows, sky_rows, records (n, 4) uint32) of one sample from its camera rows and their hit rows"""
    n = len(pid)
    n_tris = len(desc["V"])
    tri = hits[:, 1].astype(np.int64)
    on_tri = (tri >= 0) & (tri < n_tris)
    tk = np.where(on_tri, tri, 0)
    mat = np.where(on_tri, np.asarray(desc["mat_index"], np.int64)[tk], 0)
    mtype = np.asarray(desc["mat_type"], np.int64)[mat]
    kind = np.where(~on_tri, MISS, np.where(mtype == MAT_EMISSIVE, EMITTED, np.where((mtype == MAT_METALLIC) | (mtype == MAT_DIELECTRIC), SPECULAR,
                                                                                    SHADED)))
    idle = np.zeros((n, 8), F); idle[:, 3] = 1.0; idle[:, 6] = 1.0
    light_rows, sky_rows = idle.copy(), idle.copy()
    w, light = np.zeros(n, F), np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint32)
    s = np.nonzero(kind == SHADED)[0]
    L = len(tab["thresholds"]) - 1
    if len(s):
        o, d = cam[s, 0:3], cam[s, 4:7]
        n_geo = np.asarray(desc["normal"], F)[tk[s]]
        p = o + hits[s, 0][:, None] * d
        front = dot3(d, n_geo) < F(0.0)
        nrm = np.where(front[:, None], n_geo, -n_geo)
        o2 = p + EPSILON * nrm
        light_rows[s, 0:3] = o2; sky_rows[s, 0:3] = o2
        if (parts & PARTS["lights"]) and L > 0:
            q = philox(pid[s], si, 2, 0, *key)
            k = q[0] >> np.uint32(8)
            l = np.searchsorted(tab["thresholds"], k, side="right") - 1
            pl = (tab["thresholds"][l + 1] - tab["thresholds"][l]).astype(F) * F(2.0 ** -24)
            u1, u2 = u01(q[1]), u01(q[2])
            fold = u1 + u2 > F(1.0)
            u1, u2 = np.where(fold, F(1.0) - u1, u1), np.where(fold, F(1.0) - u2, u2)
            point = (tab["v0"][l] + u1[:, None] * tab["e1"][l]) + u2[:, None] * tab["e2"][l]
            dl = point - o2
            nd, r2 = dot3(nrm, dl), dot3(dl, dl)
            cl = np.abs(dot3(tab["normal"][l], dl))
            traced = (nd > 0) & (r2 > 0)
            with np.errstate(all="ignore"):
                ww = ((nd * cl) / ((r2 * r2) * PI)) * (tab["area"][l] / pl)
            w[s] = np.where(traced, ww, F(0.0))
            light[s] = l
            light_rows[s, 4:7] = dl
            light_rows[s, 3] = np.where(traced, F(0.0), F(1.0)); light_rows[s, 7] = np.where(traced, SHADOW_END, F(0.0))
            flags[s] |= np.where(traced, ROW_LIGHT, 0).astype(np.uint32)
        if (parts & PARTS["sky"]) and tab["bg_nonzero"]:
            ruv, done = nrm.copy(), np.zeros(len(s), bool)
            for t in range(SPHERE_TRIES):
                idx = np.nonzero(~done)[0]
                if not len(idx):
                    break
                q = philox(pid[s][idx], si, 3, t, *key)
                a, b, c = pm1(q[0]), pm1(q[1]), pm1(q[2])
                len2 = (a * a + b * b) + c * c
                acc = (len2 < F(1.0)) & (len2 > F(0.0))
                kk = F(1.0) / np.sqrt(len2[acc])
                ruv[idx[acc]] = kk[:, None] * np.stack([a, b, c], 1)[acc]
                done[idx[acc]] = True
            direction = nrm + ruv
            tiny = (np.abs(direction) < F(1e-8)).all(1)
            direction = np.where(tiny[:, None], nrm, direction)
            sky_rows[s, 3] = 0.0; sky_rows[s, 4:7] = direction; sky_rows[s, 7] = FLT_MAX
            flags[s] |= np.uint32(ROW_SKY)
    rec = np.stack([w.view(np.uint32), mat.astype(np.uint32), light, kind.astype(np.uint32) | flags], 1)
    return light_rows, sky_rows, rec


def contributions(tab, parts, rec, occ_light, occ_sky):
    """(e, l, k) (n, 3) float32 terms of one sample and its counters"""
    kind = rec[:, 3] & 3
    mat = rec[:, 1].astype(np.int64)
    n = len(rec)
    e, l, k = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
    if parts & PARTS["emitted"]:
        e[kind == MISS] = tab["t_bg"]
        e[kind == EMITTED] = tab["t_emit"][mat[kind == EMITTED]]
    lit = ((rec[:, 3] & ROW_LIGHT) != 0)
    lit_free = lit & ~occ_light
    if lit_free.any():
        ml = tab["mat"][rec[lit_free, 2]].astype(np.int64)
        l[lit_free] = rec[lit_free, 0].view(F)[:, None] * tab["t_light"][mat[lit_free], ml]
    sky = ((rec[:, 3] & ROW_SKY) != 0)
    sky_free = sky & ~occ_sky
    k[sky_free] = tab["t_sky"][mat[sky_free]]
    counts = [(kind == MISS).sum(), (kind == EMITTED).sum(), (kind == SPECULAR).sum(), (kind == SHADED).sum(), lit.sum(), lit_free.sum(),
              sky.sum(), sky_free.sum()]
    return e, l, k, np.array(counts, np.int64)


def run(desc, cam, w, h, ox, oy, intersect, occluded, samples=16, seed=0, first_sample=0, parts=("emitted", "lights", "sky"), tab=None,
        keep=False):
    """the pass restated: dict(sum, m2 (h, w, 3) float32, stats, tab) and, with keep, `rounds`: per sample the rows, records and answers"""
    tab = tab or tables(desc)
    mask = sum(PARTS[p] for p in parts)
    key = seed_key(seed)
    gx, gy, pid = pixels(cam, w, h, ox, oy)
    n = w * h
    total, m2 = np.zeros((n, 3), F), np.zeros((n, 3), F)
    counts = np.zeros(8, np.int64)
    kept = []
    lights_on = bool(mask & PARTS["lights"]) and len(tab["thresholds"]) > 1
    sky_on = bool(mask & PARTS["sky"]) and tab["bg_nonzero"]
    for s in range(samples):
        si = np.uint32(first_sample + s)
        cam_rows = camera_rows(cam, gx, gy, pid, si, key)
        hits = np.asarray(intersect(cam_rows), F)
        light_rows, sky_rows, rec = shade_rows(desc, tab, mask, cam_rows, hits, pid, si, key)
        occ_l = np.asarray(occluded(light_rows), bool) if lights_on else np.zeros(n, bool)
        occ_s = np.asarray(occluded(sky_rows), bool) if sky_on else np.zeros(n, bool)
        e, l, k, c = contributions(tab, mask, rec, occ_l, occ_s)
        total = ((total + e) + l) + k
        t = (e + l) + k
        m2 = m2 + t * t
        counts += c
        if keep:
            kept.append(dict(cam_rows=cam_rows, hit_rows=hits, light_rows=light_rows if lights_on else np.zeros((n, 8), F),
                             sky_rows=sky_rows if sky_on else np.zeros((n, 8), F), records=rec, occ_light=occ_l, occ_sky=occ_s))
    stats = dict(zip(COUNTERS, (int(v) for v in counts)))
    stats["lights"] = len(tab["thresholds"]) - 1
    return dict(sum=total.reshape(h, w, 3), m2=m2.reshape(h, w, 3), stats=stats, tab=tab, rounds=kept)


# ---- the float64 truth as the queries ---------------------------------------------------------------------------------------------
def truth_queries(desc):
    """(intersect, occluded) answered by ground_truth's float64 brute force on the described scene's triangles"""
    V = G.f64(desc["V"])
    mi = np.asarray(desc["mat_index"], np.int64)

    def intersect(rows):
        t, tri, _, _ = G.closest_hit(V, G.f64(rows[:, 0:3]), G.f64(rows[:, 4:7]))
        hit = tri >= 0
        out = np.zeros((len(rows), 4), F)
        out[:, 0] = np.where(hit, t, 0.0); out[:, 1] = tri; out[:, 3] = np.where(hit, mi[np.maximum(tri, 0)], 0)
        return out

    def occluded(rows):
        live = rows[:, 3] <= rows[:, 7]
        out = np.zeros(len(rows), bool)
        if live.any():
            r = rows[live]
            _, all_t = Q.scan(V, r)
            out[live] = (np.isfinite(all_t) & (all_t >= r[:, 3][None, :].astype(np.float64)) & (all_t <= r[:, 7][None, :].astype(np.float64))).any(0)
        return out

    return intersect, occluded
