"""The variance measured across frames (include/srt_c_api.h, "Variance measured across frames": srt_denoise_features_temporal_vg and the
calls around it) restated in numpy float32, operation by operation: the temporal stage with the luminance moments riding on its taps, the
choice between the moments' variance and the spatial estimate, and the chain that joins them with the variance-guided levels.  The stage
is written out here on its own -- steps 5 to 7 with the moments next to the colour; steps 1 to 4, the projection, are
temporal_reference.project / surface_motion_reference.project_moving --, so that "the moments never touch the colour" is something
tests/test_temporal_vg_reference.py can check against temporal_reference.temporal instead of something this file assumes.
tests/test_temporal_vg_reference.py holds this file to exact arithmetic; tests/test_temporal_vg.py holds the device to this file."""
import numpy as np

import denoise_vg_reference as V
import temporal_reference as T

F = np.float32
TV_DEFAULTS = dict(min_len=4)


def _div(a, b):
    return (a / b).astype(F)


def temporal_moments(c, guides, cam, hist=None, ox=0, oy=0, prev_point=None, alpha_min=0.1, max_len=32.0, sigma_normal=0.5, sigma_albedo=0.25,
                     sigma_depth=0.1):
    """the moments stage on the picture c (h, w, 3) with guides (h, w, 8) under the camera cam.  hist: None or dict(colour (h, w, 4), guides
    (h, w, 8), cam, moments (h, w, 4) or None -- a colour history that a moment-less call wrote last).  prev_point (h, w, 4): the moving
    stage.  dict(colour, guides, cam, moments -- the new history --, xyz, len, motion, stats, blended / fresh / nonfinite, tap_taken and
    tap_weight (4, h, w))."""
    c, g = np.asarray(c, F), np.asarray(guides, F)
    h, w = c.shape[:2]
    assert c.shape == (h, w, 3) and g.shape == (h, w, 8), (c.shape, g.shape)
    ys, xs = np.mgrid[0:h, 0:w]
    am, ml_cap = F(alpha_min), F(max_len)
    with np.errstate(all="ignore"):
        finite = (((c - c).astype(F) == F(0))).all(axis=-1)
    motion = np.full((h, w, 2), np.nan, F)
    sw, sl, sc = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
    s1, s2, sm = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    tap_inside, tap_taken, tap_weight = np.zeros((4, h, w), bool), np.zeros((4, h, w), bool), np.zeros((4, h, w), F)
    ok = np.zeros((h, w), bool)
    Hm = None
    with np.errstate(all="ignore"):
        if hist is not None:
            sn, sa, sz = F(sigma_normal), F(sigma_albedo), F(sigma_depth)
            kn, ka, kz = F(sn * sn), F(sa * sa), F(sz * sz)
            Hc, Hg = np.asarray(hist["colour"], F), np.asarray(hist["guides"], F)
            assert Hc.shape == (h, w, 4) and Hg.shape == (h, w, 8)
            if hist.get("moments") is not None:
                Hm = np.asarray(hist["moments"], F)
                assert Hm.shape == (h, w, 4)
            if prev_point is None:
                pr = T.project(g, cam, hist["cam"], ox, oy)
            else:
                import surface_motion_reference as M
                pr = M.project_moving(g, cam, hist["cam"], prev_point, ox, oy)
            hit, zexp, ok, u, ww = pr["hit"], pr["zexp"], pr["ok"], pr["u"], pr["w"]
            motion[..., 0] = np.where(ok, (u - xs.astype(F)).astype(F), F(np.nan))
            motion[..., 1] = np.where(ok, (ww - ys.astype(F)).astype(F), F(np.nan))
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
                hcf = ((hc[..., :3] - hc[..., :3]).astype(F) == F(0)).all(axis=-1)
                acc = (hc[..., 3] > F(0)) & hcf & ((hg[..., 7] >= F(0.5)) == hit)
                dn3 = (g[..., 0:3] - hg[..., 0:3]).astype(F)
                dn3 = (dn3 * dn3).astype(F)
                dn = ((dn3[..., 0] + dn3[..., 1]).astype(F) + dn3[..., 2]).astype(F)
                da3 = (g[..., 4:7] - hg[..., 4:7]).astype(F)
                da3 = (da3 * da3).astype(F)
                da = ((da3[..., 0] + da3[..., 1]).astype(F) + da3[..., 2]).astype(F)
                zq = hg[..., 3]
                m = np.where(zexp > zq, zexp, zq).astype(F)
                r = np.where(m > F(0), _div((zexp - zq).astype(F), m), F(0)).astype(F)
                geo = (dn <= kn) & (da <= ka) & ((r * r).astype(F) <= kz)
                take = inside & acc & (geo | ~hit) & (wt > F(0))
                tap_taken[tap], tap_weight[tap] = take, wt
                sw = np.where(take, (sw + wt).astype(F), sw).astype(F)
                sc = np.where(take[..., None], (sc + (wt[..., None] * hc[..., :3]).astype(F)).astype(F), sc).astype(F)
                sl = np.where(take, (sl + (wt * hc[..., 3]).astype(F)).astype(F), sl).astype(F)
                if Hm is not None:      # the moments ride on the taps the colour takes, with the colour's weights
                    hm = Hm[qy, qx]
                    s1 = np.where(take, (s1 + (wt * hm[..., 0]).astype(F)).astype(F), s1).astype(F)
                    s2 = np.where(take, (s2 + (wt * hm[..., 1]).astype(F)).astype(F), s2).astype(F)
                    sm = np.where(take, (sm + (wt * hm[..., 2]).astype(F)).astype(F), sm).astype(F)
        has = sw > F(0)
        nonfinite, fresh, blended = ~finite, finite & ~has, finite & has
        # the colour: step 6
        hh, lh = _div(sc, sw[..., None]), _div(sl, sw)
        ln = (lh + F(1)).astype(F)
        ln = np.where(ln < ml_cap, ln, ml_cap).astype(F)
        al = _div(F(1), ln)
        al = np.where(al > am, al, am).astype(F)
        mix = (hh + (al[..., None] * (c - hh).astype(F)).astype(F)).astype(F)
        o = np.where((blended & ~(al >= F(1)))[..., None], mix, c).astype(F)
        length = np.where(nonfinite, F(0), np.where(blended, ln, F(1))).astype(F)
        # the moments: step 6
        Y = c[..., 1]
        Q = (Y * Y).astype(F)
        moments = np.zeros((h, w, 4), F)
        moments[..., 0], moments[..., 1], moments[..., 2] = Y, Q, F(1)      # fresh, or blended with no moments history
        if Hm is not None:
            g1, g2, lm = _div(s1, sw), _div(s2, sw), _div(sm, sw)
            ml = (lm + F(1)).astype(F)
            ml = np.where(ml < ml_cap, ml, ml_cap).astype(F)
            bw = _div(F(1), ml)
            bw = np.where(bw > am, bw, am).astype(F)
            keep = bw >= F(1)
            m1 = np.where(keep, Y, (g1 + (bw * (Y - g1).astype(F)).astype(F)).astype(F)).astype(F)
            m2 = np.where(keep, Q, (g2 + (bw * (Q - g2).astype(F)).astype(F)).astype(F)).astype(F)
            moments[..., 0] = np.where(blended, m1, moments[..., 0])
            moments[..., 1] = np.where(blended, m2, moments[..., 1])
            moments[..., 2] = np.where(blended, ml, moments[..., 2])
        moments[nonfinite] = F(0)
    offscreen = np.zeros((h, w), bool)
    if hist is not None:
        offscreen = fresh & (~ok | ~tap_inside.any(axis=0))
    rejected = fresh & ~offscreen if hist is not None else np.zeros((h, w), bool)
    stats = dict(blended=int(blended.sum()), fresh=int(fresh.sum()), offscreen=int(offscreen.sum()), rejected=int(rejected.sum()),
                 nonfinite=int(nonfinite.sum()))
    colour = np.concatenate([o, length[..., None]], axis=-1).astype(F)
    return dict(colour=colour, guides=g.copy(), cam=cam, moments=moments, xyz=o, len=length, motion=motion, stats=stats, blended=blended,
                fresh=fresh, nonfinite=nonfinite, tap_taken=tap_taken, tap_weight=tap_weight)


def without_moments(stage):
    """the history a moment-less temporal call leaves: the colour history advanced, the moments marked absent"""
    return dict(colour=stage["colour"], guides=stage["guides"], cam=stage["cam"], moments=None)


def choose_variance(moments, length, spatial_var, min_len=4):
    """the choice: (v (h, w), n_temporal).  d = m2 - m1 * m1; d = d > 0 ? d : 0; vt = d / len;
    use = mlen >= (float)min_len && len > 0 && (vt - vt) == 0; v = use ? vt : vs"""
    Hm, ln, vs = np.asarray(moments, F), np.asarray(length, F), np.asarray(spatial_var, F)
    with np.errstate(all="ignore"):
        d = (Hm[..., 1] - (Hm[..., 0] * Hm[..., 0]).astype(F)).astype(F)
        d = np.where(d > F(0), d, F(0)).astype(F)
        vt = _div(d, ln)
        use = (Hm[..., 2] >= F(min_len)) & (ln > F(0)) & ((vt - vt).astype(F) == F(0))
        return np.where(use, vt, vs).astype(F), int(use.sum())


def chain(c, guides, cam, hist=None, ox=0, oy=0, prev_point=None, temporal=None, min_len=4, levels=5, sigma_variance=2.0, sigma_normal=0.5,
          sigma_albedo=0.25, sigma_depth=0.1, variance_floor=1e-8):
    """the chained call behind its prepass (and its firefly filter): c is the stage's input.  The moments stage, the spatial estimator on
    its output o, the choice, the variance-guided levels from (o, v).  dict(xyz (h, w, 3), var (h, w, 2) = (the variance chosen, the
    variance behind the last level), stage -- temporal_moments' dict, the new history --, n_temporal, spatial (h, w))."""
    stage = temporal_moments(c, guides, cam, hist, ox, oy, prev_point, **dict(T.DEFAULTS, **(temporal or {})))
    g = stage["guides"]
    N, z, A = g[..., 0:3], g[..., 3], g[..., 4:7]
    consts = V.vg_constants(sigma_variance, sigma_normal, sigma_albedo, sigma_depth, variance_floor)
    vs = V.estimate_variance(stage["xyz"], N, A, z, *consts[:3])
    v0, n_temporal = choose_variance(stage["moments"], stage["len"], vs, min_len)
    x, v = stage["xyz"], v0
    for i in range(levels):
        x, v = V.filter_level_vg(x, v, N, A, z, i, consts)
    return dict(xyz=x, var=np.stack([v0, v], axis=-1), stage=stage, n_temporal=n_temporal, spatial=vs)
