"""tests/temporal_reference.py, the numpy restatement of the temporal reprojection, held to independent arithmetic: float64 projection,
exact power-of-two geometry, fractions with one rounding per operation, and the properties srt_c_api.h lists.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import temporal_reference as T
from accum_helpers import named_workload
from helpers import bits

F = np.float32
INF = float("inf")
OFF = dict(sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)

# Reprojection error of the restatement's fp32 (u, w) against a float64 pinhole projection of the same fp32 point, in pixels: the largest
# over the six cases below was measured at 1.25e-5 (prism, static; test_reprojection_against_float64 prints every case).  Asserted at 4x;
# the bound must stay below 1/64 pixel whatever is measured: beyond it the bilinear weights are wrong in the second digit.
REPROJECTION_MEASURED = 1.25e-5
REPROJECTION_BOUND = 4 * REPROJECTION_MEASURED
assert REPROJECTION_BOUND < 1.0 / 64


def _rounded(x):
    """a Fraction rounded to the nearest float32 (ties to even, normal range), as a Fraction"""
    if x == 0:
        return Fraction(0)
    mag, e = abs(x), 0
    while mag >= Fraction(2) ** (e + 1):
        e += 1
    while mag < Fraction(2) ** e:
        e -= 1
    assert -126 <= e <= 127
    quantum = Fraction(2) ** (e - 23)
    n = mag / quantum
    lo = n.numerator // n.denominator
    rest = n - lo
    lo += 1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2) else 0
    return (lo * quantum) * (1 if x > 0 else -1)


def _f64_project(P, prev_cam):
    """image coordinates (i, j) of the points P (.., 3) under prev_cam, float64: p00 + i du + j dv = c + t (P - c) solved as a 3 x 3 system"""
    du, dv, p00, c = (np.asarray(v, np.float64) for v in T.camera_vectors(prev_cam))
    P = np.asarray(P, np.float64)
    out = np.zeros(P.shape[:-1] + (2,))
    for idx in np.ndindex(P.shape[:-1]):
        A = np.stack([du, dv, -(P[idx] - c)], axis=1)
        i, j, t = np.linalg.solve(A, c - p00)
        out[idx] = (i, j)
    return out


def _scene_guides(h, w, z=5.0, cov=1.0):
    g = np.zeros((h, w, 8), F)
    g[..., 2], g[..., 3], g[..., 4:7], g[..., 7] = 1.0, z, 0.5, cov
    return g


@pytest.mark.parametrize("name", ["cornell", "prism", "dielectric"])
@pytest.mark.parametrize("moved", [False, True], ids=["static", "moved"])
def test_reprojection_against_float64(srt, name, moved):
    _, cam0, _, _, _, _ = named_workload(srt, name)
    W, H = 64, 48
    du, dv, p00, c = T.camera_vectors(cam0)
    # the named camera at 64 x 48: the same vectors, whatever size the workload renders at
    prev = T.plain_camera(srt.CameraData, W, H, du, dv, p00, c)
    scale = float(np.linalg.norm(p00 - c))
    depth = {"cornell": 4.0, "prism": 4.0, "dielectric": 6.0}[name] * scale
    cur = T.move_camera(prev, (0.02 * depth, -0.01 * depth, 0.015 * depth), yaw_deg=1.5, pitch_deg=-0.75) if moved else prev
    rng = np.random.default_rng(5)
    g = _scene_guides(H, W)
    g[..., 3] = (depth * rng.uniform(0.5, 1.5, (H, W))).astype(F)
    pr = T.project(g, cur, prev)
    assert pr["ok"].all() and pr["hit"].all()
    want = _f64_project(pr["P"], prev)
    err = max(np.abs(pr["u"].astype(np.float64) - want[..., 0]).max(), np.abs(pr["w"].astype(np.float64) - want[..., 1]).max())
    print("%s %s: reprojection error %.3g px (bound %.3g)" % (name, "moved" if moved else "static", err, REPROJECTION_BOUND))
    assert err <= REPROJECTION_BOUND
    if not moved:      # a static camera sends every pixel to itself -- up to the rounding of the fp32 point P as well, so to the 1/64 pixel condition
        ys, xs = np.mgrid[0:H, 0:W]
        back = max(np.abs(pr["u"] - xs).max(), np.abs(pr["w"] - ys).max())
        print("%s static: a pixel returns to itself within %.3g px" % (name, back))
        assert back < 1.0 / 64


def test_exact_shift(srt):
    prev, cur, g = T.shift_case(srt.CameraData)
    H, W = g.shape[:2]
    rng = np.random.default_rng(2)
    c = rng.uniform(0, 2, (H, W, 3)).astype(F)
    hc = np.concatenate([rng.uniform(0, 2, (H, W, 3)), rng.integers(1, 6, (H, W, 1))], axis=-1).astype(F)
    pr = T.project(g, cur, prev)
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.unique(pr["u"] - xs.astype(F)).tolist() == [3.0] and np.unique(pr["w"] - ys.astype(F)).tolist() == [0.0]
    out = T.temporal(c, g, cur, dict(colour=hc, guides=g, cam=prev), **T.DEFAULTS)
    assert np.array_equal(out["motion"][..., 0], np.full((H, W), F(3))) and not out["motion"][..., 1].any()
    inner = np.zeros((H, W), bool)
    inner[:, :W - 3] = True
    assert out["stats"] == dict(blended=H * (W - 3), fresh=3 * H, offscreen=3 * H, rejected=0, nonfinite=0)
    assert np.array_equal(out["offscreen"], ~inner) and np.array_equal(out["tap_taken"].sum(axis=0)[inner], np.ones(H * (W - 3)))
    h = hc[:, 3:, :3]
    ln = np.minimum(hc[:, 3:, 3] + F(1), F(32))
    a = np.maximum(F(1) / ln, F(0.1)).astype(F)
    want = (h + (a[..., None] * (c[:, :W - 3] - h).astype(F)).astype(F)).astype(F)
    assert np.array_equal(bits(out["xyz"][:, :W - 3]), bits(want)) and np.array_equal(bits(out["len"][:, :W - 3]), bits(ln))
    assert np.array_equal(bits(out["xyz"][:, W - 3:]), bits(c[:, W - 3:])) and (out["len"][:, W - 3:] == 1).all()


def test_blend_and_classes_against_fractions(srt):
    """one pixel, one tap of weight 1 (a static power-of-two camera): the len recursion, the alpha_min floor, the a >= 1 select"""
    prev, _, g = T.shift_case(srt.CameraData)
    g = g[:1, :1]
    rng = np.random.default_rng(9)
    for trial in range(60):
        max_len = float(rng.choice([1.0, 2.0, 5.0, 7.5, 32.0]))
        alpha_min = float(F(rng.choice([1.0, 0.5, 0.3, 0.1, 1e-3])))
        c = rng.uniform(0, 4, (1, 1, 3)).astype(F)
        hcol = rng.uniform(0, 4, 3).astype(F)
        ln = F(rng.choice([0.5, 1.0, 2.0, 3.0, 6.5, 31.0, 40.0]))
        hist = dict(colour=np.concatenate([hcol, [ln]]).astype(F).reshape(1, 1, 4), guides=g, cam=prev)
        out = T.temporal(c, g, prev, hist, alpha_min=alpha_min, max_len=max_len, **OFF)
        assert out["stats"]["blended"] == 1
        l1 = _rounded(Fraction(float(ln)) + 1)
        l1 = l1 if l1 < Fraction(max_len) else Fraction(max_len)
        a = _rounded(1 / l1)
        a = a if a > Fraction(alpha_min) else Fraction(alpha_min)
        assert Fraction(float(out["len"][0, 0])) == l1
        for k in range(3):
            cp, h = Fraction(float(c[0, 0, k])), Fraction(float(hcol[k]))
            want = cp if a >= 1 else _rounded(h + _rounded(a * _rounded(cp - h)))
            assert Fraction(float(out["xyz"][0, 0, k])) == want, (trial, k)
        if a >= 1:
            assert np.array_equal(bits(out["xyz"]), bits(c))
    # the recursion: a static picture fed its own output counts 1, 2, 3 .. max_len and stays there
    c = np.full((1, 1, 3), F(0.75))
    hist, lens = None, []
    for _ in range(7):
        hist = T.temporal(c, g, prev, hist, alpha_min=0.01, max_len=5.0, **OFF)
        lens.append(float(hist["len"][0, 0]))
    assert lens == [1.0, 2.0, 3.0, 4.0, 5.0, 5.0, 5.0]


def _moving_pair(srt, W=24, H=16):
    prev = srt.camera_init(W, H, 40.0, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0))
    cur = srt.camera_init(W, H, 40.0, (0.35, 0.1, 6.0), (0.1, 0.0, 0.0))
    return prev, cur


def test_the_four_properties(srt):
    W, H = 24, 16
    prev, cur = _moving_pair(srt, W, H)
    c, g, hc, hg = T.random_case(W, H, 3)
    hist = dict(colour=hc, guides=hg, cam=prev)
    # 1. the first call returns the input bit for bit, len = 1 (0 at a non-finite pixel)
    first = T.temporal(c, g, cur, None, **T.DEFAULTS)
    bad = ~T.finite3(c)
    assert bad.sum() >= 1 and np.array_equal(bits(first["xyz"]), bits(c)) and np.array_equal(first["len"], np.where(bad, F(0), F(1)))
    assert first["stats"] == dict(blended=0, fresh=W * H - int(bad.sum()), offscreen=0, rejected=0, nonfinite=int(bad.sum())) and np.isnan(first["motion"]).all()
    # 2. alpha_min = 1 returns the input bit for bit, whatever the history
    for sig in (OFF, {}):
        out = T.temporal(c, g, cur, hist, **dict(T.DEFAULTS, alpha_min=1.0, **sig))
        assert np.array_equal(bits(out["xyz"]), bits(c))
    assert out["stats"]["blended"] > 0
    # 3. a constant picture under a camera move stays that constant exactly where it blends
    k = np.full((H, W, 3), F(0.5))
    hk = np.concatenate([k, np.full((H, W, 1), F(3))], axis=-1)
    hk[2, 3, :3] = np.inf          # (the history holds a non-finite value: it is not accepted)
    gk = _scene_guides(H, W)
    out = T.temporal(k, gk, cur, dict(colour=hk, guides=gk, cam=prev), **dict(T.DEFAULTS, **OFF))
    assert out["stats"]["blended"] > W * H // 2 and np.array_equal(bits(out["xyz"]), bits(k))
    # 4. a non-finite value never enters the history and never leaves it
    out = T.temporal(c, g, cur, hist, **dict(T.DEFAULTS, **OFF))
    assert np.array_equal(bits(out["xyz"][bad]), bits(c[bad])) and (out["len"][bad] == 0).all() and out["stats"]["nonfinite"] == bad.sum()
    assert np.isfinite(out["xyz"][~bad]).all() and (out["len"][~bad] >= 1).all()
    nxt = T.temporal(np.where(bad[..., None], F(1), c), g, cur, out, **dict(T.DEFAULTS, **OFF))      # the next frame over that history
    assert np.isfinite(nxt["xyz"]).all()


def test_disocclusion(srt):
    """two fronto-parallel planes, the near one over the left half, and a strafe: pixels of the far plane that the near plane covered
    a frame ago find a history that is too near -- rejected; with sigma_depth = +inf they blend"""
    W, H = 32, 12
    prev = srt.camera_init(W, H, 40.0, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0))
    cur = srt.camera_init(W, H, 40.0, (0.6, 0.0, 6.0), (0.6, 0.0, 0.0))

    def guides(cam):
        du, dv, p00, c = T.camera_vectors(cam)
        ys, xs = np.mgrid[0:H, 0:W]
        d = (p00 + xs[..., None] * du + ys[..., None] * dv - c).astype(np.float64)
        g = _scene_guides(H, W)
        tn, tf = (3.0 - c[2]) / d[..., 2], (0.0 - c[2]) / d[..., 2]      # the planes z = 3 (x < 0 only) and z = 0
        near = (c[0] + tn * d[..., 0]) < 0.0
        g[..., 3] = (np.where(near, tn, tf) * np.linalg.norm(d, axis=-1)).astype(F)
        return g, near

    g0, _ = guides(prev)
    g1, near1 = guides(cur)
    c = np.full((H, W, 3), F(1))
    hc = np.concatenate([np.full((H, W, 3), F(0.25)), np.full((H, W, 1), F(4))], axis=-1)
    hist = dict(colour=hc, guides=g0, cam=prev)
    strict = T.temporal(c, g1, cur, hist, **T.DEFAULTS)
    loose = T.temporal(c, g1, cur, hist, **dict(T.DEFAULTS, sigma_depth=INF))
    assert strict["stats"]["rejected"] >= H and loose["stats"]["rejected"] == 0
    assert (strict["rejected"] & ~near1).sum() >= H          # they lie on the far plane, right of the near plane's edge
    assert loose["blended"][strict["rejected"]].all() and np.array_equal(strict["offscreen"], loose["offscreen"])
    assert strict["stats"]["blended"] > W * H // 2


def test_sky_pixels_reproject_by_direction(srt):
    W, H = 24, 16
    prev = srt.camera_init(W, H, 40.0, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0))
    g = _scene_guides(H, W, z=0.0, cov=0.0)
    ys, xs = np.mgrid[0:H, 0:W]
    moved = srt.camera_init(W, H, 40.0, (1.5, -0.5, 4.0), (1.5, -0.5, -2.0))      # a pure translation
    pr = T.project(g, moved, prev)
    assert not pr["hit"].any() and pr["ok"].all()
    assert np.abs(pr["u"] - xs).max() <= REPROJECTION_BOUND and np.abs(pr["w"] - ys).max() <= REPROJECTION_BOUND
    turned = srt.camera_init(W, H, 40.0, (0.0, 0.0, 6.0), (0.5, 0.0, 0.0))      # a pure rotation
    pr = T.project(g, turned, prev)
    assert pr["ok"].all() and (pr["u"] - xs).min() > 1.0
    # sky takes sky only: a history of hits is rejected
    c = np.ones((H, W, 3), F)
    hc = np.concatenate([c, np.ones((H, W, 1), F)], axis=-1)
    out = T.temporal(c, g, turned, dict(colour=hc, guides=_scene_guides(H, W), cam=prev), **dict(T.DEFAULTS, **OFF))
    assert out["stats"]["blended"] == 0 and out["stats"]["rejected"] > 0 and out["stats"]["offscreen"] > 0
    out = T.temporal(c, g, turned, dict(colour=hc, guides=g, cam=prev), **T.DEFAULTS)
    assert out["stats"]["blended"] > 0 and out["stats"]["rejected"] == 0


def test_borders(srt):
    """u in [-1, 0) takes only the taps at x0 + 1, u >= w - 1 only those at x0; huge and NaN coordinates are offscreen with no tap read"""
    prev, _, g = T.shift_case(srt.CameraData)
    H, W = g.shape[:2]
    c = np.ones((H, W, 3), F)
    hc = np.concatenate([np.full((H, W, 3), F(0.5)), np.ones((H, W, 1), F)], axis=-1)
    hist = dict(colour=hc, guides=g, cam=prev)
    du, dv, p00, ce = T.camera_vectors(prev)
    # shifted by -2.5 pixels: columns 0 and 1 leave on the left (u = -2.5, -1.5), column 2 has u = -0.5
    left = T.plain_camera(srt.CameraData, W, H, du, dv, p00 - np.array([10.0 / 64, 0, 0], F), ce - np.array([10.0 / 64, 0, 0], F))
    out = T.temporal(c, g, left, hist, **dict(T.DEFAULTS, **OFF))
    assert np.unique(out["motion"][..., 0]).tolist() == [-2.5]
    ins = out["tap_inside"]
    assert not ins[:, :, :2].any() and out["offscreen"][:, :2].all()
    assert ins[1, 1:-1, 2].all() and ins[3, 1:-2, 2].all() and not ins[0, :, 2].any() and not ins[2, :, 2].any() and out["blended"][:, 2].all()
    # shifted by +2.5: column w - 3 has u = w - 0.5: only the taps at x0
    right = T.plain_camera(srt.CameraData, W, H, du, dv, p00 + np.array([10.0 / 64, 0, 0], F), ce + np.array([10.0 / 64, 0, 0], F))
    out = T.temporal(c, g, right, hist, **dict(T.DEFAULTS, **OFF))
    ins = out["tap_inside"]
    assert ins[0, :, W - 3].all() and not ins[1, :, W - 3].any() and not ins[3, :, W - 3].any() and out["blended"][:, W - 3].all()
    assert out["offscreen"][:, W - 2:].all() and not ins[:, :, W - 2:].any()
    # NaN coordinates: a pixel whose distance is NaN or infinite
    gz = g.copy()
    gz[1, 1, 3], gz[2, 2, 3] = np.nan, np.inf
    out = T.temporal(c, gz, right, hist, **dict(T.DEFAULTS, **OFF))
    for y, x in ((1, 1), (2, 2)):
        assert out["offscreen"][y, x] and not out["tap_inside"][:, y, x].any() and out["len"][y, x] == 1
    # huge coordinates: a previous camera whose pixels are 2^-36 wide sends pixel (i, j) to (2^30 i, 2^30 j), beyond every int
    tiny = T.plain_camera(srt.CameraData, W, H, (2.0 ** -36, 0, 0), (0, -2.0 ** -36, 0), p00, ce)
    out = T.temporal(c, g, prev, dict(colour=hc, guides=g, cam=tiny), **dict(T.DEFAULTS, **OFF))
    assert out["motion"][1, 1, 0] == F(2.0 ** 30 - 1) and out["offscreen"][1:, 1:].all() and not out["tap_inside"][:, 1:, 1:].any()
    assert out["blended"][0, 0] and out["stats"]["rejected"] == 0
    # behind the previous camera: step 4 fails, the motion vector is NaN
    back = T.move_camera(prev, yaw_deg=180.0)
    out = T.temporal(c, g, back, hist, **dict(T.DEFAULTS, **OFF))
    assert out["stats"]["offscreen"] == W * H and np.isnan(out["motion"]).all() and not out["tap_inside"].any()
