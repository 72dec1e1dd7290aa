"""The variance measured across frames on the device (srt_denoise_features_temporal_vg / srt_present_temporal_vg / srt_temporal_moments_kat /
srt_temporal_variance_kat / srt_read_temporal_moments): the device equals tests/temporal_vg_reference.py in every bit and every counter --
the moments stage and the choice on explicit inputs, the chained call on real frames under a moving camera, through the presented bytes
and across a refit --, the colour history is the moment-less stage's, the two families of calls alternate as srt_c_api.h says, and no
call changes the accumulation or, when refused, either history."""
import ctypes as C

import numpy as np
import pytest

import despeckle_reference as R
import surface_motion_reference as M
import temporal_reference as T
import temporal_vg_reference as TV
from accum_helpers import ERR_INVALID, ERR_UNSUPPORTED, assert_same_image, expect_error, fresh_context, gpu_lib, named_workload, read_frame
from features_reference import stack_features
from helpers import bits
from path_ends_reference import assert_same_floats
from test_temporal import SIZES, _camera_pairs, _device_inputs, _frame, _srgb_of

pytestmark = pytest.mark.gpu

F = np.float32
FP = C.POINTER(C.c_float)
INF = float("inf")
COUNTERS = ("blended", "fresh", "offscreen", "rejected", "nonfinite")
DS = dict(radius=2, rank_ppm=500000, gain=4.0, floor=0.0)
TCFG = dict(T.DEFAULTS, sigma_depth=0.2)
VG = dict(levels=2, sigma_variance=2.0, variance_floor=1e-6)


def _random_moments(w, h, seed):
    rng = np.random.default_rng(31 * w + h + seed)
    return np.concatenate([rng.uniform(0, 2, (h, w, 1)), rng.uniform(0, 4, (h, w, 1)), rng.integers(1, 40, (h, w, 1)), np.zeros((h, w, 1))], axis=-1).astype(F)


def _assert_stage(got, want, what):
    for key in ("colour", "guides", "motion", "moments"):
        assert_same_floats(got[key], want[key], what + " " + key)
    stats = {k: got["stats"][k] for k in COUNTERS}
    assert stats == want["stats"], (what, stats, want["stats"])


def _assert_choice(gpu, stage, seed, what):
    """the choice kernel on the stage's own moments and length against the restatement, at a threshold inside the lengths' range and one above"""
    h, w = stage["len"].shape
    vs = np.random.default_rng(seed).uniform(0, 1, (h, w)).astype(F)
    used = 0
    for min_len in (2, 7, 2 ** 24):
        want, n = TV.choose_variance(stage["moments"], stage["len"], vs, min_len)
        got, got_n = gpu.temporal_variance_kat(stage["moments"], stage["len"], vs, min_len)
        assert_same_floats(got, want, "%s choice at min_len %d" % (what, min_len))
        assert got_n == n, (what, min_len, got_n, n)
        used += n
    return used


@pytest.mark.parametrize("w,h", SIZES)
def test_stage_and_choice_equal_the_restatement(srt, gpu, w, h):
    ox, oy = 5, 3
    prev, pairs = _camera_pairs(srt, w + ox + 2, h + oy + 1)
    c, g, hc, hg = T.random_case(w, h, 1)
    hm = _random_moments(w, h, 1)
    total, used = dict.fromkeys(COUNTERS, 0), 0
    for name, cur in pairs:
        for cfg in (dict(T.DEFAULTS), dict(T.DEFAULTS, alpha_min=0.3, max_len=6.5, sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)):
            for off in ((0, 0), (ox, oy)):
                plain = gpu.temporal_kat(cur, c, g, prev, hc, hg, off[0], off[1], **cfg)
                for moments in (hm, None):
                    what = "%d x %d %s at %r %r moments %r" % (w, h, name, off, cfg["max_len"], moments is not None)
                    want = TV.temporal_moments(c, g, cur, dict(colour=hc, guides=hg, cam=prev, moments=moments), off[0], off[1], **cfg)
                    got = gpu.temporal_moments_kat(cur, c, g, prev, hc, hg, moments, None, off[0], off[1], **cfg)
                    _assert_stage(got, want, what)
                    # the colour history is the moment-less stage's, bit for bit
                    for key in ("colour", "guides", "motion"):
                        assert np.array_equal(bits(got[key]), bits(plain[key])), (what, key)
                    assert got["stats"] == plain["stats"] and got["stats"]["history_frames"] == 2
                    if moments is None:
                        assert (got["moments"][..., 2] <= 1).all()
                for k in COUNTERS:
                    total[k] += want["stats"][k]
            used += _assert_choice(gpu, want, 7, what)
        # no history at all: every finite pixel is seeded
        want = TV.temporal_moments(c, g, cur, None, ox, oy, **T.DEFAULTS)
        got = gpu.temporal_moments_kat(cur, c, g, offx=ox, offy=oy)
        _assert_stage(got, want, "%d x %d %s without history" % (w, h, name))
        assert got["stats"]["history_frames"] == 1 and got["stats"]["blended"] == 0
    # the choice on the stage that carried moments (the loop's last one seeded them: mlen 1 everywhere)
    carried = TV.temporal_moments(c, g, pairs[1][1], dict(colour=hc, guides=hg, cam=prev, moments=hm), **T.DEFAULTS)
    used += _assert_choice(gpu, carried, 8, "%d x %d carried" % (w, h))
    print("%d x %d: %r, %d pixels took the temporal variance" % (w, h, total, used))
    if w * h >= 4:
        assert total["nonfinite"] > 0
    if w * h > 100:
        assert min(total.values()) > 0 and used > 0, (total, used)
    assert gpu.temporal_last_ms() > 0 and gpu.temporal_variance_last_ms() > 0


@pytest.mark.parametrize("w,h", SIZES)
def test_moving_stage_equals_the_restatement(srt, gpu, w, h):
    """prev_point with displaced points, untracked pixels (valid = 0, valid = 0.5) and a non-finite coordinate"""
    ox, oy = 5, 3
    prev, pairs = _camera_pairs(srt, w + ox + 2, h + oy + 1)
    c, g, hc, hg = T.random_case(w, h, 2)
    hm = _random_moments(w, h, 2)
    rng = np.random.default_rng(100 * w + h)
    for name, cur in pairs[:3]:
        for off in ((0, 0), (ox, oy)):
            pts = M.static_points(g, cur, off[0], off[1])
            pts[..., :3] += rng.normal(0, 0.02, (h, w, 3)).astype(F)
            pts[rng.random((h, w)) < 0.2, 3] = 0.0
            if w * h >= 4:
                pts[rng.integers(h), rng.integers(w), 3] = 0.5
                pts[rng.integers(h), rng.integers(w), 0] = np.nan
            what = "%d x %d moving %s at %r" % (w, h, name, off)
            want = TV.temporal_moments(c, g, cur, dict(colour=hc, guides=hg, cam=prev, moments=hm), off[0], off[1], pts, **T.DEFAULTS)
            got = gpu.temporal_moments_kat(cur, c, g, prev, hc, hg, hm, pts, off[0], off[1], **T.DEFAULTS)
            _assert_stage(got, want, what)
            plain = gpu.temporal_moving_kat(cur, c, g, pts, prev, hc, hg, off[0], off[1], **T.DEFAULTS)
            for key in ("colour", "guides", "motion"):
                assert np.array_equal(bits(got[key]), bits(plain[key])), (what, key)
            assert got["stats"] == plain["stats"]
    if w * h > 100:
        assert want["stats"]["blended"] > 0 and want["stats"]["offscreen"] > 0


# ---- the chained call on real frames ---------------------------------------------------------------------------------------------------
def _dolly(cam, w, h, frames):
    """`frames` cameras, each 1 % of the focus distance further along the view direction than the one before"""
    du, dv, p00, ce = (np.asarray(v, np.float64) for v in T.camera_vectors(cam))
    step = 0.01 * (p00 + 0.5 * w * du + 0.5 * h * dv - ce)
    return [T.move_camera(cam, tuple(k * step)) for k in range(frames)]


def _assert_chain(got, want, k, what, inside=None, shape=None):
    pick = (lambda a: a) if inside is None else (lambda a: a[inside].reshape(shape + a.shape[2:]))
    assert_same_floats(pick(got["xyz"]), want["xyz"], what + " xyz")
    assert_same_floats(pick(got["var"]), want["var"], what + " var")
    stats = dict(want["stage"]["stats"], history_frames=k + 1, history_dropped=False)
    assert got["stats"] == stats, (what, got["stats"], stats)
    assert got["n_temporal"] == want["n_temporal"], (what, got["n_temporal"], want["n_temporal"])


@pytest.mark.parametrize("name,adaptive,despeckle", [("cornell", False, None), ("random_spheres", True, DS)], ids=["cornell", "random-spheres-adaptive-despeckled"])
def test_chained_call_and_presented_bytes_on_real_frames(srt, gpu, orc, name, adaptive, despeckle):
    scene, _, _, _, depth, _ = named_workload(srt, name)
    W, H = 64, 48
    cam = scene.default_camera(W, H)
    cams = _dolly(cam, W, H, 4)
    fresh_context(gpu, scene, cam, W, H, depth)
    hist, used = None, []
    for k, cur in enumerate(cams):
        _frame(gpu, cur, W, H, (2, 2), adaptive=adaptive)
        c, g = _device_inputs(gpu, W, H, adaptive=adaptive)
        pre = c if despeckle is None else R.despeckle(c, **despeckle)["xyz"]
        want = TV.chain(pre, g, cur, hist, temporal=TCFG, min_len=2, **VG)
        got = gpu.denoise_temporal_vg(W, H, temporal=TCFG, despeckle=despeckle, min_len=2, **VG)
        what = "%s frame %d" % (name, k)
        _assert_chain(got, want, k, what)
        assert_same_floats(gpu.temporal_moments(), want["stage"]["moments"], what + " moments history")
        used.append(got["n_temporal"])
        hist = want["stage"]
    print(name, "pixels with the temporal variance per frame:", used, got["stats"])
    assert used[0] == 0 and W * H // 4 < used[-1] <= got["stats"]["blended"]
    assert (bits(got["var"][..., 0]) != bits(want["spatial"])).any()
    lin, q = _srgb_of(orc, want["xyz"])
    assert_same_floats(got["lin"], lin, "unquantised sRGB")
    assert_same_floats(got["fb"], q, "quantised sRGB")
    ms = gpu.denoise_last_ms()
    assert len(ms["levels"]) == 2 and all(t > 0 for t in ms["levels"]) and ms["prepass"] > 0 and ms["epilogue"] > 0
    assert gpu.temporal_last_ms() > 0 and gpu.temporal_variance_last_ms() > 0 and gpu.denoise_estimate_last_ms() > 0
    # the history is the stage's output, not the filtered picture; the presented bytes are present_kat's of the restated chain
    for gain, kw in ((None, dict(percentile_ppm=700000, white=8.0)), (1.7, dict(curve="linear"))):
        want = TV.chain(pre, g, cur, hist, temporal=TCFG, min_len=3, **VG)
        got = gpu.present_temporal_vg(W, H, gain, temporal=TCFG, despeckle=despeckle, min_len=3, **dict(VG, **kw))
        ref = gpu.present_kat(want["xyz"], gain, **kw)
        assert np.array_equal(got["rgba"], ref["rgba"]) and got["clip"] == ref["clip"] and got["meter"] == ref["meter"], gain
        assert {k2: got["temporal"][k2] for k2 in COUNTERS} == want["stage"]["stats"] and got["n_temporal"] == want["n_temporal"] > 0
        hist = want["stage"]
        assert_same_floats(gpu.temporal_moments(), hist["moments"], "moments history behind the presented picture")
    assert got["temporal"]["history_frames"] == 6 and got["rgba"][..., :3].max() > 0


def test_offset_chunk(srt, gpu):
    """a 30 x 21 chunk at (17, 9) of a 64 x 48 image of the Cornell scene: the moments history has the chunk's rectangle and its placement"""
    scene, _, _, _, depth, _ = named_workload(srt, "cornell")
    IW, IH, cw, ch, ox, oy = 64, 48, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    cams = _dolly(cam, IW, IH, 3)
    fresh_context(gpu, scene, cam, cw, ch, depth)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    hist = None
    for k, cur in enumerate(cams):
        _frame(gpu, cur, cw, ch, (4,), ox, oy)
        c, g = _device_inputs(gpu, cw, ch, IW, IH, ox, oy)
        want = TV.chain(c, g, cur, hist, ox, oy, temporal=TCFG, min_len=2, **VG)
        got = gpu.denoise_temporal_vg(IW, IH, temporal=TCFG, min_len=2, **VG)
        _assert_chain(got, want, k, "offset chunk frame %d" % k, inside, (ch, cw))
        moments = gpu.temporal_moments()
        for key, arr in (("xyz", got["xyz"]), ("var", got["var"]), ("moments", moments)):
            assert not bits(arr[~inside]).any(), key + ": written outside the chunk's rectangle"
        assert_same_floats(moments[inside].reshape(ch, cw, 4), want["stage"]["moments"], "offset chunk frame %d moments" % k)
        hist = want["stage"]
    assert got["n_temporal"] > cw * ch // 4


def test_across_a_refit_with_tracking(srt, gpu):
    from test_temporal_moving import _workload
    scene, cam, W, H, depth, v0, v1, _ = _workload(srt)
    gpu.track_motion(True)
    try:
        fresh_context(gpu, scene, cam, W, H, depth)
        hist = None
        for k, verts in enumerate((None, None, v1)):
            if verts is not None:
                gpu.refit(verts)
                assert gpu.tracking == (True, 1)
            _frame(gpu, cam, W, H, (4,))
            c, g = _device_inputs(gpu, W, H)
            pts = gpu.surface_motion(W, H)
            want = TV.chain(c, g, cam, hist, prev_point=pts["point"], temporal=TCFG, min_len=2, **VG)
            got = gpu.denoise_temporal_vg(W, H, temporal=TCFG, min_len=2, moving=True, **VG)
            _assert_chain(got, want, k, "tracked frame %d" % k)
            assert got["surface"] == pts["stats"] and gpu.tracking == (True, 0)
            assert_same_floats(gpu.temporal_moments(), want["stage"]["moments"], "tracked frame %d moments" % k)
            hist = want["stage"]
        assert pts["stats"]["moved"] > 0 and got["stats"]["blended"] > W * H // 2 and got["n_temporal"] > W * H // 2
        # the static chain after another refit is a first frame, as its moment-less sibling is: both histories are dropped
        gpu.refit(v0)
        _frame(gpu, cam, W, H, (4,))
        first = gpu.denoise_temporal_vg(W, H, temporal=TCFG, min_len=2, **VG)
        assert first["stats"]["history_frames"] == 1 and first["n_temporal"] == 0 and (gpu.temporal_moments()[..., 2] <= 1).all()
    finally:
        gpu.track_motion(False)


# ---- identities ------------------------------------------------------------------------------------------------------------------------
def test_infinite_floor_is_the_plain_chain_with_infinite_sigma_color(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    cams = _dolly(cam, W, H, 3)
    pictures = {}
    for chain in ("plain", "vg"):
        fresh_context(gpu, scene, cam, W, H, depth)      # (the same seed: the same frames in both runs; it drops the history)
        for k, cur in enumerate(cams):
            _frame(gpu, cur, W, H, (3,))
            if chain == "plain":
                out = gpu.denoise_temporal(W, H, temporal=TCFG, levels=3, sigma_color=INF)
            else:
                out = gpu.denoise_temporal_vg(W, H, temporal=TCFG, min_len=2, levels=3, variance_floor=INF)
            pictures[chain, k] = out
    for k in range(3):
        assert np.array_equal(bits(pictures["plain", k]["xyz"]), bits(pictures["vg", k]["xyz"])), k
        assert pictures["plain", k]["stats"] == pictures["vg", k]["stats"]
    assert pictures["vg", 2]["n_temporal"] > 0 and pictures["vg", 2]["stats"]["blended"] > 0


def test_alternating_with_the_moment_less_stage(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    cams = _dolly(cam, W, H, 4)
    fresh_context(gpu, scene, cam, W, H, depth)
    expect_error(srt, lambda: gpu.temporal_moments(W, H), ERR_INVALID, "no history at all")
    hist = None
    for k, cur in enumerate(cams):
        _frame(gpu, cur, W, H, (3,))
        c, g = _device_inputs(gpu, W, H)
        if k == 2:      # a moment-less call: Hc / Hg advance as always, Hm is marked absent
            want = T.temporal(c, g, cur, hist, **TCFG)
            got = gpu.temporal(W, H, **TCFG)
            assert_same_floats(got["xyz"], want["xyz"], "the moment-less call in between")
            assert got["stats"]["history_frames"] == 3 and got["stats"]["blended"] > 0
            expect_error(srt, lambda: gpu.temporal_moments(W, H), ERR_INVALID, "moments absent behind a moment-less call")
            hist = TV.without_moments(want)
            continue
        want = TV.chain(c, g, cur, hist, temporal=TCFG, min_len=2, **VG)
        got = gpu.denoise_temporal_vg(W, H, temporal=TCFG, min_len=2, **VG)
        _assert_chain(got, want, k, "alternating frame %d" % k)
        assert_same_floats(gpu.temporal_moments(W, H), want["stage"]["moments"], "alternating frame %d moments" % k)
        hist = want["stage"]
    # the colour history kept growing across the moment-less call; the moments started again
    # (len' is a bilinear mean of equal lengths plus one: 4 up to the rounding of four products and two sums, below 1e-5)
    assert abs(float(hist["len"].max()) - 4.0) < 1e-5 and hist["moments"][..., 2].max() == 1 and got["n_temporal"] == 0 and got["stats"]["blended"] > 0
    # srt_temporal_moments_kat touches no context history
    rc, rg, rhc, rhg = T.random_case(19, 7, 4)
    gpu.temporal_moments_kat(cams[2], rc, rg, cams[1], rhc, rhg, _random_moments(19, 7, 4))
    gpu.temporal_variance_kat(_random_moments(5, 4, 0), np.ones((4, 5), F), np.ones((4, 5), F))
    assert_same_floats(gpu.temporal_moments(W, H), hist["moments"], "the kat calls leave the context's moments alone")
    gpu.temporal_reset()
    expect_error(srt, lambda: gpu.temporal_moments(W, H), ERR_INVALID, "srt_temporal_reset drops the moments")


# ---- read-only and refusals ------------------------------------------------------------------------------------------------------------
def test_the_calls_change_nothing_of_the_accumulation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")

    def run(with_calls):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_adaptive_features(0.05, 0.0, 2)
        gpu.render_chunk_accum(W, H, 4)
        if with_calls:
            gpu.denoise_temporal_vg(W, H, levels=2)
            gpu.denoise_temporal_vg(W, H, despeckle=dict(radius=1), min_len=2, levels=1)
            gpu.present_temporal_vg(W, H, levels=1)
            gpu.present_temporal_vg(W, H, gain=1.0, min_len=2, levels=1)
            gpu.temporal_moments()
            rc, rg, rhc, rhg = T.random_case(9, 5, 2)
            gpu.temporal_moments_kat(cam, rc, rg, cam, rhc, rhg, _random_moments(9, 5, 2))
            gpu.temporal_variance_kat(_random_moments(9, 5, 3), np.ones((5, 9), F), np.ones((5, 9), F))
        gpu.render_chunk_accum(W, H, 4)
        frame, rows, stats = read_frame(gpu, W, H), stack_features(gpu.read_features(W, H)), gpu.accum_stats(W, H)
        assert gpu.accum_samples == 8
        gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
        return frame, rows, stats, read_frame(gpu, W, H)

    frame_a, rows_a, stats_a, after_a = run(True)
    frame_b, rows_b, stats_b, after_b = run(False)
    assert_same_image(frame_a, frame_b, "[4], the calls, [4] against [4, 4]")
    assert np.array_equal(bits(rows_a), bits(rows_b)) and rows_b[..., 7].max() > 0
    assert np.array_equal(stats_a["samples"], stats_b["samples"]) and len(np.unique(stats_b["samples"])) > 1
    assert_same_image(after_a, after_b, "RNG state: a plain launch after the passes")


def test_refusals_leave_both_histories_alone(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L, B = gpu_lib(), srt.binding
    t, vg, tv = srt.temporal_config(), srt.denoise_vg_config(levels=1), srt.temporal_vg_config(2)
    res, pres, n = B.TemporalResult(), B.PresentResult(), C.c_uint64()
    out = np.zeros((H, W, 3), F)
    op = out.ctypes.data_as(FP)
    rgba = np.zeros((H, W, 4), np.uint8)
    rp = rgba.ctypes.data_as(C.POINTER(C.c_uint8))

    def chain(t=t, vg=vg, tv=tv, o=op):
        return L.srt_denoise_features_temporal_vg(gpu._h, C.byref(t) if t else None, None, C.byref(vg) if vg else None, C.byref(tv) if tv else None, o, None, None,
                                                  None, C.byref(res), C.byref(n), None, W, H)

    def present(tv=tv, source="denoise_vg", **kw):
        p = srt.present_config(source, 1.0, **kw)
        return L.srt_present_temporal_vg(gpu._h, C.byref(p), C.byref(t), None, C.byref(tv) if tv else None, rp, 4 * W, W, H, C.byref(pres), C.byref(res), C.byref(n),
                                         None)

    def bad_tv(**kw):
        v = srt.temporal_vg_config(2)
        for k, val in kw.items():
            if k == "reserved":
                v.reserved[1] = val
            else:
                setattr(v, k, val)
        return v

    fresh = srt.Renderer(0)
    try:
        ms = C.c_float()
        assert L.srt_temporal_variance_last_ms(fresh._h, C.byref(ms)) == ERR_INVALID
        assert L.srt_read_temporal_moments(fresh._h, op, W, H) == ERR_INVALID
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, H, 2)
    assert gpu.denoise_temporal_vg(W, H, min_len=2, levels=1)["stats"]["history_frames"] == 1
    assert gpu.denoise_temporal_vg(W, H, min_len=2, levels=1)["stats"]["history_frames"] == 2
    before = gpu.temporal_moments()
    assert before[..., 2].max() == 2
    # a bad srt_temporal_vg, the chained calls' own bad configurations, null arguments, no output
    for v in (bad_tv(min_len=1), bad_tv(min_len=0), bad_tv(min_len=2 ** 24 + 1), bad_tv(moving=2), bad_tv(reserved=1)):
        assert chain(tv=v) == ERR_INVALID and present(tv=v) == ERR_INVALID
    assert b"temporal_vg" in L.srt_last_error(gpu._h)
    bad_t = srt.temporal_config()
    bad_t.alpha_min = 0.0
    bad_vg = srt.denoise_vg_config(levels=1)
    bad_vg.sigma_variance = INF
    assert chain(t=bad_t) == ERR_INVALID and chain(vg=bad_vg) == ERR_INVALID
    assert chain(t=None) == ERR_INVALID and chain(vg=None) == ERR_INVALID and chain(tv=None) == ERR_INVALID and present(tv=None) == ERR_INVALID
    assert chain(o=None) == ERR_INVALID
    ds = srt.despeckle_config(floor=0.0)
    ds.radius = 3
    assert L.srt_denoise_features_temporal_vg(gpu._h, C.byref(t), C.byref(ds), C.byref(vg), C.byref(tv), op, None, None, None, None, None, None, W, H) == ERR_INVALID
    # moving without tracking
    assert chain(tv=bad_tv(moving=1)) == ERR_INVALID and present(tv=bad_tv(moving=1)) == ERR_INVALID
    assert b"tracking" in L.srt_last_error(gpu._h)
    # every other present source
    for source in ("accum", "denoise", "denoise_mv", "develop"):
        assert present(source=source) == ERR_UNSUPPORTED, source
    # the choice kernel's and the read-back's own refusals
    q = np.ones((2, 2, 4), F)
    qp = q.ctypes.data_as(FP)
    assert L.srt_temporal_variance_kat(gpu._h, qp, qp, qp, 1, 2, 2, qp, None) == ERR_INVALID
    assert L.srt_temporal_variance_kat(gpu._h, qp, qp, qp, 2, 0, 2, qp, None) == ERR_INVALID
    assert L.srt_temporal_variance_kat(gpu._h, qp, qp, qp, 2, 2, 2, None, None) == ERR_INVALID
    assert L.srt_temporal_variance_kat(gpu._h, None, qp, qp, 2, 2, 2, qp, None) == ERR_INVALID
    assert L.srt_temporal_variance_kat(gpu._h, qp, qp, qp, 2, 2, 2, None, C.byref(n)) == 0
    assert L.srt_read_temporal_moments(gpu._h, None, W, H) == ERR_INVALID and L.srt_read_temporal_moments(gpu._h, op, 0, H) == ERR_INVALID
    # an unfeatured accumulation (srt_accum_reset keeps the temporal history)
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    assert chain() == ERR_INVALID and present() == ERR_INVALID
    # not one of them touched either history
    assert np.array_equal(bits(gpu.temporal_moments()), bits(before))
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, H, 2)
    again = gpu.denoise_temporal_vg(W, H, min_len=2, levels=1)
    assert again["stats"]["history_frames"] == 3 and again["stats"]["blended"] > 0 and gpu.temporal_moments()[..., 2].max() == 3
    # a partition other than (0, 1)
    gpu.set_partition(1, 2)
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, H, 2)
    assert chain() == ERR_UNSUPPORTED and present() == ERR_UNSUPPORTED
    gpu.set_partition(0, 1)
