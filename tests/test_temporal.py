"""Temporal reprojection on the device (srt_temporal_accum / srt_temporal_kat / srt_denoise_features_temporal / srt_present_temporal): the
device equals tests/temporal_reference.py in every bit and every counter -- on explicit random inputs, on the exact-shift geometry, on
real frames under a moving camera, through the chain into the denoiser and the presented picture --, the history lives exactly as long as
srt_c_api.h says, and no call changes the accumulation."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as D
import despeckle_reference as R
import temporal_reference as T
from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, assert_same_image, convert_xyz, fresh_context, gpu_lib, lane_of,
                           named_workload, read_frame)
from features_reference import stack_features
from helpers import bits
from path_ends_reference import assert_same_floats

F = np.float32
FP = C.POINTER(C.c_float)
INF = float("inf")
OFF = dict(sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)
SIZES = [(1, 1), (2, 2), (5, 3), (33, 9), (67, 35)]      # tile edges (32 x 8, waves of 16 x 4), partial waves, all-outside taps


def _assert_stage(got, want, what):
    """a dict of Renderer.temporal_kat against the restatement's"""
    assert_same_floats(got["colour"], want["colour"], what + " colour and len")
    assert_same_floats(got["guides"], want["guides"], what + " guides")
    assert_same_floats(got["motion"], want["motion"], what + " motion")
    stats = {k: v for k, v in got["stats"].items() if k in want["stats"]}
    assert stats == want["stats"], (what, stats, want["stats"])


def _camera_pairs(srt, IW, IH):
    prev = srt.camera_init(IW, IH, 40.0, (0.0, 0.0, 6.0), (0.0, 0.0, 0.0))
    return prev, [
        ("static", prev),
        ("translate", srt.camera_init(IW, IH, 40.0, (0.2, 0.1, 6.0), (0.2, 0.1, 0.0))),
        ("rotate", srt.camera_init(IW, IH, 40.0, (0.0, 0.0, 6.0), (0.3, 0.05, 0.0))),
        ("half-off", T.move_camera(prev, yaw_deg=0.5 * IW * 40.0 / IH * 0.8)),
        ("behind", T.move_camera(prev, yaw_deg=180.0)),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_kat_equals_the_restatement(srt, gpu, w, h):
    ox, oy = 5, 3
    prev, pairs = _camera_pairs(srt, w + ox + 2, h + oy + 1)
    c, g, hc, hg = T.random_case(w, h, 1)
    total = dict(blended=0, fresh=0, offscreen=0, rejected=0, nonfinite=0)
    for name, cur in pairs:
        for cfg in (dict(T.DEFAULTS), dict(T.DEFAULTS, alpha_min=0.3, max_len=6.5, **OFF)):
            for off in ((0, 0), (ox, oy)):
                what = "%d x %d %s at %r %r" % (w, h, name, off, cfg["sigma_depth"])
                want = T.temporal(c, g, cur, dict(colour=hc, guides=hg, cam=prev), off[0], off[1], **cfg)
                got = gpu.temporal_kat(cur, c, g, prev, hc, hg, off[0], off[1], **cfg)
                _assert_stage(got, want, what)
                assert got["stats"]["history_frames"] == 2 and not got["stats"]["history_dropped"]
                for k in total:
                    total[k] += want["stats"][k]
        want = T.temporal(c, g, cur, None, ox, oy, **T.DEFAULTS)
        got = gpu.temporal_kat(cur, c, g, offx=ox, offy=oy)
        _assert_stage(got, want, "%d x %d %s without history" % (w, h, name))
        assert got["stats"]["history_frames"] == 1 and got["stats"]["blended"] == 0 and np.isnan(got["motion"]).all()
    print("%d x %d: %r" % (w, h, total))
    if w * h >= 4:
        assert total["nonfinite"] > 0
    if w * h > 100:
        assert min(total.values()) > 0, total
    assert gpu.temporal_last_ms() > 0


@pytest.mark.gpu
def test_exact_shift_on_the_device(srt, gpu):
    prev, cur, g = T.shift_case(srt.CameraData)
    H, W = g.shape[:2]
    rng = np.random.default_rng(2)
    c = rng.uniform(0, 2, (H, W, 3)).astype(F)
    hc = np.concatenate([rng.uniform(0, 2, (H, W, 3)), rng.integers(1, 6, (H, W, 1))], axis=-1).astype(F)
    want = T.temporal(c, g, cur, dict(colour=hc, guides=g, cam=prev), **T.DEFAULTS)
    got = gpu.temporal_kat(cur, c, g, prev, hc, g)
    _assert_stage(got, want, "exact shift")
    assert np.array_equal(got["motion"][..., 0], np.full((H, W), F(3))) and not got["motion"][..., 1].any()
    assert got["stats"]["blended"] == H * (W - 3) and got["stats"]["offscreen"] == 3 * H and got["stats"]["rejected"] == 0
    ln = np.minimum(hc[:, 3:, 3] + F(1), F(32))
    a = np.maximum(F(1) / ln, F(0.1)).astype(F)
    h = hc[:, 3:, :3]
    assert np.array_equal(bits(got["colour"][:, :W - 3, :3]), bits((h + (a[..., None] * (c[:, :W - 3] - h).astype(F)).astype(F)).astype(F)))
    # alpha_min = 1 returns the input, whatever the history
    one = gpu.temporal_kat(cur, c, g, prev, hc, g, alpha_min=1.0)
    assert np.array_equal(bits(one["colour"][..., :3]), bits(c)) and one["stats"]["blended"] == H * (W - 3)


# ---- real frames ---------------------------------------------------------------------------------------------------------------------------
def _device_inputs(gpu, W, H, IW=None, IH=None, ox=0, oy=0, adaptive=False):
    """(c, guides) of the restatement from the device's own sums, rows and counts: the chunk W x H at (ox, oy) of an IW x IH image"""
    IW, IH = IW or W, IH or H
    frame = read_frame(gpu, IW, IH)
    lane = lane_of(gpu.geom, W, H)
    S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)
    rows = stack_features(gpu.read_features(IW, IH))[oy:oy + H, ox:ox + W]
    n = gpu.accum_samples
    if adaptive:
        n = np.asarray(gpu.accum_stats(IW, IH)["samples"]).reshape(IH, IW)[oy:oy + H, ox:ox + W]
        assert len(np.unique(n)) > 1, "the schedule must leave mixed counts"
    return T.mean_of(S, n), T.guides_of(rows, n)


def _srgb_of(orc, xyz):
    flat = xyz.reshape(-1, 3)
    lin, q = convert_xyz(orc, [flat[:, c] for c in range(3)], 1)
    return np.stack(lin, axis=1).reshape(xyz.shape), np.stack(q, axis=1).reshape(xyz.shape)


def _cameras(cam, scale):
    """three cameras a small step apart: a strafe and a turn of about two pixels"""
    return [cam, T.move_camera(cam, (0.01 * scale, 0.0, 0.0), yaw_deg=1.2), T.move_camera(cam, (0.02 * scale, 0.004 * scale, 0.0), yaw_deg=2.4, pitch_deg=0.5)]


def _frame(gpu, cam, W, H, passes, ox=0, oy=0, adaptive=False):
    gpu.set_camera(cam)
    if adaptive:
        gpu.accum_reset_adaptive_features(0.05, 0.0, 2)
    else:
        gpu.accum_reset_features()
    for s in passes:
        gpu.render_chunk_accum(W, H, s, ox, oy)


@pytest.mark.gpu
@pytest.mark.parametrize("name,passes,adaptive", [("cornell", (3, 2), False), ("dielectric", (4,), False), ("dielectric", (2, 2, 2), True)],
                         ids=["cornell", "dielectric", "dielectric-adaptive"])
def test_real_frames_under_a_moving_camera(srt, gpu, orc, name, passes, adaptive):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    du, dv, p00, ce = T.camera_vectors(cam)
    cams = _cameras(cam, float(np.linalg.norm(p00 - ce)) * 4)
    fresh_context(gpu, scene, cam, W, H, depth)
    hist = None
    for k, cur in enumerate(cams):
        _frame(gpu, cur, W, H, passes, adaptive=adaptive)
        c, g = _device_inputs(gpu, W, H, adaptive=adaptive)
        want = T.temporal(c, g, cur, hist, **T.DEFAULTS)
        got = gpu.temporal(W, H)
        what = "%s frame %d" % (name, k)
        assert_same_floats(got["xyz"], want["xyz"], what + " xyz")
        assert_same_floats(got["len"], want["len"], what + " len")
        assert_same_floats(got["motion"], want["motion"], what + " motion")
        stats = dict(want["stats"], history_frames=k + 1, history_dropped=False)
        assert got["stats"] == stats, (what, got["stats"], stats)
        print(what, got["stats"])
        lin, q = _srgb_of(orc, want["xyz"])
        assert_same_floats(got["lin"], lin, what + " unquantised sRGB")
        assert_same_floats(got["fb"], q, what + " quantised sRGB")
        if k == 0:
            assert np.array_equal(bits(got["xyz"]), bits(c)) and stats["blended"] == 0
            # srt_temporal_kat leaves the context's history alone
            rc, rg, rhc, rhg = T.random_case(19, 7, 4)
            gpu.temporal_kat(cams[2], rc, rg, cams[1], rhc, rhg)
        else:
            assert stats["blended"] > W * H // 4 and stats["fresh"] > 0, stats
            assert (bits(got["xyz"]) != bits(c)).any()
        hist = want
    assert gpu.temporal_last_ms() > 0


@pytest.mark.gpu
def test_offset_chunk(srt, gpu):
    """a 30 x 21 chunk at (17, 9) of a 64 x 40 image: fi, fj and the history's coordinates carry the offset; the placement is srt_despeckle_accum's"""
    scene, _, _, _, depth, _ = named_workload(srt, "dielectric")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = srt.camera_init(IW, IH, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0))
    cams = [cam, srt.camera_init(IW, IH, 45.0, (0.62, 0.8, 7.0), (0.1, 0.33, 0.0))]
    fresh_context(gpu, scene, cam, cw, ch, depth)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    hist, hists = None, []
    for k, cur in enumerate(cams):
        _frame(gpu, cur, cw, ch, (3,), ox, oy)
        c, g = _device_inputs(gpu, cw, ch, IW, IH, ox, oy)
        want = T.temporal(c, g, cur, hist, ox, oy, **T.DEFAULTS)
        got = gpu.temporal(IW, IH)
        for key, per in (("xyz", 3), ("len", 1), ("motion", 2)):
            assert not bits(got[key][~inside]).any(), key + ": written outside the chunk's rectangle"
            assert_same_floats(got[key][inside].reshape((ch, cw, per) if per > 1 else (ch, cw)), want[key], "offset chunk frame %d %s" % (k, key))
        assert {k2: got["stats"][k2] for k2 in want["stats"]} == want["stats"]
        hist = want
        hists.append(want)
    assert want["stats"]["blended"] > cw * ch // 4
    # without the offset the restatement says something else: the test would notice an offset that is dropped
    wrong = T.temporal(c, g, cams[1], hists[0], 0, 0, **T.DEFAULTS)
    assert (bits(wrong["motion"]) != bits(want["motion"])).any()
    # one output is enough, the caller's array outside the rectangle is not written, and the counters alone are enough too
    sentinel = np.full((IH, IW), F(-7), F)
    t, res = srt.temporal_config(), srt.binding.TemporalResult()
    gpu._ck(gpu_lib().srt_temporal_accum(gpu._h, C.byref(t), None, None, None, sentinel.ctypes.data_as(FP), None, None, IW, IH))
    assert (sentinel[~inside] == F(-7)).all() and (sentinel[inside] >= 0).all() and sentinel[inside].max() > 1
    gpu._ck(gpu_lib().srt_temporal_accum(gpu._h, C.byref(t), None, None, None, None, None, C.byref(res), IW, IH))
    assert res.history_frames == 4 and res.blended + res.fresh + res.nonfinite == cw * ch


# ---- the chain into the denoiser and the presented picture ---------------------------------------------------------------------------------
def _levels(c, g, levels, sig):
    N, z, A = g[..., 0:3], g[..., 3], g[..., 4:7]
    for i in range(levels):
        c = D.filter_level(c, N, A, z, i, D.level_constants(i, **sig))
    return c


@pytest.mark.gpu
def test_chained_denoise_and_present_equal_the_restatement(srt, gpu, orc):
    scene, _, _, _, depth, _ = named_workload(srt, "dielectric")
    W, H = 37, 19
    cams = [srt.camera_init(W, H, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0)), srt.camera_init(W, H, 45.0, (0.62, 0.8, 7.0), (0.1, 0.33, 0.0))]
    fresh_context(gpu, scene, cams[0], W, H, depth)
    sig = {k: v for k, v in D.DEFAULTS.items() if k != "levels"}
    ds = dict(radius=2, rank_ppm=500000, gain=4.0, floor=0.0)
    tcfg = dict(T.DEFAULTS, sigma_depth=0.2)
    # frame 0, no history: the chained calls are the plain ones, bit for bit
    _frame(gpu, cams[0], W, H, (3, 2))
    c0, g0 = _device_inputs(gpu, W, H)
    for despeckle in (None, ds):
        for levels in (0, 2):
            gpu.temporal_reset()
            plain = gpu.denoise(W, H, levels=levels) if despeckle is None else gpu.denoise_despeckled(W, H, despeckle=ds, levels=levels)
            got = gpu.denoise_temporal(W, H, temporal=tcfg, despeckle=despeckle, levels=levels)
            for key in ("xyz", "lin", "fb"):
                assert np.array_equal(bits(got[key]), bits(plain[key])), (despeckle, levels, key)
            assert got["stats"]["history_frames"] == 1 and got["stats"]["blended"] == 0
    hist = T.temporal(R.despeckle(c0, **ds)["xyz"], g0, cams[0], None, **tcfg)      # (what the last call left: despeckled, levels 2)
    # frame 1, the camera moved: prepass -> despeckle -> stage -> levels
    _frame(gpu, cams[1], W, H, (3, 2))
    c1, g1 = _device_inputs(gpu, W, H)
    stage = T.temporal(R.despeckle(c1, **ds)["xyz"], g1, cams[1], hist, **tcfg)
    assert stage["stats"]["blended"] > W * H // 4 and stage["stats"]["fresh"] > 0
    got = gpu.denoise_temporal(W, H, temporal=tcfg, despeckle=ds, levels=3)
    want = _levels(stage["xyz"], g1, 3, sig)
    assert_same_floats(got["xyz"], want, "chained denoise, 3 levels")
    lin, q = _srgb_of(orc, want)
    assert_same_floats(got["lin"], lin, "chained denoise lin")
    assert_same_floats(got["fb"], q, "chained denoise fb")
    assert {k: got["stats"][k] for k in stage["stats"]} == stage["stats"] and got["stats"]["history_frames"] == 2
    ms = gpu.denoise_last_ms()
    assert len(ms["levels"]) == 3 and all(t > 0 for t in ms["levels"]) and ms["prepass"] > 0 and gpu.temporal_last_ms() > 0 and gpu.despeckle_last_ms() > 0
    # the history is the stage's output, not the filtered picture: the same accumulation again, without the firefly filter, levels 0
    stage2 = T.temporal(c1, g1, cams[1], stage, **tcfg)
    got = gpu.denoise_temporal(W, H, temporal=tcfg, levels=0)
    assert_same_floats(got["xyz"], stage2["xyz"], "levels 0 is the stage's output")
    assert got["stats"]["history_frames"] == 3
    # ... and srt_temporal_accum continues the same history
    stage3 = T.temporal(c1, g1, cams[1], stage2, **tcfg)
    assert_same_floats(gpu.temporal(W, H, **tcfg)["xyz"], stage3["xyz"], "temporal() after denoise_temporal()")
    ms = gpu.denoise_last_ms()      # srt_temporal_accum records no denoise event: the last denoise's timing stays
    assert len(ms["levels"]) == 0 and ms["prepass"] > 0 and ms["epilogue"] > 0
    # the presented picture: the bytes of present_kat on the stage's output, the metering meter_kat's
    hist = stage3
    for source, despeckle, kw, gain in (("accum", None, dict(percentile_ppm=700000, white=8.0), None), ("accum", ds, dict(curve="linear"), 1.7),
                                        ("denoise", None, dict(levels=2), None), ("denoise", ds, dict(levels=1), 0.6)):
        pre = c1 if despeckle is None else R.despeckle(c1, **ds)["xyz"]
        hist = T.temporal(pre, g1, cams[1], hist, **tcfg)
        picture = hist["xyz"] if source == "accum" else _levels(hist["xyz"], g1, kw["levels"], sig)
        got = gpu.present_temporal(W, H, source, gain, temporal=tcfg, despeckle=despeckle, **kw)
        want = gpu.present_kat(picture, gain, **{k: v for k, v in kw.items() if k != "levels"})
        what = "%s %r gain %r" % (source, despeckle is not None, gain)
        assert np.array_equal(got["rgba"], want["rgba"]), what
        assert got["clip"] == want["clip"] and got["meter"] == want["meter"], what
        assert {k: got["temporal"][k] for k in hist["stats"]} == hist["stats"], what
    assert got["temporal"]["history_frames"] == 8 and got["rgba"][..., :3].max() > 0 and (got["rgba"][..., 3] == 255).all()


@pytest.mark.gpu
def test_render_interactive_generator(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    du, dv, p00, ce = T.camera_vectors(cam)
    cams = _cameras(cam, float(np.linalg.norm(p00 - ce)) * 4)
    steps = list(srt.render_interactive(scene, cams, W, H, 3, depth, renderer=gpu, levels=2, temporal=dict(max_len=8)))
    assert [s[0] for s in steps] == [0, 1, 2] and [s[4]["history_frames"] for s in steps] == [1, 2, 3]
    assert steps[0][4]["blended"] == 0 and steps[1][4]["blended"] > 0 and steps[2][4]["blended"] > 0
    # the first frame is render_features' (later frames continue the RNG streams, as successive frames of one context do)
    alone = list(srt.render_features(scene, cams[0], W, H, [3], depth, renderer=gpu))[0]
    assert_same_image(steps[0][1], alone[1], "render_interactive frame 0 against render_features")
    # the manual sequence of the same calls
    gpu.upload_scene(scene); gpu.set_camera(cams[0]); gpu.init_device_params(W, H, 3, depth, 1984); gpu.set_partition(0, 1)
    gpu.set_count_traversal(False); gpu.set_gather_planes(9)
    gpu.temporal_reset()
    for k, (_, res, feat, picture, stats) in enumerate(steps):
        assert set(picture) == {"xyz", "lin", "fb", "stats"} and picture["stats"] == stats
        _frame(gpu, cams[k], W, H, (3,))
        assert_same_image(res, read_frame(gpu, W, H), "render_interactive frame %d against the manual sequence" % k, rowmajor=False)
        want = gpu.denoise_temporal(W, H, dict(max_len=8), None, levels=2)
        for key in ("xyz", "lin", "fb"):
            assert np.array_equal(bits(picture[key]), bits(want[key])), (k, key)
        assert want["stats"] == stats
        manual = gpu.read_features(W, H)
        for key in manual:
            assert np.array_equal(bits(feat[key]), bits(manual[key])), key
    only = list(srt.render_interactive(scene, cams[:2], W, H, 3, depth, renderer=gpu, denoise=False))
    assert set(only[1][3]) == {"xyz", "lin", "fb", "len", "motion", "stats"} and only[1][4]["blended"] > 0 and only[0][4]["history_frames"] == 1


# ---- lifetimes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_history_lifetimes(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    fresh_context(gpu, scene, cam, W, H, depth)

    def frame(w=W, h=H):
        _frame(gpu, cam, w, h, (2,))
        return gpu.temporal(W, H)

    def first(out, dropped=False):
        return out["stats"]["history_frames"] == 1 and out["stats"]["blended"] == 0 and out["stats"]["history_dropped"] == dropped and (out["len"][:4, :4] <= 1).all()

    assert first(frame())
    kept = frame()      # srt_set_camera and srt_accum_reset_features in between: the history survives
    assert kept["stats"]["history_frames"] == 2 and kept["stats"]["blended"] > W * H // 2
    gpu.temporal_reset()
    assert first(frame()) and frame()["stats"]["history_frames"] == 2
    gpu.upload_scene(scene)
    assert first(frame()) and frame()["stats"]["history_frames"] == 2
    gpu.init_device_params(W, H, 12, depth, 7)
    assert first(frame()) and frame()["stats"]["history_frames"] == 2
    gpu.set_partition(0, 1)
    assert first(frame()) and frame()["stats"]["history_frames"] == 2
    # another rectangle: the history is dropped, the call says so and behaves as a first frame; the next one continues
    assert first(frame(W - 8, H - 3), dropped=True)
    again = frame(W - 8, H - 3)
    assert again["stats"]["history_frames"] == 2 and not again["stats"]["history_dropped"] and again["stats"]["blended"] > 0
    assert first(frame(), dropped=True)


@pytest.mark.gpu
def test_the_stage_changes_nothing_of_the_accumulation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")

    def run(with_stage):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_adaptive_features(0.05, 0.0, 2)
        gpu.render_chunk_accum(W, H, 4)
        if with_stage:
            gpu.temporal(W, H)
            gpu.temporal(W, H, alpha_min=0.5)
            gpu.denoise_temporal(W, H, levels=2)
            gpu.denoise_temporal(W, H, despeckle=dict(radius=1), levels=1)
            gpu.present_temporal(W, H)
            gpu.present_temporal(W, H, source="denoise", gain=1.0, levels=1)
            rc, rg, rhc, rhg = T.random_case(9, 5, 2)
            gpu.temporal_kat(cam, rc, rg, cam, rhc, rhg)
        gpu.render_chunk_accum(W, H, 4)
        frame, rows, stats = read_frame(gpu, W, H), stack_features(gpu.read_features(W, H)), gpu.accum_stats(W, H)
        assert gpu.accum_samples == 8
        gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
        return frame, rows, stats, read_frame(gpu, W, H)

    frame_a, rows_a, stats_a, after_a = run(True)
    frame_b, rows_b, stats_b, after_b = run(False)
    assert_same_image(frame_a, frame_b, "[4], the stage, [4] against [4, 4]")
    assert np.array_equal(bits(rows_a), bits(rows_b)) and rows_b[..., 7].max() > 0
    assert np.array_equal(stats_a["samples"], stats_b["samples"]) and len(np.unique(stats_b["samples"])) > 1
    assert_same_image(after_a, after_b, "RNG state: a plain launch after the passes")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L, B = gpu_lib(), srt.binding
    good, dcfg = srt.temporal_config(), srt.denoise_config(levels=1)
    res, pres = B.TemporalResult(), B.PresentResult()
    out = np.zeros((H, W, 3), F)
    op = out.ctypes.data_as(FP)
    rgba = np.zeros((H, W, 4), np.uint8)
    rp = rgba.ctypes.data_as(C.POINTER(C.c_uint8))
    img, gd = np.ones((H, W, 3), F), np.ones((H, W, 8), F)
    ip, gp = img.ctypes.data_as(FP), gd.ctypes.data_as(FP)
    col = np.zeros((H, W, 4), F)
    cp = col.ctypes.data_as(FP)

    def accum(t=good, o=op, r=None):
        return L.srt_temporal_accum(gpu._h, C.byref(t), o, None, None, None, None, r, W, H)

    def chain(t=good, d=dcfg):
        return L.srt_denoise_features_temporal(gpu._h, C.byref(t), None, C.byref(d), op, None, None, None, W, H)

    def present(t=good, source="accum", **kw):
        p = srt.present_config(source, 1.0, **kw)
        return L.srt_present_temporal(gpu._h, C.byref(p), C.byref(t) if t is not None else None, None, rp, 4 * W, W, H, C.byref(pres), C.byref(res))

    def kat(t=good, w=W, h=H, o=cp, r=None, ox=0, oy=0):
        return L.srt_temporal_kat(gpu._h, C.byref(t), C.byref(cam), None, ip, gp, None, None, w, h, ox, oy, o, None, None, r)

    fresh = srt.Renderer(0)
    try:
        ms = C.c_float()
        assert L.srt_temporal_last_ms(fresh._h, C.byref(ms)) == ERR_INVALID
        assert L.srt_temporal_accum(fresh._h, C.byref(good), op, None, None, None, None, None, W, H) == ERR_INVALID      # no accumulation at all
        assert L.srt_temporal_reset(fresh._h) == 0 and L.srt_temporal_reset(None) == ERR_INVALID
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    # no featured accumulation: a plain one with a pass, a featured one without
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    assert accum() == ERR_INVALID and chain() == ERR_INVALID and present() == ERR_INVALID and present(source="denoise") == ERR_INVALID
    gpu.accum_reset_features()
    assert accum() == ERR_INVALID
    gpu.render_chunk_accum(W, H, 2)
    first = gpu.temporal(W, H)
    assert first["stats"]["history_frames"] == 1

    def cfg(**kw):
        t = srt.temporal_config()
        for k, v in kw.items():
            if k == "reserved":
                t.reserved[2] = v
            else:
                setattr(t, k, v)
        return t

    bad = [cfg(alpha_min=0.0), cfg(alpha_min=-1.0), cfg(alpha_min=1.5), cfg(alpha_min=float("nan")), cfg(max_len=0.5), cfg(max_len=INF),
           cfg(max_len=float("nan")), cfg(sigma_normal=0.0), cfg(sigma_albedo=-1.0), cfg(sigma_depth=float("nan")), cfg(reserved=1)]
    for t in bad:
        assert accum(t) == ERR_INVALID and chain(t) == ERR_INVALID and present(t) == ERR_INVALID and kat(t) == ERR_INVALID
    assert b"temporal" in L.srt_last_error(gpu._h)
    assert accum(cfg(sigma_normal=INF, sigma_albedo=INF, sigma_depth=INF)) == 0      # (+inf is allowed)
    # all outputs NULL, null arguments, empty images
    assert accum(o=None) == ERR_INVALID and accum(o=None, r=C.byref(res)) == 0
    assert L.srt_temporal_accum(gpu._h, None, op, None, None, None, None, None, W, H) == ERR_INVALID
    assert L.srt_temporal_accum(gpu._h, C.byref(good), op, None, None, None, None, None, 0, H) == ERR_INVALID
    assert L.srt_denoise_features_temporal(gpu._h, C.byref(good), None, C.byref(dcfg), None, None, None, C.byref(res), W, H) == ERR_INVALID
    assert L.srt_denoise_features_temporal(gpu._h, None, None, C.byref(dcfg), op, None, None, None, W, H) == ERR_INVALID
    assert chain(d=srt.binding.Denoise(9, 1.0, 1.0, 1.0, 1.0, (C.c_uint32 * 3)(0, 0, 0))) == ERR_INVALID
    ds = srt.despeckle_config(floor=0.0)
    ds.radius = 3
    assert L.srt_denoise_features_temporal(gpu._h, C.byref(good), C.byref(ds), C.byref(dcfg), op, None, None, None, W, H) == ERR_INVALID
    assert present(None) == ERR_INVALID
    assert kat(o=None) == ERR_INVALID and kat(o=None, r=C.byref(res)) == 0 and kat(w=0) == ERR_INVALID
    assert kat(ox=(1 << 24) - W + 1) == ERR_INVALID and kat(ox=(1 << 24) - W) == 0
    assert L.srt_temporal_kat(gpu._h, C.byref(good), None, None, ip, gp, None, None, W, H, 0, 0, cp, None, None, None) == ERR_INVALID
    assert L.srt_temporal_kat(gpu._h, C.byref(good), C.byref(cam), None, None, gp, None, None, W, H, 0, 0, cp, None, None, None) == ERR_INVALID
    # an unsupported present source
    for source in ("denoise_vg", "denoise_mv", "develop"):
        assert present(source=source) == ERR_UNSUPPORTED, source
    # the refused calls left the history alone: the successful ones above advanced it
    n_ok = 2      # (the two srt_temporal_accum calls that returned 0; srt_temporal_kat keeps no history)
    assert gpu.temporal(W, H)["stats"]["history_frames"] == 1 + n_ok + 1
    # a partition other than (0, 1)
    gpu.set_partition(1, 2)
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, H, 2)
    assert accum() == ERR_UNSUPPORTED and chain() == ERR_UNSUPPORTED and present() == ERR_UNSUPPORTED and present(source="denoise") == ERR_UNSUPPORTED
    gpu.set_partition(0, 1)
