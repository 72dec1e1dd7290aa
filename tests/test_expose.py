"""Exposure metering and tone mapping on the device (srt_meter_accum / srt_meter_kat / srt_expose_accum / srt_expose_kat,
csrc/srt_expose.hip) against the restatement of tests/expose_reference.py: histograms, counters and decisions equal as integers, every
float bit for bit (two NaNs count as equal); the conversion to sRGB behind the tone curve is the CPU oracle's.  Explicit images at the
wave- and workgroup-boundary sizes first, then real accumulations of every kind, placement, partitions, the read-only property, the
refusals, and the Python front ends."""
import ctypes as C

import numpy as np
import pytest

import expose_reference as R
from accum_helpers import (ERR_INVALID, convert_xyz, expect_error, fresh_context, gpu_lib, lane_of, named_workload, read_frame,
                           read_sum_y, run_mock_transport_child)
from helpers import assert_planes_equal, bits
from path_ends_reference import assert_same_floats

F = np.float32
FP = C.POINTER(C.c_float)
U32P = C.POINTER(C.c_uint32)
SIZES = [(1, 1), (63, 1), (64, 1), (65, 3), (257, 5), (1000, 3)]


def _f(u):
    return np.array(u, np.uint32).view(F)


def _special_luminances():
    """denormals, +-0, negatives, NaN, +-inf, the bin edges k << 19 and (k << 19) - 1 at several k, FLT_MIN, FLT_MAX"""
    edges = [k << 19 for k in (16, 17, 18, 1000, 2032, 2033, 4079)] + [(k << 19) - 1 for k in (16, 17, 18, 1000, 2032, 2033, 4079, 4080)]
    words = [0x00000001, 0x00012345, 0x007fffff, 0x00000000, 0x80000000, 0xbf800000, 0x80800000, 0xff7fffff, 0x7fc00000, 0xffc00001,
             0x7f800000, 0xff800000, 0x00800000, 0x7f7fffff] + edges
    return _f(words)


def _kat_image(w, h, seed=0):
    """(h, w, 3): Y spans every exponent (uniform exponent and mantissa bits), with the special luminances spread over the image where it
    has room for them; X and Z are finite and differ from Y, so that a kernel reading another component is caught"""
    n = w * h
    rng = np.random.default_rng(1000 + n + seed)
    y = ((rng.integers(0, 255, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32)).view(F).copy()
    sp = _special_luminances()
    if n >= 63:
        y[rng.permutation(n - 1)[:sp.size]] = sp
        y[n - 1] = sp[7]
    img = np.empty((h, w, 3), F)
    img[..., 0] = rng.random((h, w)) + 0.5
    img[..., 1] = y.reshape(h, w)
    img[..., 2] = rng.random((h, w)) * 8.0 + 8.0
    return img


def _assert_meter(got, want, what):
    assert np.array_equal(got["hist"].astype(np.uint64), want["hist"]), "%s: histogram differs in %d bins" % (what, int((got["hist"] != want["hist"]).sum()))
    for k in ("metered", "dark", "nonfinite", "bin_ref"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("y_ref", "gain"):
        assert bits(F(got[k])) == bits(want[k]), (what, k, got[k], want[k])


def _tone_want(orc, xyz, gain, curve, white, mask=None):
    """dict(xyz, lin, fb, clip) of the restatement for XYZ means xyz (h, w, 3)"""
    o = R.tone(xyz, gain, curve, white)
    flat = o.reshape(-1, 3)
    lin, q = convert_xyz(orc, [flat[:, c] for c in range(3)], 1)      # (1.0f / 1.0f) * o is o: the oracle's conversion alone
    lin, q = np.stack(lin, axis=1).reshape(o.shape), np.stack(q, axis=1).reshape(o.shape)
    return dict(xyz=o, lin=lin, fb=q, clip=R.clip_counts(o, q, mask))


def _assert_exposed(got, want, what):
    for k in ("xyz", "lin", "fb"):
        assert_same_floats(got[k], want[k], "%s %s" % (what, k))
    assert got["clip"] == want["clip"], (what, got["clip"], want["clip"])


# ---- the meter kernel on explicit images -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_meter_kat_equals_the_restatement(gpu, w, h):
    img = _kat_image(w, h)
    for cfg in (dict(), dict(percentile_ppm=1, key=3.0), dict(percentile_ppm=1000000, gain_min=0.5, gain_max=2.0)):
        got = gpu.meter_kat(img, with_hist=True, **cfg)
        want = R.meter(img[..., 1], **dict(R.DEFAULTS, **cfg))
        _assert_meter(got, want, "KAT %d x %d %r" % (w, h, cfg))
        assert got["metered"] + got["dark"] + got["nonfinite"] == w * h
    if w * h >= 63:
        assert want["dark"] >= 7 and want["nonfinite"] >= 4 and want["hist"][16] >= 2 and want["hist"][4079] >= 2
    ms = gpu.expose_last_ms()
    assert ms["meter"] > 0


@pytest.mark.gpu
def test_meter_kat_constant_image_the_hot_bin(gpu):
    """70 000 pixels of one luminance: every lane of every wave hits one bin, which ends above 65 535"""
    img = np.full((100, 700, 3), 0.18, F)
    got = gpu.meter_kat(img, with_hist=True)
    want = R.meter(img[..., 1])
    _assert_meter(got, want, "constant image")
    assert got["metered"] == 70000 and got["hist"].max() == 70000 and got["dark"] == 0 and got["nonfinite"] == 0
    assert got["gain"] == float(F(0.18) / R.bin_midpoint(got["bin_ref"]))
    black = gpu.meter_kat(np.zeros((100, 700, 3), F), with_hist=True)
    assert (black["metered"], black["dark"], black["nonfinite"], black["gain"], int(black["hist"].sum())) == (0, 70000, 0, 1.0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(65, 3), (257, 5)])
def test_meter_kat_rectangles(gpu, w, h):
    img = _kat_image(w, h, seed=1)
    for rect in ((w // 2, h // 2, 1, 1), (0, 1, w, 1), (w - 9, 0, 9, h), (0, 0, w, h), (3, 1, 40, 2)):
        got = gpu.meter_kat(img, with_hist=True, rect=rect)
        want = R.meter(img[..., 1], R.rect_mask(w, h, rect))
        _assert_meter(got, want, "rect %r of %d x %d" % (rect, w, h))
        assert got["metered"] + got["dark"] + got["nonfinite"] == rect[2] * rect[3]
    whole, explicit = gpu.meter_kat(img, with_hist=True), gpu.meter_kat(img, with_hist=True, rect=(0, 0, w, h))
    assert np.array_equal(whole.pop("hist"), explicit.pop("hist")) and whole == explicit


# ---- the tone kernel on explicit images -------------------------------------------------------------------------------------------
def _tone_image(w, h):
    """finite XYZ means over seven decades, some negative or zero, and a NaN, a +inf and a -inf pixel (in different components)"""
    rng = np.random.default_rng(77 + w * h)
    img = ((rng.random((h, w, 3)) - 0.05) * 10.0 ** rng.integers(-4, 3, (h, w, 1))).astype(F)
    bad = np.zeros((h, w), bool)
    flat = img.reshape(-1, 3)
    n = w * h
    flat[n // 7] = 0
    flat[n // 5, 1] = F(1e-41)
    for k, (pix, comp, v) in enumerate(((n // 2, 1, np.nan), (n // 3, 1, np.inf), (n - 1, 0, -np.inf), (1, 2, np.nan), (2, 1, -np.inf))):
        flat[pix, comp] = v
        bad.reshape(-1)[pix] = True
    return img, bad


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(65, 3), (257, 5)])
def test_tone_kat_equals_the_restatement(srt, gpu, orc, w, h):
    img, bad = _tone_image(w, h)
    for curve in (0, 1):
        for white in (4.0, 1.5, np.inf):
            for gain in (1.0, 0.37, 2.0 ** -9, 300.0):
                got = gpu.expose_kat(img, gain=gain, curve=curve, white=white)
                want = _tone_want(orc, img, gain, curve, white)
                what = "tone KAT %d x %d curve %d white %r gain %r" % (w, h, curve, white, gain)
                _assert_exposed(got, want, what)
                assert got["meter"] is None and got["clip"]["nonfinite"] == int(bad.sum()), what
                assert np.isfinite(got["xyz"][~bad]).all() and not np.isfinite(got["xyz"][bad]).all(axis=-1).any(), what
    assert want["clip"]["blown"] > 0 and want["clip"]["crushed"] > 0
    assert gpu.expose_last_ms()["tone"] > 0
    # one requested output alone
    only = np.zeros(img.shape, F)
    tone = srt.tone_config(gain=300.0, curve=1, white=np.inf)
    gpu._ck(gpu_lib().srt_expose_kat(gpu._h, C.byref(tone), img.ctypes.data_as(FP), w, h, None, None, only.ctypes.data_as(FP), None))
    assert_same_floats(only, want["fb"], "out_q alone, no result")
    # metered: the gain is the meter's
    auto = gpu.expose_kat(img, curve=1, white=4.0, key=0.5)
    m = R.meter(img[..., 1], **dict(R.DEFAULTS, key=0.5))
    assert bits(F(auto["meter"]["gain"])) == bits(m["gain"]) and auto["meter"]["nonfinite"] == 3
    _assert_exposed(auto, _tone_want(orc, img, m["gain"], 1, 4.0), "metered KAT")


@pytest.mark.gpu
def test_scale_invariance(gpu):
    """inputs scaled by 2^k: the histogram shifts by 16 k bins, the gain scales by exactly 2^-k, the exposed picture is the same bits"""
    rng = np.random.default_rng(5)
    w, h = 257, 5
    img = (rng.random((h, w, 3)) * 10.0 ** rng.integers(-3, 3, (h, w, 1)) + 1e-4).astype(F)
    base_m = gpu.meter_kat(img, with_hist=True)
    base = {(c, wh): gpu.expose_kat(img, curve=c, white=wh) for c in (0, 1) for wh in (4.0, np.inf)}
    assert base_m["metered"] == w * h
    for k in (-7, 3, 20):
        scaled = (img * F(2.0 ** k)).astype(F)
        assert np.isfinite(scaled).all() and (scaled[..., 1] >= R.FLT_MIN).all()
        m = gpu.meter_kat(scaled, with_hist=True)
        assert np.array_equal(np.roll(base_m["hist"], 16 * k), m["hist"]) and m["bin_ref"] == base_m["bin_ref"] + 16 * k, k
        assert m["gain"] == base_m["gain"] * 2.0 ** -k and m["y_ref"] == base_m["y_ref"] * 2.0 ** k, k
        for (c, wh), want in base.items():
            got = gpu.expose_kat(scaled, curve=c, white=wh)
            for key in ("xyz", "lin", "fb"):
                assert np.array_equal(bits(got[key]), bits(want[key])), (k, c, wh, key)
            assert got["clip"] == want["clip"]
    assert len(np.unique(base[(1, 4.0)]["fb"])) > 50


# ---- real accumulations ------------------------------------------------------------------------------------------------------------
def _setup(gpu, srt, kind, partition=(0, 1)):
    """a bound accumulation of `kind`; returns (W, H)"""
    name = "random_spheres" if kind == "plain-random_spheres" else "cornell"
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.set_partition(*partition)
    if kind.startswith("plain"):
        gpu.accum_reset(); sched = [3, 2]
    elif kind == "adaptive":
        gpu.accum_reset_adaptive(0.02, 0.0, 4); sched = [4, 4, 4]
    elif kind == "streams":
        gpu.accum_reset_streams(4); sched = [4, 8]
    else:
        gpu.accum_reset_spectral_features(); sched = [2, 3]
    for s in sched:
        gpu.render_chunk_accum(W, H, s)
    return W, H


def _read_back(gpu, kind, W, H):
    """(XYZ sums (H, W, 3), counts: the total or the (H, W) map, frame)"""
    frame = read_frame(gpu, W, H)
    lane = lane_of(gpu.geom, W, H)
    sums = np.stack([frame["xyz"][c][lane] for c in range(3)], axis=-1).reshape(H, W, 3)
    n = gpu.accum_samples
    if kind == "adaptive":
        n = gpu.accum_stats(W, H)["samples"].reshape(H, W)
        assert len(np.unique(n)) > 1, "the schedule must leave mixed counts"
    return sums, n, frame, lane


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain-cornell", "plain-random_spheres", "adaptive", "streams", "spectral-features"])
def test_accumulation_metered_and_exposed(srt, gpu, orc, kind):
    W, H = _setup(gpu, srt, kind)
    sums, n, frame, lane = _read_back(gpu, kind, W, H)
    mean = R.mean_xyz(sums, n)
    got = gpu.meter(with_hist=True)
    want = R.meter(mean[..., 1])
    _assert_meter(got, want, kind)
    assert got["metered"] + got["dark"] + got["nonfinite"] == W * H and got["metered"] >= 100      # (cornell at 64 x 48 is mostly black background)
    rect = (5, 7, 33, 20)
    _assert_meter(gpu.meter(with_hist=True, rect=rect, percentile_ppm=900000), R.meter(mean[..., 1], R.rect_mask(W, H, rect), **dict(R.DEFAULTS, percentile_ppm=900000)), kind + " rect")
    # exposed at the metered gain, both curves
    for curve in (0, 1):
        ex = gpu.expose(W, H, curve=curve)
        assert bits(F(ex["meter"]["gain"])) == bits(want["gain"])
        _assert_exposed(ex, _tone_want(orc, mean, want["gain"], curve, 4.0), "%s curve %d" % (kind, curve))
    # curve 0 at gain 1 is the frame itself
    plain = gpu.expose(W, H, gain=1.0, curve="linear")
    assert_same_floats(plain["xyz"], mean, kind + " gain 1: the XYZ mean")
    for key, plane in (("lin", "lin"), ("fb", "fb")):
        own = np.stack([frame[plane][c][lane] for c in range(3)], axis=-1).reshape(H, W, 3)
        assert np.array_equal(bits(plain[key]), bits(own)), "%s gain 1 curve 0: %s is not the frame's own plane" % (kind, key)
    assert plain["fb"].max() > 0
    if kind == "spectral-features":
        # a denoised picture through the KAT doors
        den = gpu.denoise(W, H, levels=2)["xyz"]
        _assert_meter(gpu.meter_kat(den, with_hist=True), R.meter(den[..., 1]), "denoised")
        ex = gpu.expose_kat(den, curve=1)
        _assert_exposed(ex, _tone_want(orc, den, ex["meter"]["gain"], 1, 4.0), "denoised, exposed")
        assert bits(F(ex["meter"]["gain"])) == bits(R.meter(den[..., 1])["gain"])


@pytest.mark.gpu
def test_offset_chunk(srt, gpu, orc):
    scene, _, _, _, depth, _ = named_workload(srt, "random_spheres")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    fresh_context(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset()
    for s in (1, 3):
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    frame = read_frame(gpu, IW, IH)
    lane = lane_of(gpu.geom, cw, ch)
    mean = R.mean_xyz(np.stack([frame["xyz"][c][lane] for c in range(3)], axis=-1).reshape(ch, cw, 3), 4)
    _assert_meter(gpu.meter(with_hist=True), R.meter(mean[..., 1]), "offset chunk")
    rect = (22, 0, 8, 21)      # chunk pixels: ends on the chunk's last column
    _assert_meter(gpu.meter(with_hist=True, rect=rect), R.meter(mean[..., 1], R.rect_mask(cw, ch, rect)), "offset chunk, rect")
    expect_error(srt, lambda: gpu.meter(rect=(22, 0, 9, 21)), ERR_INVALID, "a rectangle one column beyond the chunk")
    expect_error(srt, lambda: gpu.meter(rect=(0, 21, 1, 1)), ERR_INVALID, "a rectangle below the chunk")
    ex = gpu.expose(IW, IH, gain=0.7, curve=1, white=2.0)
    want = _tone_want(orc, mean, 0.7, 1, 2.0)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    for key in ("xyz", "lin", "fb"):
        assert_same_floats(ex[key][inside].reshape(ch, cw, 3), want[key], "offset chunk " + key)
        assert not bits(ex[key][~inside]).any(), key
    assert ex["clip"] == want["clip"]
    # the caller's array outside the rectangle is not written at all
    sentinel = np.full((IH, IW, 3), F(-7), F)
    gpu._ck(gpu_lib().srt_expose_accum(gpu._h, C.byref(srt.tone_config(gain=0.7, curve=1, white=2.0)), None, sentinel.ctypes.data_as(FP), None, None, IW, IH))
    assert (sentinel[~inside] == F(-7)).all() and np.array_equal(bits(sentinel[inside]), bits(ex["lin"][inside]))


@pytest.mark.gpu
def test_partition_of_three_adds_up_to_the_whole_frame(srt, gpu, orc):
    W, H = _setup(gpu, srt, "plain-random_spheres")
    whole = gpu.meter(with_hist=True, percentile_ppm=700000)
    whole_clip = gpu.expose(W, H, gain=whole["gain"])["clip"]
    sums, n, _, _ = _read_back(gpu, "plain", W, H)
    mean = R.mean_xyz(sums, n)      # (the sums do not depend on the partition: a rank holds them at its own pixels and +0 elsewhere)
    hist = np.zeros(R.BINS, np.uint64)
    counts = dict(metered=0, dark=0, nonfinite=0)
    clip = dict(blown=0, crushed=0, nonfinite=0)
    tiles_x = (gpu.geom["tx"] * gpu.geom["bx"] + 7) // 8
    for rank in range(3):
        _setup(gpu, srt, "plain-random_spheres", partition=(rank, 3))
        part = gpu.meter(with_hist=True, percentile_ppm=700000)
        own = R.owner_mask(W, H, tiles_x, rank, 3)
        assert part["metered"] + part["dark"] + part["nonfinite"] == int(own.sum()), rank
        assert np.array_equal(bits(read_sum_y(gpu, W, H).reshape(H, W)), bits(np.where(own, sums[..., 1], F(0)))), rank
        _assert_meter(part, R.meter(mean[..., 1], own, **dict(R.DEFAULTS, percentile_ppm=700000)), "rank %d of 3" % rank)
        hist += part["hist"]
        for k in counts:
            counts[k] += part[k]
        ex = gpu.expose(W, H, gain=whole["gain"])
        assert ex["clip"] == _tone_want(orc, mean, whole["gain"], 1, 4.0, own)["clip"], rank
        assert not bits(ex["xyz"][~own]).any() and ex["xyz"][own].max() > 0
        for k in clip:
            clip[k] += ex["clip"][k]
    gpu.set_partition(0, 1)
    assert np.array_equal(hist, whole["hist"].astype(np.uint64)) and counts == {k: whole[k] for k in counts}
    assert clip == whole_clip
    decided = srt.meter_decide(hist, srt.meter_config(percentile_ppm=700000))
    assert (decided["bin_ref"], decided["y_ref"], decided["gain"], decided["metered"]) == (whole["bin_ref"], whole["y_ref"], whole["gain"], whole["metered"])


@pytest.mark.gpu
def test_metering_and_exposing_between_passes_changes_nothing(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")

    def run(with_expose):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_spectral_features()
        gpu.render_chunk_accum(W, H, 3)
        if with_expose:
            gpu.meter(rect=(1, 2, 30, 20))
            gpu.expose(W, H)
            gpu.expose(W, H, gain=2.0, curve=0)
            gpu.meter_kat(np.ones((70, 33, 3), F))
            gpu.expose_kat(np.ones((9, 300, 3), F))
        gpu.render_chunk_accum(W, H, 5)
        frame, film, feats = read_frame(gpu, W, H), gpu.read_spectral(W, H), gpu.read_features(W, H)
        assert gpu.accum_samples == 8
        gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
        return frame, film, feats, read_frame(gpu, W, H)

    frame, film, feats, after = run(True)
    frame0, film0, feats0, after0 = run(False)
    assert np.array_equal(bits(film), bits(film0)) and film0.max() > 0
    for k in feats0:
        assert np.array_equal(bits(feats[k]), bits(feats0[k])), k
    for key in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(frame[key], frame0[key], "frame after pass, expose, pass: " + key)
        assert_planes_equal(after[key], after0[key], "RNG state: plain launch after the passes, " + key)


@pytest.mark.gpu
def test_render_exposed_generator_and_comm_meter(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    steps = list(srt.render_exposed(scene, cam, W, H, [2, 4], depth, renderer=gpu, percentile_ppm=600000, white=8.0))
    plain = list(srt.render_progressive(scene, cam, W, H, [2, 4], depth, renderer=gpu))
    assert [s[0] for s in steps] == [2, 6]
    for (t, res, meter, ex), (t2, res2) in zip(steps, plain):
        assert t == t2 and set(ex) == {"xyz", "lin", "fb", "meter", "clip"} and meter is ex["meter"] and meter["metered"] > 0
        for key in ("fb", "lin", "xyz", "rowmajor"):
            assert_planes_equal(res[key], res2[key], "render_exposed vs render_progressive " + key)
    with pytest.raises(ValueError):
        srt.render_exposed(scene, cam, W, H, [2], depth, gain=1.0, key=0.2)
    with pytest.raises(TypeError):
        srt.render_exposed(scene, cam, W, H, [2], depth, sigma=1.0)
    whole = steps[-1][2]
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
W, H, depth = 64, 48, 8
cam = scene.default_camera(W, H)
for _, comm in comm_accumulations(srt, 2, (9,), scene, cam, W, H, depth, 6, lambda c: c.accum_reset(), (2, 4)):
    m = comm.meter(percentile_ppm=600000)
    parts = [r.meter(percentile_ppm=600000) for r in comm.renderers]
    assert m['metered'] == sum(p['metered'] for p in parts) and all(p['metered'] > 0 for p in parts)
    assert m['metered'] + m['dark'] + m['nonfinite'] == W * H
    assert (m['metered'], m['dark'], m['nonfinite'], m['bin_ref'], m['gain']) == %r, m
print('expose mock transport ok')
""" % ((whole["metered"], whole["dark"], whole["nonfinite"], whole["bin_ref"], whole["gain"]),), "expose mock transport ok", timeout=300)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L, B = gpu_lib(), srt.binding
    mcfg, tcfg = srt.meter_config(), srt.tone_config(gain=2.0)
    res, tres = B.MeterResult(), B.ToneResult()
    out = np.zeros((H, W, 3), F)
    op = out.ctypes.data_as(FP)
    img = np.ones((H, W, 3), F)
    ip = img.ctypes.data_as(FP)
    hist = np.zeros(R.BINS, np.uint32)
    hp = hist.ctypes.data_as(U32P)
    fresh = srt.Renderer(0)
    try:
        assert L.srt_expose_last_ms(fresh._h, None, None) == ERR_INVALID
        assert L.srt_meter_accum(fresh._h, C.byref(mcfg), hp, C.byref(res)) == ERR_INVALID      # no accumulation at all
        assert L.srt_expose_accum(fresh._h, C.byref(tcfg), op, None, None, None, W, H) == ERR_INVALID
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset()
    expect_error(srt, lambda: gpu.meter(), ERR_INVALID, "meter before the first pass")
    expect_error(srt, lambda: gpu.expose(W, H, gain=1.0), ERR_INVALID, "expose before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first, first_ex = gpu.meter(with_hist=True), gpu.expose(W, H)
    frame = read_frame(gpu, W, H)

    def meter(**kw):
        m = srt.meter_config()
        for k, v in kw.items():
            if k == "reserved":
                m.reserved[2] = v
            else:
                setattr(m, k, v)
        return m

    def tone(**kw):
        t = srt.tone_config(gain=2.0)
        for k, v in kw.items():
            if k == "reserved":
                t.reserved[4] = v
            else:
                setattr(t, k, v)
        return t

    inf, nan = float("inf"), float("nan")
    bad_meters = [dict(percentile_ppm=0), dict(percentile_ppm=1000001), dict(key=0.0), dict(key=nan), dict(key=inf), dict(gain_min=0.0),
                  dict(gain_min=8.0, gain_max=4.0), dict(gain_max=inf), dict(gain_min=nan), dict(reserved=1), dict(w=4), dict(x0=1, y0=1, h=4),
                  dict(x0=W, y0=0, w=1, h=1), dict(x0=0, y0=0, w=W + 1, h=H), dict(x0=0, y0=H - 1, w=W, h=2), dict(x0=0xffffffff, y0=0, w=2, h=1)]
    bad_tones = [dict(curve=2), dict(gain=0.0), dict(gain=-1.0), dict(gain=inf), dict(gain=nan), dict(white=0.0), dict(white=-4.0), dict(white=nan), dict(reserved=7)]
    refused = [("meter: null cfg", lambda: L.srt_meter_accum(gpu._h, None, hp, C.byref(res))),
               ("meter: null result", lambda: L.srt_meter_accum(gpu._h, C.byref(mcfg), hp, None)),
               ("meter KAT: null image", lambda: L.srt_meter_kat(gpu._h, C.byref(mcfg), None, W, H, hp, C.byref(res))),
               ("meter KAT: null result", lambda: L.srt_meter_kat(gpu._h, C.byref(mcfg), ip, W, H, hp, None)),
               ("meter KAT: empty image", lambda: L.srt_meter_kat(gpu._h, C.byref(mcfg), ip, 0, H, hp, C.byref(res))),
               ("meter KAT: 2^31 pixels", lambda: L.srt_meter_kat(gpu._h, C.byref(mcfg), ip, 0x10000, 0x8000, hp, C.byref(res))),
               ("expose: null tone", lambda: L.srt_expose_accum(gpu._h, None, op, None, None, C.byref(tres), W, H)),
               ("expose: all outputs NULL", lambda: L.srt_expose_accum(gpu._h, C.byref(tcfg), None, None, None, C.byref(tres), W, H)),
               ("expose: empty image", lambda: L.srt_expose_accum(gpu._h, C.byref(tcfg), op, None, None, C.byref(tres), W, 0)),
               ("expose KAT: all outputs NULL", lambda: L.srt_expose_kat(gpu._h, C.byref(tcfg), ip, W, H, None, None, None, C.byref(tres))),
               ("expose KAT: null image", lambda: L.srt_expose_kat(gpu._h, C.byref(tcfg), None, W, H, op, None, None, C.byref(tres))),
               ("expose KAT: empty image", lambda: L.srt_expose_kat(gpu._h, C.byref(tcfg), ip, W, 0, op, None, None, C.byref(tres)))]
    for kw in bad_meters:
        refused.append(("meter %r" % kw, lambda kw=kw: L.srt_meter_accum(gpu._h, C.byref(meter(**kw)), hp, C.byref(res))))
        refused.append(("meter KAT %r" % kw, lambda kw=kw: L.srt_meter_kat(gpu._h, C.byref(meter(**kw)), ip, W, H, hp, C.byref(res))))
    for kw in bad_tones:
        refused.append(("tone %r" % kw, lambda kw=kw: L.srt_expose_accum(gpu._h, C.byref(tone(**kw)), op, None, None, C.byref(tres), W, H)))
        refused.append(("tone KAT %r" % kw, lambda kw=kw: L.srt_expose_kat(gpu._h, C.byref(tone(**kw)), ip, W, H, op, None, None, C.byref(tres))))
    for what, call in refused:
        assert call() == ERR_INVALID, what
        assert not bits(out).any() and not hist.any() and not bytes(res).strip(b"\0") and not bytes(tres).strip(b"\0"), what
    # after all of them the accumulation meters, exposes, reads and continues as before
    again = gpu.meter(with_hist=True)
    assert np.array_equal(again["hist"], first["hist"]) and {k: v for k, v in again.items() if k != "hist"} == {k: v for k, v in first.items() if k != "hist"}
    again_ex = gpu.expose(W, H)
    for key in ("xyz", "lin", "fb"):
        assert_same_floats(again_ex[key], first_ex[key], "expose after the refusals, " + key)
    for key, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, frame[key], "after the refusals " + key)
    assert gpu.accum_samples == 4
    # whatever ends the accumulation ends the metering
    gpu.accum_reset()
    expect_error(srt, lambda: gpu.meter(), ERR_INVALID, "meter after srt_accum_reset")
