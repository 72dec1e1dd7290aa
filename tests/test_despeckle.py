"""The firefly filter on the device (srt_despeckle_accum / srt_despeckle_kat / srt_denoise_features_ds / srt_present_despeckled,
csrc/srt_despeckle.hip) against the restatement of tests/despeckle_reference.py: every float bit for bit (two NaNs count as equal), every
counter as an integer.  Explicit images at the sizes where the tiling changes first, then the exact cases, real accumulations of several
kinds, placement, the sRGB outputs against the CPU oracle's conversion, the read-only property, the chain into the denoiser, the
presented picture, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as D
import despeckle_reference as R
import expose_reference as E
from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, assert_same_image, convert_xyz, expect_error, fresh_context, gpu_lib, lane_of,
                           named_workload, read_frame)
from features_reference import stack_features
from helpers import bits
from path_ends_reference import assert_same_floats

F = np.float32
FP = C.POINTER(C.c_float)
INF = float("inf")
SIZES = [(1, 1), (1, 9), (9, 1), (3, 2), (5, 5), (67, 35)]      # (w, h); 67 x 35 is no multiple of the 32 x 8 tile and crosses tiles both ways
FLT_MIN = F(1.17549435e-38)


def _assert_despeckled(got, want, what):
    assert_same_floats(got["xyz"], want["xyz"], what + " xyz")
    assert_same_floats(got["scale"], want["scale"], what + " scale")
    assert got["clip"] == want["clip"], (what, got["clip"], want["clip"])


# ---- explicit images -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_kat_equals_the_restatement(gpu, w, h):
    img = R.recipe_image(w, h)
    seen = dict(clamped=0, nonfinite=0, alone=0)
    for radius in (1, 2):
        for rank in R.RANKS:
            for gain, floor in ((4.0, 0.0), (1.5, 0.01)):
                cfg = dict(radius=radius, rank_ppm=rank, gain=gain, floor=floor)
                got = gpu.despeckle_kat(img, **cfg)
                want = R.despeckle(img, **cfg)
                _assert_despeckled(got, want, "KAT %d x %d %r" % (w, h, cfg))
                assert got["floor"] == F(floor)
                for k in seen:
                    seen[k] += got["clip"][k]
    if w * h == 1:
        assert seen["alone"] == 20
    if w * h >= 9:
        assert seen["nonfinite"] >= 40 and seen["clamped"] > 0      # a NaN and an inf pixel in every image of nine pixels and more
    assert gpu.despeckle_last_ms() > 0


def test_clamp_and_keep_shares_of_the_recipe():
    """on the restatement alone: the 67 x 35 input clamps at least a tenth of its pixels and keeps at least half"""
    img = R.recipe_image(67, 35)
    n = 67 * 35
    for radius in (1, 2):
        for rank in (250000, 500000):
            want = R.despeckle(img, radius, rank, 4.0, 0.0)
            kept = n - sum(want["clip"].values())
            print("radius %d rank %d: clamped %.3f kept %.3f of %d" % (radius, rank, want["clip"]["clamped"] / n, kept / n, n))
            assert want["clip"]["clamped"] * 10 >= n and kept * 2 >= n
            assert want["clip"]["nonfinite"] >= 2 * 47      # 2 % NaN and 2 % inf pixels


@pytest.mark.gpu
def test_kat_specials_and_denormals(gpu):
    """a window's values below FLT_MIN, zeros of both signs and negatives: the selection network keeps denormals and the canonical +0"""
    rng = np.random.default_rng(12)
    h, w = 9, 40
    img = np.zeros((h, w, 3), F)
    img[..., 1] = (rng.integers(1, 1 << 23, (h, w)).astype(np.uint32)).view(F)          # every luminance a denormal
    img[..., 0] = img[..., 1] * F(0.5)
    img[..., 2] = F(1e-39)
    img[rng.random((h, w)) < 0.2, 1] = F(-0.0)
    img[rng.random((h, w)) < 0.1, 1] = F(-3e-40)
    img[4, 7] = F(3e38)
    img[2, 30, 1] = F(2e-38)
    median = R.despeckle(img, 2, 500000, 2.0, 0.0)
    assert median["clip"]["clamped"] > 20 and (median["ref"] > 0).any() and (median["ref"] < FLT_MIN).all()
    for radius in (1, 2):
        for rank in R.RANKS:
            cfg = dict(radius=radius, rank_ppm=rank, gain=2.0, floor=0.0)
            _assert_despeckled(gpu.despeckle_kat(img, **cfg), R.despeckle(img, **cfg), "denormals %r" % cfg)


# ---- the exact cases of the header -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_power_of_two_scaling_on_the_device(gpu):
    img = R.recipe_image(41, 19, sprinkle=False)
    base = gpu.despeckle_kat(img, radius=2, rank_ppm=500000, gain=4.0, floor=0.125)
    assert base["clip"]["clamped"] > 50
    for k in (-60, 3, 40):
        sc = F(2.0 ** k)
        got = gpu.despeckle_kat((img * sc).astype(F), radius=2, rank_ppm=500000, gain=4.0, floor=float(F(0.125) * sc))
        assert np.array_equal(bits(got["xyz"]), bits((base["xyz"] * sc).astype(F))) and np.array_equal(bits(got["scale"]), bits(base["scale"])), k
        assert got["clip"] == base["clip"]


@pytest.mark.gpu
def test_flips_and_transposes_commute_on_the_device(gpu):
    img = R.recipe_image(37, 13, seed=2)
    for radius in (1, 2):
        base = gpu.despeckle_kat(img, radius=radius, rank_ppm=500000, gain=4.0, floor=0.01)
        for name, f in (("flip x", lambda a: a[:, ::-1]), ("flip y", lambda a: a[::-1]), ("transpose", lambda a: np.swapaxes(a, 0, 1))):
            got = gpu.despeckle_kat(np.ascontiguousarray(f(img)), radius=radius, rank_ppm=500000, gain=4.0, floor=0.01)
            assert_same_floats(got["xyz"], np.ascontiguousarray(f(base["xyz"])), "%s radius %d" % (name, radius))
            assert got["clip"] == base["clip"]


@pytest.mark.gpu
def test_edge_cluster_and_line_on_the_device(gpu):
    edge = R.step_edge()
    for radius in (1, 2):
        for rank in (500000, 875000, 1000000):
            for gain in (1.0, 4.0):
                got = gpu.despeckle_kat(edge, radius=radius, rank_ppm=rank, gain=gain, floor=0.0)
                assert got["clip"] == dict(clamped=0, nonfinite=0, alone=0) and np.array_equal(bits(got["xyz"]), bits(edge)), (radius, rank, gain)
    for count in (1, 12):
        img, mask = R.cluster(count)
        got = gpu.despeckle_kat(img, radius=2, rank_ppm=500000, gain=4.0, floor=0.0)
        assert np.array_equal(got["scale"] != 1, mask) and got["clip"]["clamped"] == count and (got["xyz"][mask] == F(2.0)).all()
        assert np.array_equal(bits(got["xyz"][~mask]), bits(img[~mask]))
    line, inner = R.bright_line(13)
    at_median = gpu.despeckle_kat(line, radius=2, rank_ppm=500000, gain=4.0, floor=0.0)
    default = gpu.despeckle_kat(line, floor=0.0)
    assert (at_median["scale"][inner] != 1).sum() == 9 and (default["scale"][inner] == 1).all()
    _assert_despeckled(default, R.despeckle(line, **R.DEFAULTS), "line at the defaults")
    off = gpu.despeckle_kat(line, radius=2, rank_ppm=0, gain=0.0, floor=INF)
    assert np.array_equal(bits(off["xyz"]), bits(line)) and off["clip"]["clamped"] == 0


# ---- real accumulations --------------------------------------------------------------------------------------------------------------------
def _accumulate(gpu, srt, name, kind="plain", sched=(3, 2)):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    fresh_context(gpu, scene, cam, W, H, depth)
    if kind == "plain":
        gpu.accum_reset()
    elif kind == "adaptive":
        gpu.accum_reset_adaptive(0.02, 0.0, 4)
    elif kind == "streams":
        gpu.accum_reset_streams(4)
    else:
        gpu.accum_reset_features()
    for s in sched:
        gpu.render_chunk_accum(W, H, s)
    return W, H


def _device_mean(gpu, W, H, adaptive=False):
    """the XYZ mean (H, W, 3) of the restatement from the device's own sums and counts"""
    frame = read_frame(gpu, W, H)
    lane = lane_of(gpu.geom, W, H)
    sums = np.stack([np.asarray(frame["xyz"][c], F)[lane] for c in range(3)], axis=-1).reshape(H, W, 3)
    n = gpu.accum_samples
    if adaptive:
        n = gpu.accum_stats(W, H)["samples"].reshape(H, W)
        assert len(np.unique(n)) > 1, "the schedule must leave mixed counts"
    return R.mean_xyz(sums, n)


def _srgb_of(orc, xyz):
    flat = xyz.reshape(-1, 3)
    lin, q = convert_xyz(orc, [flat[:, c] for c in range(3)], 1)      # (1.0f / 1.0f) * o is o: the oracle's conversion alone
    return np.stack(lin, axis=1).reshape(xyz.shape), np.stack(q, axis=1).reshape(xyz.shape)


def _metered_floor(gpu, mean):
    m = gpu.meter(percentile_ppm=500000)
    want = E.meter(mean[..., 1], **dict(E.DEFAULTS, percentile_ppm=500000))
    assert bits(F(m["y_ref"])) == bits(F(want["y_ref"]))
    return float(m["y_ref"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dielectric", "cornell", "random_spheres-defaults", "random_spheres"])
def test_real_accumulations(srt, gpu, orc, case):
    name = case.split("-")[0]
    W, H = _accumulate(gpu, srt, name)
    mean = _device_mean(gpu, W, H)
    lit = (mean[..., 1] >= FLT_MIN)
    n = W * H
    if case == "dielectric":
        cfgs = [dict(radius=r, rank_ppm=500000, gain=4.0, floor=0.0) for r in (1, 2)]
    elif case == "cornell":
        cfgs = [dict(radius=r, rank_ppm=875000, gain=4.0, floor=None) for r in (1, 2)]
    elif case == "random_spheres-defaults":
        cfgs = [dict()]
    else:
        cfgs = [dict(radius=r, rank_ppm=500000, gain=1.0, floor=0.0) for r in (1, 2)]
    for cfg in cfgs:
        rcfg = dict(R.DEFAULTS, **cfg)
        if rcfg.get("floor") is None or "floor" not in cfg:
            rcfg["floor"] = _metered_floor(gpu, mean)
        want = R.despeckle(mean, **rcfg)
        kept = ~(want["clamped"] | want["nonfinite"] | want["alone"])
        print("%s %r: floor %r, clamped %d, lit kept %d of %d lit, %d pixels" % (case, cfg, rcfg["floor"], want["clip"]["clamped"], int((kept & lit).sum()), int(lit.sum()), n))
        if case == "dielectric":
            assert want["clip"]["clamped"] >= 16 and kept.sum() * 2 >= n
        elif case == "cornell":
            assert rcfg["floor"] > 0 and want["clip"]["clamped"] >= 16 and (kept & lit).sum() >= 16
        elif case == "random_spheres-defaults":
            assert want["clip"] == dict(clamped=0, nonfinite=0, alone=0) and np.array_equal(bits(want["xyz"]), bits(mean))
        got = gpu.despeckle(W, H, **cfg)
        _assert_despeckled(got, want, "%s %r" % (case, cfg))
        assert bits(F(got["floor"])) == bits(F(rcfg["floor"]))
        lin, q = _srgb_of(orc, want["xyz"])
        assert_same_floats(got["lin"], lin, case + " unquantised sRGB")
        assert_same_floats(got["fb"], q, case + " quantised sRGB")
        if case == "random_spheres-defaults":
            assert np.array_equal(bits(got["xyz"]), bits(mean)) and (got["scale"] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adaptive", "streams"])
def test_other_accumulation_kinds(srt, gpu, kind):
    W, H = _accumulate(gpu, srt, "cornell", kind, (4, 4, 4) if kind == "adaptive" else (4, 8))
    mean = _device_mean(gpu, W, H, adaptive=kind == "adaptive")
    for cfg in (dict(radius=2, rank_ppm=875000, gain=4.0, floor=None), dict(radius=1, rank_ppm=500000, gain=2.0, floor=0.05)):
        rcfg = dict(cfg)
        if cfg["floor"] is None:
            rcfg["floor"] = _metered_floor(gpu, mean)
        want = R.despeckle(mean, **rcfg)
        _assert_despeckled(gpu.despeckle(W, H, **cfg), want, "%s %r" % (kind, cfg))
    assert want["clip"]["clamped"] > 0


@pytest.mark.gpu
def test_offset_chunk_placement(srt, gpu):
    """a 30 x 21 chunk (no multiple of 8 x 8, 28 x 16 or 32 x 8) at (17, 9) of a 64 x 40 image: the placement of srt_expose_accum"""
    scene, _, _, _, depth, _ = named_workload(srt, "dielectric")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = srt.camera_init(IW, IH, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0))
    fresh_context(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset()
    for s in (1, 3):
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    frame = read_frame(gpu, IW, IH)
    lane = lane_of(gpu.geom, cw, ch)
    mean = R.mean_xyz(np.stack([np.asarray(frame["xyz"][c], F)[lane] for c in range(3)], axis=-1).reshape(ch, cw, 3), 4)
    cfg = dict(radius=2, rank_ppm=500000, gain=2.0, floor=0.0)
    want = R.despeckle(mean, **cfg)
    assert want["clip"]["clamped"] > 0
    got = gpu.despeckle(IW, IH, **cfg)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    for k in ("xyz", "lin", "fb"):
        assert not bits(got[k][~inside]).any(), k + ": written outside the chunk's rectangle"
    assert not bits(got["scale"][~inside]).any()
    assert_same_floats(got["xyz"][inside].reshape(ch, cw, 3), want["xyz"], "offset chunk xyz")
    assert_same_floats(got["scale"][inside].reshape(ch, cw), want["scale"], "offset chunk scale")
    assert got["clip"] == want["clip"]
    # the caller's arrays outside the rectangle are not written at all; one output is enough, and the counters alone are too
    sentinel = np.full((IH, IW), F(-7), F)
    d, res = srt.despeckle_config(**cfg), srt.binding.DespeckleResult()
    gpu._ck(gpu_lib().srt_despeckle_accum(gpu._h, C.byref(d), None, None, None, sentinel.ctypes.data_as(FP), None, IW, IH))
    assert (sentinel[~inside] == F(-7)).all() and np.array_equal(bits(sentinel[inside]), bits(got["scale"][inside]))
    gpu._ck(gpu_lib().srt_despeckle_accum(gpu._h, C.byref(d), None, None, None, None, C.byref(res), IW, IH))
    assert dict(clamped=res.clamped, nonfinite=res.nonfinite, alone=res.alone) == want["clip"]


# ---- the call only reads -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_despeckle_between_passes_changes_nothing(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")

    def run(with_filter):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, 4)
        if with_filter:
            gpu.despeckle(W, H)
            gpu.despeckle(W, H, radius=1, rank_ppm=500000, floor=0.0)
            gpu.denoise_despeckled(W, H, levels=2)
            gpu.present_despeckled(W, H)
            gpu.present_despeckled(W, H, source="denoise", gain=1.0, levels=1)
            gpu.despeckle_kat(np.ones((9, 70, 3), F), floor=0.0)
        gpu.render_chunk_accum(W, H, 4)
        frame, rows = read_frame(gpu, W, H), stack_features(gpu.read_features(W, H))
        assert gpu.accum_samples == 8
        gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
        return frame, rows, read_frame(gpu, W, H)

    frame_a, rows_a, after_a = run(True)
    frame_b, rows_b, after_b = run(False)
    assert_same_image(frame_a, frame_b, "[4], despeckle, [4] against [4, 4]")
    assert np.array_equal(bits(rows_a), bits(rows_b)) and rows_b[..., 7].max() > 0
    assert_same_image(after_a, after_b, "RNG state: a plain launch after the passes")


# ---- the chain into the denoiser -------------------------------------------------------------------------------------------------------
def _denoise_after_despeckle(S, rows, n, ds_cfg, levels, **sigmas):
    """denoise_reference.denoise with c = Despeckle(c) between its prepass and its level 0"""
    c, N, A, z = D.prepass(S, rows, n)
    c = R.despeckle(c, **ds_cfg)["xyz"]
    for i in range(levels):
        c = D.filter_level(c, N, A, z, i, D.level_constants(i, **sigmas))
    return c


@pytest.mark.gpu
def test_chained_denoise_equals_the_restatement(srt, gpu, orc):
    scene, _, _, _, depth, _ = named_workload(srt, "dielectric")
    W, H = 37, 19
    cam = srt.camera_init(W, H, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0))
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    for s in (3, 2):
        gpu.render_chunk_accum(W, H, s)
    frame = read_frame(gpu, W, H)
    lane = lane_of(gpu.geom, W, H)
    S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)
    rows = stack_features(gpu.read_features(W, H))
    sig = {k: v for k, v in D.DEFAULTS.items() if k != "levels"}
    ds = dict(radius=2, rank_ppm=500000, gain=4.0, floor=0.0)
    clamped = R.despeckle(D.prepass(S, rows, 5)[0], **ds)["clip"]["clamped"]
    assert clamped >= 8, clamped
    for levels in (0, 1, 3):
        want = _denoise_after_despeckle(S, rows, 5, ds, levels, **sig)
        got = gpu.denoise_despeckled(W, H, despeckle=ds, levels=levels)
        assert_same_floats(got["xyz"], want, "chained denoise, %d levels" % levels)
        lin, q = _srgb_of(orc, want)
        assert_same_floats(got["lin"], lin, "chained denoise lin")
        assert_same_floats(got["fb"], q, "chained denoise fb")
        ms = gpu.denoise_last_ms()
        assert len(ms["levels"]) == levels and all(t > 0 for t in ms["levels"]) and ms["prepass"] > 0 and ms["epilogue"] > 0 and gpu.despeckle_last_ms() > 0
        plain = gpu.denoise(W, H, levels=levels)
        off = gpu.denoise_despeckled(W, H, despeckle=dict(ds, floor=INF), levels=levels)
        for k in ("xyz", "lin", "fb"):
            assert np.array_equal(bits(off[k]), bits(plain[k])), (levels, k)
        if levels:
            assert (bits(got["xyz"]) != bits(plain["xyz"])).any()
    # levels == 0 is the despeckled mean, the picture srt_despeckle_accum gives
    assert_same_floats(gpu.denoise_despeckled(W, H, despeckle=ds, levels=0)["xyz"], gpu.despeckle(W, H, **ds)["xyz"], "levels 0 against despeckle()")
    # a metered floor (the default) is metered on the accumulation
    mean = R.mean_xyz(S, 5)
    floor = _metered_floor(gpu, mean)
    want = _denoise_after_despeckle(S, rows, 5, dict(R.DEFAULTS, floor=floor), 2, **sig)
    assert_same_floats(gpu.denoise_despeckled(W, H, levels=2)["xyz"], want, "chained denoise at the defaults")
    # the variance-guided denoise still reports its estimator, the plain one still refuses to
    gpu.denoise_despeckled(W, H, despeckle=ds, levels=1)
    expect_error(srt, gpu.denoise_estimate_last_ms, ERR_INVALID, "estimate_last_ms after a chained plain denoise")
    gpu.denoise_vg(W, H, levels=1)
    assert gpu.denoise_estimate_last_ms() > 0


@pytest.mark.gpu
def test_render_despeckled_generator(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    steps = list(srt.render_despeckled(scene, cam, W, H, [2, 3], depth, renderer=gpu, levels=2, despeckle=dict(radius=1)))
    plain = list(srt.render_features(scene, cam, W, H, [2, 3], depth, renderer=gpu))
    assert [s[0] for s in steps] == [2, 5]
    for (t, res, feat, cleaned), (t2, res2, feat2) in zip(steps, plain):
        assert t == t2 and set(cleaned) == {"xyz", "lin", "fb"}
        assert_same_image(res, res2, "render_despeckled against render_features")
        for k in feat2:
            assert np.array_equal(bits(feat[k]), bits(feat2[k])), k
    only = list(srt.render_despeckled(scene, cam, W, H, [5], depth, renderer=gpu, denoise=False, despeckle=dict(radius=1)))
    assert set(only[0][3]) == {"xyz", "lin", "fb", "scale", "floor", "clip"} and only[0][3]["clip"]["clamped"] > 0


# ---- the presented picture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source", ["accum", "denoise"])
def test_present_despeckled_equals_present_kat_of_the_cleaned_picture(srt, gpu, source):
    W, H = _accumulate(gpu, srt, "cornell", "features")
    ds = dict(radius=2, rank_ppm=875000, gain=4.0, floor=None)
    stage = dict(levels=2) if source == "denoise" else {}
    if source == "accum":
        cleaned = gpu.despeckle(W, H, **ds)
        picture, counters = cleaned["xyz"], cleaned["clip"]
    else:
        picture = gpu.denoise_despeckled(W, H, despeckle=ds, **stage)["xyz"]
        counters = gpu.despeckle(W, H, **ds)["clip"]
    assert counters["clamped"] >= 16
    for gain, kw in ((None, dict(percentile_ppm=700000, white=8.0)), (1.7, dict(curve="linear")), (0.6, dict())):
        got = gpu.present_despeckled(W, H, source, gain, despeckle=ds, **dict(kw, **stage))
        want = gpu.present_kat(picture, gain, **kw)
        what = "%s gain %r" % (source, gain)
        assert np.array_equal(got["rgba"], want["rgba"]), what
        assert got["clip"] == want["clip"] and got["meter"] == want["meter"] and got["despeckle"] == counters, what
    assert got["rgba"][..., :3].max() > 0 and (got["rgba"][..., 3] == 255).all()
    plain = gpu.present(W, H, source, 0.6, **stage)
    assert (plain["rgba"] != got["rgba"]).any()
    off = gpu.present_despeckled(W, H, source, 0.6, despeckle=dict(ds, floor=INF), **stage)
    assert np.array_equal(off["rgba"], plain["rgba"]) and off["clip"] == plain["clip"] and off["despeckle"]["clamped"] == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L, B = gpu_lib(), srt.binding
    good, dcfg, pcfg = srt.despeckle_config(floor=0.0), srt.denoise_config(levels=1), srt.present_config("accum", 1.0)
    res, pres = B.DespeckleResult(), B.PresentResult()
    out = np.zeros((H, W, 3), F)
    op = out.ctypes.data_as(FP)
    scale = np.zeros((H, W), F)
    sp = scale.ctypes.data_as(FP)
    img = np.ones((H, W, 3), F)
    ip = img.ctypes.data_as(FP)
    rgba = np.zeros((H, W, 4), np.uint8)
    rp = rgba.ctypes.data_as(C.POINTER(C.c_uint8))
    fresh = srt.Renderer(0)
    try:
        ms = C.c_float()
        assert L.srt_despeckle_last_ms(fresh._h, C.byref(ms)) == ERR_INVALID
        assert L.srt_despeckle_accum(fresh._h, C.byref(good), op, None, None, None, None, W, H) == ERR_INVALID      # no accumulation at all
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    expect_error(srt, lambda: gpu.despeckle(W, H, floor=0.0), ERR_INVALID, "despeckle before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first = gpu.despeckle(W, H, floor=0.0)
    frame = read_frame(gpu, W, H)

    def cfg(**kw):
        d = srt.despeckle_config(floor=0.0)
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[3] = v
            else:
                setattr(d, k, v)
        return d

    nan = float("nan")
    bad_cfgs = [dict(radius=0), dict(radius=3), dict(rank_ppm=1000001), dict(gain=-1.0), dict(gain=INF), dict(gain=nan), dict(floor=-1.0), dict(floor=nan),
                dict(floor=-INF), dict(reserved=1)]
    refused = [("accum: null cfg", lambda: L.srt_despeckle_accum(gpu._h, None, op, None, None, None, C.byref(res), W, H)),
               ("accum: nothing asked for", lambda: L.srt_despeckle_accum(gpu._h, C.byref(good), None, None, None, None, None, W, H)),
               ("accum: empty image", lambda: L.srt_despeckle_accum(gpu._h, C.byref(good), op, None, None, None, C.byref(res), W, 0)),
               ("KAT: null image", lambda: L.srt_despeckle_kat(gpu._h, C.byref(good), None, W, H, op, sp, C.byref(res))),
               ("KAT: null cfg", lambda: L.srt_despeckle_kat(gpu._h, None, ip, W, H, op, sp, C.byref(res))),
               ("KAT: nothing asked for", lambda: L.srt_despeckle_kat(gpu._h, C.byref(good), ip, W, H, None, None, None)),
               ("KAT: empty image", lambda: L.srt_despeckle_kat(gpu._h, C.byref(good), ip, 0, H, op, sp, C.byref(res))),
               ("KAT: 2^31 pixels", lambda: L.srt_despeckle_kat(gpu._h, C.byref(good), ip, 0x10000, 0x8000, op, sp, C.byref(res))),
               ("last_ms: null", lambda: L.srt_despeckle_last_ms(gpu._h, None)),
               ("chain: null despeckle cfg", lambda: L.srt_denoise_features_ds(gpu._h, None, C.byref(dcfg), op, None, None, W, H)),
               ("chain: null denoise cfg", lambda: L.srt_denoise_features_ds(gpu._h, C.byref(good), None, op, None, None, W, H)),
               ("chain: all outputs NULL", lambda: L.srt_denoise_features_ds(gpu._h, C.byref(good), C.byref(dcfg), None, None, None, W, H)),
               ("chain: bad denoise cfg", lambda: L.srt_denoise_features_ds(gpu._h, C.byref(good), C.byref(B.Denoise(9, 1.0, 1.0, 1.0, 1.0)), op, None, None, W, H)),
               ("present: null despeckle cfg", lambda: L.srt_present_despeckled(gpu._h, C.byref(pcfg), None, rp, 4 * W, W, H, C.byref(pres), C.byref(res))),
               ("present: null present cfg", lambda: L.srt_present_despeckled(gpu._h, None, C.byref(good), rp, 4 * W, W, H, C.byref(pres), C.byref(res))),
               ("present: short pitch", lambda: L.srt_present_despeckled(gpu._h, C.byref(pcfg), C.byref(good), rp, 4 * W - 1, W, H, C.byref(pres), C.byref(res)))]
    for kw in bad_cfgs:
        refused.append(("accum %r" % kw, lambda kw=kw: L.srt_despeckle_accum(gpu._h, C.byref(cfg(**kw)), op, None, None, sp, C.byref(res), W, H)))
        refused.append(("KAT %r" % kw, lambda kw=kw: L.srt_despeckle_kat(gpu._h, C.byref(cfg(**kw)), ip, W, H, op, sp, C.byref(res))))
        refused.append(("chain %r" % kw, lambda kw=kw: L.srt_denoise_features_ds(gpu._h, C.byref(cfg(**kw)), C.byref(dcfg), op, None, None, W, H)))
        refused.append(("present %r" % kw, lambda kw=kw: L.srt_present_despeckled(gpu._h, C.byref(pcfg), C.byref(cfg(**kw)), rp, 4 * W, W, H, C.byref(pres), C.byref(res))))
    unsupported = [("present: source %s" % s, lambda s=s: L.srt_present_despeckled(gpu._h, C.byref(srt.present_config(s, 1.0)), C.byref(good), rp, 4 * W, W, H,
                                                                                  C.byref(pres), C.byref(res))) for s in ("denoise_vg", "denoise_mv", "develop")]

    def untouched(what):
        assert not bits(out).any() and not bits(scale).any() and not rgba.any() and not bytes(res).strip(b"\0") and not bytes(pres).strip(b"\0"), what

    for what, call in refused:
        assert call() == ERR_INVALID, what
        untouched(what)
    for what, call in unsupported:
        assert call() == ERR_UNSUPPORTED, what
        untouched(what)
    # after all of them the accumulation despeckles, reads and continues as before
    again = gpu.despeckle(W, H, floor=0.0)
    for key in ("xyz", "lin", "fb", "scale"):
        assert_same_floats(again[key], first[key], "despeckle after the refusals, " + key)
    assert again["clip"] == first["clip"]
    assert_same_image(read_frame(gpu, W, H), frame, "after the refusals")
    assert gpu.accum_samples == 4
    gpu.render_chunk_accum(W, H, 2)
    assert gpu.accum_samples == 6
    # a partition other than (0, 1): a pixel's neighbours would be another rank's; the rank's accumulation goes on
    fresh_context(gpu, scene, cam, W, H, depth)
    try:
        gpu.set_partition(1, 2)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, 2)
        part = stack_features(gpu.read_features(W, H))
        for what, call in (("accum", lambda: L.srt_despeckle_accum(gpu._h, C.byref(good), op, None, None, sp, C.byref(res), W, H)),
                           ("chain", lambda: L.srt_denoise_features_ds(gpu._h, C.byref(good), C.byref(dcfg), op, None, None, W, H)),
                           ("present accum", lambda: L.srt_present_despeckled(gpu._h, C.byref(pcfg), C.byref(good), rp, 4 * W, W, H, C.byref(pres), C.byref(res))),
                           ("present denoise", lambda: L.srt_present_despeckled(gpu._h, C.byref(srt.present_config("denoise", 1.0)), C.byref(good), rp, 4 * W, W, H,
                                                                                C.byref(pres), C.byref(res)))):
            assert call() == ERR_UNSUPPORTED, "partition (1, 2): " + what
            untouched("partition (1, 2): " + what)
        assert np.array_equal(bits(stack_features(gpu.read_features(W, H))), bits(part)) and part[..., 7].max() > 0, "rows of rank 1 after the refusals"
        gpu.render_chunk_accum(W, H, 2)
        assert gpu.accum_samples == 4
    finally:
        gpu.set_partition(0, 1)
    # a plain accumulation has no feature rows for the chain
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    assert L.srt_denoise_features_ds(gpu._h, C.byref(good), C.byref(dcfg), op, None, None, W, H) == ERR_INVALID
    assert L.srt_present_despeckled(gpu._h, C.byref(srt.present_config("denoise", 1.0)), C.byref(good), rp, 4 * W, W, H, C.byref(pres), C.byref(res)) == ERR_INVALID
    untouched("a plain accumulation")
    # whatever ends the accumulation ends the filter
    gpu.accum_reset()
    expect_error(srt, lambda: gpu.despeckle(W, H, floor=0.0), ERR_INVALID, "despeckle after srt_accum_reset")
