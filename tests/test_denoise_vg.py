"""The variance-guided a-trous denoiser on the device (srt_denoise_features_vg / srt_denoise_vg_kat, csrc/srt_denoise.hip), bit for
bit, colour and variance: the exact cases of tests/test_denoise_vg_reference.py, the numpy float32 restatement
(tests/denoise_vg_reference.py) on synthetic inputs of every awkward size and on real featured accumulations; the placement of an
offset chunk; that the call only reads the accumulation and leaves the plain denoiser what it was; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as D
import denoise_vg_reference as V
from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, assert_same_image, convert_xyz, fresh_context, gpu_lib, lane_of, named_workload,
                           read_frame)
from features_reference import stack_features
from helpers import bits

F = np.float32
INF = float("inf")
KEYS = ("xyz", "lin", "fb", "var")


def assert_bits_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    print("%s: %d of %d values differ" % (what, len(bad), got.size))
    assert len(bad) == 0, "%s: %d of %d values differ, first at %r: got %r want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def assert_pair_equal(got, want, what):
    assert_bits_equal(got[0], want[0], what + ", xyz")
    assert_bits_equal(got[1], want[1], what + ", var")


def xyz_sums_rowmajor(gpu, frame, W, H):
    """the accumulation's XYZ sums (H, W, 3) from the block-linear parity planes of a scattered frame"""
    lane = lane_of(gpu.geom, W, H)
    return np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)


def featured_passes(gpu, scene, cam, W, H, depth, passes, offx=0, offy=0):
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    for s in passes:
        gpu.render_chunk_accum(W, H, s, offx, offy)


# ---- the exact cases on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_variance_on_the_device(gpu):
    S, rows, n, Y, var = V.integer_variance_case()
    xyz, v = gpu.denoise_vg_kat(S, rows, n, levels=0)
    assert_bits_equal(v, np.full((4, 4, 2), var, F), "population variance, both channels")
    assert_bits_equal(xyz, S, "levels 0 returns the mean")
    flat = S.copy()
    flat[..., 1] = F(3)
    assert not bits(gpu.denoise_vg_kat(flat, rows, n, levels=0)[1]).any(), "a constant image has variance +0"
    # ... and one level carries it on as the integer sums say (the restatement is held to them on the CPU)
    cfg = dict(V.VG_DEFAULTS, levels=1, variance_floor=INF)
    assert_pair_equal(gpu.denoise_vg_kat(S, rows, n, **cfg), V.denoise_vg(S, rows, n, **cfg), "one level on the integer image")


@pytest.mark.gpu
def test_an_infinite_floor_gives_the_plain_filter_on_the_device(gpu):
    def cases():
        for levels in (1, 2, 3):
            S, rows, n = D.impulse_case(45)
            yield "impulse-%d" % levels, S, rows, n, dict(levels=levels, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
        for kind in D.EDGE_KINDS:
            S, rows, n, cfg, _ = D.edge_case(kind)
            yield "edge-" + kind, S, rows, n, {k: v for k, v in cfg.items() if k != "sigma_color"}
        for h, w in ((35, 67), (9, 33), (2, 3), (4, 4)):
            S, rows, n = D.synthetic_case(h, w)
            yield "synthetic-%dx%d" % (w, h), S, rows, n, dict(levels=5, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    for name, S, rows, n, cfg in cases():
        got, _ = gpu.denoise_vg_kat(S, rows, n, variance_floor=INF, **cfg)
        assert_bits_equal(got, gpu.denoise_kat(S, rows, n, sigma_color=INF, **cfg), name + ": against the device's plain filter")
        if name.startswith("impulse"):
            exact = D.impulse_expected(45, cfg["levels"])
            for c in range(3):
                assert_bits_equal(got[..., c], exact, name + ": the integer convolution, channel %d" % c)
        else:
            assert_bits_equal(got, D.denoise(S, rows, n, sigma_color=INF, **cfg), name + ": against the plain restatement")


@pytest.mark.gpu
def test_exposure_invariance_on_the_device(gpu):
    S, rows, n = V.finite_synthetic_case(35, 67)
    cfg = dict(V.VG_DEFAULTS, sigma_variance=1.0)
    xyz, var = gpu.denoise_vg_kat(S, rows, n, **cfg)
    xyz4, var16 = gpu.denoise_vg_kat((F(4) * S).astype(F), rows, n, **dict(cfg, variance_floor=float(F(16) * F(cfg["variance_floor"]))))
    assert_pair_equal((xyz, var), V.denoise_vg(S, rows, n, **cfg), "finite synthetic input")
    assert_bits_equal(xyz4, (F(4) * xyz).astype(F), "four times brighter: xyz x 4")
    assert_bits_equal(var16, (F(16) * var).astype(F), "four times brighter: var x 16")
    pcfg, _ = D.pick_sigmas(*D.synthetic_case(35, 67))
    plain, plain4 = gpu.denoise_kat(S, rows, n, levels=5, **pcfg), gpu.denoise_kat((F(4) * S).astype(F), rows, n, levels=5, **pcfg)
    assert (bits(plain4) != bits((F(4) * plain).astype(F))).any(), "the plain filter is not expected to be exposure invariant"


@pytest.mark.gpu
def test_non_finite_pixels_on_the_device(gpu):
    S, rows, n, bad = V.non_finite_case()
    xyz, var = gpu.denoise_vg_kat(S, rows, n, **V.VG_DEFAULTS)
    good = np.ones(S.shape[:2], bool)
    for y, x in bad:
        good[y, x] = False
        assert_bits_equal(xyz[y, x], S[y, x], "the non-finite pixel at %r keeps its colour" % ((y, x),))
    assert np.isfinite(xyz[good]).all() and np.isfinite(var).all()
    assert_bits_equal(var[..., 0], V.non_finite_case_variance(S), "the estimate from the finite pixels of each window")
    assert_pair_equal((xyz, var), V.denoise_vg(S, rows, n, **V.VG_DEFAULTS), "non-finite case")


# ---- synthetic input against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(67, 35), (33, 9), (1, 1), (1, 9), (9, 1), (3, 2), (4, 4)], ids=lambda v: str(v))
def test_synthetic_input_equals_the_restatement(gpu, w, h):
    S, rows, n = D.synthetic_case(h, w)
    sv = 1.0
    if (w, h) in ((67, 35), (33, 9)):
        sv, st = V.pick_sigma_variance(S, rows, n)      # picked on the restatement alone
        print("level 0 at sigma_variance %r: %r" % (sv, st))
        assert 4 * st["accepted"] >= st["taps"] and 4 * st["rejected"] >= st["taps"], st
        assert np.isnan(S).sum() == 1 and np.isinf(S).sum() == 1
    cfg = dict(V.VG_DEFAULTS, sigma_variance=sv)
    for levels in (0, 1, 2, 3, 4, 5, 8):
        want = V.denoise_vg(S, rows, n, **dict(cfg, levels=levels))
        got = gpu.denoise_vg_kat(S, rows, n, **dict(cfg, levels=levels))
        assert_pair_equal(got, want, "%d x %d, %d levels" % (w, h, levels))
        if levels == 0:
            assert_bits_equal(got[1][..., 0], got[1][..., 1], "levels 0: both variance channels")
    if h * w >= 6:
        assert np.isnan(got[0]).sum() == 1 and np.isinf(got[0]).sum() == 1 and np.isfinite(got[1]).all()
        assert (got[1][..., 0] > 0).any(), "the NaN pixel zeroed the estimate"


# ---- real workloads against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dielectric", "random_spheres", "cornell"])
def test_real_workloads_equal_the_restatement(srt, gpu, orc, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    featured_passes(gpu, scene, cam, W, H, depth, [4, 4, 4])
    frame = read_frame(gpu, W, H)
    S = xyz_sums_rowmajor(gpu, frame, W, H)
    rows = stack_features(gpu.read_features(W, H))
    n = gpu.accum_samples
    assert n == 12
    want, want_var = V.denoise_vg(S, rows, n, **V.VG_DEFAULTS)
    got = gpu.denoise_vg(W, H)
    assert set(got) == set(KEYS) and all(got[k].shape == (H, W, 3) and got[k].dtype == F for k in KEYS[:3]) and got["var"].shape == (H, W, 2)
    assert_bits_equal(got["xyz"], want, name + " filtered XYZ")
    assert_bits_equal(got["var"], want_var, name + " variance")
    lin, q = convert_xyz(orc, [np.ascontiguousarray(want[..., c]).ravel() for c in range(3)], 1)
    assert_bits_equal(got["lin"], np.stack(lin, axis=-1).reshape(H, W, 3), name + " unquantised sRGB")
    assert_bits_equal(got["fb"], np.stack(q, axis=-1).reshape(H, W, 3), name + " quantised sRGB")
    mean = D.denoise(S, rows, n, levels=0)
    changed = int((bits(want) != bits(mean)).any(axis=-1).sum())
    differs = int((bits(got["xyz"]) != bits(gpu.denoise(W, H)["xyz"])).any(axis=-1).sum())
    print("%s: the filter changed %d of %d pixels; %d differ from the plain denoiser's default result" % (name, changed, W * H, differs))
    if name in ("dielectric", "random_spheres"):
        assert 4 * changed >= W * H, "%s: the filter was inert (%d of %d pixels changed)" % (name, changed, W * H)
        assert differs > 0, name + ": the same result as the plain denoiser"
    assert_same_image(read_frame(gpu, W, H), frame, name + " frame after denoise")


# ---- placement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_offset_chunk_placement(srt, gpu):
    """a 30 x 21 chunk (no multiple of 8 x 8, 28 x 16 or 32 x 8) at (17, 9) of a 64 x 40 image: the placement of read_features"""
    scene, _, _, _, depth, _ = named_workload(srt, "random_spheres")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    featured_passes(gpu, scene, cam, cw, ch, depth, [1, 2], ox, oy)
    S = xyz_sums_rowmajor(gpu, read_frame(gpu, IW, IH), cw, ch)
    rows = stack_features(gpu.read_features(IW, IH))[oy:oy + ch, ox:ox + cw]
    want = V.denoise_vg(S, rows, 3, **V.VG_DEFAULTS)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    got = gpu.denoise_vg(IW, IH)
    for k in KEYS:
        assert not bits(got[k][~inside]).any(), k + ": written outside the chunk's rectangle"
    assert_pair_equal((got["xyz"][oy:oy + ch, ox:ox + cw], got["var"][oy:oy + ch, ox:ox + cw]), want, "offset chunk")
    # the library writes nothing outside: a sentinel survives; and the variance alone is enough of an output
    sentinel = F(-7.0)
    out = np.full((IH, IW, 2), sentinel, F)
    cfg = srt.denoise_vg_config()
    gpu._ck(gpu_lib().srt_denoise_features_vg(gpu._h, C.byref(cfg), None, None, None, srt.binding.fptr(out), IW, IH))
    assert (out[~inside] == sentinel).all() and np.array_equal(bits(out[inside]), bits(got["var"][inside]))


# ---- the call only reads, and the plain denoiser is what it was -----------------------------------------------------------------------
@pytest.mark.gpu
def test_denoise_vg_does_not_interfere(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")

    def run(with_denoise):
        featured_passes(gpu, scene, cam, W, H, depth, [4])
        plain_before = vg = plain_after = None
        if with_denoise:
            plain_before = gpu.denoise(W, H)
            ms_plain = gpu.denoise_last_ms()
            assert gpu_lib().srt_denoise_estimate_last_ms(gpu._h, C.byref(C.c_float())) == ERR_INVALID      # the last denoise was plain
            vg = gpu.denoise_vg(W, H)
            ms = gpu.denoise_last_ms()
            assert len(ms["levels"]) == 5 and min(ms["levels"] + [ms["prepass"], ms["epilogue"], gpu.denoise_estimate_last_ms()]) > 0.0, ms
            plain_after = gpu.denoise(W, H)
            assert len(ms_plain["levels"]) == len(gpu.denoise_last_ms()["levels"]) == 5
            assert gpu_lib().srt_denoise_estimate_last_ms(gpu._h, C.byref(C.c_float())) == ERR_INVALID
        gpu.render_chunk_accum(W, H, 4)
        frame = read_frame(gpu, W, H)
        rows = stack_features(gpu.read_features(W, H))
        den = gpu.denoise_vg(W, H)
        gpu.render_chunk(W, H)                # one more plain pass: continues every pixel's RNG stream
        return frame, rows, read_frame(gpu, W, H), plain_before, vg, plain_after, den

    frame_a, rows_a, after_a, plain_before, vg, plain_after, den_a = run(True)
    frame_b, rows_b, after_b, _, _, _, den_b = run(False)
    assert_same_image(frame_a, frame_b, "[4], denoise_vg, [4] against [4, 4]")
    assert_bits_equal(rows_a, rows_b, "feature rows")
    assert_same_image(after_a, after_b, "RNG state: a plain launch after the passes")
    for k in ("xyz", "lin", "fb"):
        assert_bits_equal(plain_before[k], plain_after[k], "plain, variance-guided, plain: the plain result, " + k)
    for k in KEYS:
        assert_bits_equal(den_a[k], den_b[k], "denoise_vg after 8 samples, " + k)
    assert (bits(vg["xyz"]) != bits(den_a["xyz"])).any() and (bits(vg["xyz"]) != bits(plain_before["xyz"])).any()


@pytest.mark.gpu
def test_the_working_buffers_regrow(srt):
    """a context of its own whose first denoise is a small plain one: the variance-guided one needs larger images, and so does the
    larger rectangle; the small ones still match afterwards"""
    r = srt.Renderer(0)
    try:
        small = D.synthetic_case(5, 7)
        large = D.synthetic_case(35, 67)
        cfg = dict(V.VG_DEFAULTS, levels=4, sigma_variance=1.0)
        assert gpu_lib().srt_denoise_estimate_last_ms(r._h, C.byref(C.c_float())) == ERR_INVALID      # nothing has run on this context yet
        assert_bits_equal(r.denoise_kat(*small, levels=4), D.denoise(*small, levels=4), "plain, small")
        for S, rows, n in (small, large, small):
            assert_pair_equal(r.denoise_vg_kat(S, rows, n, **cfg), V.denoise_vg(S, rows, n, **cfg), "%r" % (S.shape,))
        assert r.denoise_estimate_last_ms() > 0.0 and len(r.denoise_last_ms()["levels"]) == 4
        assert_bits_equal(r.denoise_kat(*large, levels=4), D.denoise(*large, levels=4), "plain, large")
        scene, cam, W, H, depth, _ = named_workload(srt, "prism")
        for w, h in ((20, 12), (W, H), (20, 12)):
            cm = scene.default_camera(w, h)
            featured_passes(r, scene, cm, w, h, depth, [3])
            S = xyz_sums_rowmajor(r, read_frame(r, w, h), w, h)
            want = V.denoise_vg(S, stack_features(r.read_features(w, h)), 3, **V.VG_DEFAULTS)
            got = r.denoise_vg(w, h)
            assert_pair_equal((got["xyz"], got["var"]), want, "chunk %d x %d" % (w, h))
    finally:
        r.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_accumulation_as_it_was(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    out = np.zeros((H, W, 3), F)
    fp = srt.binding.fptr(out)
    good = srt.denoise_vg_config()

    def call(cfg, a=fp, b=fp, c=fp, d=fp, ctx=None):
        return L.srt_denoise_features_vg(gpu._h if ctx is None else ctx, C.byref(cfg) if cfg is not None else None, a, b, c, d, W, H)

    def cfg_with(**kw):
        c = srt.denoise_vg_config()
        for k, v in kw.items():
            if k == "reserved":
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        return c

    # no featured accumulation with a pass: none at all, a plain one, a featured one before its first pass
    fresh_context(gpu, scene, cam, W, H, depth)
    assert call(good) == ERR_INVALID
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    assert call(good) == ERR_INVALID
    fresh_context(gpu, scene, cam, W, H, depth)      # (seeds the RNG streams again: the run below is compared with a fresh [2, 4])
    gpu.accum_reset_features()
    assert call(good) == ERR_INVALID
    gpu.render_chunk_accum(W, H, 2)
    frame = read_frame(gpu, W, H)
    rows = stack_features(gpu.read_features(W, H))
    want = gpu.denoise_vg(W, H)

    assert L.srt_denoise_features_vg(None, C.byref(good), fp, fp, fp, fp, W, H) == ERR_INVALID
    assert call(None) == ERR_INVALID
    assert call(good, None, None, None, None) == ERR_INVALID
    assert L.srt_denoise_features_vg(gpu._h, C.byref(good), fp, fp, fp, fp, 0, H) == ERR_INVALID
    assert call(cfg_with(levels=9)) == ERR_INVALID
    for bad in (float("nan"), 0.0, -0.0, -1.0, -INF, INF):
        assert call(cfg_with(sigma_variance=bad)) == ERR_INVALID, ("sigma_variance", bad)
    for field in ("sigma_normal", "sigma_albedo", "sigma_depth", "variance_floor"):
        for bad in (float("nan"), 0.0, -0.0, -1.0, -INF):
            assert call(cfg_with(**{field: bad})) == ERR_INVALID, (field, bad)
        assert call(cfg_with(**{field: INF})) == 0, field
    for k in range(2):
        assert call(cfg_with(reserved=k)) == ERR_INVALID
    assert call(cfg_with(levels=8)) == 0 and call(cfg_with(levels=0)) == 0
    # the plain entry point still refuses a non-zero reserved word, the one that overlays variance_floor's neighbour included
    plain = srt.denoise_config()
    for k in range(3):
        plain.reserved[k] = 1
        assert L.srt_denoise_features(gpu._h, C.byref(plain), fp, fp, fp, W, H) == ERR_INVALID
        plain.reserved[k] = 0
    # nothing of the above changed the accumulation: the same denoise, the same rows, and the passes go on
    again = gpu.denoise_vg(W, H)
    for k in KEYS:
        assert_bits_equal(again[k], want[k], "after the refusals, " + k)
    assert_bits_equal(stack_features(gpu.read_features(W, H)), rows, "rows after the refusals")
    assert_same_image(read_frame(gpu, W, H), frame, "frame after the refusals")
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == 6
    cont = read_frame(gpu, W, H)
    cont_rows = stack_features(gpu.read_features(W, H))
    featured_passes(gpu, scene, cam, W, H, depth, [2, 4])
    assert_same_image(cont, read_frame(gpu, W, H), "continued after the refusals")
    assert_bits_equal(cont_rows, stack_features(gpu.read_features(W, H)), "rows continued after the refusals")

    # a rank of a larger world: unsupported, and its accumulation goes on
    fresh_context(gpu, scene, cam, W, H, depth)
    try:
        gpu.set_partition(1, 2)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, 2)
        part = stack_features(gpu.read_features(W, H))
        assert call(good) == ERR_UNSUPPORTED
        assert_bits_equal(stack_features(gpu.read_features(W, H)), part, "rows of rank 1 after the refusal")
        gpu.render_chunk_accum(W, H, 2)
        assert gpu.accum_samples == 4
    finally:
        gpu.set_partition(0, 1)

    # the KAT entry point checks the same configuration, and its own arguments
    S, r8, n = D.synthetic_case(3, 5)
    var = np.zeros((3, 5, 2), F)
    vp = srt.binding.fptr(var)
    P = lambda a: srt.binding.fptr(a) if a is not None else None
    kat = lambda cfg, s=S, r=r8, n=n, w=5, h=3, o=fp, v=vp: L.srt_denoise_vg_kat(gpu._h, C.byref(cfg), P(s), P(r), n, w, h, o, v)
    assert kat(good) == 0
    assert kat(cfg_with(levels=9)) == ERR_INVALID and kat(cfg_with(sigma_depth=0.0)) == ERR_INVALID and kat(cfg_with(reserved=1)) == ERR_INVALID
    assert kat(cfg_with(sigma_variance=INF)) == ERR_INVALID and kat(cfg_with(variance_floor=0.0)) == ERR_INVALID
    assert kat(good, s=None) == ERR_INVALID and kat(good, r=None) == ERR_INVALID and kat(good, o=None) == ERR_INVALID and kat(good, v=None) == ERR_INVALID
    assert kat(good, n=0) == ERR_INVALID and kat(good, w=0) == ERR_INVALID and kat(good, h=0) == ERR_INVALID
    assert L.srt_denoise_vg_kat(None, C.byref(good), P(S), P(r8), n, 5, 3, fp, vp) == ERR_INVALID
    with pytest.raises(ValueError):
        gpu.denoise_vg_kat(S, r8[:, :4], n)


@pytest.mark.gpu
def test_render_denoised_yields_what_the_manual_calls_give(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    steps = list(srt.render_denoised(scene, cam, W, H, [4, 8], depth, renderer=gpu, variance_guided=True, levels=3, sigma_variance=1.5))
    assert [s[0] for s in steps] == [4, 12]
    plain = list(srt.render_features(scene, cam, W, H, [4, 8], depth, renderer=gpu))
    cfg = dict(V.VG_DEFAULTS, levels=3, sigma_variance=1.5)
    for (t, res, feat, den), (t2, res2, feat2) in zip(steps, plain):
        assert t == t2 and set(den) == set(KEYS)
        assert_same_image(res, res2, "render_denoised vs render_features at %d" % t)
        assert_bits_equal(stack_features(feat), stack_features(feat2), "features at %d" % t)
        lane = lane_of(res["geom"], W, H)
        S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in res["xyz"]], axis=-1)
        assert_pair_equal((den["xyz"], den["var"]), V.denoise_vg(S, stack_features(feat), t, **cfg), "denoised at %d" % t)
