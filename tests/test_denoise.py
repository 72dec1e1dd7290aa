"""The a-trous denoiser on the device (srt_denoise_features / srt_denoise_kat, csrc/srt_denoise.hip), bit for bit: against exact
arithmetic on the impulse and edge cases, against the numpy float32 restatement (tests/denoise_reference.py, itself held to exact
arithmetic by tests/test_denoise_reference.py) on synthetic inputs of every awkward size and on real featured accumulations; the
placement of an offset chunk; that the call only reads the accumulation; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as D
from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, assert_same_image, convert_xyz, fresh_context, gpu_lib, lane_of, named_workload,
                           read_frame)
from features_reference import stack_features
from helpers import bits

F = np.float32
INF = float("inf")


def assert_bits_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    print("%s: %d of %d values differ" % (what, len(bad), got.size))
    assert len(bad) == 0, "%s: %d of %d values differ, first at %r: got %r want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def xyz_sums_rowmajor(gpu, frame, W, H):
    """the accumulation's XYZ sums (H, W, 3) from the block-linear parity planes of a scattered frame"""
    lane = lane_of(gpu.geom, W, H)
    return np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)


def featured_passes(gpu, scene, cam, W, H, depth, passes, offx=0, offy=0):
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    for s in passes:
        gpu.render_chunk_accum(W, H, s, offx, offy)


# ---- exact arithmetic on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_impulse_response_on_the_device(gpu, levels):
    S, rows, n = D.impulse_case(45)
    want = D.impulse_expected(45, levels)
    got = gpu.denoise_kat(S, rows, n, levels=levels, sigma_color=INF)
    for c in range(3):
        assert_bits_equal(got[..., c], want, "impulse, %d levels, channel %d" % (levels, c))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", D.EDGE_KINDS)
def test_edge_stop_on_the_device(gpu, kind):
    S, rows, n, cfg, split = D.edge_case(kind)
    got = gpu.denoise_kat(S, rows, n, **cfg)
    assert (bits(got[:, split:]) == 0).all(), "%s edge: %d values of the right half are not +0" % (kind, int((bits(got[:, split:]) != 0).sum()))
    assert (got[:, split - 1] > 0).any()
    assert_bits_equal(got, D.denoise(S, rows, n, **cfg), kind + " edge against the restatement")


# ---- synthetic input against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(67, 35), (1, 1), (1, 9), (9, 1), (3, 2)], ids=lambda v: str(v))
def test_synthetic_input_equals_the_restatement(gpu, w, h):
    S, rows, n = D.synthetic_case(h, w)
    big = D.synthetic_case(35, 67)
    cfg, st = D.pick_sigmas(*big)      # the sigmas of every size are those picked on the 67 x 35 input
    if (w, h) == (67, 35):
        hits = rows[..., 7]
        assert (hits == 0).any() and ((hits > 0) & (hits < n)).any() and np.isnan(S).sum() == 1 and np.isinf(S).sum() == 1
        print("level 0 at %r: %r" % (cfg, st))
        assert 4 * st["taken"] >= st["taps"] and 4 * st["skipped"] >= st["taps"], st
    for levels in (0, 1, 2, 3, 4, 5, 8):
        want = D.denoise(S, rows, n, levels=levels, **cfg)
        got = gpu.denoise_kat(S, rows, n, levels=levels, **cfg)
        assert_bits_equal(got, want, "%d x %d, %d levels" % (w, h, levels))
    if (w, h) == (67, 35):
        assert np.isnan(got).sum() == 1 and np.isinf(got).sum() == 1      # the two pixels keep what they hold, nobody else takes it in


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
    want = D.denoise(S, rows, n, **D.DEFAULTS)
    got = gpu.denoise(W, H)
    assert set(got) == {"xyz", "lin", "fb"} and all(v.shape == (H, W, 3) and v.dtype == F for v in got.values())
    assert_bits_equal(got["xyz"], want, name + " filtered XYZ")
    lin, q = convert_xyz(orc, [np.ascontiguousarray(want[..., c]).ravel() for c in range(3)], 1)
    assert_bits_equal(got["lin"], np.stack(lin, axis=-1).reshape(H, W, 3), name + " unquantised sRGB")
    assert_bits_equal(got["fb"], np.stack(q, axis=-1).reshape(H, W, 3), name + " quantised sRGB")
    mean = D.denoise(S, rows, n, levels=0)
    changed = int((bits(want) != bits(mean)).any(axis=-1).sum())
    print("%s: the filter changed %d of %d pixels" % (name, changed, W * H))
    if name in ("dielectric", "random_spheres"):
        assert 4 * changed >= W * H, "%s: the filter was inert (%d of %d pixels changed)" % (name, changed, W * H)
    assert changed > 0
    # the frame itself is what it was
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
    assert rows[..., 7].max() > 0
    want = D.denoise(S, rows, 3, **D.DEFAULTS)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    got = gpu.denoise(IW, IH)
    for k in ("xyz", "lin", "fb"):
        assert not bits(got[k][~inside]).any(), k + ": written outside the chunk's rectangle"
    assert_bits_equal(got["xyz"][oy:oy + ch, ox:ox + cw], want, "offset chunk")
    # the library writes nothing outside: a sentinel survives; and a single output is enough
    sentinel = F(-7.0)
    out = np.full((IH, IW, 3), sentinel, F)
    cfg = srt.denoise_config()
    gpu._ck(gpu_lib().srt_denoise_features(gpu._h, C.byref(cfg), None, None, srt.binding.fptr(out), IW, IH))
    assert (out[~inside] == sentinel).all() and np.array_equal(bits(out[inside]), bits(got["fb"][inside]))


# ---- the call only reads --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_denoise_does_not_interfere(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")

    def run(with_denoise):
        featured_passes(gpu, scene, cam, W, H, depth, [4])
        first = second = None
        if with_denoise:
            first = gpu.denoise(W, H)
            second = gpu.denoise(W, H)
        gpu.render_chunk_accum(W, H, 4)
        frame = read_frame(gpu, W, H)
        rows = stack_features(gpu.read_features(W, H))
        den = gpu.denoise(W, H)
        gpu.render_chunk(W, H)                # one more plain pass: continues every pixel's RNG stream
        return frame, rows, read_frame(gpu, W, H), first, second, den

    frame_a, rows_a, after_a, first, second, den_a = run(True)
    frame_b, rows_b, after_b, _, _, den_b = run(False)
    assert_same_image(frame_a, frame_b, "[4], denoise, [4] against [4, 4]")
    assert_bits_equal(rows_a, rows_b, "feature rows")
    assert_same_image(after_a, after_b, "RNG state: a plain launch after the passes")
    for k in ("xyz", "lin", "fb"):
        assert_bits_equal(first[k], second[k], "denoise twice, " + k)
        assert_bits_equal(den_a[k], den_b[k], "denoise after 8 samples, " + k)
    assert (bits(first["xyz"]) != bits(den_a["xyz"])).any()


@pytest.mark.gpu
def test_the_working_buffers_regrow(srt):
    """a context of its own whose first denoise is a small rectangle: the larger one must get larger images, and the small one still matches"""
    r = srt.Renderer(0)
    try:
        small = D.synthetic_case(5, 7)
        large = D.synthetic_case(35, 67)
        cfg, _ = D.pick_sigmas(*large)
        assert gpu_lib().srt_denoise_last_ms(r._h, None, None, None, None) == ERR_INVALID      # nothing has run on this context yet
        for S, rows, n in (small, large, small):
            assert_bits_equal(r.denoise_kat(S, rows, n, levels=4, **cfg), D.denoise(S, rows, n, levels=4, **cfg), "%r" % (S.shape,))
        ms = r.denoise_last_ms()
        assert len(ms["levels"]) == 4 and min(ms["levels"] + [ms["prepass"], ms["epilogue"]]) > 0.0, ms
        scene, cam, W, H, depth, _ = named_workload(srt, "prism")
        for w, h in ((20, 12), (W, H), (20, 12)):
            cm = scene.default_camera(w, h)
            featured_passes(r, scene, cm, w, h, depth, [3])
            S = xyz_sums_rowmajor(r, read_frame(r, w, h), w, h)
            want = D.denoise(S, stack_features(r.read_features(w, h)), 3, **D.DEFAULTS)
            assert_bits_equal(r.denoise(w, h)["xyz"], want, "chunk %d x %d" % (w, h))
    finally:
        r.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_accumulation_as_it_was(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    out = np.zeros((H, W, 3), F)
    fp = srt.binding.fptr(out)
    good = srt.denoise_config()

    def call(cfg, a=fp, b=fp, c=fp, ctx=None):
        return L.srt_denoise_features(gpu._h if ctx is None else ctx, C.byref(cfg) if cfg is not None else None, a, b, c, W, H)

    def cfg_with(**kw):
        c = srt.denoise_config()
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
    want = gpu.denoise(W, H)

    assert L.srt_denoise_features(None, C.byref(good), fp, fp, fp, W, H) == ERR_INVALID
    assert call(None) == ERR_INVALID
    assert call(good, None, None, None) == ERR_INVALID
    assert call(cfg_with(levels=9)) == ERR_INVALID
    for field in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        for bad in (float("nan"), 0.0, -0.0, -1.0, -INF):
            assert call(cfg_with(**{field: bad})) == ERR_INVALID, (field, bad)
        assert call(cfg_with(**{field: INF})) == 0, field
    for k in range(3):
        assert call(cfg_with(reserved=k)) == ERR_INVALID
    assert call(cfg_with(levels=8)) == 0 and call(cfg_with(levels=0)) == 0
    # nothing of the above changed the accumulation: the same denoise, the same rows, and the passes go on
    again = gpu.denoise(W, H)
    for k in ("xyz", "lin", "fb"):
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
    kat = lambda cfg, s=S, r=r8, n=n, w=5, h=3, o=fp: L.srt_denoise_kat(gpu._h, C.byref(cfg), srt.binding.fptr(s) if s is not None else None,
                                                                      srt.binding.fptr(r) if r is not None else None, n, w, h, o)
    assert kat(good) == 0
    assert kat(cfg_with(levels=9)) == ERR_INVALID and kat(cfg_with(sigma_depth=0.0)) == ERR_INVALID and kat(cfg_with(reserved=2)) == ERR_INVALID
    assert kat(good, s=None) == ERR_INVALID and kat(good, r=None) == ERR_INVALID and kat(good, o=None) == ERR_INVALID
    assert kat(good, n=0) == ERR_INVALID and kat(good, w=0) == ERR_INVALID and kat(good, h=0) == ERR_INVALID
    assert L.srt_denoise_kat(None, C.byref(good), srt.binding.fptr(S), srt.binding.fptr(r8), n, 5, 3, fp) == ERR_INVALID
    with pytest.raises(ValueError):
        gpu.denoise_kat(S, r8[:, :4], n)


@pytest.mark.gpu
def test_render_denoised_yields_what_the_manual_calls_give(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    steps = list(srt.render_denoised(scene, cam, W, H, [4, 8], depth, renderer=gpu, levels=3))
    assert [s[0] for s in steps] == [4, 12]
    plain = list(srt.render_features(scene, cam, W, H, [4, 8], depth, renderer=gpu))
    for (t, res, feat, den), (t2, res2, feat2) in zip(steps, plain):
        assert t == t2
        assert_same_image(res, res2, "render_denoised vs render_features at %d" % t)
        assert_bits_equal(stack_features(feat), stack_features(feat2), "features at %d" % t)
        lane = lane_of(res["geom"], W, H)
        S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in res["xyz"]], axis=-1)
        assert_bits_equal(den["xyz"], D.denoise(S, stack_features(feat), t, **dict(D.DEFAULTS, levels=3)), "denoised at %d" % t)
