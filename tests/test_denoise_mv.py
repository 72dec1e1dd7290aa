"""The denoisers on an adaptive featured accumulation, on the device (csrc/srt_denoise.hip: denoise_prepass_counts_kernel,
denoise_measured_kernel), bit for bit against tests/denoise_mv_reference.py: srt_denoise_mv_kat on synthetic inputs of every awkward
size with a per-pixel sample map, the exact integer case, the +inf floor identity and the exposure scaling; srt_denoise_features, _vg
and _mv on real adaptive featured runs, fed from read_features, the XYZ sums and accum_stats; at a tolerance no pixel meets the first
two equal the same calls on a plain featured accumulation; the call only reads; every refusal; and render_adaptive_denoised."""
import ctypes as C

import numpy as np
import pytest

import denoise_mv_reference as M
import denoise_vg_reference as V
from accum_helpers import ERR_INVALID, ERR_UNSUPPORTED, NEVER, assert_same_image, fresh_context, gpu_lib, lane_of, named_workload, read_frame
from features_reference import stack_features
from helpers import bits

F = np.float32
INF = float("inf")
KEYS = ("xyz", "lin", "fb", "var")


def assert_bits_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(np.ascontiguousarray(got)) != bits(np.ascontiguousarray(want)))
    print("%s: %d of %d values differ" % (what, len(bad), got.size))
    assert len(bad) == 0, "%s: %d of %d values differ, first at %r: got %r want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def assert_pair_equal(got, want, what):
    assert_bits_equal(got[0], want[0], what + ", xyz")
    assert_bits_equal(got[1], want[1], what + ", var")


def adaptive_featured_passes(gpu, scene, cam, W, H, depth, rel, passes, min_spp=4):
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(rel, 0.0, min_spp)
    for s in passes:
        gpu.render_chunk_accum(W, H, s)


def accumulation_inputs(gpu, W, H):
    """(frame, S (H, W, 3), rows (H, W, 8), samples (H, W), sum_y2 (H, W)) of the context's adaptive featured accumulation"""
    frame = read_frame(gpu, W, H)
    lane = lane_of(gpu.geom, W, H)
    S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)
    st = gpu.accum_stats(W, H)
    assert_bits_equal(st["sum_y"].reshape(H, W), S[..., 1], "S1 is the Y sum")
    return frame, S, stack_features(gpu.read_features(W, H)), st["samples"].reshape(H, W), st["sum_y2"].reshape(H, W)


# ---- synthetic input ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_measured_variance_on_the_device(gpu):
    S, rows, n, s2, _, var = M.integer_measured_case()
    xyz, v = gpu.denoise_mv_kat(S, rows, n, s2, levels=0)
    assert_bits_equal(v, np.stack([var, var], axis=-1), "the rational variance of the mean, both channels")
    assert_bits_equal(xyz, M.prepass_counts(S, rows, n)[0], "levels 0 returns the per-pixel mean")
    cfg = dict(V.VG_DEFAULTS, levels=2, sigma_variance=1.0)
    assert_pair_equal(gpu.denoise_mv_kat(S, rows, n, s2, **cfg), M.denoise_mv(S, rows, n, s2, **cfg), "two levels on the integer image")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(67, 35), (33, 9), (1, 1), (1, 9), (9, 1), (3, 2), (4, 4)], ids=lambda v: str(v))
def test_synthetic_input_equals_the_restatement(gpu, w, h):
    S, rows, n, s2 = M.varying_case(h, w)
    if h * w >= 12:
        assert (n == 1).any() and (n == 2).any() and len(np.unique(n)) >= 4
        assert np.isnan(S).sum() == 1 and np.isinf(S).sum() == 1 and np.isinf(s2).sum() == 1      # the non-finite pixels
    cfg = dict(V.VG_DEFAULTS, sigma_variance=1.0)
    for levels in (0, 1, 2, 3, 5, 8):
        want = M.denoise_mv(S, rows, n, s2, **dict(cfg, levels=levels))
        got = gpu.denoise_mv_kat(S, rows, n, s2, **dict(cfg, levels=levels))
        assert_pair_equal(got, want, "%d x %d, %d levels" % (w, h, levels))
        if levels == 0:
            assert_bits_equal(got[1][..., 0], M.measured_variance(S[..., 1], s2, n), "levels 0: the estimate")
            assert_bits_equal(got[1][..., 0], got[1][..., 1], "levels 0: both variance channels")
    assert np.isfinite(got[1]).all()
    if h * w >= 12:
        assert np.isnan(got[0]).sum() == 1 and np.isinf(got[0]).sum() == 1
        v0 = got[1][..., 0]
        assert (v0 > 0).any() and not bits(v0[n == 1]).any() and (v0[n == 2] > 0).any()


@pytest.mark.gpu
def test_an_infinite_floor_gives_the_plain_filter_on_the_device(gpu):
    for h, w in ((35, 67), (9, 33), (2, 3)):
        S, rows, n, s2 = M.varying_case(h, w)
        cfg = dict(levels=5, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
        got, _ = gpu.denoise_mv_kat(S, rows, n, s2, variance_floor=INF, **cfg)
        assert_bits_equal(got, M.denoise_counts(S, rows, n, sigma_color=INF, **cfg), "%d x %d: against the plain restatement" % (w, h))
    # a uniform map: the device's own plain filter with the scalar count
    S, rows, n, s2 = M.varying_case(9, 33)
    got, _ = gpu.denoise_mv_kat(S, rows, np.full(n.shape, 6, np.uint32), s2, variance_floor=INF, **cfg)
    assert_bits_equal(got, gpu.denoise_kat(S, rows, 6, sigma_color=INF, **cfg), "uniform map: against the device's plain filter")


@pytest.mark.gpu
def test_exposure_invariance_on_the_device(gpu):
    S, rows, n, s2 = M.varying_case(35, 67, finite=True)
    cfg = dict(V.VG_DEFAULTS, sigma_variance=1.0)
    xyz, var = gpu.denoise_mv_kat(S, rows, n, s2, **cfg)
    xyz4, var16 = gpu.denoise_mv_kat((F(4) * S).astype(F), rows, n, (F(16) * s2).astype(F), **dict(cfg, variance_floor=float(F(16) * F(cfg["variance_floor"]))))
    assert_pair_equal((xyz, var), M.denoise_mv(S, rows, n, s2, **cfg), "finite synthetic input")
    assert_bits_equal(xyz4, (F(4) * xyz).astype(F), "sums x 4, S2 x 16, floor x 16: xyz x 4")
    assert_bits_equal(var16, (F(16) * var).astype(F), "sums x 4, S2 x 16, floor x 16: var x 16")


# ---- real adaptive featured runs --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,rel", [("dielectric", 0.1), ("random_spheres", 0.05)])
def test_real_adaptive_runs_equal_the_restatements(srt, gpu, name, rel):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    adaptive_featured_passes(gpu, scene, cam, W, H, depth, rel, [4, 4, 4])
    frame, S, rows, n, s2 = accumulation_inputs(gpu, W, H)
    print("%s: counts %r" % (name, dict(zip(*np.unique(n, return_counts=True)))))
    assert len(np.unique(n)) >= 2 and n.min() >= 4 and gpu.accum_active > 0       # the per-pixel count matters, and some pixel still runs
    got = gpu.denoise(W, H)
    assert_bits_equal(got["xyz"], M.denoise_counts(S, rows, n), name + " plain")
    assert (bits(got["xyz"]) != bits(M.denoise_counts(S, rows, np.full((H, W), 12, np.uint32)))).any(), "the global total would have done"
    got = gpu.denoise_vg(W, H)
    assert_pair_equal((got["xyz"], got["var"]), M.denoise_vg_counts(S, rows, n, **V.VG_DEFAULTS), name + " spatial variance")
    got = gpu.denoise_mv(W, H)
    assert set(got) == set(KEYS) and all(got[k].shape == (H, W, 3) and got[k].dtype == F for k in KEYS[:3]) and got["var"].shape == (H, W, 2)
    want = M.denoise_mv(S, rows, n, s2, **V.VG_DEFAULTS)
    assert_pair_equal((got["xyz"], got["var"]), want, name + " measured variance")
    assert_bits_equal(got["var"][..., 0], M.measured_variance(S[..., 1], s2, n), name + " the estimate")
    print("%s: the measured variance is > 0 at %d of %d pixels" % (name, int((got["var"][..., 0] > 0).sum()), W * H))
    assert (got["var"][..., 0] > 0).any() and (bits(got["var"][..., 0]) != bits(gpu.denoise_vg(W, H)["var"][..., 0])).any()
    assert gpu.denoise_estimate_last_ms() > 0.0
    # the +inf floor identity on the accumulation
    cfg = dict(levels=5, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    assert_bits_equal(gpu.denoise_mv(W, H, variance_floor=INF, **cfg)["xyz"], gpu.denoise(W, H, sigma_color=INF, **cfg)["xyz"], name + " +inf floor")
    assert_same_image(read_frame(gpu, W, H), frame, name + " frame after the denoises")


@pytest.mark.gpu
def test_at_never_the_existing_denoisers_give_what_a_plain_featured_accumulation_gives(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    adaptive_featured_passes(gpu, scene, cam, W, H, depth, NEVER, [4, 8], min_spp=12)      # (min_spp = the total: no pixel can stop early)
    assert (gpu.accum_stats(W, H)["samples"] == 12).all()
    a_plain, a_vg, a_mv = gpu.denoise(W, H), gpu.denoise_vg(W, H), gpu.denoise_mv(W, H)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    for s in (4, 8):
        gpu.render_chunk_accum(W, H, s)
    b_plain, b_vg = gpu.denoise(W, H), gpu.denoise_vg(W, H)
    for k in KEYS[:3]:
        assert_bits_equal(a_plain[k], b_plain[k], "plain denoise, " + k)
    for k in KEYS:
        assert_bits_equal(a_vg[k], b_vg[k], "variance-guided denoise, " + k)
    assert (bits(a_mv["var"][..., 0]) != bits(a_vg["var"][..., 0])).any()


@pytest.mark.gpu
def test_denoise_mv_does_not_interfere(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")

    def run(with_denoise):
        adaptive_featured_passes(gpu, scene, cam, W, H, depth, 0.1, [4, 4])
        if with_denoise:
            gpu.denoise_mv(W, H)
            ms = gpu.denoise_last_ms()
            assert len(ms["levels"]) == 5 and min(ms["levels"] + [ms["prepass"], ms["epilogue"], gpu.denoise_estimate_last_ms()]) > 0.0, ms
            gpu.denoise(W, H)
            assert gpu_lib().srt_denoise_estimate_last_ms(gpu._h, C.byref(C.c_float())) == ERR_INVALID      # the last denoise was plain
        gpu.render_chunk_accum(W, H, 4)
        active = gpu.accum_active
        frame, S, rows, n, s2 = accumulation_inputs(gpu, W, H)
        den = gpu.denoise_mv(W, H)
        gpu.render_chunk(W, H)                # one more plain pass: continues every pixel's RNG stream
        return frame, rows, n, s2, active, den, read_frame(gpu, W, H)

    a, b = run(True), run(False)
    assert_same_image(a[0], b[0], "[4, 4], denoise_mv, [4] against [4, 4, 4]")
    assert_bits_equal(a[1], b[1], "feature rows")
    assert np.array_equal(a[2], b[2]) and a[4] == b[4] and len(np.unique(a[2])) >= 2
    assert_bits_equal(a[3], b[3], "S2")
    for k in KEYS:
        assert_bits_equal(a[5][k], b[5][k], "denoise_mv after the next pass, " + k)
    assert_same_image(a[6], b[6], "RNG state: a plain launch after the passes")


@pytest.mark.gpu
def test_refusals_leave_the_accumulation_as_it_was(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    out = np.zeros((H, W, 3), F)
    fp = srt.binding.fptr(out)
    good = srt.denoise_vg_config()

    def call(cfg, a=fp, b=fp, c=fp, d=fp):
        return L.srt_denoise_features_mv(gpu._h, C.byref(cfg) if cfg is not None else None, a, b, c, d, W, H)

    def cfg_with(**kw):
        c = srt.denoise_vg_config()
        for k, v in kw.items():
            if k == "reserved":
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        return c

    # no adaptive featured accumulation with two samples: none at all, a plain one, a plain FEATURED one, a plain ADAPTIVE one, the
    # right kind before its first pass and with a single sample
    fresh_context(gpu, scene, cam, W, H, depth)
    assert call(good) == ERR_INVALID
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    assert call(good) == ERR_INVALID
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, H, 2)
    assert call(good) == ERR_INVALID and gpu.denoise_vg(W, H)["xyz"].shape == (H, W, 3)
    gpu.accum_reset_adaptive(0.1, 0.0, 2)
    gpu.render_chunk_accum(W, H, 2)
    assert call(good) == ERR_INVALID
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(0.1, 0.0, 2)
    assert call(good) == ERR_INVALID
    gpu.render_chunk_accum(W, H, 1)
    assert call(good) == ERR_INVALID and gpu.denoise(W, H)["xyz"].shape == (H, W, 3)      # spp_total 1: the plain filter runs, this one not
    gpu.render_chunk_accum(W, H, 1)
    frame, S, rows, n, s2 = accumulation_inputs(gpu, W, H)
    want = gpu.denoise_mv(W, H)

    assert L.srt_denoise_features_mv(None, C.byref(good), fp, fp, fp, fp, W, H) == ERR_INVALID
    assert call(None) == ERR_INVALID
    assert call(good, None, None, None, None) == ERR_INVALID
    assert L.srt_denoise_features_mv(gpu._h, C.byref(good), fp, fp, fp, fp, 0, H) == ERR_INVALID
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
    again = gpu.denoise_mv(W, H)
    for k in KEYS:
        assert_bits_equal(again[k], want[k], "after the refusals, " + k)
    assert_bits_equal(stack_features(gpu.read_features(W, H)), rows, "rows after the refusals")
    assert_same_image(read_frame(gpu, W, H), frame, "frame after the refusals")
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == 6

    # a rank of a larger world: unsupported, and its accumulation goes on
    fresh_context(gpu, scene, cam, W, H, depth)
    try:
        gpu.set_partition(1, 2)
        gpu.accum_reset_adaptive_features(0.1, 0.0, 2)
        gpu.render_chunk_accum(W, H, 2)
        assert call(good) == ERR_UNSUPPORTED
        gpu.render_chunk_accum(W, H, 2)
        assert gpu.accum_samples == 4
    finally:
        gpu.set_partition(0, 1)

    # the KAT entry point checks the same configuration, its own arguments, and the sample map
    S, r8, n, s2 = M.varying_case(3, 5)
    var = np.zeros((3, 5, 2), F)
    vp = srt.binding.fptr(var)
    P = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_float))
    kat = lambda cfg, s=S, r=r8, n=n, q=s2, w=5, h=3, o=fp, v=vp: L.srt_denoise_mv_kat(gpu._h, C.byref(cfg), P(s), P(r), P(n), P(q), w, h, o, v)
    assert kat(good) == 0
    assert kat(cfg_with(levels=9)) == ERR_INVALID and kat(cfg_with(sigma_depth=0.0)) == ERR_INVALID and kat(cfg_with(reserved=1)) == ERR_INVALID
    assert kat(cfg_with(sigma_variance=INF)) == ERR_INVALID and kat(cfg_with(variance_floor=0.0)) == ERR_INVALID
    for arg in ("s", "r", "n", "q", "o", "v"):
        assert kat(good, **{arg: None}) == ERR_INVALID, arg
    assert kat(good, w=0) == ERR_INVALID and kat(good, h=0) == ERR_INVALID
    assert L.srt_denoise_mv_kat(None, C.byref(good), P(S), P(r8), P(n), P(s2), 5, 3, fp, vp) == ERR_INVALID
    for at in (0, 7, 14):
        zero = n.copy()
        zero.reshape(-1)[at] = 0
        assert kat(good, n=zero) == ERR_INVALID, at
        with pytest.raises(ValueError):
            gpu.denoise_mv_kat(S, r8, zero, s2)
    assert kat(good) == 0
    with pytest.raises(ValueError):
        gpu.denoise_mv_kat(S, r8[:, :4], n, s2)
    with pytest.raises(ValueError):
        gpu.denoise_mv_kat(S, r8, n[:2], s2)
    with pytest.raises(ValueError):
        gpu.denoise_mv_kat(S, r8, n.astype(F), s2)


@pytest.mark.gpu
def test_render_adaptive_denoised_yields_what_the_manual_calls_give(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    kw = dict(min_spp=4, step=4, max_spp=12, renderer=gpu)
    plain = list(srt.render_adaptive(scene, cam, W, H, depth, 0.1, **kw))
    assert [s[0] for s in plain] == [4, 8, 12] and plain[-1][1] > 0
    for variance, cfg in (("measured", dict(levels=3, sigma_variance=1.5)), ("spatial", dict(levels=3, sigma_variance=1.5)), (None, dict(levels=3, sigma_color=0.5))):
        n_steps = 0
        # (stepped by hand: the accumulation, whose S2 the measured restatement needs, lives as long as the generator's session)
        for (t, active, res, feat, den), (t2, active2, res2) in zip(srt.render_adaptive_denoised(scene, cam, W, H, depth, 0.1, variance=variance, **kw, **cfg), plain):
            n_steps += 1
            assert (t, active) == (t2, active2) and np.array_equal(res["samples"], res2["samples"])
            assert_same_image(res, res2, "render_adaptive_denoised vs render_adaptive at %d" % t)
            lane = lane_of(res["geom"], W, H)
            S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in res["xyz"]], axis=-1)
            n, rows = res["samples"].reshape(H, W), stack_features(feat)
            if variance is None:
                assert set(den) == set(KEYS[:3])
                assert_bits_equal(den["xyz"], M.denoise_counts(S, rows, n, **cfg), "plain at %d" % t)
            elif variance == "spatial":
                assert_pair_equal((den["xyz"], den["var"]), M.denoise_vg_counts(S, rows, n, **dict(V.VG_DEFAULTS, **cfg)), "spatial at %d" % t)
            else:
                s2 = gpu.accum_stats(W, H)["sum_y2"].reshape(H, W)
                assert_pair_equal((den["xyz"], den["var"]), M.denoise_mv(S, rows, n, s2, **dict(V.VG_DEFAULTS, **cfg)), "measured at %d" % t)
        assert n_steps == len(plain)
    with pytest.raises(ValueError):
        srt.render_adaptive_denoised(scene, cam, W, H, depth, 0.1, variance="temporal", **kw)
