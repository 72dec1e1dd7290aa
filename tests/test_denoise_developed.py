"""The developed film denoised on the device (srt_denoise_developed / srt_denoise_developed_kat, csrc/srt_denoise.hip), bit for bit
(same bits, or both NaN): the payload kernels against the numpy float32 restatement (tests/denoise_developed_reference.py, itself held
to exact arithmetic by tests/test_denoise_developed_reference.py) on synthetic inputs of every awkward size and channel count; on real
spectral featured accumulations against the restatement fed the read-back sums, rows and developed planes; the XYZ output against the
plain denoiser; the placement of an offset chunk; that the call only reads the accumulation; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import denoise_developed_reference as DD
import denoise_reference as D
from accum_helpers import ERR_INVALID, ERR_UNSUPPORTED, assert_same_image, fresh_context, gpu_lib, lane_of, named_workload, read_frame
from develop_reference import one_hot
from features_reference import stack_features
from helpers import bits
from path_ends_reference import assert_same_floats

F = np.float32
INF = float("inf")
_sigmas = {}


def sigmas():
    """the sigmas of every size are those picked on the 67 x 35 input (tests/test_denoise.py does the same)"""
    if not _sigmas:
        cfg, st = D.pick_sigmas(*D.synthetic_case(35, 67))
        assert 4 * st["taken"] >= st["taps"] and 4 * st["skipped"] >= st["taps"], st
        _sigmas.update(cfg)
    return _sigmas


def check_kat(gpu, S, rows, P, n, what, **cfg):
    want_dev, want_xyz = DD.denoise_developed(S, rows, P, n, **cfg)
    dev, xyz = gpu.denoise_developed_kat(S, rows, P, n, **cfg)
    assert dev.dtype == F and xyz.dtype == F
    assert_same_floats(xyz, want_xyz, what + " XYZ")
    assert_same_floats(dev, want_dev, what + " payload")
    return dev, xyz


def xyz_sums_rowmajor(gpu, frame, W, H):
    lane = lane_of(gpu.geom, W, H)
    return np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in frame["xyz"]], axis=-1)


def passes_of(gpu, scene, cam, W, H, depth, passes, offx=0, offy=0):
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_spectral_features()
    for s in passes:
        gpu.render_chunk_accum(W, H, s, offx, offy)


def curves(k, seed=11):
    return np.random.default_rng(seed).uniform(-0.25, 1.0, (k, 95)).astype(F)


# ---- synthetic input against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(67, 35), (33, 9), (1, 1), (1, 9), (9, 1), (3, 2)], ids=lambda v: str(v))
def test_every_size_equals_the_restatement(gpu, w, h):
    """levels = 5: steps 1 and 2 through the LDS tile, steps 4, 8 and 16 direct; K = 5 leaves a partly filled second group"""
    S, rows, n = D.synthetic_case(h, w)
    P = DD.random_payload(h, w, 5)
    for levels in (5, 0, 1):
        dev, xyz = check_kat(gpu, S, rows, P, n, "%d x %d, %d levels" % (w, h, levels), levels=levels, **sigmas())
    if (w, h) == (67, 35):
        assert np.isnan(xyz).sum() == 1 and np.isinf(xyz).sum() == 1 and np.isfinite(dev).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 4, 5, 16])
def test_every_channel_count_equals_the_restatement(srt, gpu, k):
    S, rows, n = D.synthetic_case(35, 67)
    dev, _ = check_kat(gpu, S, rows, DD.random_payload(35, 67, k), n, "K = %d" % k, levels=5, **sigmas())
    assert dev.shape == (35, 67, k)
    # either output alone is enough, and gives the same bits
    L = gpu_lib()
    cfg = srt.denoise_config(levels=5, **sigmas())
    P = DD.random_payload(35, 67, k)
    only = np.zeros_like(dev)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.srt_denoise_developed_kat(gpu._h, C.byref(cfg), fp(S), fp(rows), fp(P), k, n, 67, 35, fp(only), None) == 0
    assert_same_floats(only, dev, "payload output alone")


@pytest.mark.gpu
def test_a_payload_of_copied_xyz_sums_is_the_xyz_output_and_the_plain_filter(gpu):
    S, rows, n = D.synthetic_case(35, 67)
    P = np.ascontiguousarray(S[..., [c % 3 for c in range(7)]])
    dev, xyz = check_kat(gpu, S, rows, P, n, "copied sums", levels=5, **sigmas())
    for c in range(7):
        assert_same_floats(dev[..., c], xyz[..., c % 3], "payload channel %d against XYZ" % c)
    assert_same_floats(xyz, gpu.denoise_kat(S, rows, n, levels=5, **sigmas()), "XYZ against srt_denoise_kat")


@pytest.mark.gpu
def test_non_finite_payloads_and_colours(gpu):
    # an inf payload behind an edge no tap crosses: the left half stays finite (0 * inf would have been NaN)
    S, rows, n, cfg, split = D.edge_case("albedo")
    h, w = S.shape[:2]
    P = np.ones((h, w, 3), F)
    P[:, split:] = F("inf")
    P[h // 2, split + 2, 1] = F("nan")
    dev, _ = check_kat(gpu, S, rows, P, n, "inf behind an edge", **cfg)
    assert np.isfinite(dev[:, :split]).all() and (dev[:, :split] == F(1)).all() and not np.isfinite(dev[:, split:]).any()
    # a NaN-colour pixel keeps its own payload and no neighbour takes it in
    S, rows, n = D.impulse_case(21)
    S[...] = F(0.25)
    S[10, 10, 1] = F("nan")
    P = np.full((21, 21, 4), F(2.0), F)
    P[10, 10] = (F(7.0), F("nan"), F("inf"), F(-3.0))
    dev, xyz = check_kat(gpu, S, rows, P, n, "NaN colour", **D.DEFAULTS)
    assert_same_floats(dev[10, 10], P[10, 10], "the NaN-colour pixel's payload")
    others = np.ones((21, 21), bool); others[10, 10] = False
    assert (dev[others] == F(2.0)).all() and np.isnan(xyz).sum() == 1
    # a payload NaN at a tap that counts propagates as the arithmetic says
    S[10, 10, 1] = F(0.25)
    dev, _ = check_kat(gpu, S, rows, P, n, "NaN payload", **dict(D.DEFAULTS, levels=1))
    assert np.isnan(dev[..., 1]).sum() == 25 and np.isfinite(dev[..., 0]).all()


# ---- real accumulations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "random_spheres"])
def test_real_workloads_equal_the_restatement(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    passes_of(gpu, scene, cam, W, H, depth, [2, 4])
    n = gpu.accum_samples
    frame = read_frame(gpu, W, H)
    S = xyz_sums_rowmajor(gpu, frame, W, H)
    rows = stack_features(gpu.read_features(W, H))
    resp, scale = curves(5), 0.5
    planes = gpu.develop_spectral(W, H, resp, scale)
    want_dev, want_xyz = DD.denoise_developed(S, rows, planes, n, **D.DEFAULTS)
    got = gpu.denoise_developed(W, H, resp, scale)
    assert set(got) == {"dev", "xyz"} and got["dev"].shape == (H, W, 5) and got["xyz"].shape == (H, W, 3)
    assert_same_floats(got["dev"], want_dev, name + " developed, denoised")
    assert_same_floats(got["xyz"], want_xyz, name + " XYZ")
    # both timing entries report this call's kernels
    ms_dn, ms_dev = gpu.denoise_last_ms(), gpu.develop_last_ms()
    assert len(ms_dn["levels"]) == 5 and min(ms_dn["levels"] + [ms_dn["prepass"], ms_dn["epilogue"]]) > 0 and ms_dev["contract"] > 0 and ms_dev["epilogue"] == 0
    assert_same_floats(got["xyz"], gpu.denoise(W, H)["xyz"], name + " XYZ against denoise()")
    zero = gpu.denoise_developed(W, H, resp, scale, levels=0)
    with np.errstate(all="ignore"):
        inv = F(1) / F(n)
        assert_same_floats(zero["dev"], (inv * planes).astype(F), name + " levels = 0: inv * develop_spectral")
    changed = int((bits(want_dev) != bits(zero["dev"])).any(axis=-1).sum())
    print("%s: the filter changed the payload of %d of %d pixels" % (name, changed, W * H))
    assert changed > 0
    # one-hot curves: at levels = 0 the payload is inv x the film's own samples
    hot = gpu.denoise_developed(W, H, one_hot(38, 6), levels=0)["dev"]
    with np.errstate(all="ignore"):
        assert_same_floats(hot, (inv * gpu.read_spectral(W, H, 38, 6)).astype(F), name + " one-hot curves")
    assert bits(hot).any()
    assert_same_image(read_frame(gpu, W, H), frame, name + " frame after the calls")


@pytest.mark.gpu
def test_offset_chunk_placement(srt, gpu):
    """a 30 x 21 chunk (no multiple of 8 x 8, 28 x 16 or 32 x 8) at (17, 9) of a 64 x 40 image: the placement of read_features"""
    scene, _, _, _, depth, _ = named_workload(srt, "random_spheres")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    passes_of(gpu, scene, cam, cw, ch, depth, [1, 2], ox, oy)
    S = xyz_sums_rowmajor(gpu, read_frame(gpu, IW, IH), cw, ch)
    rows = stack_features(gpu.read_features(IW, IH))[oy:oy + ch, ox:ox + cw]
    resp = curves(3)
    planes = gpu.develop_spectral(IW, IH, resp)[oy:oy + ch, ox:ox + cw]
    want_dev, want_xyz = DD.denoise_developed(S, rows, planes, 3, **D.DEFAULTS)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    got = gpu.denoise_developed(IW, IH, resp)
    for k in ("dev", "xyz"):
        assert not bits(got[k][~inside]).any(), k + ": written outside the chunk's rectangle"
    assert_same_floats(got["dev"][oy:oy + ch, ox:ox + cw], want_dev, "offset chunk payload")
    assert_same_floats(got["xyz"][oy:oy + ch, ox:ox + cw], want_xyz, "offset chunk XYZ")
    # the library writes nothing outside: a sentinel survives; and a single output is enough
    sentinel = F(-7.0)
    out = np.full((IH, IW, 3), sentinel, F)
    cfg = srt.denoise_config()
    gpu._ck(gpu_lib().srt_denoise_developed(gpu._h, C.byref(cfg), srt.binding.fptr(resp), 3, 1.0, srt.binding.fptr(out), None, IW, IH))
    assert (out[~inside] == sentinel).all() and np.array_equal(bits(out[inside]), bits(got["dev"][inside]))


@pytest.mark.gpu
def test_the_call_only_reads_the_accumulation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    resp = curves(4)

    def run(with_call):
        passes_of(gpu, scene, cam, W, H, depth, [3])
        first = second = None
        if with_call:
            first = gpu.denoise_developed(W, H, resp)
            second = gpu.denoise_developed(W, H, resp)
        gpu.render_chunk_accum(W, H, 3)
        out = dict(frame=read_frame(gpu, W, H), rows=stack_features(gpu.read_features(W, H)), film=gpu.read_spectral(W, H),
                   den=gpu.denoise_developed(W, H, resp), first=first, second=second)
        gpu.render_chunk(W, H)                # one more plain pass: continues every pixel's RNG stream
        out["after"] = read_frame(gpu, W, H)
        return out
    a, b = run(True), run(False)
    assert_same_image(a["frame"], b["frame"], "[3], denoise_developed, [3] against [3, 3]")
    assert_same_image(a["after"], b["after"], "RNG state: a plain launch after the passes")
    assert_same_floats(a["rows"], b["rows"], "feature rows")
    assert_same_floats(a["film"], b["film"], "film")
    for k in ("dev", "xyz"):
        assert_same_floats(a["first"][k], a["second"][k], "the call twice, " + k)
        assert_same_floats(a["den"][k], b["den"][k], "after 6 samples, " + k)
    assert (bits(a["first"]["dev"]) != bits(a["den"]["dev"])).any()


@pytest.mark.gpu
def test_the_working_buffers_regrow(srt):
    """a context of its own whose first call is a small rectangle with one group: the larger one with four groups must get larger
    images, and the small one still matches"""
    r = srt.Renderer(0)
    try:
        for (h, w), k in (((5, 7), 2), ((35, 67), 13), ((5, 7), 2), ((9, 33), 16)):
            S, rows, n = D.synthetic_case(h, w)
            check_kat(r, S, rows, DD.random_payload(h, w, k), n, "%d x %d, K = %d" % (w, h, k), levels=3, **sigmas())
        ms = r.denoise_last_ms()
        assert len(ms["levels"]) == 3 and min(ms["levels"] + [ms["prepass"], ms["epilogue"]]) > 0.0, ms
        scene, cam, W, H, depth, _ = named_workload(srt, "prism")
        for (w, h), k in (((20, 12), 3), ((W, H), 9), ((20, 12), 3)):
            cm = scene.default_camera(w, h)
            passes_of(r, scene, cm, w, h, depth, [3])
            S = xyz_sums_rowmajor(r, read_frame(r, w, h), w, h)
            resp = curves(k)
            want_dev, want_xyz = DD.denoise_developed(S, stack_features(r.read_features(w, h)), r.develop_spectral(w, h, resp), 3, **D.DEFAULTS)
            got = r.denoise_developed(w, h, resp)
            assert_same_floats(got["dev"], want_dev, "chunk %d x %d payload" % (w, h))
            assert_same_floats(got["xyz"], want_xyz, "chunk %d x %d XYZ" % (w, h))
    finally:
        r.close()


@pytest.mark.gpu
def test_render_developed_denoised_yields_what_the_manual_calls_give(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    steps = list(srt.render_developed_denoised(scene, cam, W, H, [2, 4], depth, renderer=gpu, levels=3))
    assert [s[0] for s in steps] == [2, 6]
    plain = list(srt.render_spectral(scene, cam, W, H, [2, 4], depth, renderer=gpu))
    feats = list(srt.render_features(scene, cam, W, H, [2, 4], depth, renderer=gpu))
    cie = srt.renderer.cie_response()
    cfg = dict(D.DEFAULTS, levels=3)
    for (t, res, dev, den), (t2, res2, _), (_, _, feat) in zip(steps, plain, feats):
        assert t == t2
        assert_same_image(res, res2, "render_developed_denoised vs render_spectral at %d" % t)
        lane = lane_of(res["geom"], W, H)
        S = np.stack([np.asarray(p, F)[lane].reshape(H, W) for p in res["xyz"]], axis=-1)
        want_dev, want_xyz = DD.denoise_developed(S, stack_features(feat), dev, t, **cfg)
        assert dev.shape == (H, W, 3) and set(den) == {"dev", "xyz"}
        assert_same_floats(den["dev"], want_dev, "denoised developed planes at %d" % t)
        assert_same_floats(den["xyz"], want_xyz, "denoised XYZ at %d" % t)
        # response=None: the colour-matching rows at the float32 470/7, on sums -- the film's own XYZ sums up to reassociation (the
        # bound tests/test_develop.py and tests/test_spectral.py hold that contraction to)
        ok = np.isfinite(S).all(axis=-1)
        np.testing.assert_allclose(dev[ok].astype(np.float64), S[ok].astype(np.float64), rtol=2e-4, atol=1e-9)
    # other curves through a filter: what the manual calls give on the same accumulation
    resp, t_j = curves(2), np.linspace(0.2, 1.0, 95).astype(F)
    (t, res, dev, den), = srt.render_developed_denoised(scene, cam, W, H, [6], depth, response=resp, filter=t_j, renderer=gpu, levels=2)
    passes_of(gpu, scene, cam, W, H, depth, [6])
    assert_same_floats(dev, gpu.develop_spectral(W, H, resp, 1.0, t_j), "generator's developed planes")
    manual = gpu.denoise_developed(W, H, resp, 1.0, t_j, levels=2)
    for k in ("dev", "xyz"):
        assert_same_floats(den[k], manual[k], "generator's denoised " + k)
    assert_same_floats(den["dev"], gpu.denoise_developed(W, H, srt.sensor_response(resp, t_j), levels=2)["dev"], "the filter folded by hand")
    assert cie.shape == (3, 95)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_accumulation_as_it_was(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    K = 3
    resp = curves(K)
    dev, xyz = np.zeros((H, W, K), F), np.zeros((H, W, 3), F)
    fp = srt.binding.fptr
    good = srt.denoise_config()

    def call(cfg=good, r=resp, k=K, scale=1.0, a=dev, b=xyz, ctx=None, w=W, h=H):
        return L.srt_denoise_developed(gpu._h if ctx is None else ctx, C.byref(cfg) if cfg is not None else None, fp(r) if r is not None else None,
                                       k, scale, fp(a) if a is not None else None, fp(b) if b is not None else None, w, h)

    def cfg_with(**kw):
        c = srt.denoise_config()
        for k, v in kw.items():
            if k == "reserved":
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        return c

    # not a spectral featured accumulation with a pass: none, plain, spectral, featured, adaptive featured, the right kind before its pass
    fresh_context(gpu, scene, cam, W, H, depth)
    assert call() == ERR_INVALID
    for reset in (gpu.accum_reset, gpu.accum_reset_spectral, gpu.accum_reset_features, lambda: gpu.accum_reset_adaptive_features(0.1, 0.0, 2)):
        reset()
        gpu.render_chunk_accum(W, H, 2)
        assert call() == ERR_INVALID
    fresh_context(gpu, scene, cam, W, H, depth)      # (seeds the RNG streams again: the run below is compared with a fresh [2, 4])
    gpu.accum_reset_spectral_features()
    assert call() == ERR_INVALID
    gpu.render_chunk_accum(W, H, 2)
    frame, rows, film = read_frame(gpu, W, H), stack_features(gpu.read_features(W, H)), gpu.read_spectral(W, H)
    want = gpu.denoise_developed(W, H, resp)

    assert call(ctx=C.c_void_p(None)) == ERR_INVALID and call(cfg=None) == ERR_INVALID and call(r=None) == ERR_INVALID
    assert call(a=None, b=None) == ERR_INVALID and call(w=0) == ERR_INVALID and call(h=0) == ERR_INVALID
    assert call(a=None) == 0 and call(b=None) == 0
    assert call(cfg_with(levels=9)) == ERR_INVALID
    for field in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        for bad in (float("nan"), 0.0, -1.0, -INF):
            assert call(cfg_with(**{field: bad})) == ERR_INVALID, (field, bad)
        assert call(cfg_with(**{field: INF})) == 0, field
    for k in range(3):
        assert call(cfg_with(reserved=k)) == ERR_INVALID
    # response, channels and scale as srt_develop_spectral refuses them
    assert call(k=0) == ERR_INVALID and call(r=curves(16), k=17) == ERR_INVALID
    assert call(scale=float("nan")) == ERR_INVALID and call(scale=INF) == ERR_INVALID
    for bad in (float("nan"), INF):
        r2 = resp.copy(); r2[K - 1, 94] = bad
        assert call(r=r2) == ERR_INVALID
    assert call(cfg_with(levels=8)) == 0 and call(cfg_with(levels=0)) == 0
    # nothing of the above changed the accumulation
    again = gpu.denoise_developed(W, H, resp)
    for k in ("dev", "xyz"):
        assert_same_floats(again[k], want[k], "after the refusals, " + k)
    assert_same_floats(stack_features(gpu.read_features(W, H)), rows, "rows after the refusals")
    assert_same_floats(gpu.read_spectral(W, H), film, "film after the refusals")
    assert_same_image(read_frame(gpu, W, H), frame, "frame after the refusals")
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == 6
    cont, cont_film = read_frame(gpu, W, H), gpu.read_spectral(W, H)
    passes_of(gpu, scene, cam, W, H, depth, [2, 4])
    assert_same_image(cont, read_frame(gpu, W, H), "continued after the refusals")
    assert_same_floats(cont_film, gpu.read_spectral(W, H), "film continued after the refusals")

    # a rank of a larger world: unsupported, and its accumulation goes on
    fresh_context(gpu, scene, cam, W, H, depth)
    try:
        gpu.set_partition(1, 2)
        gpu.accum_reset_spectral_features()
        gpu.render_chunk_accum(W, H, 2)
        part = gpu.read_spectral(W, H)
        assert call() == ERR_UNSUPPORTED
        assert_same_floats(gpu.read_spectral(W, H), part, "film of rank 1 after the refusal")
        gpu.render_chunk_accum(W, H, 2)
        assert gpu.accum_samples == 4
    finally:
        gpu.set_partition(0, 1)

    # the KAT entry point checks the same configuration, and its own arguments
    S, r8, n = D.synthetic_case(3, 5)
    P = DD.random_payload(3, 5, 2)
    o_dev, o_xyz = np.zeros((3, 5, 2), F), np.zeros((3, 5, 3), F)

    def kat(cfg=good, s=S, r=r8, p=P, k=2, n=n, w=5, h=3, a=o_dev, b=o_xyz):
        f = lambda v: fp(v) if v is not None else None
        return L.srt_denoise_developed_kat(gpu._h, C.byref(cfg), f(s), f(r), f(p), k, n, w, h, f(a), f(b))
    assert kat() == 0 and kat(a=None) == 0 and kat(b=None) == 0
    assert kat(cfg_with(levels=9)) == ERR_INVALID and kat(cfg_with(sigma_depth=0.0)) == ERR_INVALID and kat(cfg_with(reserved=2)) == ERR_INVALID
    assert kat(s=None) == ERR_INVALID and kat(r=None) == ERR_INVALID and kat(p=None) == ERR_INVALID and kat(a=None, b=None) == ERR_INVALID
    assert kat(n=0) == ERR_INVALID and kat(w=0) == ERR_INVALID and kat(h=0) == ERR_INVALID and kat(k=0) == ERR_INVALID and kat(k=17) == ERR_INVALID
    with pytest.raises(ValueError):
        gpu.denoise_developed_kat(S, r8, P[:, :4], n)
