"""The presented picture on the device (srt_present / srt_present_kat, csrc/srt_present.hip): every comparison is byte for byte and
integer for integer against the composition of the calls that existed before it -- the stage's own call with its float outputs, then
expose / expose_kat, then the packing rule of tests/present_reference.py -- never against the code under test.  Explicit images at the
sizes that split the vector from the scalar path first, then every source on real accumulations, placement, partitions, the read-only
property, the refusals and the generator."""
import ctypes as C
import os

import numpy as np
import pytest

import expose_reference as R
import present_reference as P
from accum_helpers import ERR_INVALID, ERR_UNSUPPORTED, expect_error, fresh_context, gpu_lib, named_workload, read_frame
from helpers import assert_planes_equal, bits
from test_expose import _setup as _expose_setup

F = np.float32
U8P = C.POINTER(C.c_uint8)
FP = C.POINTER(C.c_float)
# widths below four, multiples of four and not, odd widths (every row starts at another alignment), more pixels on a row than one workgroup takes
SIZES = [(1, 1), (3, 1), (4, 1), (5, 3), (8, 2), (63, 1), (65, 3), (257, 5), (1000, 3)]
SPECIALS = [np.nan, np.inf, -np.inf, -1.0, 1e-41, 1e30, 0.0]


def _image(w, h, seed=0):
    """test_expose.py's _tone_image at any size: finite XYZ means over seven decades, some negative; where there is room, a zero pixel, a
    denormal, and NaN / +inf / -inf pixels in different components"""
    rng = np.random.default_rng(77 + w * h + seed)
    img = ((rng.random((h, w, 3)) - 0.05) * 10.0 ** rng.integers(-4, 3, (h, w, 1))).astype(F)
    flat = img.reshape(-1, 3)
    n = w * h
    if n >= 8:
        flat[n // 7] = 0
        flat[n // 5, 1] = F(1e-41)
        for pix, comp, v in ((n // 2, 1, np.nan), (n // 3, 1, np.inf), (n - 1, 0, -np.inf), (1, 2, np.nan), (2, 1, -np.inf)):
            flat[pix, comp] = v
    return img


def _assert_same_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = (got != want).any(axis=-1)
    assert not diff.any(), "%s: %d of %d pixels differ, first at %r: got %r, want %r" % (
        what, int(diff.sum()), diff.size, tuple(np.argwhere(diff)[0]), got[diff][0].tolist(), want[diff][0].tolist())


def _meter_equal(got, want, what):
    assert got is not None and set(got) == set(want), what
    for k in want:
        assert bits(F(got[k])) == bits(F(want[k])) if isinstance(want[k], float) else got[k] == want[k], (what, k, got[k], want[k])


# ---- the kernel on explicit images -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_present_kat_equals_the_packed_expose_kat(gpu, w, h):
    img = _image(w, h)
    for curve in (0, 1):
        for gain, white in ((0.37, 4.0), (300.0, 1.5), (2.0 ** -9, np.inf)):
            what = "present KAT %d x %d curve %d gain %r white %r" % (w, h, curve, gain, white)
            want = gpu.expose_kat(img, gain=gain, curve=curve, white=white)
            got = gpu.present_kat(img, gain=gain, curve=curve, white=white)
            _assert_same_bytes(got["rgba"], P.pack(want["fb"]), what)
            assert got["clip"] == want["clip"] and got["meter"] is None, (what, got["clip"], want["clip"])
    assert gpu.present_last_ms() > 0
    # metered: the gain is the meter's, the metering meter_kat's
    for cfg in (dict(), dict(key=0.5, percentile_ppm=900000, curve=0)):
        want = gpu.expose_kat(img, **cfg)
        got = gpu.present_kat(img, **cfg)
        mcfg = {k: v for k, v in cfg.items() if k != "curve"}
        _meter_equal(got["meter"], gpu.meter_kat(img, **mcfg), "metered KAT %d x %d" % (w, h))
        _assert_same_bytes(got["rgba"], P.pack(want["fb"]), "metered KAT %d x %d %r" % (w, h, cfg))
        assert got["clip"] == want["clip"]
    if w * h >= 195:
        assert want["clip"]["blown"] > 0 and want["clip"]["crushed"] > 0 and want["clip"]["nonfinite"] >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("w,row", [(12, 0), (13, 1)], ids=["vector-group", "scalar-group"])
def test_a_special_pixel_changes_only_its_own_word(gpu, w, row):
    """NaN, +-inf, -1, a denormal, 1e30 and 0 in each of the four positions of one 4-pixel group, one at a time: in a 12-wide image the
    group is whole and aligned (the 16-byte path), in row 1 of a 13-wide image it starts off the 16-byte grid (the scalar path)"""
    h = 2
    rng = np.random.default_rng(12)
    base = (rng.random((h, w, 3)) * 0.8 + 0.1).astype(F)
    base_out = gpu.present_kat(base, gain=1.0, curve=1)["rgba"]
    _assert_same_bytes(base_out, P.pack(gpu.expose_kat(base, gain=1.0, curve=1)["fb"]), "base image")
    assert len(np.unique(P.words(base_out))) > w
    for v in SPECIALS:
        for pos in range(4):
            for comp in ((0, 1, 2) if np.isnan(v) else (1,)):
                img = base.copy()
                img[row, 4 + pos, comp] = v
                what = "%r in component %d of position %d" % (v, comp, pos)
                want = gpu.expose_kat(img, gain=1.0, curve=1)
                got = gpu.present_kat(img, gain=1.0, curve=1)
                _assert_same_bytes(got["rgba"], P.pack(want["fb"]), what)
                assert got["clip"] == want["clip"], what
                changed = (got["rgba"] != base_out).any(axis=-1)
                changed[row, 4 + pos] = False
                assert not changed.any(), what + ": another pixel's word changed"
                if np.isnan(v):
                    assert tuple(got["rgba"][row, 4 + pos]) == (255, 255, 255, 255) and got["clip"]["nonfinite"] == 1, what


@pytest.mark.gpu
def test_vector_and_scalar_paths_write_the_same_bytes(srt, gpu):
    """a second context whose kernel never takes the 16-byte path (the fenced test knob) against the default one"""
    saved = {k: os.environ.get(k) for k in ("SRT_TEST_KNOBS", "SRT_PRESENT_SCALAR")}
    os.environ.update(SRT_TEST_KNOBS="1", SRT_PRESENT_SCALAR="1")
    try:
        scalar = srt.Renderer(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        for w, h in ((8, 2), (257, 5), (1000, 3), (1024, 4)):
            img = _image(w, h, seed=1)
            a, b = gpu.present_kat(img, gain=0.7, curve=1), scalar.present_kat(img, gain=0.7, curve=1)
            _assert_same_bytes(b["rgba"], a["rgba"], "scalar against vector, %d x %d" % (w, h))
            assert a["clip"] == b["clip"]
    finally:
        scalar.close()


# ---- real accumulations ------------------------------------------------------------------------------------------------------------
def _setup(gpu, srt, kind, partition=(0, 1)):
    """test_expose.py's _setup, and the two adaptive kinds it does not have, on its adaptive schedule; returns (W, H)"""
    if kind not in ("adaptive-features", "adaptive-spectral", "adaptive-spectral-features"):
        return _expose_setup(gpu, srt, kind, partition)
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.set_partition(*partition)
    {"adaptive-features": gpu.accum_reset_adaptive_features, "adaptive-spectral": gpu.accum_reset_adaptive_spectral,
     "adaptive-spectral-features": gpu.accum_reset_adaptive_spectral_features}[kind](0.02, 0.0, 4)
    for s in (4, 4, 4):
        gpu.render_chunk_accum(W, H, s)
    return W, H


def _counts(gpu, kind, W, H):
    """the sample total, or on an adaptive kind the (H, W) map with 0 replaced by 1"""
    if not kind.startswith("adaptive"):
        return gpu.accum_samples
    n = gpu.accum_stats(W, H)["samples"].reshape(H, W)
    assert len(np.unique(n)) > 1, "the schedule must leave mixed counts"
    return np.where(n == 0, 1, n)


_CURVES = np.random.default_rng(21).random((3, 95)).astype(F)
_FILTER = np.linspace(0.2, 1.0, 95).astype(F)
SOURCES = [("accum", "plain-cornell", {}), ("accum", "adaptive", {}), ("accum", "streams", {}),
           ("denoise", "spectral-features", dict(levels=2)), ("denoise_vg", "spectral-features", dict(levels=2)),
           ("denoise_mv", "adaptive-features", dict(levels=2)),
           ("develop", "spectral-features", {}), ("develop", "adaptive-spectral", {}),
           ("develop", "spectral-features", dict(response=_CURVES, filter=_FILTER, scale=0.5)),
           ("develop", "adaptive-spectral", dict(response=_CURVES, filter=_FILTER, scale=0.5))]


def _source_picture(gpu, source, kind, W, H, scfg):
    """the source's XYZ mean (H, W, 3) from the calls that existed before srt_present; None for the sums themselves"""
    if source == "accum":
        return None
    if source == "develop":
        d = gpu.develop_spectral_srgb(W, H, **scfg)["xyz"]
        n = _counts(gpu, kind, W, H)
        inv = (F(1) / np.asarray(n).astype(F)).astype(F)
        return (inv[..., None] * d).astype(F) if inv.ndim else (inv * d).astype(F)
    return {"denoise": gpu.denoise, "denoise_vg": gpu.denoise_vg, "denoise_mv": gpu.denoise_mv}[source](W, H, **scfg)["xyz"]


@pytest.mark.gpu
@pytest.mark.parametrize("source,kind,scfg", SOURCES, ids=["%s-%s%s" % (s, k, "-curves" if "response" in c else "") for s, k, c in SOURCES])
def test_sources_equal_the_composition_of_the_existing_calls(srt, gpu, source, kind, scfg):
    W, H = _setup(gpu, srt, kind)
    pic = _source_picture(gpu, source, kind, W, H, scfg)
    expose = (lambda **kw: gpu.expose(W, H, **kw)) if pic is None else (lambda **kw: gpu.expose_kat(pic, **kw))
    meter = gpu.meter() if pic is None else gpu.meter_kat(pic)
    assert meter["metered"] > 100, "a trivially dark picture"
    for tag, kw in (("metered", dict(curve=1)), ("fixed gain", dict(gain=0.8, curve=0, white=2.0))):
        what = "%s on %s, %s" % (source, kind, tag)
        want = expose(**kw)
        got = gpu.present(W, H, source, **dict(scfg, **kw))
        _assert_same_bytes(got["rgba"], P.pack(want["fb"]), what)
        assert got["clip"] == want["clip"], (what, got["clip"], want["clip"])
        if "gain" in kw:
            assert got["meter"] is None
        else:
            _meter_equal(got["meter"], meter, what)
        assert got["rgba"][..., :3].any() and (got["rgba"][..., 3] == 255).all(), what
        assert len(np.unique(P.words(got["rgba"]))) > 10, what
    assert gpu.present_last_ms() > 0
    # the stages' own timers report the stages the present ran
    if source.startswith("denoise"):
        assert len(gpu.denoise_last_ms()["levels"]) == 2
    if source == "develop":
        assert gpu.develop_last_ms()["contract"] > 0
    # a metering rectangle and percentile go through to the meter
    rect = (5, 7, 33, 20)
    got = gpu.present(W, H, source, **dict(scfg, rect=rect, percentile_ppm=900000))
    want_m = gpu.meter(rect=rect, percentile_ppm=900000) if pic is None else gpu.meter_kat(pic, rect=rect, percentile_ppm=900000)
    _meter_equal(got["meter"], want_m, "%s on %s, rectangle" % (source, kind))
    _assert_same_bytes(got["rgba"], P.pack(expose(gain=want_m["gain"])["fb"]), "%s on %s, rectangle" % (source, kind))


def _raw_present(gpu, srt, buf, pitch, IW, IH, source="accum", gain=None, **cfg):
    res = srt.binding.PresentResult()
    p = srt.present_config(source, gain, **cfg)
    return gpu_lib().srt_present(gpu._h, C.byref(p), buf.ctypes.data_as(U8P), pitch, IW, IH, C.byref(res)), res


@pytest.mark.gpu
def test_offset_chunk_pitch_and_clipping(srt, gpu):
    """test_expose.py's offset chunk: a 30 x 21 chunk at (17, 9) of a larger image, a pitch beyond 4 * image_width, and every byte
    outside the copied rectangle -- the pitch padding included -- as the caller left it; then an image that clips the chunk"""
    scene, _, _, _, depth, _ = named_workload(srt, "random_spheres")
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    fresh_context(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset()
    for s in (1, 3):
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    for iw, ih in ((IW, IH), (40, 25), (ox + 1, oy + 1), (ox, IH), (IW, oy)):      # whole; clipped to 23 x 16; to one pixel; outside twice
        want = gpu.expose(iw, ih, gain=0.7, curve=1, white=2.0)
        pitch = 4 * iw + 12
        buf = np.full((ih, pitch), 0xA5, np.uint8)
        rc, res = _raw_present(gpu, srt, buf, pitch, iw, ih, gain=0.7, curve=1, white=2.0)
        assert rc == 0, (iw, ih, gpu_lib().srt_last_error(gpu._h))
        inside = np.zeros((ih, iw), bool)
        inside[oy:oy + ch, ox:ox + cw] = True
        assert int(inside.sum()) == max(0, min(cw, iw - ox)) * max(0, min(ch, ih - oy))
        pixels = buf[:, :4 * iw].reshape(ih, iw, 4)
        _assert_same_bytes(pixels[inside], P.pack(want["fb"][inside]), "offset chunk in %d x %d" % (iw, ih))
        assert (pixels[~inside] == 0xA5).all() and (buf[:, 4 * iw:] == 0xA5).all(), "a byte outside the rectangle was written (%d x %d)" % (iw, ih)
        assert (res.tone.blown, res.tone.crushed, res.tone.nonfinite) == tuple(want["clip"][k] for k in ("blown", "crushed", "nonfinite"))      # the whole chunk's, clipped or not
        assert not bytes(res.meter).strip(b"\0")
    assert inside.sum() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("source,kind", [("accum", "plain-random_spheres"), ("develop", "spectral-features")])
def test_partition_of_three_presents_its_own_tiles(srt, gpu, source, kind):
    W, H = _setup(gpu, srt, kind)
    whole = gpu.present(W, H, source, gain=0.6)
    tiles_x = (gpu.geom["tx"] * gpu.geom["bx"] + 7) // 8
    clip = dict(blown=0, crushed=0, nonfinite=0)
    for rank in range(3):
        _setup(gpu, srt, kind, partition=(rank, 3))
        part = gpu.present(W, H, source, gain=0.6)
        own = R.owner_mask(W, H, tiles_x, rank, 3)
        _assert_same_bytes(part["rgba"][own], whole["rgba"][own], "rank %d of 3: its own tiles" % rank)
        assert (part["rgba"][~own] == np.array([0, 0, 0, 255], np.uint8)).all(), "rank %d of 3: another rank's pixel is not (0, 0, 0, 255)" % rank
        assert part["rgba"][own][:, :3].any()
        for k in clip:
            clip[k] += part["clip"][k]
    gpu.set_partition(0, 1)
    assert clip == whole["clip"]


@pytest.mark.gpu
def test_denoise_sources_refuse_a_partition(srt, gpu):
    W, H = _setup(gpu, srt, "spectral-features", partition=(1, 3))
    for source in ("denoise", "denoise_vg"):
        expect_error(srt, lambda: gpu.present(W, H, source, levels=1), ERR_UNSUPPORTED, source + " under (1, 3)")
    expect_error(srt, lambda: gpu.present(W, H, "denoise_mv", levels=1), ERR_INVALID, "denoise_mv on an accumulation that is not adaptive")
    W, H = _setup(gpu, srt, "adaptive-features", partition=(2, 3))
    expect_error(srt, lambda: gpu.present(W, H, "denoise_mv", levels=1), ERR_UNSUPPORTED, "denoise_mv under (2, 3)")
    gpu.set_partition(0, 1)


@pytest.mark.gpu
def test_presenting_between_passes_changes_nothing(srt, gpu):
    """frame, sums, film, feature rows, sample map, S2 and RNG state after pass, presents of every source, pass -- against a run that
    never presented (an adaptive spectral featured accumulation holds all of them)"""
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")

    def run(with_present):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_adaptive_spectral_features(0.02, 0.0, 4)
        gpu.render_chunk_accum(W, H, 4)
        if with_present:
            gpu.present(W, H)
            gpu.present(W, H, "accum", gain=2.0, curve=0)
            gpu.present(W, H, "denoise", levels=2, rect=(1, 2, 30, 20))
            gpu.present(W, H, "denoise_vg", levels=1, gain=1.0)
            gpu.present(W, H, "denoise_mv", levels=1)
            gpu.present(W, H, "develop")
            gpu.present(W, H, "develop", response=_CURVES, filter=_FILTER, gain=3.0)
            gpu.present_kat(np.ones((9, 300, 3), F))
        gpu.render_chunk_accum(W, H, 4)
        frame, film, feats, stats = read_frame(gpu, W, H), gpu.read_spectral(W, H), gpu.read_features(W, H), gpu.accum_stats(W, H)
        assert gpu.accum_samples == 8
        gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
        return frame, film, feats, stats, read_frame(gpu, W, H)

    frame, film, feats, stats, after = run(True)
    frame0, film0, feats0, stats0, after0 = run(False)
    assert np.array_equal(bits(film), bits(film0)) and film0.max() > 0
    for k in feats0:
        assert np.array_equal(bits(feats[k]), bits(feats0[k])), k
    assert np.array_equal(stats["samples"], stats0["samples"]) and len(np.unique(stats0["samples"])) > 1
    for k in ("sum_y", "sum_y2"):
        assert np.array_equal(bits(stats[k]), bits(stats0[k])), k
    for key in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(frame[key], frame0[key], "frame after pass, present, pass: " + key)
        assert_planes_equal(after[key], after0[key], "RNG state: plain launch after the passes, " + key)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L, B = gpu_lib(), srt.binding
    pitch = 4 * W
    buf = np.full((H, pitch), 0xA5, np.uint8)
    bp = buf.ctypes.data_as(U8P)
    res, tres = B.PresentResult(), B.ToneResult()
    img = np.ones((H, W, 3), F)
    ip = img.ctypes.data_as(FP)
    good, tcfg = srt.present_config(gain=2.0), srt.tone_config(gain=2.0)
    fresh = srt.Renderer(0)
    try:
        ms = C.c_float()
        assert L.srt_present_last_ms(fresh._h, C.byref(ms)) == ERR_INVALID
        assert L.srt_present(fresh._h, C.byref(good), bp, pitch, W, H, C.byref(res)) == ERR_INVALID      # no accumulation at all
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset()
    expect_error(srt, lambda: gpu.present(W, H, gain=1.0), ERR_INVALID, "present before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first = gpu.present(W, H)
    frame = read_frame(gpu, W, H)

    def cfg(source="accum", gain=2.0, **edits):
        p = srt.present_config(source, gain)
        for k, v in edits.items():
            if k == "reserved":
                p.reserved[3] = v
            elif k == "source_word":
                p.source = v
            elif k == "scale":
                p.scale = v
            else:
                sub, field = k.split("__")
                if field == "reserved":
                    getattr(p, sub).reserved[1] = v
                else:
                    setattr(getattr(p, sub), field, v)
        return p

    inf, nan = float("inf"), float("nan")
    nan_curves = np.ones((3, 95), F)
    nan_curves[1, 40] = nan
    with_nan_curves = cfg("develop")
    with_nan_curves.response3 = nan_curves.ctypes.data_as(FP)
    bad = [("unknown source", cfg(source_word=5)), ("unknown source 0xffffffff", cfg(source_word=0xffffffff)), ("reserved word", cfg(reserved=1)),
           ("tone: curve 2", cfg(tone__curve=2)), ("tone: gain 0", cfg(tone__gain=0.0)), ("tone: gain nan", cfg(tone__gain=nan)), ("tone: gain inf", cfg(tone__gain=inf)),
           ("tone: white 0", cfg(tone__white=0.0)), ("tone: white nan", cfg(tone__white=nan)), ("tone: reserved", cfg(tone__reserved=7)),
           ("metered: tone gain still checked", cfg(gain=None, tone__gain=-1.0)),
           ("meter: percentile 0", cfg(gain=None, meter__percentile_ppm=0)), ("meter: key nan", cfg(gain=None, meter__key=nan)),
           ("meter: gain_min > gain_max", cfg(gain=None, meter__gain_min=8.0, meter__gain_max=4.0)), ("meter: reserved", cfg(gain=None, meter__reserved=1)),
           ("meter: half a rectangle", cfg(gain=None, meter__w=4)), ("meter: rectangle beyond the chunk", cfg(gain=None, meter__x0=0, meter__y0=H - 1, meter__w=W, meter__h=2)),
           ("denoise on a plain accumulation", cfg("denoise")), ("denoise_vg on a plain accumulation", cfg("denoise_vg")), ("denoise_mv on a plain accumulation", cfg("denoise_mv")),
           ("denoise: levels 9", cfg("denoise", denoise__levels=9)), ("denoise: sigma 0", cfg("denoise", denoise__sigma_color=0.0)), ("denoise: reserved", cfg("denoise", denoise__reserved=1)),
           ("denoise_vg: sigma_variance inf", cfg("denoise_vg", denoise_vg__sigma_variance=inf)), ("denoise_mv: floor 0", cfg("denoise_mv", denoise_vg__variance_floor=0.0)),
           ("develop without a film", cfg("develop")), ("develop: scale inf", cfg("develop", scale=inf)), ("develop: scale nan", cfg("develop", scale=nan)),
           ("develop: a NaN in the curves", with_nan_curves)]
    refused = [(what, lambda p=p: L.srt_present(gpu._h, C.byref(p), bp, pitch, W, H, C.byref(res))) for what, p in bad]
    refused += [("null ctx", lambda: L.srt_present(None, C.byref(good), bp, pitch, W, H, C.byref(res))),
                ("null cfg", lambda: L.srt_present(gpu._h, None, bp, pitch, W, H, C.byref(res))),
                ("null output", lambda: L.srt_present(gpu._h, C.byref(good), None, pitch, W, H, C.byref(res))),
                ("empty image: width", lambda: L.srt_present(gpu._h, C.byref(good), bp, pitch, 0, H, C.byref(res))),
                ("empty image: height", lambda: L.srt_present(gpu._h, C.byref(good), bp, pitch, W, 0, C.byref(res))),
                ("pitch below 4 * image_width", lambda: L.srt_present(gpu._h, C.byref(good), bp, 4 * W - 1, W, H, C.byref(res))),
                ("pitch 0", lambda: L.srt_present(gpu._h, C.byref(good), bp, 0, W, H, C.byref(res))),
                ("KAT: null tone", lambda: L.srt_present_kat(gpu._h, None, ip, W, H, bp, C.byref(tres))),
                ("KAT: null image", lambda: L.srt_present_kat(gpu._h, C.byref(tcfg), None, W, H, bp, C.byref(tres))),
                ("KAT: null output", lambda: L.srt_present_kat(gpu._h, C.byref(tcfg), ip, W, H, None, C.byref(tres))),
                ("KAT: empty image", lambda: L.srt_present_kat(gpu._h, C.byref(tcfg), ip, W, 0, bp, C.byref(tres))),
                ("KAT: 2^31 pixels", lambda: L.srt_present_kat(gpu._h, C.byref(tcfg), ip, 0x10000, 0x8000, bp, C.byref(tres))),
                ("KAT: curve 2", lambda: L.srt_present_kat(gpu._h, C.byref(cfg(tone__curve=2).tone), ip, W, H, bp, C.byref(tres))),
                ("KAT: gain nan", lambda: L.srt_present_kat(gpu._h, C.byref(cfg(tone__gain=nan).tone), ip, W, H, bp, C.byref(tres)))]
    assert len(refused) == len(bad) + 14
    for what, call in refused:
        assert call() == ERR_INVALID, what
        assert (buf == 0xA5).all() and not bytes(res).strip(b"\0") and not bytes(tres).strip(b"\0"), what
    # after all of them the accumulation presents, reads and continues as before
    again = gpu.present(W, H)
    _assert_same_bytes(again["rgba"], first["rgba"], "present after the refusals")
    assert again["meter"] == first["meter"] and again["clip"] == first["clip"]
    for key, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, frame[key], "after the refusals " + key)
    assert gpu.accum_samples == 4
    # the measured variance needs two samples
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive_features(0.02, 0.0, 4)
    gpu.render_chunk_accum(W, H, 1)
    expect_error(srt, lambda: gpu.present(W, H, "denoise_mv", levels=1), ERR_INVALID, "denoise_mv on one sample")
    assert gpu.present(W, H, "denoise_vg", levels=1)["rgba"][..., :3].any()
    # whatever ends the accumulation ends the presenting
    gpu.accum_reset()
    expect_error(srt, lambda: gpu.present(W, H), ERR_INVALID, "present after srt_accum_reset")


# ---- the generator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source,scfg", [("accum", {}), ("denoise", dict(levels=2)), ("denoise_mv", dict(levels=1)), ("develop", dict(filter=_FILTER))])
def test_render_presented_yields_the_manual_sequence(srt, gpu, source, scfg):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    sched = [2, 3]
    kw = dict(scfg, curve=1, white=8.0, percentile_ppm=600000)
    steps = list(srt.render_presented(scene, cam, W, H, sched, depth, source=source, renderer=gpu, min_spp=4, **kw))
    assert [s[0] for s in steps] == [2, 5]
    fresh_context(gpu, scene, cam, W, H, depth, spp=sum(sched))
    {"accum": gpu.accum_reset, "denoise": gpu.accum_reset_features, "develop": gpu.accum_reset_spectral,
     "denoise_mv": lambda: gpu.accum_reset_adaptive_features(0.02, 0.0, 4)}[source]()
    for (total, res, shown), spp_add in zip(steps, sched):
        gpu.render_chunk_accum(W, H, spp_add)
        manual = gpu.present(W, H, source, **kw)
        assert total == gpu.accum_samples and set(shown) == {"rgba", "meter", "clip"}
        _assert_same_bytes(shown["rgba"], manual["rgba"], "render_presented %s at %d spp" % (source, total))
        assert shown["meter"] == manual["meter"] and shown["clip"] == manual["clip"] and shown["meter"]["metered"] > 0
        for key, v in read_frame(gpu, W, H).items():
            assert_planes_equal(res[key], v, "render_presented %s: the frame, %s" % (source, key))
    assert not np.array_equal(steps[0][2]["rgba"], steps[1][2]["rgba"])
