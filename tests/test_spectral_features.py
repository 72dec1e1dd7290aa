"""The spectral film with first-hit features in one accumulation (srt_accum_reset_spectral_features + srt_render_chunk_accum,
render_kernel MODE 9).  Under the same pass schedule and seed the frame, all nine planes, the XYZ sums, the RNG state and the 95 film
sums are a spectral accumulation's (MODE 5) bit for bit, and the eight feature sums a featured accumulation's (MODE 7); film and rows are
also held to the CPU predictions directly (tests/path_ends_reference.py, tests/features_reference.py); the result does not depend on
launch shape, partition, chunk offset or the split into passes; every consumer of either parent returns on the new kind the bits it
returns on the single-kind accumulations; and what is adaptive keeps refusing it."""
import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, N_GRID, assert_same_image, expect_error,
                           forced_shape, fresh_context, gpu_lib, named_workload, read_frame, run_mock_transport_child, shape_case,
                           split_passes)
from develop_reference import one_hot
from features_reference import shape_prediction, stack_features, workload_prediction
from helpers import bits
from path_ends_reference import FILM_SPP, assert_same_floats, shape_ends, workload_ends

RESETS = {"both": lambda g: g.accum_reset_spectral_features(), "spectral": lambda g: g.accum_reset_spectral(),
          "features": lambda g: g.accum_reset_features()}


def run(gpu, kind, scene, cam, W, H, depth, passes, offx=0, offy=0, IW=None, IH=None, after=False):
    """an accumulation of `kind` over `passes`: dict(frame, film (spectral kinds), rows (featured kinds), after: the frame of a plain
    launch that continues every pixel's RNG stream)"""
    IW, IH = IW or W, IH or H
    fresh_context(gpu, scene, cam, W, H, depth)
    RESETS[kind](gpu)
    for s in passes:
        gpu.render_chunk_accum(W, H, s, offx, offy)
    assert gpu.accum_samples == sum(passes)
    out = dict(frame=read_frame(gpu, IW, IH))
    if kind != "features":
        out["film"] = gpu.read_spectral(IW, IH)
    if kind != "spectral":
        out["rows"] = stack_features(gpu.read_features(IW, IH))
    if after:
        gpu.render_chunk(W, H, offx, offy)
        out["after"] = read_frame(gpu, IW, IH)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "cornell", "dielectric", "random_spheres"])
def test_film_and_frame_are_mode_5s_and_rows_are_mode_7s(srt, gpu, orc, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    passes = split_passes(FILM_SPP)
    both = run(gpu, "both", scene, cam, W, H, depth, passes, after=True)
    spec = run(gpu, "spectral", scene, cam, W, H, depth, passes, after=True)
    feat = run(gpu, "features", scene, cam, W, H, depth, passes)
    assert_same_image(both["frame"], spec["frame"], name + " against MODE 5")
    assert_same_image(both["after"], spec["after"], name + " RNG state: a plain launch after the passes")
    assert_same_floats(both["film"], spec["film"], name + " film against MODE 5")
    assert_same_floats(both["rows"], feat["rows"], name + " rows against MODE 7")
    assert both["film"].max() > 0 and both["rows"][..., 7].max() > 0
    # ... and the split does not matter: one pass gives the same bits
    one = run(gpu, "both", scene, cam, W, H, depth, [FILM_SPP])
    assert_same_image(one["frame"], both["frame"], name + " one pass")
    assert_same_floats(one["film"], both["film"], name + " film in one pass")
    assert_same_floats(one["rows"], both["rows"], name + " rows in one pass")
    if name in ("dielectric", "random_spheres"):
        # held to the CPU predictions directly, not only to its siblings
        _, ends = workload_ends(srt, orc, name)
        assert_same_floats(both["film"], ends["film"], name + " film against predict_film")
        _, pred = workload_prediction(srt, orc, name, FILM_SPP)
        assert_same_floats(both["rows"], pred["rows"], name + " rows against predict_features")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_shape(srt, gpu, orc, knobs, paired, expect):
    n = 4
    (scene, cam, W, H, depth), ends = shape_ends(srt, orc, paired, n)
    _, pred = shape_prediction(srt, orc, paired, n)
    gpu.set_test_knobs()
    spec = run(gpu, "spectral", scene, cam, W, H, depth, [1, 3])
    with forced_shape(gpu, scene, knobs, expect):
        got = run(gpu, "both", scene, cam, W, H, depth, [1, 3])
    assert_same_image(got["frame"], spec["frame"], "shape %r against MODE 5" % (expect,))
    assert_same_floats(got["film"], ends["film"], "shape %r film" % (expect,))
    assert_same_floats(got["rows"], pred["rows"], "shape %r rows" % (expect,))
    assert ends["film"].max() > 0 and pred["rows"][..., 7].max() > 0


@pytest.mark.gpu
def test_a_partition_and_an_offset_chunk(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    passes = [2, 4]
    ref = run(gpu, "both", scene, cam, W, H, depth, passes)
    films, rows = [], []
    for rank in range(3):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.set_partition(rank, 3)
        gpu.accum_reset_spectral_features()
        for s in passes:
            gpu.render_chunk_accum(W, H, s)
        films.append(gpu.read_spectral(W, H))
        rows.append(stack_features(gpu.read_features(W, H)))      # (pixels of the other ranks read +0)
    gpu.set_partition(0, 1)
    for parts, want, what in ((films, ref["film"], "film"), (rows, ref["rows"], "rows")):
        nonzero = np.stack([(bits(p) != 0).any(axis=-1) for p in parts])
        assert (nonzero.sum(axis=0) <= 1).all() and all(nz.any() for nz in nonzero), what
        assert_same_floats(parts[0] + parts[1] + parts[2], want, what + " summed over 3 ranks")
    # a 30 x 21 chunk (no multiple of 8 x 8 or 28 x 16) at (17, 9) of a 64 x 40 image
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam2 = scene.default_camera(IW, IH)
    kw = dict(offx=ox, offy=oy, IW=IW, IH=IH)
    both = run(gpu, "both", scene, cam2, cw, ch, depth, [1, 3], **kw)
    spec = run(gpu, "spectral", scene, cam2, cw, ch, depth, [1, 3], **kw)
    feat = run(gpu, "features", scene, cam2, cw, ch, depth, [1, 3], **kw)
    assert_same_image(both["frame"], spec["frame"], "offset chunk against MODE 5")
    assert_same_floats(both["film"], spec["film"], "offset chunk film")
    assert_same_floats(both["rows"], feat["rows"], "offset chunk rows")
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert not bits(both["film"][~inside]).any() and not bits(both["rows"][~inside]).any()
    assert both["film"][inside].max() > 0 and both["rows"][inside][:, 7].max() > 0


@pytest.mark.gpu
def test_every_consumer_returns_what_it_returns_on_the_single_kinds(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    rng = np.random.default_rng(5)
    curves = rng.uniform(-0.5, 1.0, (5, N_GRID)).astype(np.float32)

    def consumers(kind):
        fresh_context(gpu, scene, cam, W, H, depth)
        RESETS[kind](gpu)
        for s in (2, 3):
            gpu.render_chunk_accum(W, H, s)
        out = {}
        if kind != "features":
            out["read_spectral"] = gpu.read_spectral(W, H, 30, 9)
            out["develop_spectral"] = gpu.develop_spectral(W, H, curves, 0.75)
            out.update(("develop_spectral_srgb " + k, v) for k, v in gpu.develop_spectral_srgb(W, H).items())
        if kind != "spectral":
            out["read_features"] = stack_features(gpu.read_features(W, H))
            out.update(("denoise " + k, v) for k, v in gpu.denoise(W, H).items())
            out.update(("denoise_vg " + k, v) for k, v in gpu.denoise_vg(W, H).items())
        return out
    both, spec, feat = consumers("both"), consumers("spectral"), consumers("features")
    assert set(both) == set(spec) | set(feat) and len(both) == len(spec) + len(feat)
    for single in (spec, feat):
        for k, want in single.items():
            assert_same_floats(both[k], want, k)
    assert bits(both["develop_spectral"]).any() and bits(both["denoise xyz"]).any()


@pytest.mark.gpu
def test_what_is_adaptive_keeps_refusing_and_other_resets_change_the_kind(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_spectral_features()
    expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read_spectral before the first pass")
    expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    expect_error(srt, lambda: gpu.accum_active, ERR_INVALID, "accum_active")
    expect_error(srt, lambda: gpu.accum_stats(W, H), ERR_INVALID, "accum_stats")
    expect_error(srt, lambda: gpu.denoise_mv(W, H), ERR_INVALID, "denoise_mv")
    assert gpu.accum_samples == 4 and gpu.read_spectral(W, H).max() > 0
    resets = {"plain": gpu.accum_reset, "adaptive": lambda: gpu.accum_reset_adaptive(0.1, 0.0, 4), "features": gpu.accum_reset_features,
              "spectral": gpu.accum_reset_spectral, "streams": lambda: gpu.accum_reset_streams(2),
              "adaptive features": lambda: gpu.accum_reset_adaptive_features(0.1, 0.0, 4)}
    resp = one_hot(40, 2)
    for kind, reset in resets.items():
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_spectral_features()
        gpu.render_chunk_accum(W, H, 4)
        gpu.denoise_developed(W, H, resp)
        reset()
        gpu.render_chunk_accum(W, H, 4)
        assert gpu.accum_samples == 4
        expect_error(srt, lambda: gpu.denoise_developed(W, H, resp), ERR_INVALID, "denoise_developed on a %s accumulation" % kind)
        if kind != "spectral":
            expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read_spectral on a %s accumulation" % kind)
        if "features" not in kind:
            expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read_features on a %s accumulation" % kind)
    # the invalidations, the chunk binding and the sample limit are srt_accum_reset's
    for what, call in (("srt_set_camera", lambda: gpu.set_camera(cam)), ("srt_render_chunk", lambda: gpu.render_chunk(W, H)),
                       ("srt_upload_scene", lambda: gpu.upload_scene(scene)), ("srt_set_partition", lambda: gpu.set_partition(0, 1))):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_spectral_features()
        gpu.render_chunk_accum(W, H, 2)
        call()
        expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 2), ERR_INVALID, what)
        expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, what)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_spectral_features()
    gpu.render_chunk_accum(W, H, 2)
    expect_error(srt, lambda: gpu.render_chunk_accum(W - 8, H, 2), ERR_INVALID, "another chunk")
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 65534), ERR_INVALID, "more than 65535 samples")
    gpu.render_chunk_accum(W, H, 2)
    assert gpu.accum_samples == 4


@pytest.mark.gpu
def test_refusals_leave_the_previous_accumulation_as_it_was(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    fresh = srt.Renderer(0)
    try:
        assert L.srt_accum_reset_spectral_features(fresh._h) == ERR_INVALID       # device parameters not set
    finally:
        fresh.close()
    assert L.srt_accum_reset_spectral_features(None) == ERR_INVALID
    for kind in ("both", "features"):
        fresh_context(gpu, scene, cam, W, H, depth)
        RESETS[kind](gpu)
        gpu.render_chunk_accum(W, H, 3)
        frame = read_frame(gpu, W, H)
        rows = stack_features(gpu.read_features(W, H))
        film = gpu.read_spectral(W, H) if kind == "both" else None
        gpu.set_count_traversal(True)
        expect_error(srt, lambda: gpu.accum_reset_spectral_features(), ERR_UNSUPPORTED, "instrumented context")
        gpu.set_count_traversal(False)
        assert gpu.accum_samples == 3
        assert_same_image(read_frame(gpu, W, H), frame, kind + ": frame after the refusal")
        assert_same_floats(stack_features(gpu.read_features(W, H)), rows, kind + ": rows after the refusal")
        if film is not None:
            assert_same_floats(gpu.read_spectral(W, H), film, "film after the refusal")
        gpu.render_chunk_accum(W, H, 3)          # the accumulation goes on, and ends where an undisturbed one ends
        cont = dict(frame=read_frame(gpu, W, H), rows=stack_features(gpu.read_features(W, H)))
        again = run(gpu, kind, scene, cam, W, H, depth, [3, 3])
        assert_same_image(cont["frame"], again["frame"], kind + ": continued after the refusal")
        assert_same_floats(cont["rows"], again["rows"], kind + ": rows continued after the refusal")


@pytest.mark.gpu
def test_growth_of_the_grid_reallocates_both_blocks(srt):
    """a context of its own: a small grid first, then a larger one, then the small one again -- film and rows of each are those of a
    spectral and a featured accumulation on the shared context's blocks"""
    scene, _, W, H, depth, _ = named_workload(srt, "prism")
    r = srt.Renderer(0)
    try:
        for w, h in ((20, 12), (W, H), (20, 12)):
            cm = scene.default_camera(w, h)
            both = run(r, "both", scene, cm, w, h, depth, [2, 1])
            spec = run(r, "spectral", scene, cm, w, h, depth, [2, 1])
            feat = run(r, "features", scene, cm, w, h, depth, [2, 1])
            assert_same_image(both["frame"], spec["frame"], "%d x %d frame" % (w, h))
            assert_same_floats(both["film"], spec["film"], "%d x %d film" % (w, h))
            assert_same_floats(both["rows"], feat["rows"], "%d x %d rows" % (w, h))
            assert both["film"].max() > 0
    finally:
        r.close()


@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
from features_reference import stack_features
from helpers import assert_planes_equal, bits
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth = 80, 45, 16
cam = scene.default_camera(W, H)
total, ref, _ = list(srt.render_spectral(scene, cam, W, H, [2, 3], depth))[-1]
_, _, feat = list(srt.render_features(scene, cam, W, H, [2, 3], depth))[-1]
assert total == 5 and ref['film'].max() > 0
for _, comm in comm_accumulations(srt, 2, (9,), scene, cam, W, H, depth, 5, lambda c: c.accum_reset_spectral_features(), (2, 3)):
    assert_planes_equal(comm.root.read_fb(), ref['fb'], 'fb')
    assert_planes_equal(comm.root.read_fb_aux(2), ref['xyz'], 'xyz')
    assert np.array_equal(bits(comm.read_spectral(W, H)), bits(ref['film']))
    rows = sum(stack_features(r.read_features(W, H)) for r in comm.renderers)
    assert np.array_equal(bits(rows), bits(stack_features(feat)))
print('spectral features mock transport ok')
""", "spectral features mock transport ok", timeout=300)
