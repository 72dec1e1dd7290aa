"""Sample-parallel pixels (srt_accum_reset_streams, render_kernel MODE 6 + stream_combine_kernel): a frame of K streams per pixel is,
bit for bit, the fixed-order float32 sum of K plain frames -- frame k rendered by a context seeded 1984 + k * n_lanes with n / K
samples -- and the plain conversion of that sum.  The plain frames are held to the CPU oracle by the parity suite (and once here), so
every comparison is against an exact reference."""
import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, SEED, assert_same_image, expect_error,
                           forced_shape, fresh_context, gather_ranks, lane_of, named_workload, predicted_frame, progressive_steps,
                           read_frame, run_mock_transport_child, shape_case, stream_prediction, stream_subframes, sum_in_stream_order)
from helpers import assert_planes_equal, oracle_scene_for

WORKLOADS = ["dielectric", "random_spheres", "cornell"]


def _named(srt, name):
    scene, cam, W, H, depth, mode = named_workload(srt, name)
    return (scene, cam, W, H, depth), mode


def _streams(srt, gpu, workload, passes, K):
    scene, cam, W, H, depth = workload
    return list(srt.render_streams(scene, cam, W, H, passes, depth, K, renderer=gpu))


# ---- 1. one stream is the plain accumulation ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "cornell", "random_spheres", "dielectric"])
def test_one_stream_equals_plain_accumulation_and_one_shot(srt, gpu, name):
    wl, _ = _named(srt, name)
    scene, cam, W, H, depth = wl
    one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
    for passes in ([12], [5, 7], [1, 1, 10]):
        steps = _streams(srt, gpu, wl, passes, 1)
        assert [t for t, _ in steps] == list(np.cumsum(passes))
        plain = progressive_steps(srt, gpu, scene, cam, W, H, passes, depth)
        for (_, got), (_, want) in zip(steps, plain):
            assert_same_image(got, want, "%s K = 1 split %r vs srt_accum_reset" % (name, passes))
        assert_same_image(steps[-1][1], one_shot, "%s K = 1 split %r vs one shot" % (name, passes))
        assert steps[-1][1]["stats"]["paths"] == W * H * passes[-1]


# ---- 2. K streams, one pass --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3, 4, 8])
@pytest.mark.parametrize("name", WORKLOADS)
def test_streamed_frame_equals_the_ordered_sum_of_plain_frames(srt, gpu, orc, name, K):
    wl, _ = _named(srt, name)
    want = stream_prediction(srt, gpu, orc, name, wl, 24, K)
    (total, got), = _streams(srt, gpu, wl, [24], K)
    assert total == 24 and gpu.accum_streams == K
    assert_same_image(got, want, "%s K = %d" % (name, K))
    assert got["stats"]["paths"] == wl[2] * wl[3] * 24


@pytest.mark.gpu
def test_streamed_frame_against_oracle_renders(srt, gpu, orc):
    """once without any GPU frame in the reference: K oracle renders of dielectric"""
    wl, mode = _named(srt, "dielectric")
    scene, cam, W, H, depth = wl
    K, n = 3, 24
    (_, got), = _streams(srt, gpu, wl, [n], K)
    n_lanes = got["geom"]["n_lanes"]
    osc = oracle_scene_for(orc, scene, mode)
    refs = [osc.render(cam, W, H, n // K, depth, seed=SEED + k * n_lanes) for k in range(K)]
    want = predicted_frame(orc, [r["xyz"] for r in refs], n, check_plain=refs[0])
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(got[k], want[k], "dielectric K = 3 vs oracle " + k)


@pytest.mark.gpu
def test_sixteen_streams_of_one_sample_and_more_streams_than_rows(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    want = stream_prediction(srt, gpu, orc, "dielectric", wl, 16, 16)
    (_, got), = _streams(srt, gpu, wl, [16], 16)
    assert_same_image(got, want, "dielectric K = 16, one sample per stream")
    # a 9 x 7 chunk: the grid's eight tiles (two of them in the chunk), sixteen copies of each row
    scene = wl[0]
    small = (scene, srt.camera_init(9, 7, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0)), 9, 7, wl[4])
    want = stream_prediction(srt, gpu, orc, "dielectric 9x7", small, 16, 16, must_differ=False)
    (_, got), = _streams(srt, gpu, small, [16], 16)
    assert_same_image(got, want, "9 x 7 chunk K = 16")


# ---- 3. passes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_pass_equals_the_single_pass_frame_of_its_total(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    steps = _streams(srt, gpu, wl, [4, 8, 12], 4)
    assert [t for t, _ in steps] == [4, 12, 24]
    for (total, got), last in zip(steps, (4, 8, 12)):
        (_, single), = _streams(srt, gpu, wl, [total], 4)
        assert_same_image(got, single, "after %d samples in passes vs one pass" % total)
        assert got["stats"]["paths"] == wl[2] * wl[3] * last
    assert_same_image(steps[-1][1], stream_prediction(srt, gpu, orc, "dielectric", wl, 24, 4), "passes [4, 8, 12] vs prediction")


# ---- 4. every launch shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_streamed_shape_is_exact(srt, gpu, orc, knobs, paired, expect):
    wl = shape_case(srt, paired)
    want = stream_prediction(srt, gpu, orc, "soup %d" % (600 if paired else 601), wl, 16, 4)      # (plain frames of the default shape: one per tree)
    with forced_shape(gpu, wl[0], knobs, expect):
        (_, got), = _streams(srt, gpu, wl, [16], 4)
        assert_same_image(got, want, "shape %r K = 4" % (expect,))


# ---- 5. partition, chunks, communicator -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_partition_and_offset_chunk(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    scene, cam, W, H, depth = wl
    K, n = 4, 24
    want = stream_prediction(srt, gpu, orc, "dielectric", wl, n, K)
    for world in (2, 3):
        def one_rank(rank):
            fresh_context(gpu, scene, cam, W, H, depth)
            gpu.set_partition(rank, world)
            gpu.accum_reset_streams(K)
            for s in (8, 16):
                gpu.render_chunk_accum(W, H, s)
        gather_ranks(gpu, world, one_rank)
        assert_planes_equal(gpu.read_fb(), want["fb"], "world %d fb" % world)
        assert_planes_equal(gpu.read_fb_aux(1), want["lin"], "world %d lin" % world)
        assert_planes_equal(gpu.read_fb_aux(2), want["xyz"], "world %d xyz" % world)

    # a 30 x 20 chunk at (17, 9) of a 64 x 40 image
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 20, 17, 9
    cam = srt.camera_init(IW, IH, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0))
    subs, n_lanes = [], 0
    for k in range(K):
        fresh_context(gpu, scene, cam, cw, ch, depth, seed=SEED + k * n_lanes, spp=n // K)
        n_lanes = gpu.geom["n_lanes"]
        gpu.render_chunk(cw, ch, ox, oy)
        subs.append(read_frame(gpu, IW, IH))
    want = predicted_frame(orc, [s["xyz"] for s in subs], n, check_plain=subs[0])
    fresh_context(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset_streams(K)
    for s in (4, 8, 12):
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    got = read_frame(gpu, IW, IH)
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(got[k], want[k], "offset chunk " + k)
    # the row-major image holds the chunk's rectangle of the quantised planes and nothing else
    for c in range(3):
        img = got["rowmajor"][c].reshape(IH, IW)
        assert np.array_equal(img[oy:oy + ch, ox:ox + cw].ravel(), want["fb"][c][lane_of(gpu.geom, cw, ch)])
        assert img.sum() == img[oy:oy + ch, ox:ox + cw].sum()


@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    """srt_comm_accum_reset_streams / srt_render_frame_multi_accum at W = 2 on ONE GPU over the test transport, against the ordered sum
    of four plain frames (in a child process: the library caches its RCCL handle per process)"""
    run_mock_transport_child("""
from accum_helpers import sum_in_stream_order, comm_accumulations, stream_subframes
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth, K, n = 80, 45, 16, 4, 16
cam = scene.default_camera(W, H)
xyz = sum_in_stream_order([s['xyz'] for s in stream_subframes(srt, None, (scene, cam, W, H, depth), n, K)])
single = list(srt.render_streams(scene, cam, W, H, [n], depth, K))[-1][1]
assert_planes_equal(single['xyz'], xyz, 'one rank vs the ordered sum')
for planes, comm in comm_accumulations(srt, 2, (3, 9), scene, cam, W, H, depth, 12, lambda c: c.accum_reset_streams(K), (4, 12)):
    root = comm.root
    assert all(r.accum_samples == n and r.accum_streams == K for r in comm.renderers)
    assert_planes_equal(root.read_fb(), single['fb'], 'world 2 planes %d fb' % planes)
    if planes == 9:
        assert_planes_equal(root.read_fb_aux(1), single['lin'], 'world 2 lin')
        assert_planes_equal(root.read_fb_aux(2), xyz, 'world 2 xyz')
    assert comm.stats()['paths'] == W * H * 12
print('streams mock transport ok')
""", "streams mock transport ok", timeout=300)


# ---- 6. the streams persist ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_streams_continue_across_resets_and_reseed_with_device_params(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    scene, cam, W, H, depth = wl
    K, n1, n2 = 4, 8, 12
    # per stream: a context seeded seed_k accumulates n1 / K, resets, accumulates n2 / K
    subs, n_lanes = [], 0
    for k in range(K):
        fresh_context(gpu, scene, cam, W, H, depth, seed=SEED + k * n_lanes)
        n_lanes = gpu.geom["n_lanes"]
        gpu.accum_reset(); gpu.render_chunk_accum(W, H, n1 // K)
        gpu.accum_reset(); gpu.render_chunk_accum(W, H, n2 // K)
        subs.append(read_frame(gpu, W, H))
    want = predicted_frame(orc, [s["xyz"] for s in subs], n2, check_plain=subs[0])
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, n1)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, n2)
    assert gpu.accum_samples == n2
    got = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(got[k], want[k], "second streamed accumulation " + k)

    # a plain launch after a streamed accumulation continues stream 0: the plain context after n / K samples
    fresh_context(gpu, scene, cam, W, H, depth, spp=3)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, 8)
    gpu.render_chunk(W, H)
    after_streams = read_frame(gpu, W, H)
    fresh_context(gpu, scene, cam, W, H, depth, spp=3)
    gpu.accum_reset(); gpu.render_chunk_accum(W, H, 8 // K)
    gpu.render_chunk(W, H)
    assert_same_image(after_streams, read_frame(gpu, W, H), "plain launch after a streamed accumulation")

    # srt_init_device_params with another seed: the fresh prediction of that seed (the streams above had advanced)
    other = 77001
    want = stream_prediction(srt, gpu, orc, "dielectric", wl, 24, K, seed=other)
    fresh_context(gpu, scene, cam, W, H, depth, seed=other)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, 24)
    assert_same_image(read_frame(gpu, W, H), want, "after srt_init_device_params with another seed")
    # ... and with the first seed again
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, 24)
    assert_same_image(read_frame(gpu, W, H), stream_prediction(srt, gpu, orc, "dielectric", wl, 24, K), "re-seeded with the first seed")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_change_nothing(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    scene, cam, W, H, depth = wl
    K = 4
    want = stream_prediction(srt, gpu, orc, "dielectric", wl, 24, K)
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_streams(K)
    assert gpu.accum_streams == K and gpu.accum_samples == 0
    gpu.render_chunk_accum(W, H, 8)
    after_first = read_frame(gpu, W, H)
    refusals = [
        (lambda: gpu.accum_reset_streams(0), ERR_INVALID, "K = 0"),
        (lambda: gpu.accum_reset_streams(17), ERR_INVALID, "K = 17"),
        (lambda: gpu.render_chunk_accum(W, H, 0), ERR_INVALID, "spp_add 0"),
        (lambda: gpu.render_chunk_accum(W, H, 6), ERR_INVALID, "spp_add no multiple of K"),
        (lambda: gpu.render_chunk_accum(W, H, 15), ERR_INVALID, "spp_add no multiple of K"),
        (lambda: gpu.render_chunk_accum(W, H, 65528), ERR_INVALID, "total 65536"),
        (lambda: gpu.render_chunk_accum(W - 1, H, 16), ERR_INVALID, "another chunk width"),
        (lambda: gpu.render_chunk_accum(W, H - 8, 16), ERR_INVALID, "another chunk height"),
        (lambda: gpu.render_chunk_accum(W, H, 16, 1, 0), ERR_INVALID, "another offset"),
        (lambda: gpu.render_chunk_accum(W, H, 16, 0, 2), ERR_INVALID, "another offset"),
    ]
    for fn, code, what in refusals:
        expect_error(srt, fn, code, what)
        assert gpu.accum_samples == 8 and gpu.accum_streams == K, what
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 16), ERR_UNSUPPORTED, "instrumented pass")
    expect_error(srt, lambda: gpu.accum_reset_streams(K), ERR_UNSUPPORTED, "instrumented reset")
    gpu.set_count_traversal(False)
    assert gpu.accum_samples == 8 and gpu.accum_streams == K
    assert_same_image(read_frame(gpu, W, H), after_first, "frame after the refused calls")
    gpu.render_chunk_accum(W, H, 16)              # sums and RNG states of every stream were untouched: the exact total
    assert gpu.accum_samples == 24
    assert_same_image(read_frame(gpu, W, H), want, "accumulation continued after the refused calls")

    # device parameters not set
    bare = srt.Renderer(0)
    try:
        bare.upload_scene(scene); bare.set_camera(cam)
        expect_error(srt, lambda: bare.accum_reset_streams(2), ERR_INVALID, "device parameters not set")
        assert bare.accum_streams == 0
    finally:
        bare.close()

    # the other kinds end it
    for reset in (gpu.accum_reset, lambda: gpu.accum_reset_adaptive(0.05), gpu.accum_reset_spectral):
        gpu.accum_reset_streams(K)
        assert gpu.accum_streams == K
        reset()
        assert gpu.accum_streams == 0
    # ... and so does what invalidates any accumulation
    gpu.accum_reset_streams(K)
    gpu.render_chunk(W, H)
    assert gpu.accum_streams == 0
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 8), ERR_INVALID, "after a plain launch")


# ---- 8. one frame at a BASELINE size ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_baseline_size_frame(srt, gpu):
    """1280 x 720 (BASELINE cfg 2's frame), K = 4, n = 8: ordered queues of thousands of rows and split rows, XYZ planes against four
    plain 2-spp frames"""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    W, H, depth, K, n = 1280, 720, 16, 4, 8
    cam = scene.default_camera(W, H)
    frames = [s["xyz"] for s in stream_subframes(srt, gpu, (scene, cam, W, H, depth), n, K)]
    (total, got), = list(srt.render_streams(scene, cam, W, H, [n], depth, K, renderer=gpu))
    assert total == n and got["stats"]["paths"] == W * H * n
    assert_planes_equal(got["xyz"], sum_in_stream_order(frames), "1280 x 720 K = 4 XYZ")
