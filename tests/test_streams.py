"""Sample-parallel pixels (srt_accum_reset_streams, render_kernel MODE 6 + stream_combine_kernel): a frame of K streams per pixel is,
bit for bit, the fixed-order float32 sum of K plain frames -- frame k rendered by a context seeded 1984 + k * n_lanes with n / K
samples -- and the plain conversion of that sum.  The plain frames are held to the CPU oracle by the parity suite (and once here), so
every comparison is against an exact reference."""
import ctypes as C

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, _assert_same_image, _expect_error, _lane_of,
                           _progressive, _soup, _workload, run_mock_transport_child)
from helpers import assert_planes_equal, bits, oracle_scene_for

SEED = 1984
WORKLOADS = ["dielectric", "random_spheres", "cornell"]
# Sub-frames 0 and 1 must differ in at least a quarter of the chunk's pixels, else the sum order and the stream indexing go untested:
# asserted on the two workloads that carry the condition.  cornell at 64 x 48 is mostly background (measured: 629 of 3072 pixels
# differ at n / K = 12, 20.5 %), so, like prism, it is never used alone: it must differ somewhere, and runs next to the other two.
QUARTER = ("dielectric", "random_spheres")
_cache = {}


def _convert(orc, xyz, n):
    """the sRGB and quantised planes of XYZ sums over n samples: orc_XYZ_to_sRGB of float32(1) / float32(n) * sum, lane by lane"""
    inv = np.float32(1) / np.float32(n)
    c = np.stack([inv * np.asarray(p, np.float32) for p in xyz], axis=1).astype(np.float32)
    lin, q = np.zeros_like(c), np.zeros_like(c)
    f3 = C.c_float * 3
    fn = orc.lib().orc_XYZ_to_sRGB
    for i in range(c.shape[0]):
        a, l3, q3 = f3(*c[i]), f3(), f3()
        fn(a, l3, q3)
        lin[i] = l3[:]; q[i] = q3[:]
    return tuple(np.ascontiguousarray(lin[:, k]) for k in range(3)), tuple(np.ascontiguousarray(q[:, k]) for k in range(3))


def _sum_in_stream_order(frames):
    total = [np.asarray(p, np.float32).copy() for p in frames[0]]
    for f in frames[1:]:
        total = [(t + np.asarray(p, np.float32)).astype(np.float32) for t, p in zip(total, f)]
    return tuple(total)


def _predicted(orc, xyz_frames, n, check_plain=None):
    """dict(fb, lin, xyz) of a streamed frame from the XYZ planes of its K plain frames.  check_plain: a plain frame of n / K samples,
    whose own planes the restatement of the conversion must reproduce before it is used"""
    if check_plain is not None:
        lin, q = _convert(orc, check_plain["xyz"], n // len(xyz_frames))
        assert_planes_equal(lin, check_plain["lin"], "restated conversion, plain frame sRGB")
        assert_planes_equal(q, check_plain["fb"], "restated conversion, plain frame quantised")
    xyz = _sum_in_stream_order(xyz_frames)
    lin, q = _convert(orc, xyz, n)
    return dict(fb=q, lin=lin, xyz=xyz)


def _prediction(srt, gpu, orc, name, workload, n, K, seed=SEED, must_differ=True):
    """the prediction of the issue for a whole-image frame of `workload` = (scene, cam, W, H, depth), computed once per (name, n, K, seed)"""
    key = (name, n, K, seed)
    if key not in _cache:
        scene, cam, W, H, depth = workload
        subs, n_lanes = [], 0
        for k in range(K):
            subs.append(srt.render_image(scene, cam, W, H, n // K, depth, seed=seed + k * n_lanes, renderer=gpu))
            n_lanes = subs[0]["geom"]["n_lanes"]
        if must_differ and K > 1:      # else the sum order and the stream indexing would go untested
            lane = _lane_of(subs[0]["geom"], W, H)
            differ = np.zeros(W * H, bool)
            for c in range(3):
                differ |= bits(subs[0]["xyz"][c])[lane] != bits(subs[1]["xyz"][c])[lane]
            print("%s n/K = %d: sub-frames 0 and 1 differ in %d of %d pixels" % (name, n // K, differ.sum(), W * H))
            assert differ.sum() * (4 if name in QUARTER else W * H) >= W * H, "%s: sub-frames 0 and 1 differ in only %d of %d pixels" % (name, differ.sum(), W * H)
        want = _predicted(orc, [s["xyz"] for s in subs], n, check_plain=subs[0])
        want["rowmajor"] = tuple(p[_lane_of(subs[0]["geom"], W, H)] for p in want["fb"])
        want["subs"] = subs
        _cache[key] = want
    return _cache[key]


def _named(srt, name):
    scene, cam, W, H, depth, mode = _workload(srt, name)
    return (scene, cam, W, H, depth), mode


def _streams(srt, gpu, workload, passes, K):
    scene, cam, W, H, depth = workload
    return list(srt.render_streams(scene, cam, W, H, passes, depth, K, renderer=gpu))


def _planes(gpu, W, H):
    gpu.scatter_tiles()
    return dict(fb=gpu.read_fb(), lin=gpu.read_fb_aux(1), xyz=gpu.read_fb_aux(2), rowmajor=gpu.read_fb_rowmajor(W, H))


def _setup(gpu, scene, cam, cw, ch, depth, seed=SEED, spp=12):
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1); gpu.set_count_traversal(False)
    gpu.set_gather_planes(9)
    gpu.init_device_params(cw, ch, spp, depth, seed)


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
        plain = _progressive(srt, gpu, scene, cam, W, H, passes, depth)
        for (_, got), (_, want) in zip(steps, plain):
            _assert_same_image(got, want, "%s K = 1 split %r vs srt_accum_reset" % (name, passes))
        _assert_same_image(steps[-1][1], one_shot, "%s K = 1 split %r vs one shot" % (name, passes))
        assert steps[-1][1]["stats"]["paths"] == W * H * passes[-1]


# ---- 2. K streams, one pass --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3, 4, 8])
@pytest.mark.parametrize("name", WORKLOADS)
def test_streamed_frame_equals_the_ordered_sum_of_plain_frames(srt, gpu, orc, name, K):
    wl, _ = _named(srt, name)
    want = _prediction(srt, gpu, orc, name, wl, 24, K)
    (total, got), = _streams(srt, gpu, wl, [24], K)
    assert total == 24 and gpu.accum_streams == K
    _assert_same_image(got, want, "%s K = %d" % (name, K))
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
    want = _predicted(orc, [r["xyz"] for r in refs], n, check_plain=refs[0])
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(got[k], want[k], "dielectric K = 3 vs oracle " + k)


@pytest.mark.gpu
def test_sixteen_streams_of_one_sample_and_more_streams_than_rows(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    want = _prediction(srt, gpu, orc, "dielectric", wl, 16, 16)
    (_, got), = _streams(srt, gpu, wl, [16], 16)
    _assert_same_image(got, want, "dielectric K = 16, one sample per stream")
    # a 9 x 7 chunk: the grid's eight tiles (two of them in the chunk), sixteen copies of each row
    scene = wl[0]
    small = (scene, srt.camera_init(9, 7, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0)), 9, 7, wl[4])
    want = _prediction(srt, gpu, orc, "dielectric 9x7", small, 16, 16, must_differ=False)
    (_, got), = _streams(srt, gpu, small, [16], 16)
    _assert_same_image(got, want, "9 x 7 chunk K = 16")


# ---- 3. passes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_pass_equals_the_single_pass_frame_of_its_total(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    steps = _streams(srt, gpu, wl, [4, 8, 12], 4)
    assert [t for t, _ in steps] == [4, 12, 24]
    for (total, got), last in zip(steps, (4, 8, 12)):
        (_, single), = _streams(srt, gpu, wl, [total], 4)
        _assert_same_image(got, single, "after %d samples in passes vs one pass" % total)
        assert got["stats"]["paths"] == wl[2] * wl[3] * last
    _assert_same_image(steps[-1][1], _prediction(srt, gpu, orc, "dielectric", wl, 24, 4), "passes [4, 8, 12] vs prediction")


# ---- 4. every launch shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_streamed_shape_is_exact(srt, gpu, orc, knobs, paired, expect):
    n_tri = 600 if paired else 601          # the SAH builder pairs an even triangle count
    scene = _soup(srt, n_tri, n_tri).build_bvh(srt.BVH_SAH, 1984)
    assert scene.is_paired == paired
    W, H, depth = 48, 32, 8
    cam = srt.camera_init(W, H, 50.0, (0.5, 1.0, 16.0), (0.0, 0.0, 0.0), defocus_angle=0.6, focus_dist=14.0)
    wl = (scene, cam, W, H, depth)
    want = _prediction(srt, gpu, orc, "soup %d" % n_tri, wl, 16, 4)      # (plain frames of the default shape: one per tree)
    gpu.set_test_knobs(**knobs)
    try:
        (_, got), = _streams(srt, gpu, wl, [16], 4)
        plan = gpu.launch_plan()
        assert (int(plan["narrow_refs"]), int(plan["all_cached"]), int(plan["paired"])) == expect, (plan, knobs)
        _assert_same_image(got, want, "shape %r K = 4" % (expect,))
    finally:
        gpu.set_test_knobs()
        gpu.upload_scene(scene)


# ---- 5. partition, chunks, communicator -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_partition_and_offset_chunk(srt, gpu, orc):
    import torch
    wl, _ = _named(srt, "dielectric")
    scene, cam, W, H, depth = wl
    K, n = 4, 24
    want = _prediction(srt, gpu, orc, "dielectric", wl, n, K)
    for world in (2, 3):
        parts = []
        for rank in range(world):
            _setup(gpu, scene, cam, W, H, depth)
            gpu.set_partition(rank, world)
            gpu.accum_reset_streams(K)
            for s in (8, 16):
                gpu.render_chunk_accum(W, H, s)
            gpu.synchronize()
            _, n_floats, _, _ = gpu.tile_buffer()
            staging = torch.empty(n_floats, dtype=torch.float32, device="cuda")
            gpu.copy_tile_buffer(staging.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            parts.append(staging.cpu().numpy().copy())
        gathered = torch.from_numpy(np.concatenate(parts)).cuda()
        gpu.scatter_tiles(gathered.data_ptr())
        gpu.synchronize()
        assert_planes_equal(gpu.read_fb(), want["fb"], "world %d fb" % world)
        assert_planes_equal(gpu.read_fb_aux(1), want["lin"], "world %d lin" % world)
        assert_planes_equal(gpu.read_fb_aux(2), want["xyz"], "world %d xyz" % world)
    gpu.set_partition(0, 1)

    # a 30 x 20 chunk at (17, 9) of a 64 x 40 image
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 20, 17, 9
    cam = srt.camera_init(IW, IH, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0))
    subs, n_lanes = [], 0
    for k in range(K):
        _setup(gpu, scene, cam, cw, ch, depth, seed=SEED + k * n_lanes, spp=n // K)
        n_lanes = gpu.geom["n_lanes"]
        gpu.render_chunk(cw, ch, ox, oy)
        subs.append(_planes(gpu, IW, IH))
    want = _predicted(orc, [s["xyz"] for s in subs], n, check_plain=subs[0])
    _setup(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset_streams(K)
    for s in (4, 8, 12):
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    got = _planes(gpu, IW, IH)
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(got[k], want[k], "offset chunk " + k)
    # the row-major image holds the chunk's rectangle of the quantised planes and nothing else
    for c in range(3):
        img = got["rowmajor"][c].reshape(IH, IW)
        assert np.array_equal(img[oy:oy + ch, ox:ox + cw].ravel(), want["fb"][c][_lane_of(gpu.geom, cw, ch)])
        assert img.sum() == img[oy:oy + ch, ox:ox + cw].sum()


@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    """srt_comm_accum_reset_streams / srt_render_frame_multi_accum at W = 2 on ONE GPU over the test transport, against the ordered sum
    of four plain frames (in a child process: the library caches its RCCL handle per process)"""
    run_mock_transport_child("""
import numpy as np
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth, K, n = 80, 45, 16, 4, 16
cam = scene.default_camera(W, H)
subs, n_lanes = [], 0
for k in range(K):
    subs.append(srt.render_image(scene, cam, W, H, n // K, depth, seed=1984 + k * n_lanes))
    n_lanes = subs[0]['geom']['n_lanes']
xyz = [p.copy() for p in subs[0]['xyz']]
for s in subs[1:]:
    xyz = [(a + b).astype(np.float32) for a, b in zip(xyz, s['xyz'])]
single = list(srt.render_streams(scene, cam, W, H, [n], depth, K))[-1][1]
assert_planes_equal(single['xyz'], xyz, 'one rank vs the ordered sum')
comm = srt.Comm.init_all([0, 0])
for planes in (3, 9):
    comm.set_gather_planes(planes)
    comm.upload_scene(scene); comm.set_camera(cam)
    comm.init_device_params(W, H, 12, depth, 1984)
    comm.accum_reset_streams(K)
    for s in (4, 12):
        comm.render_frame_accum(W, H, s)
    comm.synchronize()
    root = comm.root
    assert all(r.accum_samples == n and r.accum_streams == K for r in comm.renderers)
    assert_planes_equal(root.read_fb(), single['fb'], 'world 2 planes %d fb' % planes)
    if planes == 9:
        assert_planes_equal(root.read_fb_aux(1), single['lin'], 'world 2 lin')
        assert_planes_equal(root.read_fb_aux(2), xyz, 'world 2 xyz')
    assert comm.stats()['paths'] == W * H * 12
comm.close()
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
        _setup(gpu, scene, cam, W, H, depth, seed=SEED + k * n_lanes)
        n_lanes = gpu.geom["n_lanes"]
        gpu.accum_reset(); gpu.render_chunk_accum(W, H, n1 // K)
        gpu.accum_reset(); gpu.render_chunk_accum(W, H, n2 // K)
        subs.append(_planes(gpu, W, H))
    want = _predicted(orc, [s["xyz"] for s in subs], n2, check_plain=subs[0])
    _setup(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, n1)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, n2)
    assert gpu.accum_samples == n2
    got = _planes(gpu, W, H)
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(got[k], want[k], "second streamed accumulation " + k)

    # a plain launch after a streamed accumulation continues stream 0: the plain context after n / K samples
    _setup(gpu, scene, cam, W, H, depth, spp=3)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, 8)
    gpu.render_chunk(W, H)
    after_streams = _planes(gpu, W, H)
    _setup(gpu, scene, cam, W, H, depth, spp=3)
    gpu.accum_reset(); gpu.render_chunk_accum(W, H, 8 // K)
    gpu.render_chunk(W, H)
    _assert_same_image(after_streams, _planes(gpu, W, H), "plain launch after a streamed accumulation")

    # srt_init_device_params with another seed: the fresh prediction of that seed (the streams above had advanced)
    other = 77001
    want = _prediction(srt, gpu, orc, "dielectric", wl, 24, K, seed=other)
    _setup(gpu, scene, cam, W, H, depth, seed=other)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, 24)
    _assert_same_image(_planes(gpu, W, H), want, "after srt_init_device_params with another seed")
    # ... and with the first seed again
    _setup(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_streams(K); gpu.render_chunk_accum(W, H, 24)
    _assert_same_image(_planes(gpu, W, H), _prediction(srt, gpu, orc, "dielectric", wl, 24, K), "re-seeded with the first seed")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_change_nothing(srt, gpu, orc):
    wl, _ = _named(srt, "dielectric")
    scene, cam, W, H, depth = wl
    K = 4
    want = _prediction(srt, gpu, orc, "dielectric", wl, 24, K)
    _setup(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_streams(K)
    assert gpu.accum_streams == K and gpu.accum_samples == 0
    gpu.render_chunk_accum(W, H, 8)
    after_first = _planes(gpu, W, H)
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
        _expect_error(srt, fn, code, what)
        assert gpu.accum_samples == 8 and gpu.accum_streams == K, what
    gpu.set_count_traversal(True)
    _expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 16), ERR_UNSUPPORTED, "instrumented pass")
    _expect_error(srt, lambda: gpu.accum_reset_streams(K), ERR_UNSUPPORTED, "instrumented reset")
    gpu.set_count_traversal(False)
    assert gpu.accum_samples == 8 and gpu.accum_streams == K
    _assert_same_image(_planes(gpu, W, H), after_first, "frame after the refused calls")
    gpu.render_chunk_accum(W, H, 16)              # sums and RNG states of every stream were untouched: the exact total
    assert gpu.accum_samples == 24
    _assert_same_image(_planes(gpu, W, H), want, "accumulation continued after the refused calls")

    # device parameters not set
    bare = srt.Renderer(0)
    try:
        bare.upload_scene(scene); bare.set_camera(cam)
        _expect_error(srt, lambda: bare.accum_reset_streams(2), ERR_INVALID, "device parameters not set")
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
    _expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 8), ERR_INVALID, "after a plain launch")


# ---- 8. one frame at a BASELINE size ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_baseline_size_frame(srt, gpu):
    """1280 x 720 (BASELINE cfg 2's frame), K = 4, n = 8: ordered queues of thousands of rows and split rows, XYZ planes against four
    plain 2-spp frames"""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    W, H, depth, K, n = 1280, 720, 16, 4, 8
    cam = scene.default_camera(W, H)
    frames, n_lanes = [], 0
    for k in range(K):
        res = srt.render_image(scene, cam, W, H, n // K, depth, seed=SEED + k * n_lanes, renderer=gpu)
        n_lanes = res["geom"]["n_lanes"]
        frames.append(res["xyz"])
    (total, got), = list(srt.render_streams(scene, cam, W, H, [n], depth, K, renderer=gpu))
    assert total == n and got["stats"]["paths"] == W * H * n
    assert_planes_equal(got["xyz"], _sum_in_stream_order(frames), "1280 x 720 K = 4 XYZ")
