"""Progressive rendering (srt_accum_reset / srt_render_chunk_accum, render_kernel MODE 3): passes of s1 .. sk samples accumulated into
one frame are bit-identical to a one-shot render of s1 + .. + sk samples -- framebuffer, parity planes, row-major image and RNG state.
The one-shot frames are themselves held to the CPU oracle and to the frozen digests by the parity suite, so every comparison here is
against an exact reference."""
import json
import os

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, ROOT, assert_same_image, expect_error,
                           forced_shape, gather_ranks, named_workload, progressive_steps, read_frame, run_mock_transport_child, shape_case,
                           split_passes)
from helpers import DIGEST_PLANES, assert_planes_equal, digest_of_render, digest_workloads, oracle_scene_for

SPLITS = [[12], [5, 7], [1, 1, 10], [4, 4, 4]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "cornell", "random_spheres", "dielectric"])
def test_split_equals_one_shot_bit_for_bit(srt, gpu, orc, name):
    scene, cam, W, H, depth, mode = named_workload(srt, name)
    one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
    for passes in SPLITS:
        steps = progressive_steps(srt, gpu, scene, cam, W, H, passes, depth)
        assert [t for t, _ in steps] == list(np.cumsum(passes)), steps
        total, last = steps[-1]
        assert_same_image(last, one_shot, "%s split %r" % (name, passes))
        assert set(last) == set(one_shot)
        pixels = W * H
        assert last["stats"]["paths"] == pixels * passes[-1], (last["stats"], passes)     # the stats of the last pass
        assert last["kernel_ms"] > 0.0
    if name == "prism":     # once directly against the CPU oracle as well
        ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, 12, depth)
        for k in ("fb", "lin", "xyz"):
            assert_planes_equal(last[k], ref[k], "prism [4, 4, 4] vs oracle " + k)


@pytest.mark.gpu
def test_intermediate_passes_equal_one_shot_of_their_total(srt, gpu):
    """every yielded frame, not only the last, is the one-shot frame of the samples so far"""
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    steps = progressive_steps(srt, gpu, scene, cam, W, H, [2, 3, 7], depth)
    for total, res in steps:
        assert_same_image(res, srt.render_image(scene, cam, W, H, total, depth, renderer=gpu), "after %d samples" % total)


@pytest.mark.gpu
def test_frozen_digests_in_several_passes(srt, gpu):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_digests.json")))
    for name, (scene, cam, W, H, spp, depth, _) in sorted(digest_workloads(srt).items()):
        passes = split_passes(spp)
        total, res = progressive_steps(srt, gpu, scene, cam, W, H, passes, depth)[-1]
        assert total == spp == golden[name]["spp"]
        got = digest_of_render(res)
        for plane in DIGEST_PLANES:
            assert got[plane] == golden[name][plane], (name, passes, plane)


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_accumulating_shape_is_exact(srt, gpu, knobs, paired, expect):
    scene, cam, W, H, depth = shape_case(srt, paired)
    with forced_shape(gpu, scene, knobs, expect):
        one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
        for passes in ([5, 7], [1, 1, 10]):
            _, last = progressive_steps(srt, gpu, scene, cam, W, H, passes, depth)[-1]
            assert_same_image(last, one_shot, "shape %r split %r" % (expect, passes))


@pytest.mark.gpu
def test_partition_and_offset_chunk(srt, gpu):
    """ranks 0..W-1 of a partition, each accumulated on its own and scattered together, equal the one-shot frame; so does a chunk at a
    non-zero offset of a larger image"""
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    ref = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)
    for world in (2, 3):
        def one_rank(rank):         # (not fresh_context: the gather planes and the counting stay as the session left them)
            gpu.upload_scene(scene); gpu.set_camera(cam)
            gpu.init_device_params(W, H, 12, depth, 1984)
            gpu.set_partition(rank, world)
            gpu.accum_reset()
            for s in (5, 7):
                gpu.render_chunk_accum(W, H, s)
        gather_ranks(gpu, world, one_rank)
        assert_planes_equal(gpu.read_fb(), ref["fb"], "world %d fb" % world)
        assert_planes_equal(gpu.read_fb_aux(1), ref["lin"], "world %d lin" % world)
        assert_planes_equal(gpu.read_fb_aux(2), ref["xyz"], "world %d xyz" % world)

    # a 30 x 20 chunk at (17, 9) of a 64 x 40 image
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 20, 17, 9
    cam = scene.default_camera(IW, IH)

    def chunk(accumulate):
        gpu.upload_scene(scene); gpu.set_camera(cam)
        gpu.init_device_params(cw, ch, 12, depth, 1984)
        if accumulate:
            gpu.accum_reset()
            for s in (1, 4, 7):
                gpu.render_chunk_accum(cw, ch, s, ox, oy)
        else:
            gpu.render_chunk(cw, ch, ox, oy)
        return read_frame(gpu, IW, IH)
    assert_same_image(chunk(True), chunk(False), "offset chunk")


@pytest.mark.gpu
def test_comm_two_and_three_ranks_one_gpu_mock_transport():
    """srt_comm_accum_reset / srt_render_frame_multi_accum at W = 2 and 3 on ONE GPU over the test transport (tests/cpp/mock_rccl.cpp,
    as the parity suite's communicator test does; the library caches its RCCL handle per process, so this runs in a child process)"""
    run_mock_transport_child("""
from accum_helpers import comm_accumulations
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth = 150, 90, 16
cam = scene.default_camera(W, H)
ref = srt.render_image(scene, cam, W, H, 12, depth)
for world in (2, 3):
    for planes, comm in comm_accumulations(srt, world, (3, 9), scene, cam, W, H, depth, 12, lambda c: c.accum_reset(), (5, 7)):
        root = comm.root
        assert all(r.accum_samples == 12 for r in comm.renderers)
        assert_planes_equal(root.read_fb(), ref['fb'], 'world %d planes %d fb' % (world, planes))
        if planes == 9:
            assert_planes_equal(root.read_fb_aux(1), ref['lin'], 'world %d lin' % world)
            assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'world %d xyz' % world)
        st = comm.stats()
        assert st['paths'] == W * H * 7, st
print('progressive mock transport ok')
""", "progressive mock transport ok", timeout=300)


@pytest.mark.gpu
def test_plain_render_after_accumulation_continues_rng_streams(srt, gpu, orc):
    """the RNG state an accumulation leaves is the one-shot's: a plain launch after [5, 7] equals the oracle continued from the states
    after 12 samples"""
    import ctypes as C
    scene, cam, W, H, depth, mode = named_workload(srt, "prism")
    spp_next = 3
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1)
    gpu.init_device_params(W, H, spp_next, depth, 1984)
    gpu.accum_reset()
    for s in (5, 7):
        gpu.render_chunk_accum(W, H, s)
    gpu.render_chunk(W, H)
    gpu.scatter_tiles()
    after = dict(fb=gpu.read_fb(), xyz=gpu.read_fb_aux(2))
    osc = oracle_scene_for(orc, scene, mode)
    n = gpu.geom["n_lanes"]
    states = np.zeros(6 * n, np.uint32)
    for idx in range(n):
        s = orc.Rng()
        orc.lib().orc_rng_init(1984 + idx, C.byref(s))
        states[6 * idx: 6 * idx + 6] = [s.d] + list(s.v)
    osc.render(cam, W, H, 12, depth, states=states)           # the accumulation's 12 samples
    ref = osc.render(cam, W, H, spp_next, depth, states=states)
    assert_planes_equal(after["xyz"], ref["xyz"], "plain launch after the accumulation, XYZ")
    assert_planes_equal(after["fb"], ref["fb"], "plain launch after the accumulation, fb")


@pytest.mark.gpu
def test_refused_calls_and_invalidation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    one_shot = srt.render_image(scene, cam, W, H, 12, depth, renderer=gpu)

    def fresh():
        gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1)
        gpu.init_device_params(W, H, 12, depth, 1984)

    # no accumulation yet
    fresh()
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 4), ERR_INVALID, "pass before srt_accum_reset")
    assert gpu.accum_samples == 0
    gpu.accum_reset()
    assert gpu.accum_samples == 0
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 65536), ERR_INVALID, "total above 65535")
    gpu.render_chunk_accum(W, H, 5)
    assert gpu.accum_samples == 5 and gpu.stats()["paths"] == W * H * 5
    after_first = read_frame(gpu, W, H)

    # refusals: nothing changes on the device (framebuffer, tile buffer, sums, RNG state)
    refusals = [
        (lambda: gpu.render_chunk_accum(W, H, 0), ERR_INVALID, "spp_add 0"),
        (lambda: gpu.render_chunk_accum(W, H, 65531), ERR_INVALID, "total 65536"),
        (lambda: gpu.render_chunk_accum(W - 1, H, 7), ERR_INVALID, "another chunk width"),
        (lambda: gpu.render_chunk_accum(W, H - 8, 7), ERR_INVALID, "another chunk height"),
        (lambda: gpu.render_chunk_accum(W, H, 7, 1, 0), ERR_INVALID, "another offset"),
        (lambda: gpu.render_chunk_accum(W, H, 7, 0, 2), ERR_INVALID, "another offset"),
    ]
    for fn, code, what in refusals:
        expect_error(srt, fn, code, what)
        assert gpu.accum_samples == 5, what
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 7), ERR_UNSUPPORTED, "instrumented context")
    gpu.set_count_traversal(False)
    assert_same_image(read_frame(gpu, W, H), after_first, "framebuffer after the refused calls")
    gpu.render_chunk_accum(W, H, 7)               # the sums and the RNG states were untouched: the total is the one-shot frame
    assert gpu.accum_samples == 12
    assert_same_image(read_frame(gpu, W, H), one_shot, "accumulation continued after the refused calls")

    # invalidation: each of these calls ends the accumulation until the next reset
    invalidators = [
        ("srt_init_device_params", lambda: gpu.init_device_params(W, H, 12, depth, 1984)),
        ("srt_set_partition", lambda: gpu.set_partition(0, 1)),
        ("srt_upload_scene", lambda: gpu.upload_scene(scene)),
        ("srt_set_camera", lambda: gpu.set_camera(cam)),
        ("srt_render_chunk", lambda: gpu.render_chunk(W, H)),
    ]
    for what, call in invalidators:
        fresh()
        gpu.accum_reset()
        gpu.render_chunk_accum(W, H, 2)
        call()
        expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 2), ERR_INVALID, what)
        assert gpu.accum_samples == 0, what
        gpu.accum_reset()
        gpu.render_chunk_accum(W, H, 2)       # a reset makes the context usable again
        assert gpu.accum_samples == 2, what
    # srt_order_children_by_profile (on a scene of its own: it re-orders the tree in place) uploads a scene and spends the RNG state
    fresh()
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    other = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    try:
        gpu.order_children_by_profile(other, W, H, 2, depth, 1)
    except srt.SrtError:
        pass            # (a probe frame that records nothing is declined: the accumulation is dropped before anything else)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 2), ERR_INVALID, "srt_order_children_by_profile")
    assert gpu.accum_samples == 0

    # a refused pass after a plain launch leaves the plain frame alone
    fresh()
    gpu.render_chunk(W, H)
    plain = read_frame(gpu, W, H)
    expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 3), ERR_INVALID, "after a plain launch")
    assert_same_image(read_frame(gpu, W, H), plain, "plain frame after a refused pass")
    assert_same_image(plain, one_shot, "plain frame")
