"""First-hit feature buffers, the interface.  Without a GPU: the entry points are declared, bound and exported, the code object holds
render_kernel<7, ...> for every shape the launcher picks, feature_means on a hand-made array, and the draw count of the CPU prediction's
restated camera ray (tests/features_reference.py) against the oracle on emissive-only scenes.  On the GPU: refusals and invalidations
with nothing changed on the device, the growth of the grid, the communicator over the test transport, and render_features."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, ROOT, SHAPES, expect_error, fresh_context, gpu_lib, kernel_id, lane_of,
                           named_workload, read_frame, run_mock_transport_child)
from features_reference import camera_rays, grid_of, seeded_states, stack_features, workload_prediction
from helpers import assert_planes_equal, bits, custom_scene, oracle_scene_for

NEW_SYMBOLS = ("srt_accum_reset_features", "srt_read_features", "srt_comm_accum_reset_features")
FEATURES_SYM = re.compile(r"^_ZN3srt13render_kernelILi7ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, fp = C.c_uint32, C.POINTER(C.c_float)
    assert srt.binding.PROTOTYPES["srt_accum_reset_features"] == (C.c_int, [C.c_void_p])
    assert srt.binding.PROTOTYPES["srt_read_features"] == (C.c_int, [C.c_void_p, fp, u32, u32])
    assert srt.binding.PROTOTYPES["srt_comm_accum_reset_features"] == (C.c_int, [C.c_void_p])
    for name in ("render_features", "feature_means"):
        assert name in srt.__all__ and callable(getattr(srt, name)), name
    for attr in ("accum_reset_features", "read_features"):
        assert hasattr(srt.Renderer, attr), attr
    assert hasattr(srt.Comm, "accum_reset_features")
    # the deposit rule and the intended next step are part of the contract the header states
    for phrase in ("F[0..2] normal, F[3..5] albedo, F[6] distance, F[7] hits", "front_face ? n_geo : -n_geo", "t * sqrtf(dx*dx + dy*dy + dz*dz)",
                   "adaptive + features is the intended next step"):
        assert phrase in header, phrase


def test_code_object_holds_every_featured_variant(srt):
    found = set()
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        m = FEATURES_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)
    assert {k[1:] for k in kernel_id().render_code_hashes(srt.binding.LIB_PATH) if k[0] == 7} == SHAPES


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    out = np.zeros(8, np.float32)
    assert lib.srt_accum_reset_features(None) == ERR_INVALID
    assert lib.srt_read_features(None, srt.binding.fptr(out), 1, 1) == ERR_INVALID
    assert lib.srt_comm_accum_reset_features(None) == ERR_INVALID


def test_feature_means_on_a_hand_made_array(srt):
    feat = dict(normal=np.array([[[0, 0, 4], [0, -2, 0]], [[0, 0, 0], [1, 1, 2]]], np.float32),
                albedo=np.array([[[2, 1, 0.5], [0.5, 0.5, 0.5]], [[0, 0, 0], [4, 4, 4]]], np.float32),
                distance=np.array([[20, 3], [0, 10]], np.float32), hits=np.array([[4, 2], [0, 4]], np.float32))
    m = srt.feature_means(feat, 4)
    assert set(m) == {"normal", "albedo", "distance", "coverage"} and all(v.dtype == np.float64 for v in m.values())
    np.testing.assert_array_equal(m["normal"], [[[0, 0, 1], [0, -0.5, 0]], [[0, 0, 0], [0.25, 0.25, 0.5]]])
    np.testing.assert_array_equal(m["albedo"], [[[0.5, 0.25, 0.125], [0.125, 0.125, 0.125]], [[0, 0, 0], [1, 1, 1]]])
    np.testing.assert_array_equal(m["distance"], [[5, 1.5], [np.inf, 2.5]])
    np.testing.assert_array_equal(m["coverage"], [[1, 0.5], [0, 1]])
    # a per-pixel sample map
    m = srt.feature_means(feat, np.array([[4, 2], [8, 16]]))
    np.testing.assert_array_equal(m["coverage"], [[1, 1], [0, 0.25]])
    np.testing.assert_array_equal(m["normal"][0, 1], [0, -1, 0])
    np.testing.assert_array_equal(m["distance"], [[5, 1.5], [np.inf, 2.5]])
    with pytest.raises(ValueError):
        srt.renderer.split_features(np.zeros((2, 2, 7), np.float32))
    rows = np.arange(16, dtype=np.float32).reshape(1, 2, 8)
    parts = srt.renderer.split_features(rows)
    assert parts["normal"].shape == (1, 2, 3) and parts["hits"].tolist() == [[7, 15]] and parts["distance"].tolist() == [[6, 14]]
    np.testing.assert_array_equal(stack_features(parts), rows)


@pytest.mark.parametrize("kw", [dict(passes=[]), dict(passes=[0]), dict(passes=[4, -1]), dict(passes=[65535, 1])],
                         ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_render_features_rejects_bad_schedules_before_touching_a_device(srt, kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_features created a device context for a schedule it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_features(None, None, 16, 16, bounce_limit=8, **kw)


@pytest.mark.parametrize("defocus", [0.0, 1.5], ids=["pinhole", "lens"])
def test_restated_camera_ray_draws_what_the_oracle_draws(srt, orc, defocus):
    """On an emissive-only scene no path draws after its camera ray (a miss and an emissive hit both end the path without a draw): the
    restated per-sample draws -- jitter, lens, hero wavelength -- must leave every pixel's state where the oracle's 1-spp render does."""
    tris = [((-2, -2, 0), (2, -2, 0), (0, 2, 0), 0, 0), ((-4, -1, -3), (-1, -1, -3), (-2, 3, -3), 1, 0), ((1, -3, -2), (4, -3, -2), (3, 1, -2), 0, 0)]
    mats = [(srt.binding.MAT_EMISSIVE, (1.0, 1.0, 1.0), 0.0, 2.0), (srt.binding.MAT_EMISSIVE, (0.5, 0.5, 0.5), 0.0, 1.0)]
    scene = custom_scene(srt, tris, mats).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, depth = 37, 21, 5
    cam = srt.camera_init(W, H, 55.0, (0.3, 0.2, 8.0), (0.0, 0.0, 0.0), defocus_angle=defocus, focus_dist=8.0)
    osc = oracle_scene_for(orc, scene, 0)
    geom = grid_of(W, H)
    lane = lane_of(geom, W, H)
    states = seeded_states(orc, geom)
    hit_any = False
    for _ in range(3):
        o, d, after = camera_rays(orc, cam, states, lane, W, H)
        if defocus > 0:
            assert (o != o[0]).any(), "the lens moved no origin"
        else:
            assert (o == o[0]).all()
        before = states.copy()
        ref = osc.render(cam, W, H, 1, depth, states=states)
        assert ref["stats"]["rays"] == W * H      # one query per path: nothing scattered
        hit_any |= max(float(p.max()) for p in ref["xyz"]) > 0
        assert np.array_equal(states[lane], after), "%d of %d states differ" % (int((states[lane] != after).any(axis=1).sum()), W * H)
        assert (states[lane] != before[lane]).any(axis=1).all()
    assert hit_any, "the camera saw no emitter"


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------
def _run(gpu, W, H, passes):
    gpu.accum_reset_features()
    for s in passes:
        gpu.render_chunk_accum(W, H, s)
    return stack_features(gpu.read_features(W, H))


@pytest.mark.gpu
def test_refusals_leave_the_accumulation_as_it_was(srt, gpu, orc):
    n = 6
    (scene, cam, W, H, depth, _), want = workload_prediction(srt, orc, "prism", n)
    L = gpu_lib()
    buf = np.zeros(W * H * 8, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    # device parameters not set
    fresh = srt.Renderer(0)
    try:
        assert L.srt_accum_reset_features(fresh._h) == ERR_INVALID
        assert L.srt_read_features(fresh._h, fp, W, H) == ERR_INVALID
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, "read before the first pass")
    gpu.render_chunk_accum(W, H, 2)
    first = stack_features(gpu.read_features(W, H))
    frame = read_frame(gpu, W, H)
    assert L.srt_read_features(gpu._h, None, W, H) == ERR_INVALID
    assert L.srt_read_features(gpu._h, fp, 0, H) == ERR_INVALID and L.srt_read_features(gpu._h, fp, W, 0) == ERR_INVALID
    # refused passes (srt_accum_reset's rules): nothing enqueued
    assert L.srt_render_chunk_accum(gpu._h, W, H, 0, 0, 0, None) == ERR_INVALID
    assert L.srt_render_chunk_accum(gpu._h, W, H, 0, 0, 65534, None) == ERR_INVALID            # 2 + 65534 > 65535
    assert L.srt_render_chunk_accum(gpu._h, W - 1, H, 0, 0, 1, None) == ERR_INVALID             # another chunk
    assert L.srt_render_chunk_accum(gpu._h, W, H, 1, 0, 1, None) == ERR_INVALID                 # another offset
    # a refused reset (instrumented context) leaves the accumulation usable
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.accum_reset_features(), ERR_UNSUPPORTED, "instrumented context")
    gpu.set_count_traversal(False)
    assert gpu.accum_samples == 2
    assert np.array_equal(bits(stack_features(gpu.read_features(W, H))), bits(first))
    for k, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, frame[k], "after the refusals " + k)
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == n and gpu.stats()["paths"] == W * H * 4
    assert np.array_equal(bits(stack_features(gpu.read_features(W, H))), bits(want["rows"]))


@pytest.mark.gpu
def test_invalidations_and_other_accumulation_kinds(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    for what, call in (("srt_set_camera", lambda: gpu.set_camera(cam)), ("srt_render_chunk", lambda: gpu.render_chunk(W, H)),
                       ("srt_upload_scene", lambda: gpu.upload_scene(scene)), ("srt_set_partition", lambda: gpu.set_partition(0, 1)),
                       ("srt_init_device_params", lambda: gpu.init_device_params(W, H, 12, depth, 1984)),
                       ("srt_accum_reset", lambda: gpu.accum_reset()),
                       ("srt_accum_reset_adaptive", lambda: gpu.accum_reset_adaptive(0.1, 0.0, 4)),
                       ("srt_accum_reset_spectral", lambda: gpu.accum_reset_spectral()),
                       ("srt_accum_reset_streams", lambda: gpu.accum_reset_streams(2))):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_features()
        gpu.render_chunk_accum(W, H, 2)
        gpu.read_features(W, H)
        call()
        if what.startswith("srt_accum_reset"):
            gpu.render_chunk_accum(W, H, 2)      # a pass of the new accumulation, which keeps no feature rows
            assert gpu.accum_samples == 2
        else:
            expect_error(srt, lambda: gpu.render_chunk_accum(W, H, 2), ERR_INVALID, what + ": pass on an invalidated accumulation")
        expect_error(srt, lambda: gpu.read_features(W, H), ERR_INVALID, what)
    # ... and the other way round: a featured accumulation has no film, no sample map and no streams
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, H, 2)
    expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "film of a featured accumulation")
    expect_error(srt, lambda: gpu.accum_stats(W, H), ERR_INVALID, "sample map of a featured accumulation")
    assert gpu.accum_streams == 0
    gpu.set_gather_planes(9)


@pytest.mark.gpu
def test_growth_of_the_grid_reallocates_the_rows(srt, orc):
    n = 6
    (scene, cam, W, H, depth, _), want = workload_prediction(srt, orc, "prism", n)
    # a context of its own, whose first rows are those of a small grid (one block); the workload's larger grid must get larger ones
    r = srt.Renderer(0)
    try:
        small = scene.default_camera(20, 12)
        fresh_context(r, scene, small, 20, 12, depth)
        assert r.geom["n_lanes"] == 448
        a = _run(r, 20, 12, [2])
        assert a.shape == (12, 20, 8) and a[..., 7].max() > 0
        fresh_context(r, scene, cam, W, H, depth)
        assert r.geom["n_lanes"] > 448
        b = _run(r, W, H, [n])
        assert np.array_equal(bits(b), bits(want["rows"]))
        # ... and back to the small one: its rows start from zero again
        fresh_context(r, scene, small, 20, 12, depth)
        assert np.array_equal(bits(_run(r, 20, 12, [2])), bits(a))
    finally:
        r.close()


@pytest.mark.gpu
def test_render_features_yields_what_the_manual_calls_give(srt, gpu, orc):
    n = 6
    (scene, cam, W, H, depth, _), want = workload_prediction(srt, orc, "dielectric", n)
    steps = list(srt.render_features(scene, cam, W, H, [2, 4], depth, renderer=gpu))
    assert [t for t, _, _ in steps] == [2, 6]
    for t, res, feat in steps:
        assert set(res) == {"fb", "lin", "xyz", "rowmajor", "stats", "kernel_ms", "geom"}
        assert set(feat) == {"normal", "albedo", "distance", "hits"}
        assert feat["normal"].shape == (H, W, 3) and feat["albedo"].shape == (H, W, 3) and feat["distance"].shape == (H, W) and feat["hits"].shape == (H, W)
        assert feat["hits"].max() <= t
    assert np.array_equal(bits(stack_features(steps[-1][2])), bits(want["rows"]))
    fresh_context(gpu, scene, cam, W, H, depth)
    manual = _run(gpu, W, H, [2])
    assert np.array_equal(bits(stack_features(steps[0][2])), bits(manual))
    one_shot = srt.render_image(scene, cam, W, H, n, depth, renderer=gpu)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(steps[-1][1][k], one_shot[k], "render_features vs render_image " + k)
    means = srt.feature_means(steps[-1][2], n)
    assert means["coverage"].min() == 0.0 and means["coverage"].max() == 1.0 and np.isinf(means["distance"]).any()
    unit = np.linalg.norm(means["normal"][means["coverage"] == 1.0], axis=-1)
    assert unit.max() <= 1.0 + 1e-6


@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations, named_workload
from features_reference import stack_features
from helpers import assert_planes_equal, bits
scene, cam, W, H, depth, _ = named_workload(srt, 'random_spheres')
steps = list(srt.render_features(scene, cam, W, H, [2, 4], depth))
total, ref, feat = steps[-1]
want = stack_features(feat)
assert total == 6 and want[..., 7].max() == 6
for _, comm in comm_accumulations(srt, 2, (9,), scene, cam, W, H, depth, 6, lambda c: c.accum_reset_features(), (2, 4)):
    root = comm.root
    assert_planes_equal(root.read_fb(), ref['fb'], 'fb')
    assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'xyz')
    parts = [stack_features(r.read_features(W, H)) for r in comm.renderers]
    assert len(parts) == 2
    nonzero = np.stack([(bits(p) != 0).any(axis=-1) for p in parts])
    assert (nonzero.sum(axis=0) <= 1).all() and nonzero[0].any() and nonzero[1].any()
    assert np.array_equal(bits(parts[0] + parts[1]), bits(want))
r = srt.Renderer(0)
c1 = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
c1.set_gather_planes(9)
c1.upload_scene(scene); c1.set_camera(cam); c1.init_device_params(W, H, 6, depth, 1984)
c1.accum_reset_features()
for s in (2, 4):
    c1.render_frame_accum(W, H, s)
c1.synchronize()
assert np.array_equal(bits(stack_features(r.read_features(W, H))), bits(want))
c1.close(); r.close()
print('features mock transport ok')
""", "features mock transport ok", timeout=300)
