"""Shared by the accumulation suites (test_progressive, test_adaptive, test_spectral, test_streams, their *_api modules and
test_accum_full_size): workloads, the context set-up and plane read-back, the runs of each accumulation kind, the one-GPU emulation
of a partition, the every-shape scaffold, the float32 restatement of the adaptive criterion, the prediction of a streamed frame, and
the child process and communicator driver of the mock-transport tests.  No test module imports another: what two of them need lives
here (or in helpers.py)."""
import contextlib
import ctypes as C
import importlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_planes_equal, bits, custom_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
# the six shapes launch_render_mode can pick: (narrow, all_cached, paired)
SHAPES = {(1, 1, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0)}
# ... and the test knobs / tree that make the launcher pick each of them: (knobs, paired tree, expected shape)
EVERY_SHAPE_CASES = [
    (dict(), True, (1, 1, 1)),                                   # PAIRED, LDS resident, 16-bit references (the headline's shape)
    (dict(wide_refs=True, lds_cache_max=3), True, (0, 0, 1)),    # PAIRED, 32-bit references, inner tree partly from L2 (cfg 5's shape)
    (dict(), False, (1, 1, 0)),
    (dict(lds_cache_max=3), False, (1, 0, 0)),
    (dict(wide_refs=True), False, (0, 1, 0)),
    (dict(wide_refs=True, lds_cache_max=0), False, (0, 0, 0)),
]
EVERY_SHAPE_IDS = ["narrow-cached-paired", "wide-partial-paired", "narrow-cached", "narrow-partial", "wide-cached", "wide-partial"]
SCHED, MIN_SPP = [8, 4, 4, 4, 4], 8
SEED = 1984
NEVER = 1e-30          # a relative tolerance no pixel with any variance meets (tol^2 underflows to 0)
N_GRID = 95


def kernel_id():
    """tools/kernel_id.py as a module (tools/ is no package): the bundle walk and the render-kernel hashes"""
    spec = importlib.util.spec_from_file_location("kernel_id", os.path.join(ROOT, "tools", "kernel_id.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- workloads and progressive runs ------------------------------------------------------------------------------------------
def dielectric_scene(srt):
    """glass triangles in front of a lambertian floor and a light: refraction, total internal reflection and the valid-wavelength
    cut of dispersive paths"""
    tris = [((-4, -1, -4), (4, -1, -4), (4, -1, 4), 0, 0), ((-4, -1, -4), (4, -1, 4), (-4, -1, 4), 0, 0),
            ((-1.5, -0.8, 0.5), (1.5, -0.8, 0.5), (0.0, 1.8, 0.0), 1, 0), ((-1.2, -0.8, -0.6), (1.4, -0.8, -0.4), (0.1, 1.5, 0.9), 1, 0),
            ((-2, 3, -2), (2, 3, -2), (0, 3, 2), 2, 0), ((2.5, -1, -1), (3.5, -1, 0), (3.0, 1.0, -0.5), 3, 0)]
    mats = [(0, (0.73, 0.73, 0.73), 0.0, 0.0), (2, (1.0, 1.0, 1.0), 0.0, 0.0), (4, (1.0, 1.0, 1.0), 0.0, 3.0), (1, (0.8, 0.8, 0.8), 0.1, 0.0)]
    return custom_scene(srt, tris, mats, (0.5, 0.5, 0.5)).build_bvh(srt.BVH_SAH, 1984)      # (grey: no rgb2spec table)


def soup(srt, seed, n):
    """n small random triangles (lambertian, metallic, dielectric, emissive): an even n gives a PAIRED SAH tree"""
    rng = np.random.default_rng(7000 + seed)
    c = rng.uniform(-6, 6, (n, 3))
    v = [(c + rng.normal(0, 0.3, (n, 3))).astype(np.float32).astype(np.float64) for _ in range(3)]
    mat = rng.integers(0, 4, n)
    tris = [(tuple(v[0][k]), tuple(v[1][k]), tuple(v[2][k]), int(mat[k]), 0) for k in range(n)]
    mats = [(0, (0.6, 0.6, 0.6), 0.0, 0.0), (1, (1.0, 1.0, 1.0), 0.2, 0.0), (2, (1.0, 1.0, 1.0), 0.0, 0.0), (4, (1.0, 1.0, 1.0), 0.0, 2.0)]
    return custom_scene(srt, tris, mats, (0.5, 0.5, 0.5))


def named_workload(srt, name):
    if name == "prism":
        sc = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
        return sc, sc.default_camera(48, 40), 48, 40, 8, 0
    if name == "cornell":
        sc = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
        return sc, sc.default_camera(64, 48), 64, 48, 8, 0
    if name == "random_spheres":
        sc = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
        return sc, sc.default_camera(80, 45), 80, 45, 16, 1       # defocus lens, sky background
    sc = dielectric_scene(srt)
    return sc, srt.camera_init(56, 40, 45.0, (0.5, 0.8, 7.0), (0.0, 0.3, 0.0)), 56, 40, 12, 1


def split_passes(spp):
    """spp in two or three passes (one pass when spp == 1)"""
    k = min(3, spp)
    base, rem = divmod(spp, k)
    return [base + (1 if i < rem else 0) for i in range(k)]


def assert_same_image(got, want, what, rowmajor=True):
    assert_planes_equal(got["fb"], want["fb"], what + " fb")
    assert_planes_equal(got["lin"], want["lin"], what + " unquantised sRGB")
    assert_planes_equal(got["xyz"], want["xyz"], what + " XYZ sums")
    if rowmajor:
        assert_planes_equal(got["rowmajor"], want["rowmajor"], what + " row-major")


def progressive_steps(srt, gpu, scene, cam, W, H, passes, depth):
    """runs render_progressive to the end; returns the list of (spp_total, result)"""
    return list(srt.render_progressive(scene, cam, W, H, passes, depth, renderer=gpu))


def expect_error(srt, fn, code, what):
    with pytest.raises(srt.SrtError) as e:
        fn()
    assert e.value.code == code, (what, e.value)


# ---- the context: set-up, read-back, partitions on one GPU, forced launch shapes ---------------------------------------------------
def lane_of(geom, W, H):
    """block-linear lane of every row-major pixel of a W x H chunk at (0, 0) (rendering.cu:156-165)"""
    tx, ty, bx = geom["tx"], geom["ty"], geom["bx"]
    j, i = np.divmod(np.arange(W * H), W)
    gbx, gby = i // tx, j // ty
    return (j - gby * ty) * tx + (i - gbx * tx) + tx * ty * (gby * bx + gbx)


def fresh_context(gpu, scene, cam, W, H, depth, spp=12, seed=SEED):
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1); gpu.set_count_traversal(False)
    gpu.set_gather_planes(9)
    gpu.init_device_params(W, H, spp, depth, seed)


def read_frame(gpu, W, H):
    gpu.scatter_tiles()
    return dict(fb=gpu.read_fb(), lin=gpu.read_fb_aux(1), xyz=gpu.read_fb_aux(2), rowmajor=gpu.read_fb_rowmajor(W, H))


def gather_ranks(gpu, world, per_rank):
    """A partition of `world` ranks on one GPU.  per_rank(rank) sets the context up, sets the partition (rank, world), resets the
    accumulation and runs its passes; after each rank its tile buffer is copied out, and after the last the concatenated buffers are
    scattered into the framebuffer as an all-gather would leave them.  The partition is (0, 1) again afterwards.  Returns the
    list of what per_rank returned."""
    import torch
    values, parts = [], []
    for rank in range(world):
        values.append(per_rank(rank))
        gpu.synchronize()
        _, n_floats, _, _ = gpu.tile_buffer()
        staging = torch.empty(n_floats, dtype=torch.float32, device="cuda")
        gpu.copy_tile_buffer(staging.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        parts.append(staging.cpu().numpy().copy())
    gathered = torch.from_numpy(np.concatenate(parts)).cuda()
    del parts
    gpu.scatter_tiles(gathered.data_ptr())
    gpu.synchronize()
    gpu.set_partition(0, 1)
    return values


def shape_case(srt, paired):
    """the scene of the every-shape tests: (scene, cam, W, H, depth) of a triangle soup with a PAIRED tree or without"""
    n = 600 if paired else 601          # the SAH builder pairs an even triangle count
    scene = soup(srt, n, n).build_bvh(srt.BVH_SAH, 1984)
    assert scene.is_paired == paired
    W, H, depth = 48, 32, 8
    return scene, srt.camera_init(W, H, 50.0, (0.5, 1.0, 16.0), (0.0, 0.0, 0.0), defocus_angle=0.6, focus_dist=14.0), W, H, depth


@contextlib.contextmanager
def forced_shape(gpu, scene, knobs, expect):
    """the body's launches run under the test knobs `knobs`, which must have made the launcher pick the shape `expect`; the knobs are
    reset and the scene uploaded again whatever the body did"""
    gpu.set_test_knobs(**knobs)
    try:
        yield
        plan = gpu.launch_plan()
        assert (int(plan["narrow_refs"]), int(plan["all_cached"]), int(plan["paired"])) == expect, (plan, knobs)
    finally:
        gpu.set_test_knobs()
        gpu.upload_scene(scene)


# ---- adaptive runs and the restatement of their stop decisions -----------------------------------------------------------------
def converged_f32(s1, s2, n, min_spp, rel_tol, abs_tol):
    """render_kernel MODE 4's stopping test (srt_c_api.h, srt_kernels.hip adaptive_converged) in numpy float32, operation by operation:
    mean = S1 / n; v = S2 / n - mean * mean; v = max(v, 0); var_mean = v / (n - 1); tol = rel_tol * mean + abs_tol;
    converged = n >= min_spp && var_mean <= tol * tol, never when S1, S2, mean * mean or tol * tol is NaN or infinite.
    s1, s2: float32 arrays (or scalars); n: the samples (int array or scalar)."""
    f = np.float32
    s1 = np.asarray(s1, f); s2 = np.asarray(s2, f); n_i = np.asarray(n, np.int64)
    with np.errstate(all="ignore"):
        nf = n_i.astype(f)
        mean = s1 / nf
        mm = mean * mean
        v = s2 / nf - mm
        v = np.where(v > f(0), v, f(0)).astype(f)
        var_mean = v / (nf - f(1))
        tol = f(rel_tol) * mean + f(abs_tol)
        tt = tol * tol
        finite = np.isfinite(s1) & np.isfinite(s2) & np.isfinite(mm) & np.isfinite(tt)
        return (n_i >= min_spp) & finite & (var_mean <= tt)


def adaptive_run(gpu, scene, cam, W, H, depth, rel_tol, sched=SCHED, min_spp=MIN_SPP, abs_tol=0.0):
    """an adaptive run; per pass: dict(total, active, paths, stats (accum_stats), frame)"""
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_adaptive(rel_tol, abs_tol, min_spp)
    assert gpu.accum_active == 0
    out = []
    for s in sched:
        gpu.render_chunk_accum(W, H, s)
        out.append(dict(total=gpu.accum_samples, active=gpu.accum_active, paths=gpu.stats()["paths"], stats=gpu.accum_stats(W, H),
                        frame=read_frame(gpu, W, H)))
    return out


def predict_stops(never, rel_tol, abs_tol=0.0, min_spp=MIN_SPP):
    """samples map after every pass, from a run that never stops (its S1 / S2 at every boundary are those of every run)"""
    n_pix = never[0]["stats"]["sum_y"].size
    stop = np.zeros(n_pix, np.int64)           # 0: still active
    maps, actives = [], []
    for p in never:
        t = p["total"]
        conv = converged_f32(p["stats"]["sum_y"], p["stats"]["sum_y2"], t, min_spp, rel_tol, abs_tol)
        stop[(stop == 0) & conv] = t
        maps.append(np.where(stop == 0, t, stop))
        actives.append(int((stop == 0).sum()))
    return maps, stop, actives


def pick_tolerance(never):
    """the relative tolerance (on a fine geometric grid) under which the schedule ends with the most distinct sample counts while some
    pixels are still active: scenes with much background (constant luminance: those pixels stop at min_spp) have few pixels to spread"""
    best, best_n = None, 0
    for rel in np.geomspace(1e-4, 10.0, 241):
        maps, stop, _ = predict_stops(never, float(rel))
        n = len(np.unique(maps[-1]))
        if (stop == 0).any() and n > best_n:
            best, best_n = float(rel), n
    assert best is not None, "no tolerance leaves a pixel active"
    return best


def assert_pixels_equal(got, want, mask, lane, what):
    """the pixels of `mask` (row-major) are bit-identical in the quantised, sRGB and XYZ planes and in the row-major image"""
    for k in ("fb", "lin", "xyz"):
        for c in range(3):
            a, b = bits(got[k][c])[lane[mask]], bits(want[k][c])[lane[mask]]
            assert np.array_equal(a, b), "%s %s plane %d: %d of %d pixels differ" % (what, k, c, int((a != b).sum()), a.size)
    for c in range(3):
        a, b = bits(got["rowmajor"][c])[mask], bits(want["rowmajor"][c])[mask]
        assert np.array_equal(a, b), "%s row-major plane %d: %d of %d pixels differ" % (what, c, int((a != b).sum()), a.size)


def gpu_lib():
    return importlib.import_module("cuda-spectral-ray-tracer_amd").binding.lib()


def read_sum_y(gpu, W, H):
    """Y sums of a plain accumulation (sum_y needs no adaptive one)"""
    y = np.zeros(W * H, np.float32)
    gpu._ck(gpu_lib().srt_read_accum_stats(gpu._h, None, y.ctypes.data_as(C.POINTER(C.c_float)), None, W, H))
    return y


# ---- spectral runs ---------------------------------------------------------------------------------------------------------------
def spectral_run(gpu, scene, cam, W, H, depth, passes, spp=12):
    """a spectral accumulation of `passes`; returns (frame after the last pass, film (H, W, 95))"""
    fresh_context(gpu, scene, cam, W, H, depth, spp=spp)
    gpu.accum_reset_spectral()
    for s in passes:
        gpu.render_chunk_accum(W, H, s)
    return read_frame(gpu, W, H), gpu.read_spectral(W, H)


# ---- streamed runs and their prediction ------------------------------------------------------------------------------------------
# Sub-frames 0 and 1 must differ in at least a quarter of the chunk's pixels, else the sum order and the stream indexing go untested:
# asserted on the two workloads that carry the condition.  cornell at 64 x 48 is mostly background (measured: 629 of 3072 pixels
# differ at n / K = 12, 20.5 %), so, like prism, it is never used alone: it must differ somewhere, and runs next to the other two.
QUARTER = ("dielectric", "random_spheres")
_predictions = {}


def convert_xyz(orc, xyz, n):
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


def sum_in_stream_order(frames):
    total = [np.asarray(p, np.float32).copy() for p in frames[0]]
    for f in frames[1:]:
        total = [(t + np.asarray(p, np.float32)).astype(np.float32) for t, p in zip(total, f)]
    return tuple(total)


def predicted_frame(orc, xyz_frames, n, check_plain=None):
    """dict(fb, lin, xyz) of a streamed frame from the XYZ planes of its K plain frames.  check_plain: a plain frame of n / K samples,
    whose own planes the restatement of the conversion must reproduce before it is used"""
    if check_plain is not None:
        lin, q = convert_xyz(orc, check_plain["xyz"], n // len(xyz_frames))
        assert_planes_equal(lin, check_plain["lin"], "restated conversion, plain frame sRGB")
        assert_planes_equal(q, check_plain["fb"], "restated conversion, plain frame quantised")
    xyz = sum_in_stream_order(xyz_frames)
    lin, q = convert_xyz(orc, xyz, n)
    return dict(fb=q, lin=lin, xyz=xyz)


def stream_subframes(srt, gpu, workload, n, K, seed=SEED):
    """the K plain frames whose ordered sum a streamed frame of `workload` = (scene, cam, W, H, depth) is: frame k has n / K samples and
    the seed `seed` + k * n_lanes (gpu: the renderer, or None for one of render_image's own)"""
    scene, cam, W, H, depth = workload
    subs, n_lanes = [], 0
    for k in range(K):
        subs.append(srt.render_image(scene, cam, W, H, n // K, depth, seed=seed + k * n_lanes, renderer=gpu))
        n_lanes = subs[0]["geom"]["n_lanes"]
    return subs


def stream_prediction(srt, gpu, orc, name, workload, n, K, seed=SEED, must_differ=True):
    """the prediction of a whole-image streamed frame of `workload` = (scene, cam, W, H, depth), computed once per (name, n, K, seed)"""
    key = (name, n, K, seed)
    if key not in _predictions:
        W, H = workload[2:4]
        subs = stream_subframes(srt, gpu, workload, n, K, seed)
        lane = lane_of(subs[0]["geom"], W, H)
        if must_differ and K > 1:      # else the sum order and the stream indexing would go untested
            differ = np.zeros(W * H, bool)
            for c in range(3):
                differ |= bits(subs[0]["xyz"][c])[lane] != bits(subs[1]["xyz"][c])[lane]
            print("%s n/K = %d: sub-frames 0 and 1 differ in %d of %d pixels" % (name, n // K, differ.sum(), W * H))
            assert differ.sum() * (4 if name in QUARTER else W * H) >= W * H, "%s: sub-frames 0 and 1 differ in only %d of %d pixels" % (name, differ.sum(), W * H)
        want = predicted_frame(orc, [s["xyz"] for s in subs], n, check_plain=subs[0])
        want["rowmajor"] = tuple(p[lane] for p in want["fb"])
        want["subs"] = subs
        _predictions[key] = want
    return _predictions[key]


# ---- the communicator over the test transport ------------------------------------------------------------------------------------
def run_mock_transport_child(body, ok_token, timeout):
    """Runs `body` (Python source; `srt` is the imported package, tests/ is on sys.path) in a FRESH process with the test transport
    (tests/cpp/mock_rccl.cpp) in place of RCCL and all ranks on device 0, and asserts that it exits with 0 after printing ok_token.
    A child process because the library caches its RCCL handle per process.  Returns what the child printed."""
    mock = os.path.join(ROOT, "tests", "cpp", "_build", "libmock_rccl.so")
    assert os.path.exists(mock), "tests/cpp/_build/libmock_rccl.so is built by __graft_entry__.build()"
    code = """
import importlib, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
srt = importlib.import_module('cuda-spectral-ray-tracer_amd')
""" % (ROOT, os.path.join(ROOT, "tests")) + body
    env = dict(os.environ, SRT_RCCL_LIB=mock, SRT_COMM_TEST_SAME_DEVICE="1", SRT_TEST_KNOBS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and ok_token in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
    return out.stdout


def comm_accumulations(srt, world, planes, scene, cam, W, H, depth, spp, reset, passes):
    """For the child processes above: one communicator of `world` ranks on device 0 and, for every p of `planes` in turn, gather
    planes p, scene, camera, device parameters, reset(comm) and the passes of `passes`.  Yields (p, comm) with comm synchronised;
    closes the communicator after the last."""
    comm = srt.Comm.init_all([0] * world)
    for p in planes:
        comm.set_gather_planes(p)
        comm.upload_scene(scene); comm.set_camera(cam)
        comm.init_device_params(W, H, spp, depth, SEED)
        reset(comm)
        for s in passes:
            comm.render_frame_accum(W, H, s)
        comm.synchronize()
        yield p, comm
    comm.close()
