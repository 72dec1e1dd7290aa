"""BVH refit on the device (srt_refit_vertices / srt_refit_vertices_dev) against the upload of the host-refitted scene.

Every case uses two contexts.  Context A uploads the original scene, gets its camera and device parameters, and is refitted; context B
uploads the scene srt_scene_refit left (tests/test_refit_host.py holds that one to a fresh build and to the oracle).  Then: all five
scene images are equal as values (bits equal, both NaN, or both zero -- srt_c_api.h), the launch plans agree, explicit rays hit
bit-identically, a small frame is bit-identical in all nine planes, and so is the frame after it -- the RNG state of a context is visible
through the streams it continues, and only there.  A's frame also equals the oracle's on the moved scene."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import refit_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_b(srt):
    r = srt.Renderer(0)
    r.set_gather_planes(9)
    yield r
    r.close()


def _images(r):
    return {name: r.scene_image(name) for name in R.IMAGES}


def _assert_images(a, b, what, exact=False):
    for name in R.IMAGES:
        assert a[name].shape == b[name].shape, (what, name, a[name].shape, b[name].shape)
        if exact:
            assert np.array_equal(a[name], b[name]), "%s: image %s differs in bits" % (what, name)
        else:
            R.assert_values_equal(a[name], b[name], "%s: image %s" % (what, name))


def _setup(r, scene, cam, W, Hh, spp, depth):
    r.upload_scene(scene); r.set_camera(cam); r.set_partition(0, 1)
    r.init_device_params(W, Hh, spp, depth, 1984)
    r.set_count_traversal(False)


def _frame(r, W, Hh):
    r.render_chunk(W, Hh); r.scatter_tiles()
    return r.read_fb() + r.read_fb_aux(1) + r.read_fb_aux(2)


def _lds_bytes(srt, r):
    n = C.c_size_t()
    srt.binding.check(srt.binding.lib().srt_launch_lds_bytes(r._h, C.byref(n)), r._h)
    return n.value


def _rays(scene, n=300):
    """a few hundred rays from around the scene towards points near its triangles' vertices, some of them exactly through a vertex"""
    rng = np.random.default_rng(4242)
    v = scene.vertices().reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    o = rng.uniform(lo - 3, hi + 3, (n, 3))
    target = v[rng.integers(0, v.shape[0], n)] + np.where(rng.random((n, 1)) < 0.2, 0.0, rng.normal(0, 0.3, (n, 3)))
    return np.ascontiguousarray(np.concatenate([o, target - o], axis=1), np.float32)


def _check_against_upload(srt, orc, A, B, scene, cam, W, Hh, spp, depth, what, oracle=True):
    """A holds the refitted images and its camera and device parameters from before the refit; `scene` is the host-refitted scene"""
    _setup(B, scene, cam, W, Hh, spp, depth)
    _assert_images(_images(A), _images(B), what)
    assert A.launch_plan() == B.launch_plan(), what
    assert _lds_bytes(srt, A) == _lds_bytes(srt, B), what
    rays = _rays(scene)
    assert np.array_equal(A.trace_rays(rays).view(np.uint32), B.trace_rays(rays).view(np.uint32)), what + ": srt_trace_rays differs"
    first_a, first_b = _frame(A, W, Hh), _frame(B, W, Hh)
    H.assert_planes_equal(first_a, first_b, what + ": frame")
    assert A.stats()["rays"] == B.stats()["rays"]
    H.assert_planes_equal(_frame(A, W, Hh), _frame(B, W, Hh), what + ": the frame after it (RNG state)")
    if oracle:
        ref = H.oracle_scene_for(orc, scene, 1).render(cam, W, Hh, spp, depth)
        H.assert_planes_equal(first_a[0:3], ref["fb"], what + ": fb against the oracle")
        H.assert_planes_equal(first_a[6:9], ref["xyz"], what + ": XYZ against the oracle")


def _refit_case(srt, orc, A, B, scene, cam, W, Hh, spp, depth, motions, what, via=None):
    """A: upload, camera, device parameters, then every motion in turn, each checked against B's upload of the host-refitted scene"""
    _setup(A, scene, cam, W, Hh, spp, depth)
    for k, v in enumerate(motions):
        if k:      # (the frames of the motion before advanced A's RNG streams: seed them again, still before the refit)
            A.init_device_params(W, Hh, spp, depth, 1984)
        A.refit(v if via is None else via(v))
        scene.refit(v)
        _check_against_upload(srt, orc, A, B, scene, cam, W, Hh, spp, depth, "%s, motion %d" % (what, k))


def _small(W, Hh, spp):
    return min(W, 64), min(Hh, 48), min(spp, 3)


@pytest.mark.parametrize("case", ["one_triangle", "two_triangles"])
def test_refit_smallest_trees(srt, gpu, gpu_b, orc, case):
    """one_triangle: the root is a leaf, there is no record and no FRINGE block to copy into; two_triangles: one FRINGE record, no INNER"""
    scene, cam, W, Hh, spp, depth = H.edge_case_scene(srt, case)
    v0 = scene.vertices()
    _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [R.jitter(v0, 1, 0.5), R.smooth(v0), v0], case)
    assert gpu.refit_last_ms()["n_levels"] == (0 if case == "one_triangle" else 1)


@pytest.mark.parametrize("case", ["degenerate", "axis_aligned", "thin", "signed_zero"])
def test_refit_edge_motions(srt, gpu, gpu_b, orc, case):
    """degenerate_and_odd_materials with a motion that makes a triangle degenerate and one that undoes it; triangles that become axis
    aligned and stop being so (the projection axes, and with them the record layout, change); an extent below 1e-4 (the padded box);
    +0 and -0 on one axis (where the value-equality clause is needed)"""
    scene, cam, W, Hh, spp, depth, v1, v2 = R.motion_scene(srt, case)
    v0 = scene.vertices()
    _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [v1, v2, v0], case)


@pytest.mark.parametrize("seed", [0, 1, 3, 7, 11])
def test_refit_fuzz(srt, gpu, gpu_b, orc, seed):
    """random soups of both builders (seeds 0, 1: the reference's; 3, 7, 11: SAH, 7 and 11 paired trees; tests/test_refit_host.py checks that)"""
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, seed)
    W, Hh, spp = _small(W, Hh, spp)
    v0 = scene.vertices()
    _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [R.jitter(v0, seed), R.smooth(v0)], "fuzz seed %d" % seed)


@pytest.mark.parametrize("which", R.UNPAIRED)
def test_refit_unpaired_sah_trees(srt, gpu, gpu_b, orc, which):
    """SAH trees with a leaf + INNER node -- a FRINGE record whose internal child is an INNER record, which lies in front of it in the record
    order: from an odd count with an outlier, from a fuzz soup, and after srt_scene_optimise_bvh"""
    scene, cam, W, Hh, spp, depth = R.unpaired_scene(srt, which)
    assert R.leaf_plus_inner_nodes(scene) >= 1
    v0 = scene.vertices()
    _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [R.jitter(v0, 11), R.smooth(v0), v0], which)
    assert gpu.refit_last_ms()["n_levels"] == scene.refit_schedule().size


@pytest.mark.parametrize("knobs, seed, stride_env", [
    (dict(wide_refs=True), 2, None),
    (dict(lds_cache_max=0), 1, None),            # every INNER record from memory: the swizzled image, the L2 FRINGE stride
    (dict(lds_cache_max=0), 10, "128"),          # ... and that stride padded to 128 bytes
    (dict(lds_cache_max=8), 9, None),            # the tree partly cached
], ids=["wide_refs", "lds_cache_max=0", "lds_cache_max=0, 128-byte FRINGE stride", "partly cached"])
def test_refit_under_test_knobs(srt, gpu, gpu_b, orc, monkeypatch, knobs, seed, stride_env):
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, seed)
    W, Hh, spp = _small(W, Hh, spp)
    v0 = scene.vertices()
    if stride_env:
        monkeypatch.setenv("SRT_FRINGE_STRIDE", stride_env)
    try:
        gpu.set_test_knobs(**knobs); gpu_b.set_test_knobs(**knobs)
        _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [R.jitter(v0, seed), v0], "knobs %r" % (knobs,))
        plan = gpu.launch_plan()
        if "wide_refs" in knobs:
            assert not plan["narrow_refs"]
        else:
            assert not plan["all_cached"] and gpu.scene_image("nodes_sw").size == 20 * (gpu.scene_image("nodes").size // 16)
            assert plan["n_cached"] <= knobs["lds_cache_max"]
            n_fringe_floats = gpu.scene_image("fringe").size
            assert n_fringe_floats % (32 if stride_env else 24) == 0
            if stride_env:      # the padding words of every record are still +0
                assert not gpu.scene_image("fringe").reshape(-1, 32)[:, 24:].any()
    finally:
        gpu.set_test_knobs(); gpu_b.set_test_knobs()


def test_refit_random_spheres_smooth_deformation(srt, gpu, gpu_b, orc):
    """the headline scene's tree: 2 400 INNER records, so the lower levels are wider than one workgroup"""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    W, Hh, spp, depth = 64, 48, 2, 5
    cam = scene.default_camera(W, Hh)
    v0 = scene.vertices()
    _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [R.smooth(v0, 0.9, 0.2)], "random spheres")
    ms = gpu.refit_last_ms()
    assert ms["n_levels"] >= 12 and ms["triangles"] > 0 and ms["levels"] > 0      # (2 401 FRINGE records and 2 400 INNER ones need at least 12 heights)


def test_refit_sequence_and_return(srt, gpu, gpu_b):
    """refit(v1); refit(v2) equals refit(v2) bit for bit, and refit(v0) equals the original upload as values"""
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 9)
    v0 = scene.vertices()
    v1, v2 = R.jitter(v0, 1), R.jitter(v0, 2, 1.0)
    gpu.upload_scene(scene); gpu_b.upload_scene(scene)
    original = _images(gpu_b)
    gpu.refit(v1); gpu.refit(v2)
    gpu_b.refit(v2)
    _assert_images(_images(gpu), _images(gpu_b), "refit(v1); refit(v2) against refit(v2)", exact=True)
    gpu.refit(v0)
    _assert_images(_images(gpu), original, "refit(v0) against the original upload")


def test_refit_device_pointer_entry_equals_host_entry(srt, gpu, gpu_b, orc):
    import torch
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 3)
    W, Hh, spp = _small(W, Hh, spp)
    v0 = scene.vertices()
    v1 = R.jitter(v0, 5)
    gpu_b.upload_scene(scene); gpu_b.refit(v1)
    host_entry = _images(gpu_b)
    dev = torch.device("cuda", 0)
    _refit_case(srt, orc, gpu, gpu_b, scene, cam, W, Hh, spp, depth, [v1], "device-pointer entry", via=lambda v: torch.from_numpy(v).to(dev))
    _assert_images(_images(gpu), host_entry, "device-pointer entry against host entry", exact=True)
    # an animation computed on the GPU never visits the host: the tensor is made there
    t = torch.from_numpy(v0).to(dev)
    t = (t + 0.125 * torch.sin(t)).contiguous()
    gpu.refit(t)
    gpu_b.refit(t.cpu().numpy())
    _assert_images(_images(gpu), _images(gpu_b), "a tensor computed on the device", exact=True)


def test_refit_invalidates_what_an_upload_invalidates_and_nothing_else(srt, gpu, gpu_b):
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 0)
    W, Hh, spp = _small(W, Hh, spp)
    v0 = scene.vertices()
    _setup(gpu, scene, cam, W, Hh, spp, depth)
    gpu.temporal_reset()
    gpu.accum_reset_features()
    for want in (1, 2):
        gpu.render_chunk_accum(W, Hh, spp); gpu.scatter_tiles()
        assert gpu.temporal(W, Hh)["stats"]["history_frames"] == want
    gpu.refit(R.jitter(v0, 3))
    with pytest.raises(srt.SrtError) as e:      # the accumulation from before the refit shows the old geometry
        gpu.render_chunk_accum(W, Hh, spp)
    assert e.value.code == -1
    gpu.accum_reset_features()
    gpu.render_chunk_accum(W, Hh, spp); gpu.scatter_tiles()
    st = gpu.temporal(W, Hh)["stats"]
    assert st["history_frames"] == 1 and st["blended"] == 0, st      # no history: a first frame
    # camera and device parameters survived: A's next plain frame is B's, which was set up from scratch with them
    scene.refit(R.jitter(v0, 3))
    _setup(gpu_b, scene, cam, W, Hh, spp, depth)
    gpu.init_device_params(W, Hh, spp, depth, 1984)      # (the passes above advanced A's RNG streams; the camera is the one from before the refit)
    H.assert_planes_equal(_frame(gpu, W, Hh), _frame(gpu_b, W, Hh), "frame with the camera from before the refit")


def test_refit_device_parameters_survive(srt, gpu, gpu_b):
    """no call between the refit and the frame: grid, spp, bounce limit, seed and RNG state are those from before it"""
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 5)
    v1 = R.jitter(scene.vertices(), 4)
    _setup(gpu, scene, cam, W, Hh, spp, depth)
    before = dict(gpu.geom)
    gpu.refit(v1)
    scene.refit(v1)
    _setup(gpu_b, scene, cam, W, Hh, spp, depth)
    H.assert_planes_equal(_frame(gpu, W, Hh), _frame(gpu_b, W, Hh), "frame right after the refit")
    assert gpu.geom == before and gpu.stats()["paths"] == gpu_b.stats()["paths"]


def test_refit_refusals_change_nothing(srt, gpu):
    import torch
    B = srt.binding
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 1)
    v0 = scene.vertices()
    good = R.jitter(v0, 6)
    gpu.upload_scene(scene)
    before = _images(gpu)
    L = B.lib()
    dev = torch.device("cuda", 0)

    def refused(call, what):
        with pytest.raises(B.SrtError) as e:
            call()
        assert e.value.code == -1, what
        _assert_images(_images(gpu), before, what, exact=True)

    refused(lambda: gpu.refit(good[:-1]), "n_tris too small")
    refused(lambda: gpu.refit(np.concatenate([good, good[:1]])), "n_tris too large")
    refused(lambda: gpu._ck(L.srt_refit_vertices(gpu._h, None, n)), "null host pointer")
    refused(lambda: gpu._ck(L.srt_refit_vertices_dev(gpu._h, None, n)), "null device pointer")
    for poison in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[n - 1, 2, 2] = poison
        refused(lambda: gpu.refit(bad), "host entry, %r" % poison)
        refused(lambda: gpu.refit(torch.from_numpy(bad).to(dev)), "device-pointer entry, %r" % poison)
    refused(lambda: gpu.refit(torch.from_numpy(good[:-1].copy()).to(dev)), "device-pointer entry, n_tris too small")
    # no scene uploaded: a fresh context, and a context whose knobs changed since its upload
    fresh = srt.Renderer(0)
    try:
        for v in (good, torch.from_numpy(good).to(dev)):
            with pytest.raises(B.SrtError) as e:
                fresh.refit(v)
            assert e.value.code == -1
        with pytest.raises(B.SrtError):
            fresh.refit_last_ms()
        fresh.upload_scene(scene)
        fresh.set_test_knobs(wide_refs=True)
        with pytest.raises(B.SrtError) as e:
            fresh.refit(good)
        assert e.value.code == -1
    finally:
        fresh.close()
    gpu.refit(good)      # and the accepted call still works afterwards
    assert not np.array_equal(_images(gpu)["tris"], before["tris"])


def test_refit_through_both_communicators(srt, gpu_b, orc):
    """the two ways a communicator exists on one GPU (ncclCommInitAll with one device, ncclCommInitRank with world 1): Comm.refit, then
    the communicator's frame, against the single context that uploaded the host-refitted scene"""
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 3)
    W, Hh, spp = _small(W, Hh, spp)
    v0 = scene.vertices()
    v1 = R.jitter(v0, 8)
    moved = R.moved(srt, scene, v0).build_bvh(mode, 1984)      # (the same inputs: the same tree)
    moved.refit(v1)
    _setup(gpu_b, moved, cam, W, Hh, spp, depth)
    want_images, want = _images(gpu_b), _frame(gpu_b, W, Hh)

    def through(comm):
        comm.set_gather_planes(9)
        comm.upload_scene(scene); comm.set_camera(cam)
        comm.init_device_params(W, Hh, spp, depth, 1984)
        comm.refit(v1)
        comm.render_frame(W, Hh); comm.synchronize()
        root = comm.root
        _assert_images(_images(root), want_images, "communicator")
        H.assert_planes_equal(root.read_fb() + root.read_fb_aux(1) + root.read_fb_aux(2), want, "communicator frame")
        with pytest.raises(srt.SrtError) as e:
            comm.refit(v1[:-1])
        assert e.value.code == -1

    comm = srt.Comm.init_all([0])
    try:
        through(comm)
    finally:
        comm.close()
    r = srt.Renderer(0)
    comm = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
    try:
        through(comm)
    finally:
        comm.close(); r.close()


def test_render_animated_frames_equal_uploads(srt, gpu, gpu_b):
    """render_animated uploads once and refits per frame: every frame's planes are those of a context that uploaded the moved scene, and
    the temporal stage sees a first frame each time"""
    scene, cam, W, Hh, spp, depth, mode, n = H.fuzz_case(srt, 7)
    W, Hh, spp = 32, 24, 2
    cam = srt.camera_init(W, Hh, 50.0, (0.0, 0.0, 14.0), (0.0, 0.0, 0.0))
    v0 = scene.vertices()
    frames = [v0, R.smooth(v0), R.jitter(v0, 2)]
    seen = 0
    for k, res, feats, picture, stats in srt.render_animated(scene, cam, frames, W, Hh, spp, depth, renderer=gpu, levels=2):
        assert stats["history_frames"] == 1 and stats["blended"] == 0
        ref_scene = R.moved(srt, scene, v0).build_bvh(mode, 1984)
        ref_scene.refit(frames[k])
        _setup(gpu_b, ref_scene, cam, W, Hh, spp, depth)
        gpu_b.accum_reset_features()
        gpu_b.render_chunk_accum(W, Hh, spp); gpu_b.scatter_tiles()
        if k == 0:      # later frames continue A's RNG streams: only the first is comparable to a freshly seeded context
            H.assert_planes_equal(res["xyz"], gpu_b.read_fb_aux(2), "animated frame 0")
        _assert_images(_images(gpu), _images(gpu_b), "animated frame %d" % k)
        seen += 1
    assert seen == len(frames)
    assert bytes(scene.triangles()) == bytes(R.moved(srt, scene, v0).triangles()), "render_animated changed the scene"
