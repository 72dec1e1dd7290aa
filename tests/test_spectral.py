"""Spectral film (srt_accum_reset_spectral + srt_render_chunk_accum, render_kernel MODE 5).  The film holds, per pixel, the raw fp32 sums
of every path end's seven powers deposited on the 5 nm CIE grid by the rule of srt_c_api.h.  Contracted with the colour-matching rows it
gives the accumulation's XYZ sums (up to reassociation), and it is additive: the colour planes, XYZ sums and RNG state of a spectral
accumulation are those of a plain one.  The film itself is held bit for bit to the deposit rule applied in numpy float32 to the CPU
oracle's path ends (tests/path_ends_reference.py): on six workloads that together cover dispersive paths, emitter ends, bounce-limit
ends, the first and the clamped last bin pair and every bin, for a split of the samples, every launch shape, a partition and an offset
chunk; and on a miss-only frame to the same rule applied to a numpy restatement of the RNG."""
import ctypes as C

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, ERR_UNSUPPORTED, EVERY_SHAPE_CASES, EVERY_SHAPE_IDS, N_GRID, expect_error, forced_shape,
                           fresh_context, gpu_lib, lane_of, named_workload, read_frame, read_sum_y, run_mock_transport_child, shape_case,
                           spectral_run, split_passes)
from helpers import _xorwow_host, assert_planes_equal, bits, custom_scene, fuzz_with_lens, oracle_scene_for
from path_ends_reference import (FILM_WORKLOADS, assert_film_coverage, assert_same_floats, cached_ends, deposit, shape_ends,
                                 workload_ends)


def _miss_scene(srt, bg):
    """one small triangle far behind a camera that looks down -z: every camera ray misses; background spectrum `bg` (95 floats)"""
    sc = custom_scene(srt, [((-1, -1, 60), (1, -1, 60), (0, 1, 60), 0, 0)], [(0, (0.5, 0.5, 0.5), 0.0, 0.0)])
    bg = np.ascontiguousarray(bg, np.float32)
    srt.binding.check(srt.binding.lib().srt_scene_set_background(sc.handle, srt.binding.fptr(bg)))
    sc.build_bvh(srt.BVH_SAH, 1984)
    return sc


def _miss_camera(srt, W, H):
    return srt.camera_init(W, H, 40.0, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "prism", "fuzz", "random_spheres"])
def test_film_contracts_to_the_xyz_sums(srt, gpu, name):
    if name == "fuzz":
        scene, cam, W, H, spp, depth, _ = fuzz_with_lens(srt)
    else:
        scene, cam, W, H, depth, _ = named_workload(srt, name)
        spp = 6
    frame, film = spectral_run(gpu, scene, cam, W, H, depth, [spp])
    lane = lane_of(gpu.geom, W, H)
    want = np.stack([frame["xyz"][c][lane] for c in range(3)], axis=-1).reshape(H, W, 3).astype(np.float64)
    assert np.array_equal(bits(read_sum_y(gpu, W, H)), bits(want[..., 1].astype(np.float32).ravel()))
    got = srt.film_to_xyz(film)
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    ok = ~np.isnan(want)
    assert np.abs(want[ok]).max() > 0, name
    np.testing.assert_allclose(got[ok], want[ok], rtol=2e-4, atol=1e-9, err_msg=name)
    assert (film[~np.isnan(film)] >= 0).all()
    assert gpu.stats()["paths"] == W * H * spp


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [[1], [2, 3], [4]], ids=["1", "2+3", "4"])
def test_miss_only_film_equals_the_float32_restatement(srt, gpu, orc, passes):
    """every sample draws two jitter floats and a hero wavelength, misses, and deposits the interpolated background at 7 wavelengths"""
    f = np.float32
    lam_grid = np.arange(N_GRID, dtype=np.float64)
    bg = (0.2 + 0.6 * (0.5 + 0.5 * np.sin(lam_grid / 7.0)) + 0.01 * lam_grid / N_GRID).astype(f)
    scene = _miss_scene(srt, bg)
    W, H, depth = 23, 14, 4
    cam = _miss_camera(srt, W, H)
    frame, film = spectral_run(gpu, scene, cam, W, H, depth, passes)
    assert gpu.stats()["rays"] == W * H * passes[-1]
    seeds = 1984 + lane_of(gpu.geom, W, H).astype(np.uint64)
    st, nxt = _xorwow_host(seeds)
    every = np.ones(seeds.size, bool)

    def unit(r):      # fma((float)r, 2^-32, 2^-33): one rounding
        return (r.astype(f).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(f)
    step, scale = f(470.0) / f(7.0), f(94.0) / f(470.0)
    want = np.zeros((seeds.size, N_GRID), f)
    bg_p = bg.ctypes.data_as(C.POINTER(C.c_float))
    with np.errstate(over="ignore"):
        for _ in range(sum(passes)):
            nxt(every); nxt(every)                             # the pixel jitter
            hero = unit(nxt(every)) * f(470.0) + f(360.0)      # rng_range(360, 830), two roundings
            lam = hero
            lams, powers = np.zeros((seeds.size, 7), f), np.zeros((seeds.size, 7), f)
            for k in range(7):
                if k:
                    lam = lam + step
                    lam = np.where(lam > f(830.0), f(360.0) + (lam - f(830.0)), lam).astype(f)
                x = (lam - f(360.0)) * scale
                off = np.clip(x.astype(np.int32), 0, 93)
                w = x - off.astype(f)
                p = (f(1.0) - w) * bg[off] + w * bg[off + 1]
                for q in range(0, seeds.size, 37):               # the interpolation is the oracle's spectrum_interp
                    assert bits(np.float32(orc.lib().orc_spectrum_interp(bg_p, float(lam[q]), N_GRID))) == bits(p[q])
                lams[:, k], powers[:, k] = lam, f(1.0) * p       # the path's power starts at 1
            deposit(want, lams, powers)                          # all seven wavelengths valid (path_ends_reference: the deposit rule)
    want = want.reshape(H, W, N_GRID)
    assert np.array_equal(bits(film), bits(want)), "%d of %d sums differ" % (int((bits(film) != bits(want)).sum()), film.size)


def _film_of(gpu, scene, cam, W, H, depth, passes, offx=0, offy=0):
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_spectral()
    for s in passes:
        gpu.render_chunk_accum(W, H, s, offx, offy)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FILM_WORKLOADS)
def test_film_equals_the_deposits_of_the_oracles_path_ends(srt, gpu, orc, name):
    """every one of the 95 sums of every pixel == the deposit rule applied to the oracle's path ends, bit for bit (or both NaN)"""
    assert_film_coverage(srt, orc)             # ... of all the workloads together, before the GPU runs
    (scene, cam, W, H, n, depth, _), ends = workload_ends(srt, orc, name)
    frame, film = spectral_run(gpu, scene, cam, W, H, depth, [n])
    assert_same_floats(film, ends["film"], name + " film")
    assert_planes_equal(frame["xyz"], ends["render"]["xyz"], name + " XYZ sums")
    assert gpu.stats()["paths"] == W * H * n


@pytest.mark.gpu
def test_film_prediction_holds_for_a_split_a_partition_and_an_offset_chunk(srt, gpu, orc):
    (scene, cam, W, H, n, depth, _), ends = workload_ends(srt, orc, "dielectric")
    _, film = spectral_run(gpu, scene, cam, W, H, depth, split_passes(n))
    assert_same_floats(film, ends["film"], "dielectric in passes %r" % (split_passes(n),))
    # three ranks: every pixel's row is on its tile's owner and +0 elsewhere, so the sum over the ranks is the prediction
    (scene, cam, W, H, n, depth, mode), ends = workload_ends(srt, orc, "random_spheres")
    total = np.zeros((H, W, N_GRID), np.float32)
    for rank in range(3):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.set_partition(rank, 3)
        gpu.accum_reset_spectral()
        for s in (2, n - 2):
            gpu.render_chunk_accum(W, H, s)
        part = gpu.read_spectral(W, H)
        assert bits(part).any()
        total = total + part
    gpu.set_partition(0, 1)
    assert_same_floats(total, ends["film"], "random_spheres, rows summed over 3 ranks")
    # a 30 x 21 chunk (no multiple of 8 x 8 or 28 x 16) at (17, 9) of a 64 x 40 image
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    ends = cached_ends(orc, ("random_spheres chunk", cw, ch, ox, oy), lambda: oracle_scene_for(orc, scene, mode), cam, cw, ch, 4, depth,
                       offx=ox, offy=oy)
    assert ends["film"].max() > 0
    _film_of(gpu, scene, cam, cw, ch, depth, (1, 3), ox, oy)
    full = gpu.read_spectral(IW, IH)
    assert_same_floats(full[oy:oy + ch, ox:ox + cw], ends["film"], "offset chunk")
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert not bits(full[~inside]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_spectral_shape_equals_the_prediction(srt, gpu, orc, knobs, paired, expect):
    n = 4
    (scene, cam, W, H, depth), ends = shape_ends(srt, orc, paired, n)
    assert ends["film"].max() > 0 and {1, 7} <= set(np.unique(ends["valid"]).tolist())
    with forced_shape(gpu, scene, knobs, expect):
        _, film = spectral_run(gpu, scene, cam, W, H, depth, [1, 3])
    assert_same_floats(film, ends["film"], "shape %r" % (expect,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["prism", "dielectric"])
def test_film_is_additive_and_split_invariant(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    one, film_one = spectral_run(gpu, scene, cam, W, H, depth, [32], spp=3)
    split, film_split = spectral_run(gpu, scene, cam, W, H, depth, [8, 8, 16], spp=3)
    assert np.array_equal(bits(film_split), bits(film_one)), name
    sum_y = read_sum_y(gpu, W, H)
    gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
    after = read_frame(gpu, W, H)
    # the same passes of a plain accumulation
    fresh_context(gpu, scene, cam, W, H, depth, spp=3)
    gpu.accum_reset()
    for s in (8, 8, 16):
        gpu.render_chunk_accum(W, H, s)
    plain = read_frame(gpu, W, H)
    plain_y = read_sum_y(gpu, W, H)
    gpu.render_chunk(W, H)
    plain_after = read_frame(gpu, W, H)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(split[k], plain[k], "%s spectral vs plain %s" % (name, k))
        assert_planes_equal(one[k], plain[k], "%s one-pass spectral vs plain %s" % (name, k))
        assert_planes_equal(after[k], plain_after[k], "%s RNG state: plain launch after the passes, %s" % (name, k))
    assert np.array_equal(bits(sum_y), bits(plain_y))


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,paired,expect", EVERY_SHAPE_CASES, ids=EVERY_SHAPE_IDS)
def test_every_spectral_shape_gives_the_same_film(srt, gpu, knobs, paired, expect):
    scene, cam, W, H, depth = shape_case(srt, paired)
    gpu.set_test_knobs()
    ref, film_ref = spectral_run(gpu, scene, cam, W, H, depth, [3, 5])
    with forced_shape(gpu, scene, knobs, expect):
        got, film = spectral_run(gpu, scene, cam, W, H, depth, [3, 5])
    assert np.array_equal(bits(film), bits(film_ref)), expect
    assert film_ref.max() > 0
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(got[k], ref[k], "shape %r %s" % (expect, k))


@pytest.mark.gpu
def test_partitions_offset_chunk_and_sub_range(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "random_spheres")
    passes = [3, 4]
    _, ref = spectral_run(gpu, scene, cam, W, H, depth, passes)
    assert ref.max() > 0
    for world in (2, 3):
        films = []
        for rank in range(world):
            fresh_context(gpu, scene, cam, W, H, depth)
            gpu.set_partition(rank, world)
            gpu.accum_reset_spectral()
            for s in passes:
                gpu.render_chunk_accum(W, H, s)
            films.append(gpu.read_spectral(W, H))
        total = films[0]
        for f_ in films[1:]:
            total = total + f_
        assert np.array_equal(bits(total), bits(ref)), world
        # every pixel belongs to one rank: on all the others its 95 sums are +0
        nonzero = np.stack([(bits(f_) != 0).any(axis=-1) for f_ in films])
        owners = np.stack([(bits(f_) == 0).all(axis=-1) for f_ in films])
        assert (nonzero.sum(axis=0) <= 1).all() and ((~owners).sum(axis=0) <= 1).all(), world
        assert nonzero.any(axis=0).sum() > 0.9 * W * H
    gpu.set_partition(0, 1)

    # sub-ranges of the full read
    _, full = spectral_run(gpu, scene, cam, W, H, depth, passes)
    for first, count in ((0, 1), (10, 17), (94, 1), (0, 95), (47, 48)):
        part = gpu.read_spectral(W, H, first, count)
        assert part.shape == (H, W, count)
        assert np.array_equal(bits(part), bits(full[..., first:first + count])), (first, count)

    # a 30 x 20 chunk at (17, 9) of a 64 x 40 image writes its rectangle of the caller's array and nothing else
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 20, 17, 9
    cam = scene.default_camera(IW, IH)
    fresh_context(gpu, scene, cam, cw, ch, depth)
    gpu.accum_reset_spectral()
    for s in passes:
        gpu.render_chunk_accum(cw, ch, s, ox, oy)
    sentinel = np.float32(-7.0)
    out = np.full((IH, IW, 12), sentinel, np.float32)
    gpu.read_spectral(IW, IH, 40, 12, into=out)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert (out[~inside] == sentinel).all()
    assert (out[inside] >= 0).all() and out[inside].max() > 0
    full = gpu.read_spectral(IW, IH)
    assert np.array_equal(bits(out[inside]), bits(full[inside][:, 40:52]))
    y = read_sum_y(gpu, IW, IH).reshape(IH, IW)
    got_y = srt.film_to_xyz(full)[..., 1]
    np.testing.assert_allclose(got_y[inside], y[inside], rtol=2e-4, atol=1e-9)
    assert (full[~inside] == 0).all()


@pytest.mark.gpu
def test_comm_two_and_three_ranks_one_gpu_mock_transport():
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
from helpers import assert_planes_equal, bits
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, depth = 150, 90, 16
cam = scene.default_camera(W, H)
steps = list(srt.render_spectral(scene, cam, W, H, [4, 4], depth))
total, ref, _ = steps[-1]
assert total == 8 and ref['film'].max() > 0
for world in (2, 3):
    for _, comm in comm_accumulations(srt, world, (9,), scene, cam, W, H, depth, 8, lambda c: c.accum_reset_spectral(), (4, 4)):
        root = comm.root
        assert_planes_equal(root.read_fb(), ref['fb'], 'world %d fb' % world)
        assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'world %d xyz' % world)
        film = comm.read_spectral(W, H)
        assert np.array_equal(bits(film), bits(ref['film'])), world
        part = comm.read_spectral(W, H, 30, 5)
        assert np.array_equal(bits(part), bits(ref['film'][..., 30:35])), world
r = srt.Renderer(0)
c1 = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
c1.set_gather_planes(9)
c1.upload_scene(scene); c1.set_camera(cam); c1.init_device_params(W, H, 8, depth, 1984)
c1.accum_reset_spectral()
for s in (4, 4):
    c1.render_frame_accum(W, H, s)
c1.synchronize()
assert np.array_equal(bits(c1.read_spectral(W, H)), bits(ref['film']))
c1.close(); r.close()
print('spectral mock transport ok')
""", "spectral mock transport ok", timeout=300)


@pytest.mark.gpu
def test_estimator_recovers_a_constant_background(srt, gpu):
    """A miss-only frame under a constant background c: the image-mean spectral_radiance is c at every grid sample, the half-width end
    samples (edge factor 2) included.  (At 64 x 64 x 64 spp the standard error of one sample's mean is about 0.55 % inside the grid and
    0.8 % at its ends -- a 1 % bound would be a 1.3-1.8 sigma test; 128 x 128 x 256 spp brings it to 0.07 / 0.1 %.)"""
    c = 0.75
    scene = _miss_scene(srt, np.full(N_GRID, c, np.float32))
    W = H = 128
    spp = 256
    _, film = spectral_run(gpu, scene, _miss_camera(srt, W, H), W, H, 4, [spp])
    L = srt.spectral_radiance(film, spp).reshape(-1, N_GRID).mean(axis=0)
    rel = np.abs(L / c - 1.0)
    assert rel.max() < 0.01, (int(rel.argmax()), float(rel.max()))
    assert rel[0] < 0.01 and rel[94] < 0.01
    # without the edge factor the ends would read c / 2
    raw = film.reshape(-1, N_GRID).mean(axis=0).astype(np.float64) * 470.0 / (35.0 * spp)
    assert abs(raw[0] / c - 0.5) < 0.01 and abs(raw[94] / c - 0.5) < 0.01


@pytest.mark.gpu
def test_refusals_and_invalidation(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    buf = np.zeros(W * H * N_GRID, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    # device parameters not set
    fresh = srt.Renderer(0)
    try:
        assert L.srt_accum_reset_spectral(fresh._h) == ERR_INVALID
    finally:
        fresh.close()
    fresh_context(gpu, scene, cam, W, H, depth)
    # a plain accumulation has no film
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read of a plain accumulation")
    gpu.accum_reset_spectral()
    expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, "read before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first = gpu.read_spectral(W, H)
    frame = read_frame(gpu, W, H)
    for f0, n in ((0, 0), (90, 6), (95, 1), (0, 96), (0xffffffff, 2)):
        assert L.srt_read_spectral(gpu._h, f0, n, fp, W, H) == ERR_INVALID, (f0, n)
    assert L.srt_read_spectral(gpu._h, 0, 95, None, W, H) == ERR_INVALID
    assert L.srt_read_spectral(gpu._h, 0, 95, fp, 0, H) == ERR_INVALID
    # a refused reset (instrumented context) leaves the accumulation usable
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.accum_reset_spectral(), ERR_UNSUPPORTED, "instrumented context")
    gpu.set_count_traversal(False)
    assert gpu.accum_samples == 4
    assert np.array_equal(bits(gpu.read_spectral(W, H)), bits(first))
    for k, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, frame[k], "after the refusal " + k)
    gpu.render_chunk_accum(W, H, 4)
    assert gpu.accum_samples == 8 and gpu.stats()["paths"] == W * H * 4
    _, want = spectral_run(gpu, scene, cam, W, H, depth, [8])
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset_spectral()
    gpu.render_chunk_accum(W, H, 4)
    gpu.set_count_traversal(True)
    expect_error(srt, lambda: gpu.accum_reset_spectral(), ERR_UNSUPPORTED, "instrumented context")
    gpu.set_count_traversal(False)
    gpu.render_chunk_accum(W, H, 4)
    assert np.array_equal(bits(gpu.read_spectral(W, H)), bits(want))
    # every invalidation of an accumulation makes the film unreadable
    for what, call in (("srt_set_camera", lambda: gpu.set_camera(cam)), ("srt_render_chunk", lambda: gpu.render_chunk(W, H)),
                       ("srt_upload_scene", lambda: gpu.upload_scene(scene)), ("srt_set_partition", lambda: gpu.set_partition(0, 1)),
                       ("srt_init_device_params", lambda: gpu.init_device_params(W, H, 12, depth, 1984)),
                       ("srt_accum_reset", lambda: gpu.accum_reset()),
                       ("srt_accum_reset_adaptive", lambda: gpu.accum_reset_adaptive(0.1, 0.0, 4))):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_spectral()
        gpu.render_chunk_accum(W, H, 2)
        gpu.read_spectral(W, H)
        call()
        if what.startswith("srt_accum_reset"):
            gpu.render_chunk_accum(W, H, 2)      # a pass of the new accumulation, which keeps no film
        expect_error(srt, lambda: gpu.read_spectral(W, H), ERR_INVALID, what)
    gpu.set_gather_planes(9)


@pytest.mark.gpu
def test_render_spectral_generator(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    steps = list(srt.render_spectral(scene, cam, W, H, [3, 5], depth, renderer=gpu))
    assert [t for t, _, _ in steps] == [3, 8]
    for t, res, rad in steps:
        assert set(res) == {"fb", "lin", "xyz", "rowmajor", "stats", "kernel_ms", "geom", "film"}
        assert res["film"].shape == (H, W, N_GRID) and rad.shape == (H, W, N_GRID)
        np.testing.assert_array_equal(rad, srt.spectral_radiance(res["film"], t))
    one_shot = srt.render_image(scene, cam, W, H, 8, depth, renderer=gpu)
    for k in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(steps[-1][1][k], one_shot[k], "render_spectral vs render_image " + k)
    # a single pass is the one-shot spectral image; a sub-range reads the same sums
    (t, res, rad), = srt.render_spectral(scene, cam, W, H, [8], depth, renderer=gpu, first=20, count=30)
    assert t == 8 and res["film"].shape == (H, W, 30)
    assert np.array_equal(bits(res["film"]), bits(steps[-1][1]["film"][..., 20:50]))
    np.testing.assert_array_equal(rad, srt.spectral_radiance(res["film"], 8, first=20))
    for k in ("fb", "lin", "xyz"):
        assert_planes_equal(res[k], one_shot[k], "one-pass render_spectral " + k)
