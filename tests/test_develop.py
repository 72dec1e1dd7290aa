"""The film developed on the device (srt_develop_spectral / _srgb / _kat, csrc/srt_develop.hip): out_k = (sum over the 95 grid samples,
ascending, of F_j * R[k][j]) * scale.  The device is held bit for bit to the float32 restatement of tests/develop_reference.py -- on
explicit films at the wave- and tile-boundary sizes with every channel count that picks another kernel variant, and on real spectral
accumulations, where one-hot responses must return read_spectral's film itself -- and the sRGB variant to the CPU oracle's conversion.
Placement, partitions, the communicator, the read-only property and every refusal follow."""
import ctypes as C

import numpy as np
import pytest

from accum_helpers import (ERR_INVALID, convert_xyz, expect_error, fresh_context, gpu_lib, lane_of, named_workload, read_frame,
                           run_mock_transport_child)
from develop_reference import CIE_SCALE, N_GRID, develop, normalise, one_hot
from helpers import assert_planes_equal, bits
from path_ends_reference import assert_same_floats, bits_equal_or_both_nan

F = np.float32
ERR_HIP = -3
FP = C.POINTER(C.c_float)


def _responses(k, seed=11):
    """k curves of both signs over a few magnitudes"""
    rng = np.random.default_rng(seed + k)
    return ((rng.random((k, N_GRID)) - 0.4) * 10.0 ** rng.integers(-3, 3, (k, N_GRID))).astype(F)


def _accumulate(gpu, scene, cam, W, H, depth, passes, offx=0, offy=0, partition=(0, 1)):
    """a spectral accumulation of `passes` left bound in the context"""
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.set_partition(*partition)
    gpu.accum_reset_spectral()
    for s in passes:
        gpu.render_chunk_accum(W, H, s, offx, offy)


# ---- the kernel on explicit films ------------------------------------------------------------------------------------------------
def _kat_film(n):
    """n rows spanning sixty decades with denormals; row n // 2 holds a NaN, row n - 1 (n > 1) a +inf"""
    rng = np.random.default_rng(100 + n)
    film = (rng.random((n, N_GRID)) * 10.0 ** rng.integers(-30, 30, (n, N_GRID))).astype(F)
    film[rng.random((n, N_GRID)) < 0.05] = F(1e-41)          # denormal
    film[rng.random((n, N_GRID)) < 0.05] = F(0)
    bad = np.zeros(n, bool)
    film[n // 2, 17 % N_GRID] = np.nan
    bad[n // 2] = True
    if n > 1:
        film[n - 1, 94] = np.inf
        bad[n - 1] = True
    return film, bad


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 4, 5, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 191, 257])
def test_kat_equals_the_restatement_bit_for_bit(gpu, n, k):
    film, bad = _kat_film(n)
    resp = _responses(k)
    scale = F(-0.75) if k % 2 else CIE_SCALE
    got = gpu.develop_kat(film, resp, scale)
    want = develop(film, resp, scale)
    assert got.shape == (n, k)
    assert_same_floats(got, want, "KAT n = %d, K = %d" % (n, k))
    # the non-finite rows stay where they are: every other pixel is finite (a kernel that mixed two pixels' tiles would not be)
    assert np.isfinite(want[~bad]).all() and np.isfinite(got[~bad]).all()
    assert not np.isfinite(got[bad]).any()
    ms = gpu.develop_last_ms()
    assert ms["contract"] > 0 and ms["epilogue"] == 0


@pytest.mark.gpu
def test_kat_one_hot_returns_the_rows_and_the_pad_word_never_enters(gpu):
    """finite rows through the 95 one-hot curves are the rows themselves, so neither the library's 96th word (a NaN) nor a neighbour's
    sample entered any sum"""
    rng = np.random.default_rng(9)
    film = (rng.random((130, N_GRID)) * 10.0 ** rng.integers(-20, 20, (130, N_GRID))).astype(F)
    for first in range(0, N_GRID, 16):
        count = min(16, N_GRID - first)
        got = gpu.develop_kat(film, one_hot(first, count))
        assert np.array_equal(bits(got), bits(film[:, first:first + count])), first


# ---- real accumulations ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_hot_responses_reproduce_read_spectral(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    _accumulate(gpu, scene, cam, W, H, depth, [3, 3])
    film = gpu.read_spectral(W, H)
    finite = np.isfinite(film).all(axis=-1)
    assert finite.mean() > 0.9 and film[finite].max() > 0
    calls = 0
    for first in range(0, N_GRID, 16):
        count = min(16, N_GRID - first)
        got = gpu.develop_spectral(W, H, one_hot(first, count))
        assert got.shape == (H, W, count)
        assert bits_equal_or_both_nan(got, film[..., first:first + count])[finite].all(), first
        calls += 1
    assert calls == 6


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "random_spheres"])
def test_developed_workload_equals_the_restatement_and_the_xyz_sums(srt, gpu, name):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    _accumulate(gpu, scene, cam, W, H, depth, [2, 4])
    film = gpu.read_spectral(W, H)
    assert film.max() > 0
    for k, scale in ((5, F(0.37)), (16, F(-2.0)), (1, F(1))):
        resp = _responses(k, seed=23)
        got = gpu.develop_spectral(W, H, resp, scale)
        assert_same_floats(got, develop(film, resp, scale), "%s K = %d" % (name, k))
    # the colour-matching rows at the kernel's 470/7: the accumulation's XYZ sums up to reassociation
    cie = srt.renderer.cie_response()
    got = gpu.develop_spectral(W, H, cie, CIE_SCALE)
    assert_same_floats(got, develop(film, cie, CIE_SCALE), name + " CIE rows")
    frame = read_frame(gpu, W, H)
    lane = lane_of(gpu.geom, W, H)
    want = np.stack([frame["xyz"][c][lane] for c in range(3)], axis=-1).reshape(H, W, 3)
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    ok = ~np.isnan(want)
    assert np.abs(want[ok]).max() > 0
    np.testing.assert_allclose(got[ok].astype(np.float64), want[ok].astype(np.float64), rtol=2e-4, atol=1e-9, err_msg=name)


@pytest.mark.gpu
def test_srgb_variant_is_the_render_kernels_conversion_and_a_filter_halves(srt, gpu, orc):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    _accumulate(gpu, scene, cam, W, H, depth, [2, 4])
    n = gpu.accum_samples
    assert n == 6
    film = gpu.read_spectral(W, H)
    cie = srt.renderer.cie_response()
    res = gpu.develop_spectral_srgb(W, H)
    assert set(res) == {"xyz", "lin", "fb"} and all(v.shape == (H, W, 3) for v in res.values())
    assert_same_floats(res["xyz"], develop(film, cie, CIE_SCALE), "sRGB variant, developed sums")
    ms = gpu.develop_last_ms()
    assert ms["contract"] > 0 and ms["epilogue"] > 0
    sums = res["xyz"].reshape(-1, 3)
    lin, q = convert_xyz(orc, [sums[:, c] for c in range(3)], n)
    assert_same_floats(res["lin"].reshape(-1, 3), np.stack(lin, axis=1), "sRGB variant, unquantised")
    assert_same_floats(res["fb"].reshape(-1, 3), np.stack(q, axis=1), "sRGB variant, quantised")
    assert res["fb"].max() > 0 and len(np.unique(res["fb"])) > 8
    # the header's normalising step is what convert_xyz applies before the oracle's conversion
    assert np.array_equal(bits(normalise(sums, n)), bits((F(1) / F(n)) * sums))
    # explicit curves give the same bits as the NULL default; a single requested output works
    again = gpu.develop_spectral_srgb(W, H, cie, CIE_SCALE)
    for key in res:
        assert_same_floats(again[key], res[key], "explicit CIE rows " + key)
    only = np.zeros((H, W, 3), F)
    gpu._ck(gpu_lib().srt_develop_spectral_srgb(gpu._h, None, CIE_SCALE, None, only.ctypes.data_as(FP), None, W, H))
    assert_same_floats(only, res["lin"], "out_lin alone")
    # a neutral filter of 0.5: every product and every sum halves exactly
    dev = gpu.develop_spectral(W, H, cie, CIE_SCALE)
    half = gpu.develop_spectral(W, H, cie, CIE_SCALE, filter=np.full(N_GRID, 0.5))
    assert_same_floats(half, (F(0.5) * dev).astype(F), "0.5 filter")
    half_srgb = gpu.develop_spectral_srgb(W, H, filter=np.full(N_GRID, 0.5))
    assert_same_floats(half_srgb["xyz"], (F(0.5) * dev).astype(F), "0.5 filter, sRGB variant")
    assert dev[np.isfinite(dev)].max() > 0


# ---- placement, partitions, the communicator -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_offset_chunk_and_a_rank_of_a_partition(srt, gpu):
    scene, _, W, H, depth, _ = named_workload(srt, "random_spheres")
    resp, scale = _responses(4, seed=31), F(-1.5)
    # a 30 x 21 chunk (no multiple of 8 x 8 or 28 x 16) at (17, 9) of a 64 x 40 image
    IW, IH, cw, ch, ox, oy = 64, 40, 30, 21, 17, 9
    cam = scene.default_camera(IW, IH)
    _accumulate(gpu, scene, cam, cw, ch, depth, [1, 3], ox, oy)
    film = gpu.read_spectral(IW, IH)
    got = gpu.develop_spectral(IW, IH, resp, scale)
    inside = np.zeros((IH, IW), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    assert film[inside].max() > 0 and not bits(film[~inside]).any()
    assert_same_floats(got[inside], develop(film[inside], resp, scale), "offset chunk")
    assert not bits(got[~inside]).any()
    # the caller's array outside the rectangle is not written at all
    sentinel = np.full((IH, IW, 4), F(-7), F)
    gpu._ck(gpu_lib().srt_develop_spectral(gpu._h, resp.ctypes.data_as(FP), 4, scale, sentinel.ctypes.data_as(FP), IW, IH))
    assert (sentinel[~inside] == F(-7)).all() and np.array_equal(bits(sentinel[inside]), bits(got[inside]))
    # rank 1 of two: its own pixels developed, the other rank's pixels (a zero film row) zero in value
    cam = scene.default_camera(W, H)
    _accumulate(gpu, scene, cam, W, H, depth, [2, 2], partition=(1, 2))
    film = gpu.read_spectral(W, H)
    got = gpu.develop_spectral(W, H, resp, scale)
    gpu.set_partition(0, 1)
    assert_same_floats(got, develop(film, resp, scale), "rank 1 of 2")
    other = ~bits(film).any(axis=-1)
    assert 0.3 < other.mean() < 0.7
    assert (got[other] == 0).all() and np.abs(got[~other]).max() > 0


@pytest.mark.gpu
def test_comm_two_ranks_one_gpu_mock_transport():
    run_mock_transport_child("""
import numpy as np
from accum_helpers import comm_accumulations
from path_ends_reference import assert_same_floats
scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
W, H, depth = 48, 40, 8
cam = scene.default_camera(W, H)
rng = np.random.default_rng(41)
resp = (rng.random((5, 95)) - 0.4).astype(np.float32)
filt = rng.random(95).astype(np.float32)
steps = list(srt.render_developed(scene, cam, W, H, [3, 3], depth, response=resp, filter=filt, scale=0.5))
total, _, ref = steps[-1]
assert total == 6 and ref.shape == (H, W, 5) and np.abs(ref[np.isfinite(ref)]).max() > 0
for _, comm in comm_accumulations(srt, 2, (9,), scene, cam, W, H, depth, 6, lambda c: c.accum_reset_spectral(), (3, 3)):
    got = comm.develop_spectral(W, H, resp, 0.5, filter=filt)
    assert_same_floats(got, ref, 'two ranks')
    parts = [r.develop_spectral(W, H, resp, 0.5, filter=filt) for r in comm.renderers]
    assert all(np.abs(p[np.isfinite(p)]).max() > 0 for p in parts) and ((parts[0] == 0).all(axis=-1) | (parts[1] == 0).all(axis=-1)).all()
print('develop mock transport ok')
""", "develop mock transport ok", timeout=300)


# ---- the develop only reads ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_develop_between_passes_changes_nothing(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    resp = _responses(16, seed=51)

    def run(with_develop):
        _accumulate(gpu, scene, cam, W, H, depth, [3])
        if with_develop:
            gpu.develop_spectral(W, H, resp, 2.0)
            gpu.develop_spectral_srgb(W, H)
            gpu.develop_kat(np.ones((70, N_GRID), F), resp[:2])
        gpu.render_chunk_accum(W, H, 5)
        frame, film = read_frame(gpu, W, H), gpu.read_spectral(W, H)
        assert gpu.accum_samples == 8
        gpu.render_chunk(W, H)                # continues every pixel's RNG stream from where the passes left it
        return frame, film, read_frame(gpu, W, H)

    frame, film, after = run(True)
    frame0, film0, after0 = run(False)
    assert np.array_equal(bits(film), bits(film0)) and film0.max() > 0
    for key in ("fb", "lin", "xyz", "rowmajor"):
        assert_planes_equal(frame[key], frame0[key], "frame after pass, develop, pass: " + key)
        assert_planes_equal(after[key], after0[key], "RNG state: plain launch after the passes, " + key)


@pytest.mark.gpu
def test_render_developed_generator(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    steps = list(srt.render_developed(scene, cam, W, H, [2, 4], depth, renderer=gpu))
    assert [t for t, _, _ in steps] == [2, 6]
    spectral = list(srt.render_spectral(scene, cam, W, H, [2, 4], depth, renderer=gpu))
    cie = srt.renderer.cie_response()
    for (t, res, dev), (t2, res2, _) in zip(steps, spectral):
        assert t == t2 and set(dev) == {"xyz", "lin", "fb"}
        for key in ("fb", "lin", "xyz", "rowmajor"):
            assert_planes_equal(res[key], res2[key], "render_developed vs render_spectral " + key)
        assert_same_floats(dev["xyz"], develop(res2["film"], cie, CIE_SCALE), "developed after %d samples" % t)
    (t, _, band), = srt.render_developed(scene, cam, W, H, [6], depth, response=one_hot(40, 3), renderer=gpu)
    film = spectral[-1][1]["film"]
    ok = np.isfinite(film).all(axis=-1)
    assert t == 6 and np.array_equal(bits(band[ok]), bits(film[ok][:, 40:43]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(srt, gpu):
    scene, cam, W, H, depth, _ = named_workload(srt, "prism")
    L = gpu_lib()
    resp = _responses(3, seed=61)
    rp = resp.ctypes.data_as(FP)
    out = np.zeros((H, W, 16), F)
    op = out.ctypes.data_as(FP)
    # before the first develop of a context there are no times
    fresh = srt.Renderer(0)
    try:
        assert L.srt_develop_last_ms(fresh._h, None, None) == ERR_INVALID
        assert L.srt_develop_spectral(fresh._h, rp, 3, 1.0, op, W, H) == ERR_INVALID      # no accumulation at all
    finally:
        fresh.close()
    # a plain accumulation has no film; a spectral one needs a pass
    fresh_context(gpu, scene, cam, W, H, depth)
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    expect_error(srt, lambda: gpu.develop_spectral(W, H, resp), ERR_INVALID, "develop of a plain accumulation")
    expect_error(srt, lambda: gpu.develop_spectral_srgb(W, H), ERR_INVALID, "sRGB develop of a plain accumulation")
    gpu.accum_reset_spectral()
    expect_error(srt, lambda: gpu.develop_spectral(W, H, resp), ERR_INVALID, "develop before the first pass")
    gpu.render_chunk_accum(W, H, 4)
    first = gpu.develop_spectral(W, H, resp, 0.5)
    first_srgb = gpu.develop_spectral_srgb(W, H)
    film, frame = gpu.read_spectral(W, H), read_frame(gpu, W, H)
    bad = resp.copy()
    bad[2, 94] = np.nan
    inf = resp.copy()
    inf[0, 0] = -np.inf
    bp, ip = bad.ctypes.data_as(FP), inf.ctypes.data_as(FP)
    wide = np.zeros((17, N_GRID), F)
    small = np.zeros((4, N_GRID), F)
    sp = small.ctypes.data_as(FP)
    refused = [
        ("null response", lambda: L.srt_develop_spectral(gpu._h, None, 3, 1.0, op, W, H)),
        ("null out", lambda: L.srt_develop_spectral(gpu._h, rp, 3, 1.0, None, W, H)),
        ("no channel", lambda: L.srt_develop_spectral(gpu._h, rp, 0, 1.0, op, W, H)),
        ("17 channels", lambda: L.srt_develop_spectral(gpu._h, wide.ctypes.data_as(FP), 17, 1.0, op, W, H)),
        ("empty image, width", lambda: L.srt_develop_spectral(gpu._h, rp, 3, 1.0, op, 0, H)),
        ("empty image, height", lambda: L.srt_develop_spectral(gpu._h, rp, 3, 1.0, op, W, 0)),
        ("NaN response", lambda: L.srt_develop_spectral(gpu._h, bp, 3, 1.0, op, W, H)),
        ("infinite response", lambda: L.srt_develop_spectral(gpu._h, ip, 3, 1.0, op, W, H)),
        ("NaN scale", lambda: L.srt_develop_spectral(gpu._h, rp, 3, float("nan"), op, W, H)),
        ("infinite scale", lambda: L.srt_develop_spectral(gpu._h, rp, 3, float("inf"), op, W, H)),
        ("sRGB: no output", lambda: L.srt_develop_spectral_srgb(gpu._h, None, 1.0, None, None, None, W, H)),
        ("sRGB: empty image", lambda: L.srt_develop_spectral_srgb(gpu._h, None, 1.0, op, None, None, W, 0)),
        ("sRGB: NaN response", lambda: L.srt_develop_spectral_srgb(gpu._h, bp, 1.0, op, None, None, W, H)),
        ("sRGB: infinite scale", lambda: L.srt_develop_spectral_srgb(gpu._h, None, float("-inf"), op, None, None, W, H)),
        ("KAT: null film", lambda: L.srt_develop_kat(gpu._h, None, 4, rp, 3, 1.0, op)),
        ("KAT: null out", lambda: L.srt_develop_kat(gpu._h, sp, 4, rp, 3, 1.0, None)),
        ("KAT: no pixel", lambda: L.srt_develop_kat(gpu._h, sp, 0, rp, 3, 1.0, op)),
        ("KAT: 2^31 pixels", lambda: L.srt_develop_kat(gpu._h, sp, 0x80000000, rp, 3, 1.0, op)),
        ("KAT: 17 channels", lambda: L.srt_develop_kat(gpu._h, sp, 4, wide.ctypes.data_as(FP), 17, 1.0, op)),
        ("KAT: NaN response", lambda: L.srt_develop_kat(gpu._h, sp, 4, bp, 3, 1.0, op)),
        ("KAT: NaN scale", lambda: L.srt_develop_kat(gpu._h, sp, 4, rp, 3, float("nan"), op)),
    ]
    for what, call in refused:
        assert call() == ERR_INVALID, what
        assert not bits(out).any(), what
    # a film of 2^31 - 1 rows is 824 GB: the allocation fails before anything is read or launched
    assert L.srt_develop_kat(gpu._h, sp, 0x7fffffff, rp, 3, 1.0, op) == ERR_HIP
    assert not bits(out).any()
    # after all of them the accumulation develops, reads and continues as before
    assert_same_floats(gpu.develop_spectral(W, H, resp, 0.5), first, "develop after the refusals")
    again = gpu.develop_spectral_srgb(W, H)
    for key in first_srgb:
        assert_same_floats(again[key], first_srgb[key], "sRGB develop after the refusals, " + key)
    assert np.array_equal(bits(gpu.read_spectral(W, H)), bits(film))
    for key, v in read_frame(gpu, W, H).items():
        assert_planes_equal(v, frame[key], "after the refusals " + key)
    assert gpu.accum_samples == 4
    assert np.array_equal(bits(gpu.develop_kat(small + F(1), resp)), bits(develop(small + F(1), resp)))
    # whatever ends the accumulation ends the develop
    gpu.accum_reset()
    gpu.render_chunk_accum(W, H, 2)
    expect_error(srt, lambda: gpu.develop_spectral(W, H, resp), ERR_INVALID, "develop after srt_accum_reset")
    gpu.set_gather_planes(9)
