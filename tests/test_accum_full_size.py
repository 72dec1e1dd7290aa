"""Progressive (MODE 3), adaptive (MODE 4) and spectral (MODE 5) accumulations at the frame sizes people render, where code runs that
the small frames of test_progressive / test_adaptive / test_spectral never reach: adapt_scan_kernel's runs of more than one queue row
per thread (more than 1024 rows), adapt_flag_kernel's stride loop (more than 4096 rows), the ordered queue with split rows at full
size, a film of more than 2^31 and of more than 2^32 bytes, and the headline frame's frozen checksum through every accumulating mode.
Every case asserts the size property that makes it worth running, so that a change of tile or block sizes cannot quietly turn it
into a small-frame test.  The references are those of the small-frame suites: one-shot frames (themselves held to the oracle and
the frozen digests), the numpy float32 restatement of every stop decision, the oracle on 28 x 16 blocks, and the contraction of the
film to the XYZ sums."""
import numpy as np
import pytest

from accum_helpers import (MIN_SPP, NEVER, N_GRID, SCHED, adaptive_run, assert_pixels_equal, assert_same_image, fresh_context, gather_ranks,
                           lane_of, pick_tolerance, predict_stops, read_frame, read_sum_y, run_mock_transport_child, spectral_run)
from helpers import _blocks_bit_exact, assert_planes_equal, bits, oracle_scene_for

pytestmark = pytest.mark.gpu

HW, HH, HSPP, HDEPTH = 1920, 1080, 1024, 16      # the headline frame (bench.py's flagship workload)
HEADLINE_CHECKSUM = 895685025                    # test_oracle_digests.test_headline_frame_checksum_is_frozen
HEADLINE_PASSES = [16, 48, 960]
FILM_BYTES_PER_LANE = (N_GRID + 1) * 4           # kFilmStride floats per lane
ORACLE_THREADS = 16


def _headline_scene(srt):
    return srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)


def _checksum(gpu):
    """the sum of the quantised planes, as bench.py prints it (the tile buffer must have been scattered)"""
    return int(sum(int(p.astype(np.int64).sum()) for p in gpu.read_fb()))


def _tiles_local(r):
    return r.tile_buffer()[2]


def _film_bytes(r):
    return r.geom["n_lanes"] * FILM_BYTES_PER_LANE


def _xyz_rows(srt):
    """(95, 3) float64: film_to_xyz of each unit film, so that a sub-range [first, first + count) contracts with rows first .."""
    return srt.film_to_xyz(np.eye(N_GRID, dtype=np.float32))


def _film_ranges(r, IW, IH, step):
    """the whole film, `step` grid samples at a time: (first, (IH, IW, count) float32); host memory stays at one range"""
    for first in range(0, N_GRID, step):
        count = min(step, N_GRID - first)
        yield first, r.read_spectral(IW, IH, first, count)


def _xyz_rowmajor(frame, lane, W, H):
    return np.stack([frame["xyz"][c][lane] for c in range(3)], axis=-1).reshape(H, W, 3).astype(np.float64)


def _assert_xyz_close(got, want, what):
    """test_spectral.test_film_contracts_to_the_xyz_sums's comparison (NaN where the sums are NaN, rtol 2e-4)"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.abs(want[ok]).max() > 0, what
    np.testing.assert_allclose(got[ok], want[ok], rtol=2e-4, atol=1e-9, err_msg=what)


def _contract_and_check(srt, r, W, H, frame, what, step=5, other=None, full=None, edges=True):
    """the film of r (a W x H chunk at (0, 0)) contracted in float64 over sub-range reads of `step` grid samples against the XYZ sums
    of `frame`; with `edges`, the first and last image rows are checked on their own as well (they must hold light).  `other`: a
    renderer whose film must be the same bits, range by range; `full`: a full read of r's film that every range must equal bit for
    bit."""
    rows = _xyz_rows(srt)
    got = np.zeros((H, W, 3), np.float64)
    for first, part in _film_ranges(r, W, H, step):
        count = part.shape[-1]
        assert (part[~np.isnan(part)] >= 0).all(), (what, first)
        for tag, want in (("split", None if other is None else other.read_spectral(W, H, first, count)),
                          ("sub-range of the full read", None if full is None else full[..., first:first + count])):
            if want is not None:
                differ = int((bits(part) != bits(want)).sum())
                assert differ == 0, "%s, %s, grid samples %d..%d: %d of %d sums differ" % (what, tag, first, first + count - 1, differ, part.size)
            del want
        got += part.astype(np.float64) @ rows[first:first + count]
        del part
    want = _xyz_rowmajor(frame, lane_of(r.geom, W, H), W, H)
    _assert_xyz_close(got, want, what)
    if edges:
        _assert_xyz_close(got[-8:], want[-8:], what + ": the last 8 rows")
        _assert_xyz_close(got[:8], want[:8], what + ": the first 8 rows")


def _blocks_at_counts(r, orc, scene, mode, cam, W, H, depth, frame, counts, block_lo, stride, max_blocks):
    """the 28 x 16 blocks block_lo, block_lo + stride, .. of an adaptive frame against the oracle: each pixel at its own count, bit for
    bit in the quantised and XYZ planes"""
    g = r.geom
    lane_counts = np.zeros(g["n_lanes"], np.int64)
    lane_counts[lane_of(g, W, H)] = counts
    blocks = list(range(block_lo, g["bx"] * g["by"], stride))
    assert 1 <= len(blocks) <= max_blocks, blocks
    osc = oracle_scene_for(orc, scene, mode)
    bs = g["tx"] * g["ty"]
    compared = np.zeros(len(blocks), np.int64)
    for c in np.unique(counts):
        ref = osc.render(cam, W, H, int(c), depth, block_lo=block_lo, block_stride=stride, threads=ORACLE_THREADS)
        for k, b in enumerate(blocks):
            sl = slice(b * bs, (b + 1) * bs)
            m = lane_counts[sl] == c
            for p in range(3):
                assert np.array_equal(bits(frame["xyz"][p][sl])[m], bits(ref["xyz"][p][sl])[m]), ("block", b, c, "xyz", p)
                assert np.array_equal(frame["fb"][p][sl][m], ref["fb"][p][sl][m]), ("block", b, c, "fb", p)
            compared[k] += int(m.sum())
    assert (compared > 0).all(), compared
    return len(blocks)


def _check_adaptive_run(srt, r, run, never, rel, scene, cam, W, H, depth, one_shots, what):
    """run (accum_helpers.adaptive_run) against the float32 restatement: samples map and active count after every pass, the paths of
    every pass; and every pixel against the one-shot frame of its count (one_shots: count -> frame, filled on demand)"""
    maps, _, actives = predict_stops(never, rel)
    before = W * H
    for k, (p, want, act) in enumerate(zip(run, maps, actives)):
        got = p["stats"]["samples"]
        assert np.array_equal(got, want), "%s pass %d: %d pixels differ" % (what, k, int((got != want).sum()))
        assert p["active"] == act, (what, k, p["active"], act)
        assert p["paths"] == before * (p["total"] - (run[k - 1]["total"] if k else 0)), (what, k, p["paths"], before)
        before = act
    last = run[-1]
    counts = last["stats"]["samples"]
    lane = lane_of(r.geom, W, H)
    for c in np.unique(counts):
        if int(c) not in one_shots:
            one_shots[int(c)] = srt.render_image(scene, cam, W, H, int(c), depth, renderer=r)
        mask = counts == c
        assert_pixels_equal(last["frame"], one_shots[int(c)], mask, lane, "%s: %d pixels at %d spp" % (what, mask.sum(), c))
    return counts


def _lean(run):
    """drops the frames of every pass but the last (a 1080p frame is ~100 MB of host memory)"""
    for p in run[:-1]:
        p.pop("frame", None)
    return run


@pytest.fixture(scope="module")
def headline(srt, gpu):
    """the headline scene at 1080p: a never-stopping adaptive run of SCHED (its sums at every boundary are those of every run), the
    tolerance pick_tolerance takes, and one under which about 1 % of the pixels render in the last pass"""
    scene = _headline_scene(srt)
    cam = scene.default_camera(HW, HH)
    never = _lean(adaptive_run(gpu, scene, cam, HW, HH, HDEPTH, NEVER))
    never[-1].pop("frame")
    rel = pick_tolerance(never)
    n = HW * HH
    best, best_d = None, None
    for cand in np.geomspace(1e-4, 10.0, 241):
        _, _, actives = predict_stops(never, float(cand))
        d = abs(actives[-2] / n - 0.01)          # the queue the last pass renders from
        if actives[-1] > 0 and (best is None or d < best_d):
            best, best_d = float(cand), d
    return dict(scene=scene, cam=cam, never=never, rel=rel, rel_sparse=best)


# ---- 1. the headline frame through every accumulating mode -------------------------------------------------------------------

def test_headline_frame_checksum_through_every_accumulating_mode(srt, gpu):
    scene = _headline_scene(srt)
    cam = scene.default_camera(HW, HH)
    n_pix = HW * HH
    assert sum(HEADLINE_PASSES) == HSPP and len(set(HEADLINE_PASSES)) == len(HEADLINE_PASSES)

    # plain (MODE 3)
    fresh_context(gpu, scene, cam, HW, HH, HDEPTH, spp=HSPP)
    gpu.accum_reset()
    for s in HEADLINE_PASSES:
        gpu.render_chunk_accum(HW, HH, s)
        assert gpu.stats()["paths"] == n_pix * s
    assert gpu.accum_samples == HSPP
    gpu.scatter_tiles()
    assert _checksum(gpu) == HEADLINE_CHECKSUM, "plain accumulation"
    assert _tiles_local(gpu) > 4096

    # adaptive (MODE 4) with a tolerance nothing meets: every pixel renders every pass
    fresh_context(gpu, scene, cam, HW, HH, HDEPTH, spp=HSPP)
    gpu.accum_reset_adaptive(NEVER, 0.0, MIN_SPP)
    for s in HEADLINE_PASSES:
        gpu.render_chunk_accum(HW, HH, s)
        assert gpu.stats()["paths"] == n_pix * s
        assert gpu.accum_active == n_pix
    samples = gpu.accum_stats(HW, HH)["samples"]
    assert (samples == HSPP).all()
    gpu.scatter_tiles()
    assert _checksum(gpu) == HEADLINE_CHECKSUM, "adaptive accumulation, rel_tol = NEVER"

    # spectral (MODE 5): the checksum, and the film (807 MB) contracts to the XYZ sums
    fresh_context(gpu, scene, cam, HW, HH, HDEPTH, spp=HSPP)
    gpu.accum_reset_spectral()
    for s in HEADLINE_PASSES:
        gpu.render_chunk_accum(HW, HH, s)
        assert gpu.stats()["paths"] == n_pix * s
    assert _film_bytes(gpu) > 2 ** 29
    frame = read_frame(gpu, HW, HH)
    assert _checksum(gpu) == HEADLINE_CHECKSUM, "spectral accumulation"
    full = gpu.read_spectral(HW, HH)
    _contract_and_check(srt, gpu, HW, HH, frame, "headline film", step=5, full=full)
    for first, count in ((94, 1), (0, 1), (13, 29), (47, 48)):
        part = gpu.read_spectral(HW, HH, first, count)
        assert np.array_equal(bits(part), bits(full[..., first:first + count])), (first, count)


# ---- 2. adaptive at full size, three kinds of queue ------------------------------------------------------------------------

QUEUES = [({}, "ordered, split rows"), ({"SRT_SPLIT_LOAD": "0"}, "ordered, no split"), ({"SRT_PROBE_SPP": "0"}, "identity")]


@pytest.mark.parametrize("env,kind", QUEUES, ids=["split", "no-split", "identity"])
def test_adaptive_full_size_queues(srt, orc, headline, monkeypatch, env, kind):
    """The queue of an adaptive pass (adapt_flag_kernel + adapt_scan_kernel) at 1080p: 242 x 136 tiles of 8 x 8 pixels.  The
    identity queue (no cost probe) has one row per local tile: above 4096 rows adapt_flag_kernel's waves take several rows each.
    The ordered queue holds at least one row per tile, so adapt_scan_kernel's threads compact runs of several rows.  With splitting
    on (SRT_SPLIT_LOAD, default 200) the queue is bounded by 64 rows per tile and its rows carry the part / split-level fields of a
    split tile (whether order_tiles_kernel actually splits a tile here depends on the probe's costs: it is not visible through the
    C-ABI).  Each run: the tolerance pick_tolerance takes, and one under which about 1 % of the pixels stay active, so that the
    queue of the last pass is long, sparse and interleaved."""
    for k in ("SRT_SPLIT_LOAD", "SRT_PROBE_SPP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene, cam, never = headline["scene"], headline["cam"], headline["never"]
    r = srt.Renderer(0)                       # the knobs are read when the context is created
    try:
        one_shots = {}
        for rel, tag in ((headline["rel"], "picked tolerance"), (headline["rel_sparse"], "~1 % active")):
            what = "%s queue, %s" % (kind, tag)
            run = _lean(adaptive_run(r, scene, cam, HW, HH, HDEPTH, rel))
            tiles = _tiles_local(r)
            assert tiles > 4096, tiles                     # the identity queue's rows; a lower bound of the ordered queue's
            assert -(-tiles // 1024) > 1                   # adapt_scan_kernel: rows per thread
            counts = _check_adaptive_run(srt, r, run, never, rel, scene, cam, HW, HH, HDEPTH, one_shots, what)
            if tag == "picked tolerance":
                assert len(np.unique(counts)) >= 3, np.unique(counts)
            else:
                frac = run[-2]["active"] / (HW * HH)
                assert 0.002 < frac < 0.05, frac
            n = _blocks_at_counts(r, orc, scene, srt.BVH_SAH, cam, HW, HH, HDEPTH, run[-1]["frame"], counts, 97, 1100, 5)
            assert n >= 4
            del run
    finally:
        r.close()


# ---- 3. the 100k-triangle mesh at 4K: the partly-cached kernel shape ------------------------------------------------------

def test_mesh100k_4k_partly_cached_shape(srt, gpu, orc):
    W, H, depth = 3840, 2160, 16
    scene = srt.Scene.builtin(srt.SCENE_MESH100K, 0).build_bvh(srt.BVH_SAH, 1984)
    cam = scene.default_camera(W, H)
    gpu.upload_scene(scene)
    plan = gpu.launch_plan()
    assert not plan["all_cached"] and plan["n_cached"] > 0 and not plan["narrow_refs"], plan

    # progressive split == one-shot, and the one-shot's blocks against the oracle (_blocks_bit_exact renders it)
    fresh_context(gpu, scene, cam, W, H, depth, spp=8)
    gpu.accum_reset()
    for s in (3, 5):
        gpu.render_chunk_accum(W, H, s)
        assert gpu.stats()["paths"] == W * H * s
    split = read_frame(gpu, W, H)
    assert _tiles_local(gpu) > 4096
    assert _blocks_bit_exact(srt, gpu, orc, srt.SCENE_MESH100K, srt.BVH_SAH, W, H, 8, depth, 2000, 4100, 6) >= 4
    one_shot = dict(fb=gpu.read_fb(), lin=gpu.read_fb_aux(1), xyz=gpu.read_fb_aux(2), rowmajor=gpu.read_fb_rowmajor(W, H))
    assert_same_image(split, one_shot, "4K mesh [3, 5] vs one-shot 8 spp")
    del split, one_shot
    gpu.upload_scene(scene)
    assert not gpu.launch_plan()["all_cached"]

    # adaptive, as in the 1080p test (a shorter schedule)
    sched = [8, 4, 4]
    never = _lean(adaptive_run(gpu, scene, cam, W, H, depth, NEVER, sched=sched))
    never[-1].pop("frame")
    rel = pick_tolerance(never)
    run = _lean(adaptive_run(gpu, scene, cam, W, H, depth, rel, sched=sched))
    counts = _check_adaptive_run(srt, gpu, run, never, rel, scene, cam, W, H, depth, {}, "4K mesh adaptive")
    assert len(np.unique(counts)) >= 2, np.unique(counts)
    _blocks_at_counts(gpu, orc, scene, srt.BVH_SAH, cam, W, H, depth, run[-1]["frame"], counts, 3001, 9000, 2)
    del run

    # spectral: a 3.2 GB film contracts to the XYZ sums
    fresh_context(gpu, scene, cam, W, H, depth, spp=4)
    gpu.accum_reset_spectral()
    for s in (2, 2):
        gpu.render_chunk_accum(W, H, s)
    assert _film_bytes(gpu) > 2 ** 31
    _contract_and_check(srt, gpu, W, H, read_frame(gpu, W, H), "4K mesh film", edges=False)    # (its bottom rows are black)


# ---- 4. a film of more than 2^32 bytes ------------------------------------------------------------------------------------

def test_film_above_4_gib(srt, gpu):
    """4608 x 2592 (165 x 163 blocks of 28 x 16 lanes, 384 bytes each: 4.6 GB), 2 spp of the headline scene: the film contracts to
    the XYZ sums over the whole frame (the pixels past byte 2^32 of the film are the image's last ~170 rows), two passes of 1 sample
    are the same film as one of 2, and an offset chunk near the bottom-right corner of the same image writes its rectangle only"""
    W, H, depth = 4608, 2592, 8
    scene = _headline_scene(srt)
    cam = scene.default_camera(W, H)
    other = srt.Renderer(0)
    try:
        fresh_context(other, scene, cam, W, H, depth, spp=2)
        other.accum_reset_spectral()
        other.render_chunk_accum(W, H, 2)
        fresh_context(gpu, scene, cam, W, H, depth, spp=2)
        gpu.accum_reset_spectral()
        for s in (1, 1):
            gpu.render_chunk_accum(W, H, s)
        assert _film_bytes(gpu) > 2 ** 32, _film_bytes(gpu)
        last_lane = int(lane_of(gpu.geom, W, H)[-1])
        assert last_lane * FILM_BYTES_PER_LANE > 2 ** 32                  # the last pixel's row lies past 2^32 bytes
        _contract_and_check(srt, gpu, W, H, read_frame(gpu, W, H), "4.6 GB film", step=5, other=other)
    finally:
        other.close()

    # a 1000 x 600 chunk at the bottom-right corner of the 4608 x 2592 image
    cw, ch = 1000, 600
    ox, oy = W - cw - 3, H - ch - 5
    fresh_context(gpu, scene, cam, cw, ch, depth, spp=2)
    gpu.accum_reset_spectral()
    gpu.render_chunk_accum(cw, ch, 2, ox, oy)
    inside = np.zeros((H, W), bool)
    inside[oy:oy + ch, ox:ox + cw] = True
    sentinel = np.float32(-7.0)
    out = np.full((H, W, 5), sentinel, np.float32)
    gpu.read_spectral(W, H, 90, 5, into=out)
    assert (out[~inside] == sentinel).all()
    assert (out[inside] >= 0).all() and out[inside].max() > 0
    del out
    rows = _xyz_rows(srt)
    got_y = np.zeros(int(inside.sum()), np.float64)
    for first, part in _film_ranges(gpu, W, H, 5):
        assert (part[~inside] == 0).all(), first
        got_y += part[inside].astype(np.float64) @ rows[first:first + part.shape[-1], 1]
        del part
    want_y = read_sum_y(gpu, W, H).reshape(H, W)[inside].astype(np.float64)      # (a spectral accumulation has no sample map)
    assert want_y.max() > 0
    np.testing.assert_allclose(got_y, want_y, rtol=2e-4, atol=1e-9)


# ---- 5. partitions and the communicator at full size ---------------------------------------------------------------------

def _owner_mask(W, H, geom, rank, world):
    """row-major pixels whose 8 x 8 tile belongs to `rank` (tile % world, tiles over the reference grid's cover)"""
    tiles_x = (geom["tx"] * geom["bx"] + 7) // 8
    j, i = np.divmod(np.arange(W * H), W)
    return (((j // 8) * tiles_x + i // 8) % world == rank).reshape(H, W)


@pytest.mark.parametrize("world", [3, 7])
def test_partitions_full_size(srt, gpu, headline, world):
    """ragged tile shares (32 912 tiles over 3 or 7 ranks): the merged adaptive frame, its samples map and active count, and the
    merged spectral frame and film are bit-identical to world 1"""
    scene, cam, rel = headline["scene"], headline["cam"], headline["rel"]
    ref = adaptive_run(gpu, scene, cam, HW, HH, HDEPTH, rel)[-1]

    def adaptive_rank(rank):
        fresh_context(gpu, scene, cam, HW, HH, HDEPTH)
        gpu.set_partition(rank, world)
        gpu.accum_reset_adaptive(rel, 0.0, MIN_SPP)
        for s in SCHED:
            gpu.render_chunk_accum(HW, HH, s)
        assert _tiles_local(gpu) > 4096
        return gpu.accum_stats(HW, HH)["samples"], gpu.accum_active
    samples, actives = zip(*gather_ranks(gpu, world, adaptive_rank))
    assert np.array_equal(sum(samples), ref["stats"]["samples"]), world
    assert sum(actives) == ref["active"], world
    assert_planes_equal(gpu.read_fb(), ref["frame"]["fb"], "adaptive world %d fb" % world)
    assert_planes_equal(gpu.read_fb_aux(1), ref["frame"]["lin"], "adaptive world %d lin" % world)
    assert_planes_equal(gpu.read_fb_aux(2), ref["frame"]["xyz"], "adaptive world %d xyz" % world)
    del ref

    passes = [4, 8]
    ref_frame, ref_film = spectral_run(gpu, scene, cam, HW, HH, HDEPTH, passes)
    assert ref_film.max() > 0

    def spectral_rank(rank):
        fresh_context(gpu, scene, cam, HW, HH, HDEPTH)
        gpu.set_partition(rank, world)
        gpu.accum_reset_spectral()
        for s in passes:
            gpu.render_chunk_accum(HW, HH, s)
        film = gpu.read_spectral(HW, HH)
        own = _owner_mask(HW, HH, gpu.geom, rank, world)
        assert np.array_equal(bits(film[own]), bits(ref_film[own])), (world, rank)
        assert (bits(film[~own]) == 0).all(), (world, rank)
    gather_ranks(gpu, world, spectral_rank)
    for k, i in (("fb", 0), ("lin", 1), ("xyz", 2)):
        got = gpu.read_fb() if i == 0 else gpu.read_fb_aux(i)
        assert_planes_equal(got, ref_frame[k], "spectral world %d %s" % (world, k))


def test_comm_three_ranks_full_size_mock_transport(headline):
    """srt_comm_* at W = 3 on one GPU over the test transport (tests/cpp/mock_rccl.cpp; in a child process, as the small-frame
    communicator tests): an adaptive and a spectral accumulation of the 1080p headline scene equal those of one renderer"""
    run_mock_transport_child("""
import numpy as np
from helpers import assert_planes_equal, bits
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
W, H, depth, rel, world = %d, %d, %d, %r, 3
cam = scene.default_camera(W, H)
for total, active, ref in srt.render_adaptive(scene, cam, W, H, depth, rel, min_spp=8, step=4, max_spp=24):
    pass
assert total == 24 and active > 0 and len(np.unique(ref['samples'])) >= 3, (total, active)
comm = srt.Comm.init_all([0] * world)
comm.set_gather_planes(9)
comm.upload_scene(scene); comm.set_camera(cam)
comm.init_device_params(W, H, 24, depth, 1984)
comm.accum_reset_adaptive(rel, 0.0, 8)
for s in (8, 4, 4, 4, 4):
    comm.render_frame_accum(W, H, s)
comm.synchronize()
assert comm.accum_active == active, (comm.accum_active, active)
root = comm.root
assert_planes_equal(root.read_fb(), ref['fb'], 'adaptive fb')
assert_planes_equal(root.read_fb_aux(1), ref['lin'], 'adaptive lin')
assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'adaptive xyz')
samples = sum(r.accum_stats(W, H)['samples'] for r in comm.renderers)
assert np.array_equal(samples, ref['samples'])
del ref
for total, ref, _ in srt.render_spectral(scene, cam, W, H, [4, 4], depth):
    pass
comm.init_device_params(W, H, 8, depth, 1984)
comm.accum_reset_spectral()
for s in (4, 4):
    comm.render_frame_accum(W, H, s)
comm.synchronize()
assert_planes_equal(root.read_fb(), ref['fb'], 'spectral fb')
assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'spectral xyz')
assert np.array_equal(bits(comm.read_spectral(W, H)), bits(ref['film']))
assert np.array_equal(bits(comm.read_spectral(W, H, 94, 1)), bits(ref['film'][..., 94:95]))
comm.close()
print('full-size mock transport ok')
""" % (HW, HH, HDEPTH, headline["rel"]), "full-size mock transport ok", timeout=600)
