"""The pixel queue against tests/schedule_policy.py, the numpy restatement of the tile scheduler's policy.

The queue is scheduling only -- images are invariant under it by design (test_queue_scheduling_does_not_change_results) -- so
nothing else holds order_tiles_kernel and the order of adapt_scan_kernel's output to anything.  Here: synthetic cost tables
through srt_order_tiles_kat, the queues of real launches through srt_read_tile_schedule, and the compacted queues of an
adaptive accumulation.  Tile counts above 2^20 (where the kernel must not split) are left out: a kernel that wrongly split
them would write out of bounds, and this suite does not provoke faults."""
import ctypes

import numpy as np
import pytest

import schedule_policy as SP
from accum_helpers import NEVER, adaptive_run, fresh_context, named_workload, predict_stops

ERR_INVALID = -1
# The kernel sums at most 4097 positive float32 terms with atomics in any order: relative error at most n * 2^-24 = 2.4e-4.  A halving
# decides like the restatement when its margin is four times that; the final target keeps 1e-5 (about 100 float32 ulps, five times
# schedule_policy.TARGET_EPS) clear of every threshold.
MIN_MARGIN, MIN_THRESHOLD_DISTANCE = 1e-3, 1e-5


def _lognormal(n, seed):
    """n tile costs exp(N(6, 1.2)) * 64 with a most expensive pixel of 1/64 .. 1/4 of the tile (the spread of a real probe)"""
    rng = np.random.default_rng(seed)
    cost = np.maximum(np.exp(rng.normal(6.0, 1.2, n)) * 64.0, 1.0).astype(np.uint32)
    mx = np.maximum(cost * rng.uniform(1 / 64, 1 / 4, n), 1.0).astype(np.uint32)
    return np.concatenate([cost, mx])


def _wide_keys(n, seed):
    """costs log-uniform over 1e6 .. 3e9 and a most expensive pixel of 1/64 .. 1 of the tile: 64 x that pixel reorders neighbours in
    cost and passes 2^32 for the top of the table"""
    rng = np.random.default_rng(seed)
    cost = np.exp(rng.uniform(np.log(1e6), np.log(3e9), n)).astype(np.uint32)
    mx = np.maximum(cost * np.exp(rng.uniform(np.log(1 / 64), 0.0, n)), 1.0).astype(np.uint32)
    return np.concatenate([cost, mx])


def _const(n, c):
    return np.full(2 * n, c, np.uint32)


def _outlier(n, seed):
    t = _lognormal(n, seed)
    t[:n] = np.clip(t[:n] % 64 + 70, 1, None)      # tiles of ~100 ...
    t[n:] = 2
    t[n // 3] = 2 ** 31                            # ... and one of 2^31
    t[n + n // 3] = 2 ** 25
    return t


# name -> (cost[2n], n_waves, split_load_pct, order_max_pct, pinned).  pinned: the bisection decides every halving with MIN_MARGIN, so the
# levels are the restatement's; the one table that is not pinned must come out unsplit for any target the kernel can reach (see
# test_tables_pin_their_levels).  Seeds: the first of 0, 1, 2, .. whose table is pinned (n = 4097 misses it at seed 0, the keyed table at seeds 0 .. 4).
TABLES = {}
for _n, _seed in ((2, 0), (4, 0), (63, 0), (1023, 0), (1024, 0), (1025, 0), (3000, 0), (4097, 1)):
    TABLES["tiles_%d" % _n] = (_lognormal(_n, _seed), 1024, 200, 0, True)      # chain-bound: levels up to 6
TABLES["throughput_bound_4097"] = (_lognormal(4097, 1), 64, 200, 0, False)     # nothing split; the upper bound sits on the constraint
TABLES["no_waves_63"] = (_lognormal(63, 0), 0, 200, 0, True)                   # the guard against n_waves = 0
TABLES["split_off_1025"] = (_lognormal(1025, 0), 1024, 0, 0, True)
TABLES["full_buffer_4"] = (_const(4, 3000000000), 1024, 200, 0, True)          # every tile at level 6: 64 n rows exactly
TABLES["all_equal_1000"] = (_const(1000, 5000), 4096, 200, 0, True)            # one bin
TABLES["all_ones_1000"] = (_const(1000, 1), 4096, 200, 0, True)                # empty tiles
TABLES["one_outlier_500"] = (_outlier(500, 0), 1024, 200, 0, True)
for _pct in (0, 100, 400):
    TABLES["order_max_pct_%d" % _pct] = (_wide_keys(1000, 5), 1024, 200, _pct, True)


def _policy(name):
    cost2, n_waves, split, order, _ = TABLES[name]
    return SP.schedule(cost2, n_waves, split, order)


# ---- CPU: the tables and the restatement itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TABLES))
def test_tables_pin_their_levels(name):
    """Every synthetic table decides each of the 14 halvings with a margin of MIN_MARGIN and ends MIN_THRESHOLD_DISTANCE away from every
    threshold, so a correct kernel must arrive at the restatement's levels.  The throughput-bound table cannot: with nothing split
    its upper bound IS the capacity constraint and every midpoint misses it by its distance from that bound (5e-5 at the last one);
    there the upper bound is at least twice the largest cost instead, so every target the kernel can hold gives level 0."""
    cost2, n_waves, split, order, pinned = TABLES[name]
    n = cost2.size // 2
    pol = SP.schedule(cost2, n_waves, split, order)
    print(name, "margin", pol.target and pol.target.margin, "distance", pol.target and pol.target.threshold_distance, "rows", pol.n_rows,
          "levels", np.bincount(pol.levels, minlength=7))
    assert (cost2[n:] <= cost2[:n]).all()
    if pol.target is not None:
        assert len(pol.target.feasible) == SP.HALVINGS
        if pinned:
            assert pol.target.margin >= MIN_MARGIN
            assert pol.target.threshold_distance >= MIN_THRESHOLD_DISTANCE
        else:
            assert pol.target.target >= 2.0 * cost2[:n].max() and not any(pol.target.feasible)
    # invariants of the restatement: levels never fall as the cost grows, and the queue fits the largest row buffer
    by_cost = np.argsort(cost2[:n], kind="stable")
    assert (np.diff(pol.levels[by_cost]) >= 0).all()
    assert pol.n_rows == np.sum(2 ** pol.levels) <= 64 * n
    assert 0 <= pol.bins.min() <= 1 and pol.bins.max() <= SP.BINS - 1      # the largest key: bin 0, or 1 when the float32 product rounds below 4095
    assert (np.diff(pol.bins[np.argsort(-pol.key.astype(np.int64), kind="stable")]) >= 0).all()


def test_tables_reach_the_cases_they_stand_for():
    assert _policy("tiles_4097").levels.max() == 6 and _policy("tiles_4097").levels.min() == 0      # more tiles than bins, every kind of row
    assert all(_policy("tiles_%d" % n).levels.max() > 0 for n in (2, 4, 63, 1023, 1024, 1025, 3000))
    for name in ("throughput_bound_4097", "no_waves_63", "split_off_1025"):
        assert not _policy(name).levels.any(), name
    full = _policy("full_buffer_4")
    assert (full.levels == 6).all() and full.n_rows == 64 * 4
    assert len(np.unique(_policy("all_equal_1000").bins)) == 1
    assert _policy("all_ones_1000").cost_max == 1
    out = _policy("one_outlier_500")
    assert out.cost_max == 2 ** 31 and out.levels.max() == 6 and (out.levels > 0).sum() == 1
    # the keyed tables: the key reorders at least a quarter of the pairs that are adjacent in cost order into other bins, one key
    # clamps, and the levels are those of the unkeyed table (they follow the cost)
    cost2 = TABLES["order_max_pct_0"][0]
    n = cost2.size // 2
    by_cost = np.argsort(-cost2[:n].astype(np.int64), kind="stable")
    plain = _policy("order_max_pct_0")
    assert np.array_equal(plain.key, cost2[:n]) and (np.diff(plain.bins[by_cost]) >= 0).all()
    for pct in (100, 400):
        pol = _policy("order_max_pct_%d" % pct)
        reordered = np.diff(pol.bins[by_cost]) < 0
        print("order_max_pct", pct, "reordered pairs", reordered.mean(), "clamped keys", (pol.key == SP.KEY_MAX).sum())
        assert reordered.mean() >= 0.25
        assert (pol.key == SP.KEY_MAX).any() and (pol.key < SP.KEY_MAX).sum() > n // 2
        assert np.array_equal(pol.levels, plain.levels) and pol.levels.max() > 0


def test_key_of_small_cases():
    c, mx = np.array([100, 100, 100, 4000000000, 7], np.uint32), np.array([1, 2, 100, 70000000, 7], np.uint32)
    assert list(SP.key_of(c, mx, 0)) == [100, 100, 100, 4000000000, 7]
    assert list(SP.key_of(c, mx, 100)) == [100, 128, 6400, SP.KEY_MAX, 448]      # never below the cost; 64 x 7e7 passes 2^32
    assert list(SP.key_of(c, mx, 50)) == [100, 114, 3250, 4240000000, 227]       # halfway, truncated: 7 + 441 * 50 / 100 = 227
    assert list(SP.key_of(c, mx, 400)) == [100, 212, 25300, SP.KEY_MAX, 1771]


def test_rows_pack_and_unpack():
    rows = SP.rows_of([5, 0, 3], {5: 1, 0: 0, 3: 2})
    assert list(rows) == [5 | 1 << 28, 5 | 1 << 22 | 1 << 28, 0, 3 | 2 << 28, 3 | 1 << 22 | 2 << 28, 3 | 2 << 22 | 2 << 28, 3 | 3 << 22 | 2 << 28]
    t, part, s = SP.row_unpack(rows)
    assert list(t) == [5, 5, 0, 3, 3, 3, 3] and list(part) == [0, 1, 0, 0, 1, 2, 3] and list(s) == [1, 1, 0, 2, 2, 2, 2]
    assert SP.row_pack((1 << 22) - 1, 63, 6) == np.uint32(0x6fffffff)
    assert SP.single_target_explains([100, 50, 10], [1, 0, 0]) and not SP.single_target_explains([100, 50, 10], [0, 1, 0])


def test_tile_grid_covers_every_pixel_once():
    geom = dict(tx=28, ty=16, bx=2, by=2)
    for rank, world in ((0, 1), (1, 3)):
        seen = np.zeros(29 * 17, np.int64)
        for r in range(world):
            g = SP.TileGrid(geom, 29, 17, r, world)
            assert g.tiles_x == 7 and g.n_tiles == 28
            for t in range(g.tiles_local):
                px = g.slot_pixels(t)
                np.add.at(seen, px[px >= 0], 1)
        assert (seen == 1).all()
    g = SP.TileGrid(geom, 29, 17)
    # tile 3 holds columns 24 .. 28 of the chunk; the halves of a level-1 split are its rows 0 .. 3 and 4 .. 7
    assert list(g.row_pixels(SP.row_pack(3, 0, 1))) == [j * 29 + i for j in range(4) for i in range(24, 29)]
    assert list(g.row_pixels(SP.row_pack(3, 1, 1))) == [j * 29 + i for j in range(4, 8) for i in range(24, 29)]
    assert list(g.row_pixels(SP.row_pack(17, 7, 3))) == [23 * 29 + i for i in range(24, 29)][:0]      # rows 16 .. 23 of the grid: only row 16 is in the chunk
    assert list(g.row_pixels(SP.row_pack(17, 0, 3))) == [16 * 29 + i for i in range(24, 29)]
    assert g.pixels_per_tile().sum() == 29 * 17 and g.pixels_per_tile()[6] == 0


# ---- GPU: synthetic costs through srt_order_tiles_kat ------------------------------------------------------------------------------
def _assert_queue_obeys(rows, order, n_rows, cost_max, cost2, pol, what, levels=None):
    """the assertions every queue meets: `order` a permutation in non-decreasing bin order, n_rows and cost_max the policy's, the rows
    those of the tiles in `order` at `levels` (default: the policy's), part = 0 .. 2^s - 1 in order"""
    n = cost2.size // 2
    assert np.array_equal(np.sort(order), np.arange(n)), what + ": the sorted tiles are no permutation"
    assert (np.diff(pol.bins[order]) >= 0).all(), what + ": the tiles are not in descending key order"
    assert cost_max == pol.cost_max, what + ": cost_max %d, the largest tile cost is %d" % (cost_max, pol.cost_max)
    levels = pol.levels if levels is None else levels
    assert n_rows == int(np.sum(2 ** levels)), what + ": %d rows, the policy has %d" % (n_rows, int(np.sum(2 ** levels)))
    want = SP.rows_of(order, levels)
    if not np.array_equal(rows[:n_rows], want):
        k = int(np.nonzero(rows[:n_rows] != want)[0][0])
        raise AssertionError("%s: row %d is (tile, part, level) = %r, the policy has %r" % (
            what, k, tuple(int(v[0]) for v in SP.row_unpack(rows[k:k + 1])), tuple(int(v[0]) for v in SP.row_unpack(want[k:k + 1]))))


def _levels_of_rows(rows, n):
    """the level every tile has in a queue (-1: the tile has no row)"""
    t, _, s = SP.row_unpack(rows)
    out = np.full(n, -1, np.int64)
    out[t[t < n]] = s[t < n]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLES))
def test_synthetic_costs(gpu, name):
    cost2, n_waves, split, order_pct, _ = TABLES[name]
    n = cost2.size // 2
    pol = _policy(name)
    rows, order, info = gpu.order_tiles_kat(cost2, n_waves, split, order_pct)
    assert rows.size == 64 * n + 64
    got = _levels_of_rows(rows[:min(int(info[0]), 64 * n)], n)
    assert np.array_equal(got, pol.levels), "%s: levels %r, the policy has %r" % (name, np.bincount(got[got >= 0], minlength=7), np.bincount(pol.levels, minlength=7))
    _assert_queue_obeys(rows, order, int(info[0]), int(info[1]), cost2, pol, name)
    assert int(info[1]) == max(int(cost2[:n].max()), 1)
    assert (rows[int(info[0]):] == SP.UNWRITTEN).all(), name + ": words behind the queue were written"
    if split == 0:
        assert np.array_equal(rows[:n], order)      # a queue that is not split is the sorted tiles themselves


@pytest.mark.gpu
def test_kat_refusals(srt, gpu):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    cost, rows, order, info = np.ones(8, np.uint32), np.zeros(64 * 4 + 64, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    call = lambda n, cap: srt.binding.lib().srt_order_tiles_kat(gpu._h, cost.ctypes.data_as(u32p), n, 1024, 200, 0, rows.ctypes.data_as(u32p), cap,
                                                               order.ctypes.data_as(u32p), info.ctypes.data_as(u32p))
    assert call(0, rows.size) == ERR_INVALID
    assert call((1 << 20) + 1, 1 << 40) == ERR_INVALID      # (refused before anything is read or allocated)
    assert call(4, 64 * 4 + 63) == ERR_INVALID
    assert not rows.any() and not order.any() and not info.any()
    assert call(4, 64 * 4 + 64) == 0 and info[0] >= 4


# ---- GPU: the queues of real launches through srt_read_tile_schedule ---------------------------------------------------------------
PROBE_SPP = 2      # the library's default (SRT_PROBE_SPP)
WORKLOADS = {
    "spheres_29x17": (100, 1, 29, 17, 12, 16),
    "spheres_120x72": (100, 1, 120, 72, 12, 16),
    "prism_sah_57x31": (1, 1, 57, 31, 9, 16),
}
_scenes = {}


def _setup(srt, r, name, spp=None, rank=0, world=1, counted=False):
    sid, mode, W, H, spp0, depth = WORKLOADS[name]
    if name not in _scenes:
        sc = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
        _scenes[name] = (sc, sc.default_camera(W, H))
    scene, cam = _scenes[name]
    r.upload_scene(scene); r.set_camera(cam)
    r.init_device_params(W, H, spp0 if spp is None else spp, depth, 1984)
    r.set_partition(rank, world)
    r.set_count_traversal(counted)
    return W, H


def _launch(srt, r, name, rank=0, world=1):
    """a plain frame of the workload; returns (rows, info, cost[2n], grid)"""
    W, H = _setup(srt, r, name, rank=rank, world=world)
    r.render_chunk(W, H)
    rows, info = r.tile_schedule(0)
    cost = np.concatenate(r.tile_costs(with_max_pixel=True))
    return rows, info, cost, SP.TileGrid(r.geom, W, H, rank, world)


def _assert_cover(rows, grid, what):
    """the shares of the rows hold every pixel of the rank's part of the chunk exactly once, and name local tiles only"""
    t, _, _ = SP.row_unpack(rows)
    assert (t < grid.tiles_local).all(), what + ": a row names a tile the rank does not own"
    seen = np.zeros(grid.width * grid.height, np.int64)
    for row in rows:
        np.add.at(seen, grid.row_pixels(row), 1)
    own = np.zeros_like(seen)
    for k in range(grid.tiles_local):
        px = grid.slot_pixels(k)
        own[px[px >= 0]] = 1
    assert np.array_equal(seen, own), what + ": the rows do not cover the rank's pixels once each"


def _assert_real_queue(rows, info, cost, grid, what):
    """cover, order and rows as for a synthetic table, from the probe's costs and the recorded arguments.  Returns whether the table
    pins the levels (MIN_MARGIN); one that does not is held to: a single target explains every level."""
    n = grid.tiles_local
    assert info["tiles_local"] == n and info["n_rows"] == rows.size and cost.size == 2 * n
    pol = SP.schedule(cost, info["n_waves_plan"], info["split_load_pct"], info["order_max_pct"])
    _assert_cover(rows, grid, what)
    got = _levels_of_rows(rows, n)
    order = SP.row_unpack(rows)[0][SP.row_unpack(rows)[1] == 0]      # the tiles in queue order: one row with part 0 each
    pinned = pol.target is None or (pol.target.margin >= MIN_MARGIN and pol.target.threshold_distance >= MIN_THRESHOLD_DISTANCE)
    print(what, "tiles", n, "rows", rows.size, "waves", info["n_waves_plan"], "margin", pol.target and pol.target.margin,
          "distance", pol.target and pol.target.threshold_distance, "levels", np.bincount(got[got >= 0], minlength=7))
    if pinned:
        assert np.array_equal(got, pol.levels), what + ": levels %r, the policy has %r" % (got, pol.levels)
    else:
        assert (got >= 0).all() and SP.single_target_explains(cost[:n], got), what + ": no single target explains the levels"
    _assert_queue_obeys(rows, order, info["n_rows"], info["cost_max"], cost, pol, what, levels=got)
    return pinned


@pytest.mark.gpu
def test_real_launches_obey_the_policy(srt, gpu):
    """The default policy on the three workloads.  At most one of them may miss MIN_MARGIN (and is then held to the weaker level
    property); the smallest frame must really split a tile."""
    weak = []
    for name in WORKLOADS:
        rows, info, cost, grid = _launch(srt, gpu, name)
        assert info["streams"] == 1 and info["split_load_pct"] == 200 and info["n_waves_plan"] >= 256
        if not _assert_real_queue(rows, info, cost, grid, name):
            weak.append(name)
        if name == "spheres_29x17":
            assert SP.row_unpack(rows)[2].max() > 0, "the default policy split no tile of the 29 x 17 frame"
    assert len(weak) <= 1, weak


@pytest.mark.gpu
@pytest.mark.parametrize("name,rank,world", [("spheres_29x17", 0, 1), ("prism_sah_57x31", 0, 1), ("spheres_120x72", 1, 3)])
def test_probe_costs_are_the_node_visits_of_a_probe_frame(srt, gpu, name, rank, world):
    """sum(cost[:n]) = the instrumented node_visits counter of a plain PROBE_SPP-sample frame from the same seed + one per in-chunk
    pixel (the +1 that sorts empty pixels behind real ones).  Probe and instrumented kernel count the same traversal steps -- a
    NaN-direction query is answered without a walk in both -- so no util[2] term is needed between them."""
    _, _, cost, grid = _launch(srt, gpu, name, rank, world)
    n = grid.tiles_local
    W, H = _setup(srt, gpu, name, spp=PROBE_SPP, rank=rank, world=world, counted=True)
    gpu.render_chunk(W, H)
    visits = gpu.stats()["node_visits"]
    gpu.set_count_traversal(False); gpu.set_partition(0, 1)
    with pytest.raises(srt.SrtError) as e:      # spp <= 4 x probe_spp: that frame ran the identity queue
        gpu.tile_schedule(0)
    assert e.value.code == ERR_INVALID
    pixels = grid.pixels_per_tile()
    print(name, "sum", int(cost[:n].sum(dtype=np.int64)), "node visits", visits, "pixels", int(pixels.sum()))
    assert int(cost[:n].sum(dtype=np.int64)) == visits + int(pixels.sum())
    assert (cost[n:] <= cost[:n]).all()
    assert (cost[:n] >= pixels).all()
    assert (pixels == 0).any() and not cost[:n][pixels == 0].any() and not cost[n:][pixels == 0].any()      # tiles wholly outside the chunk


@pytest.mark.gpu
def test_partition_names_local_tiles(srt, gpu):
    rows, info, cost, grid = _launch(srt, gpu, "spheres_120x72", rank=1, world=3)
    gpu.set_partition(0, 1)
    assert grid.tiles_local == info["tiles_local"] == (grid.n_tiles - 1 + 2) // 3
    _assert_real_queue(rows, info, cost, grid, "rank 1 of 3")


@pytest.mark.gpu
def test_knobs(srt, monkeypatch):
    """each on a fresh context: the knobs are read when it is created"""
    for k in ("SRT_SPLIT_LOAD", "SRT_PROBE_SPP", "SRT_ORDER_MAX_PCT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SRT_SPLIT_LOAD", "0")
    r = srt.Renderer(0)
    rows, info, cost, grid = _launch(srt, r, "spheres_29x17")
    assert info["split_load_pct"] == 0 and rows.size == grid.tiles_local and not SP.row_unpack(rows)[2].any()
    _assert_real_queue(rows, info, cost, grid, "SRT_SPLIT_LOAD=0")
    r.close()
    monkeypatch.delenv("SRT_SPLIT_LOAD")
    monkeypatch.setenv("SRT_ORDER_MAX_PCT", "100")
    r = srt.Renderer(0)
    rows, info, cost, grid = _launch(srt, r, "spheres_29x17")
    assert info["order_max_pct"] == 100
    _assert_real_queue(rows, info, cost, grid, "SRT_ORDER_MAX_PCT=100")
    r.close()
    monkeypatch.delenv("SRT_ORDER_MAX_PCT")
    monkeypatch.setenv("SRT_PROBE_SPP", "0")
    r = srt.Renderer(0)
    W, H = _setup(srt, r, "spheres_29x17")
    r.render_chunk(W, H)
    with pytest.raises(srt.SrtError) as e:
        r.tile_schedule(0)
    assert e.value.code == ERR_INVALID
    r.close()
    monkeypatch.delenv("SRT_PROBE_SPP")
    r = srt.Renderer(0)
    W, H = _setup(srt, r, "spheres_29x17", spp=4 * PROBE_SPP)      # too few samples for a probe to pay
    with pytest.raises(srt.SrtError) as e:
        r.tile_schedule(0)                                          # (and nothing rendered yet)
    assert e.value.code == ERR_INVALID
    r.render_chunk(W, H)
    for which in (0, 1):
        with pytest.raises(srt.SrtError) as e:
            r.tile_schedule(which)
        assert e.value.code == ERR_INVALID
    r.close()


@pytest.mark.gpu
def test_streamed_pass_plans_for_a_quarter_of_the_waves(srt, gpu):
    rows, plain, _, _ = _launch(srt, gpu, "spheres_29x17")
    W, H = _setup(srt, gpu, "spheres_29x17")
    gpu.accum_reset_streams(4)
    gpu.render_chunk_accum(W, H, 12)
    rows, info = gpu.tile_schedule(0)
    cost = np.concatenate(gpu.tile_costs(with_max_pixel=True))
    assert info["streams"] == 4 and info["n_waves_plan"] == max(plain["n_waves_plan"] // 4, 1)
    _assert_real_queue(rows, info, cost, SP.TileGrid(gpu.geom, W, H), "4 streams")
    with pytest.raises(srt.SrtError):
        gpu.tile_schedule(1)


# ---- GPU: the compacted queue of adaptive passes -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_compacted_queue_keeps_the_probes_order(srt, gpu):
    """Three adaptive passes of 16 samples.  After pass p the compacted queue is the probe's rows whose share holds a pixel that
    pass p + 1 then renders (its sample count grows), in the probe's order, once each; the second compaction removes rows again."""
    scene, cam, W, H, depth, _ = named_workload(srt, "dielectric")
    # the tolerance: the middle one of a grid under which, by the criterion's restatement on a run that never stops, fewer pixels are
    # active after every pass and some still are after the second
    never = adaptive_run(gpu, scene, cam, W, H, depth, NEVER, sched=[16, 16], min_spp=16)
    shrinking = [float(rel) for rel in np.geomspace(1e-3, 10.0, 81) if W * H > predict_stops(never, float(rel), min_spp=16)[2][0] > predict_stops(never, float(rel), min_spp=16)[2][1] > 0]
    assert shrinking, "no tolerance lets the active pixels shrink over two passes"
    rel_tol = shrinking[len(shrinking) // 2]
    fresh_context(gpu, scene, cam, W, H, depth, spp=48)
    gpu.accum_reset_adaptive(rel_tol, 0.0, 16)
    grid = SP.TileGrid(gpu.geom, W, H)
    gpu.render_chunk_accum(W, H, 16)
    grown, kept = [], []
    for p in (1, 2):
        probe, pinfo = gpu.tile_schedule(0)
        compact, cinfo = gpu.tile_schedule(1)
        before = gpu.accum_stats(W, H)["samples"].astype(np.int64)
        gpu.render_chunk_accum(W, H, 16)
        active = np.nonzero(gpu.accum_stats(W, H)["samples"].astype(np.int64) > before)[0]
        grown.append(active.size); kept.append(compact.size)
        assert cinfo["n_rows"] == compact.size and pinfo["n_rows"] == probe.size and cinfo["cost_max"] == pinfo["cost_max"]
        assert len(np.unique(probe)) == probe.size and len(np.unique(compact)) == compact.size
        keep = np.array([np.isin(grid.row_pixels(row), active).any() for row in probe])
        print("pass", p, "probe rows", probe.size, "compacted", compact.size, "pixels that rendered next", active.size)
        assert np.array_equal(compact, probe[keep]), "after pass %d: the compacted queue is not the probe's rows with an active pixel, in its order" % p
        assert 0 < compact.size < probe.size
        assert SP.row_unpack(probe)[2].max() > 0      # (the probe's queue of this frame has split rows: shares smaller than a tile)
    assert 0 < grown[1] < grown[0] and kept[1] < kept[0], (grown, kept)      # the second compaction really removes rows
