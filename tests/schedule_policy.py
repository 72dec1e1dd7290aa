"""The tile scheduler's policy in plain numpy: what order_tiles_kernel must produce for a table of tile costs, written from the
kernel's comments and srt_kernel_common.h.  No GPU, no library.

A launch's pixel queue is a list of rows.  The local tiles go in descending order of a sort key (4096 bins, order inside a bin
free); a tile whose estimated latency exceeds the launch's makespan target T is split into 2^s rows of 64 >> s pixel slots, s its
level.  T is the smallest target at which the rows, at the smallest levels that fit them into T, still fit the machine; the kernel
finds it by 14 halvings in float32 with a sum whose order is not fixed, so a table pins the levels only when every halving decides
with a margin (`Target.margin`) and the result keeps clear of every threshold (`Target.threshold_distance`)."""
import collections

import numpy as np

BINS = 4096
KEY_MAX = 2 ** 32 - 1
# latency of a tile at split level s (64 >> s pixels per wave) relative to the unsplit tile; level s is taken while c * G[s - 1] > T
G = np.array([1.0, 0.934, 0.925, 0.797, 0.747, 0.656, 0.485], np.float32)
MAX_LEVEL = 6
HALVINGS = 14
TILE_MASK, PART_SHIFT, PART_MASK, LEVEL_SHIFT, LEVEL_MASK = (1 << 22) - 1, 22, 63, 28, 7
UNWRITTEN = 0xFFFFFFFF
# Relative error granted to the kernel's float32 target at any halving: both bounds come from a handful of float32 operations
# (2^-24 each) and every midpoint adds half an ulp, 14 times: below 2e-6 in all.
TARGET_EPS = 2e-6


def key_of(cost, cost_max_pixel, order_max_pct):
    """sort key of every tile: its cost moved order_max_pct % of the way towards 64 x its most expensive pixel (never downwards), in
    64-bit integers with a truncating division, clamped to 2^32 - 1"""
    c = np.asarray(cost, np.uint64)
    if order_max_pct == 0:
        return c.astype(np.uint32)
    mx64 = np.asarray(cost_max_pixel, np.uint64) * np.uint64(64)
    up = np.where(mx64 > c, mx64 - np.minimum(c, mx64), np.uint64(0))
    key = c + up * np.uint64(order_max_pct) // np.uint64(100)
    return np.minimum(key, np.uint64(KEY_MAX)).astype(np.uint32)


def bin_of(key, kmax):
    """bin of a key among 4096, bin 0 the most expensive: float32 scale = 4095 / kmax (kmax: the largest key, at least 1), the product
    truncated and clamped"""
    f = np.float32
    scale = f(BINS - 1) / f(np.uint32(max(int(kmax), 1)))
    b = np.minimum((np.asarray(key, np.uint32).astype(f) * scale).astype(np.int64), BINS - 1)
    return (BINS - 1) - b


def level_for(cost, target):
    """split level of every tile under target T: the smallest s with float32(c) * G[s] <= T, 6 when none is (float32 compare)"""
    lat = np.asarray(cost, np.uint32).astype(np.float32)[:, None] * G[None, :MAX_LEVEL]
    return np.cumprod(lat > np.float32(target), axis=1).sum(axis=1).astype(np.int64)


def _load(c64, g64, mid):
    """sum over the rows of their latency at target mid, float64: a tile at level s is 2^s rows of latency c * G[s]"""
    s = np.cumprod(c64[:, None] * g64[None, :MAX_LEVEL] > mid, axis=1).sum(axis=1).astype(np.int64)
    return float(np.sum(np.exp2(s) * c64 * g64[s]))


Target = collections.namedtuple("Target", "target margin threshold_distance feasible")


def makespan_target(cost, n_waves, split_load_pct):
    """The bisection in float64.  Bounds [c_max * G[6], max(c_max, load_factor * sum(c) / max(n_waves, 1))], c_max at least 1; 14
    halvings, a midpoint being feasible when load_factor * load(mid) <= n_waves * mid; the result is the upper bound.

    margin: the smallest |load_factor * load - n_waves * mid| / (n_waves * mid) over the halvings, where load is taken at mid and at
    mid * (1 -+ TARGET_EPS) -- load never grows with the target, so these bracket the load at any target the kernel can hold there --
    and 0 when the three do not decide alike.  (n_waves = 0: nothing is feasible while a tile has a cost; the margin is infinite.)
    threshold_distance: the smallest |T - c * G[s]| / T over all tiles and the seven ratios."""
    c64 = np.asarray(cost, np.uint32).astype(np.float64)
    g64 = G.astype(np.float64)
    lf = float(np.float32(split_load_pct) * np.float32(0.01))
    c_max = max(float(c64.max()), 1.0)
    lo, hi = c_max * g64[6], max(c_max, lf * float(c64.sum()) / max(int(n_waves), 1))
    margin, decided = np.inf, []
    for _ in range(HALVINGS):
        mid = 0.5 * (lo + hi)
        cap = float(n_waves) * mid
        slack = [cap - lf * _load(c64, g64, m) for m in (mid * (1 - TARGET_EPS), mid, mid * (1 + TARGET_EPS))]
        feasible = slack[1] >= 0.0
        if any((s >= 0.0) != feasible for s in slack):
            margin = 0.0
        elif cap > 0.0:
            margin = min(margin, min(abs(s) for s in slack) / cap)
        decided.append(feasible)
        if feasible:
            hi = mid
        else:
            lo = mid
    dist = float(np.min(np.abs(hi - c64[:, None] * g64[None, :]))) / hi
    return Target(hi, margin, dist, decided)


Schedule = collections.namedtuple("Schedule", "key bins levels target n_rows cost_max")


def schedule(cost2, n_waves, split_load_pct, order_max_pct):
    """the policy on cost2 = [n tile costs | n most-expensive-pixel costs]: keys and bins for the order, levels from the COST, the
    number of rows, the largest cost (at least 1).  Tables of more than 2^20 tiles are never split."""
    cost2 = np.asarray(cost2, np.uint32)
    n = cost2.size // 2
    cost, cmp_ = cost2[:n], cost2[n:]
    key = key_of(cost, cmp_, order_max_pct)
    bins = bin_of(key, key.max())
    if split_load_pct != 0 and n <= (1 << 20):
        tgt = makespan_target(cost, n_waves, split_load_pct)
        levels = level_for(cost, tgt.target)
    else:
        tgt, levels = None, np.zeros(n, np.int64)
    return Schedule(key, bins, levels, tgt, int(np.sum(1 << levels)), max(int(cost.max()), 1))


def row_pack(tile_local, part, s):
    return np.uint32(tile_local | (part << PART_SHIFT) | (s << LEVEL_SHIFT))


def row_unpack(rows):
    """(local tile, part, level) of every row"""
    r = np.asarray(rows, np.uint32).astype(np.int64)
    return r & TILE_MASK, (r >> PART_SHIFT) & PART_MASK, (r >> LEVEL_SHIFT) & LEVEL_MASK


def rows_of(order, levels):
    """the queue for the tiles in `order`: tile t gives 2^s rows, part = 0 .. 2^s - 1, s = levels[t]"""
    out = []
    for t in np.asarray(order, np.int64):
        s = int(levels[t])
        out.extend(int(t) | (part << PART_SHIFT) | (s << LEVEL_SHIFT) for part in range(1 << s))
    return np.array(out, np.uint32)


def single_target_explains(cost, levels):
    """is there ONE target T under which every tile of `cost` has its level of `levels` (float32 products, as level_for)?  A tile at
    level s needs c * G[s - 1] > T (s > 0) and c * G[s] <= T (s < 6)."""
    c = np.asarray(cost, np.uint32).astype(np.float32)
    s = np.asarray(levels, np.int64)
    at_least = np.where(s < MAX_LEVEL, c * G[np.minimum(s, MAX_LEVEL - 1)], np.float32(0))
    below = np.where(s > 0, c * G[np.maximum(s, 1) - 1], np.float32(np.inf))
    return bool(at_least.max() < below.min())


class TileGrid:
    """The slot -> pixel map of a chunk (srt_kernel_common.h): slot lt of local tile t is pixel (lt & 7, lt >> 3) of global tile
    rank + world * t; the 8 x 8 tiles run row-major over ceil(tx * bx / 8) columns and ceil(ty * by / 8) rows; a pixel belongs to the
    chunk when it lies inside width x height (the grid tx * bx x ty * by covers that)."""

    def __init__(self, geom, width, height, rank=0, world=1):
        self.width, self.height, self.rank, self.world = width, height, rank, world
        self.tiles_x = (geom["tx"] * geom["bx"] + 7) // 8
        self.tiles_y = (geom["ty"] * geom["by"] + 7) // 8
        self.n_tiles = self.tiles_x * self.tiles_y
        self.tiles_local = (self.n_tiles - rank + world - 1) // world if self.n_tiles > rank else 0
        self.limit_w, self.limit_h = min(width, geom["tx"] * geom["bx"]), min(height, geom["ty"] * geom["by"])

    def slot_pixels(self, tile_local):
        """row-major pixel index (j * width + i) of the 64 slots of a local tile, -1 for a slot outside the chunk"""
        tile = self.rank + self.world * int(tile_local)
        lt = np.arange(64)
        i, j = (tile % self.tiles_x) * 8 + (lt & 7), (tile // self.tiles_x) * 8 + (lt >> 3)
        inside = (tile < self.n_tiles) & (i < self.limit_w) & (j < self.limit_h)
        return np.where(inside, j * self.width + i, -1)

    def row_pixels(self, row):
        """the chunk's pixels in the share of a queue row: slots [part * (64 >> s), (part + 1) * (64 >> s)) of its tile"""
        t, part, s = (int(v[0]) for v in row_unpack([row]))
        px = self.slot_pixels(t)[part * (64 >> s):(part + 1) * (64 >> s)]
        return px[px >= 0]

    def pixels_per_tile(self):
        return np.array([(self.slot_pixels(t) >= 0).sum() for t in range(self.tiles_local)], np.int64)
