"""The exchange unit of a gathered accumulation (srt_pack_accum / srt_unpack_accum; csrc/srt_gather.hip, the layout stated in
csrc/srt_internal.h at GatherParams), restated in numpy from three things alone: tile_geometry (csrc/srt_capi.cpp), the slot -> pixel
map of the pixel queue and block_linear_idx (csrc/srt_kernel_common.h).  tests/test_gather_reference.py holds it to a brute-force
per-pixel statement of ownership; tests/test_gather.py holds the kernels to it."""
import numpy as np

TILE = 8
SLOTS = 64
FEATURE_STRIDE = 8
FILM_STRIDE = 96
SUMS, COUNTS, FEATURES, FILM = 1, 2, 4, 8


def tile_geometry(tx, ty, bx, by, world):
    """tiles cover the whole reference grid, whatever the chunk: (tiles_x, tiles_y, n_tiles, tiles_padded)"""
    tiles_x, tiles_y = (tx * bx + 7) // 8, (ty * by + 7) // 8
    n_tiles = tiles_x * tiles_y
    return tiles_x, tiles_y, n_tiles, (n_tiles + world - 1) // world


def tiles_local(n_tiles, rank, world):
    return (n_tiles - rank + world - 1) // world if n_tiles > rank else 0


def block_linear_idx(i, j, tx, ty, bx):
    gbx, gby = i // tx, j // ty
    return (j - gby * ty) * tx + (i - gbx * tx) + tx * ty * (gby * bx + gbx)


def slot_pixels(tile, tiles_x):
    """chunk pixel (i, j) of the 64 slots of global tile `tile`: slot lt is (lt & 7, lt >> 3) of the tile"""
    lt = np.arange(SLOTS)
    return (tile % tiles_x) * TILE + (lt & 7), (tile // tiles_x) * TILE + (lt >> 3)


def tile_floats(parts):
    """floats of one tile record: 64 * (3 + 2 a + 8 f + 96 s)"""
    return SLOTS * (3 + (2 if parts & COUNTS else 0) + (FEATURE_STRIDE if parts & FEATURES else 0) + (FILM_STRIDE if parts & FILM else 0))


def unit_floats(parts, tx, ty, bx, by, world):
    return tile_geometry(tx, ty, bx, by, world)[3] * tile_floats(parts)


def unit_lanes(rank, world, w, h, tx, ty, bx, by):
    """(tiles_padded, 64) int64: the block-linear lane behind slot lt of record t of rank's unit -- local tile t is global tile
    rank + world * t -- or -1 where the slot is no pixel of the w x h chunk (or the tile lies beyond the grid)"""
    tiles_x, _, n_tiles, padded = tile_geometry(tx, ty, bx, by, world)
    out = np.full((padded, SLOTS), -1, np.int64)
    for t in range(padded):
        tile = rank + world * t
        if tile >= n_tiles:
            continue
        i, j = slot_pixels(tile, tiles_x)
        ok = (i < w) & (j < h) & (i // tx < bx) & (j // ty < by)
        out[t, ok] = block_linear_idx(i[ok], j[ok], tx, ty, bx)
    return out


def pack_unit(lanes, planes, features=None, film=None):
    """The packed unit (uint32 words) of a rank whose unit_lanes are `lanes`.  planes: the lane-indexed plane words, uint32 arrays of
    n_lanes (X, Y, Z sums, then state and S2 when the counts travel); features: (n_lanes, 8) words or None; film: (n_lanes, 96) words or
    None.  Slots without a pixel are +0."""
    padded = lanes.shape[0]
    ok = lanes >= 0
    safe = np.where(ok, lanes, 0)
    blocks = []
    for p in planes:                                        # [word][slot]
        blocks.append(np.where(ok, np.asarray(p, np.uint32)[safe], 0).astype(np.uint32).reshape(padded, 1, SLOTS))
    rec = [np.concatenate(blocks, axis=1).reshape(padded, -1)]
    for rows in (features, film):                           # [slot][row]
        if rows is not None:
            rows = np.asarray(rows, np.uint32)
            rec.append(np.where(ok[:, :, None], rows[safe], 0).astype(np.uint32).reshape(padded, -1))
    return np.concatenate(rec, axis=1).reshape(-1)


def to_lanes(rowmajor, w, h, tx, ty, bx, by):
    """a row-major (h, w[, k]) read-back of the chunk at the image's origin as lane-indexed words (n_lanes[, k]), +0 elsewhere"""
    a = np.ascontiguousarray(rowmajor).view(np.uint32)
    a = a.reshape(h, w, -1)
    out = np.zeros((tx * ty * bx * by, a.shape[2]), np.uint32)
    j, i = np.divmod(np.arange(w * h), w)
    ok = (i // tx < bx) & (j // ty < by)
    out[block_linear_idx(i[ok], j[ok], tx, ty, bx)] = a.reshape(w * h, -1)[ok]
    return out


def same(a, b, what):
    """a and b -- arrays, numbers, None, or dicts / sequences of those -- are equal in every bit (timings aside)"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), what
        for k in a:
            if not str(k).endswith("ms"):
                same(a[k], b[k], "%s.%s" % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (what, k))
    elif isinstance(a, (np.ndarray, float, np.floating)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, what
        x, y = a.reshape(-1).view(np.uint8).reshape(a.size, -1), b.reshape(-1).view(np.uint8).reshape(a.size, -1)
        assert np.array_equal(x, y), "%s: %d of %d elements differ" % (what, int((x != y).any(axis=1).sum()), a.size)
    else:
        assert a == b, (what, a, b)
