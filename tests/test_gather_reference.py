"""tests/gather_reference.py against a brute-force per-pixel statement of ownership: pixel (i, j) of the chunk lies in 8 x 8 tile
(j // 8) * tiles_x + i // 8, which belongs to rank tile % world and is that rank's local tile tile // world; its slot is
(j % 8) * 8 + i % 8.  No GPU."""
import numpy as np
import pytest

import gather_reference as G

# (w, h, tx, ty, world): the shapes of tests/test_gather.py
SHAPES = [(45, 27, 28, 16, 3), (45, 27, 10, 6, 3), (8, 8, 8, 8, 5), (64, 48, 28, 16, 2), (45, 27, 28, 16, 1), (56, 40, 28, 16, 4)]


def _grid(w, h, tx, ty):
    return w // tx + 1, h // ty + 1      # reference_grid


@pytest.mark.parametrize("w,h,tx,ty,world", SHAPES)
def test_every_chunk_pixel_lies_in_exactly_one_unit_once(w, h, tx, ty, world):
    bx, by = _grid(w, h, tx, ty)
    tiles_x, tiles_y, n_tiles, padded = G.tile_geometry(tx, ty, bx, by, world)
    assert tiles_x * 8 >= tx * bx and tiles_y * 8 >= ty * by and padded * world >= n_tiles
    n_lanes = tx * ty * bx * by
    seen = np.zeros(n_lanes, np.int64)
    owner = np.full(n_lanes, -1, np.int64)
    where = {}
    for rank in range(world):
        lanes = G.unit_lanes(rank, world, w, h, tx, ty, bx, by)
        assert lanes.shape == (padded, 64)
        assert (lanes[G.tiles_local(n_tiles, rank, world):] == -1).all(), "records past the rank's last tile hold no pixel"
        t, lt = np.nonzero(lanes >= 0)
        np.add.at(seen, lanes[t, lt], 1)
        owner[lanes[t, lt]] = rank
        for a, b in zip(t, lt):
            where[int(lanes[a, b])] = (int(a), int(b))
    # brute force, pixel by pixel
    n_pix = 0
    for j in range(h):
        for i in range(w):
            if i // tx >= bx or j // ty >= by:
                continue
            n_pix += 1
            gbx, gby = i // tx, j // ty
            lane = (j % ty) * tx + (i % tx) + tx * ty * (gby * bx + gbx)
            tile = (j // 8) * tiles_x + i // 8
            assert seen[lane] == 1 and owner[lane] == tile % world, (i, j)
            assert where[lane] == (tile // world, (j % 8) * 8 + i % 8), (i, j)
    assert seen.sum() == n_pix == min(w, tx * bx) * min(h, ty * by), "a unit holds a lane that is no pixel of the chunk"
    assert sum(G.tiles_local(n_tiles, r, world) for r in range(world)) == n_tiles


def test_the_listed_shapes_have_the_edge_cases_they_were_chosen_for():
    bx, by = _grid(45, 27, 28, 16)
    tiles_x, tiles_y, n_tiles, padded = G.tile_geometry(28, 16, bx, by, 3)
    assert (tiles_x, tiles_y, n_tiles, padded) == (7, 4, 28, 10)
    assert [G.tiles_local(n_tiles, r, 3) for r in range(3)] == [10, 9, 9]
    counts = {}
    for rank in range(3):
        lanes = G.unit_lanes(rank, 3, 45, 27, 28, 16, bx, by)
        for t in range(G.tiles_local(n_tiles, rank, 3)):
            counts[rank + 3 * t] = int((lanes[t] >= 0).sum())
    assert counts[0] == 64 and counts[5] == 8 * 5 and counts[6] == 0 and counts[21] == 8 * 3      # whole | cut at x = 45 | outside | cut at y = 27
    i, _ = G.slot_pixels(3, tiles_x)
    assert i.min() < 28 <= i.max(), "tile column 3 straddles the block boundary x = 28"
    # an 8 x 8 chunk in 8 x 8 blocks: a 2 x 2 grid, four tiles, so rank 4 of 5 owns none
    tiles = G.tile_geometry(8, 8, 2, 2, 5)
    assert tiles[2] == 4 and tiles[3] == 1 and G.tiles_local(4, 4, 5) == 0
    assert (G.unit_lanes(4, 5, 8, 8, 8, 8, 2, 2) == -1).all()


@pytest.mark.parametrize("parts,per_slot", [(G.SUMS, 3), (G.SUMS | G.COUNTS, 5), (G.SUMS | G.FEATURES, 11), (G.SUMS | G.COUNTS | G.FEATURES, 13),
                                            (G.SUMS | G.FEATURES | G.FILM, 107), (G.SUMS | G.COUNTS | G.FEATURES | G.FILM, 109), (G.SUMS | G.FILM, 99)])
def test_sizes_equal_the_formula(parts, per_slot):
    a, f, s = int(bool(parts & G.COUNTS)), int(bool(parts & G.FEATURES)), int(bool(parts & G.FILM))
    assert G.tile_floats(parts) == 64 * (3 + 2 * a + 8 * f + 96 * s) == 64 * per_slot
    for w, h, tx, ty, world in SHAPES:
        bx, by = _grid(w, h, tx, ty)
        padded = G.tile_geometry(tx, ty, bx, by, world)[3]
        assert G.unit_floats(parts, tx, ty, bx, by, world) == padded * 64 * per_slot


def test_pack_unit_lays_the_record_out_plane_words_then_rows():
    """every word of a synthetic accumulation is its own address, so each word of the unit says where it came from"""
    w, h, tx, ty, world, rank = 45, 27, 28, 16, 3, 1
    bx, by = _grid(w, h, tx, ty)
    n_lanes = tx * ty * bx * by
    lane = np.arange(n_lanes, dtype=np.uint32)
    planes = [lane + np.uint32((p + 1) << 24) for p in range(5)]
    feat = (lane[:, None] * 8 + np.arange(8, dtype=np.uint32)) | np.uint32(6 << 24)
    film = (lane[:, None] * 96 + np.arange(96, dtype=np.uint32)) | np.uint32(7 << 24)
    lanes = G.unit_lanes(rank, world, w, h, tx, ty, bx, by)
    unit = G.pack_unit(lanes, planes, feat, film)
    rec_words = G.tile_floats(15)
    assert unit.size == lanes.shape[0] * rec_words
    rec = unit.reshape(lanes.shape[0], rec_words)
    for t in (0, 1, 5, 9):
        for lt in (0, 7, 8, 37, 63):
            ln = lanes[t, lt]
            for p in range(5):
                assert rec[t, p * 64 + lt] == (0 if ln < 0 else planes[p][ln])
            f0, s0 = 5 * 64 + lt * 8, 5 * 64 + 64 * 8 + lt * 96
            assert (rec[t, f0:f0 + 8] == (0 if ln < 0 else feat[ln])).all()
            assert (rec[t, s0:s0 + 96] == (0 if ln < 0 else film[ln])).all()
    # to_lanes is the inverse of reading a lane-indexed plane back row-major
    j, i = np.divmod(np.arange(w * h), w)
    rowmajor = planes[0][G.block_linear_idx(i, j, tx, ty, bx)].reshape(h, w)
    back = G.to_lanes(rowmajor, w, h, tx, ty, bx, by)[:, 0]
    chunk = np.zeros(n_lanes, bool)
    chunk[G.block_linear_idx(i, j, tx, ty, bx)] = True
    assert (back[chunk] == planes[0][chunk]).all() and (back[~chunk] == 0).all()
