"""numpy restatement of srt_scene_bvh_ray_cost, the objective of the ray-weighted reinsertion.  TEST INFRASTRUCTURE ONLY.

Written from the text of include/srt_c_api.h (srt_scene_optimise_bvh_for_rays, srt_scene_bvh_ray_cost) and DESIGN.md 5.4, on the arrays of
srt_scene_get_bvh (pre-order: a child's index is greater than its parent's), all segments at once per node:

  usable segment   origin finite, direction without NaN and not all zero, t_end > 0
  reciprocal       float32 1 / d per axis (a zero component gives an infinity of its sign)
  slab planes      (b - o) * inv in float32; near / far of an axis by `lo < hi` selects, so a NaN (0 x inf: an origin on a slab's plane of
                   a ray along it) ends up where the compares below drop it
  meets            e = max(0, nears), m = min(t_end, fars), both by compares (`x > e ? x : e`, `x < m ? x : m`); met when not (m <= e)
  count of a node  the segments that meet its box and the box of every ancestor
  price            area + mu count, area = 2 (dx dy + dy dz + dz dx) in float64, mu = 4 area(root) / usable segments (0 with none)
  objective        sum over the internal nodes of price x (2.5 when a child is a leaf, else 1), float64

The two keyword arguments exist for ONE test, which shows that the comparison with the library tells a wrong restatement apart."""
import numpy as np

RAY_WEIGHT = 4.0
FRINGE_WEIGHT = 2.5


def usable(segments):
    """bool per row of an (n, 7) float32 segment array: the rows the objective counts"""
    s = np.asarray(segments, np.float32).reshape(-1, 7)
    with np.errstate(all="ignore"):
        return (np.isfinite(s[:, 0:3]).all(1) & ~np.isnan(s[:, 3:6]).any(1) & ~(s[:, 3:6] == 0).all(1) & (s[:, 6] > 0))


def box_area(b):
    b = np.asarray(b, np.float32).astype(np.float64)
    dx, dy, dz = b[..., 1] - b[..., 0], b[..., 3] - b[..., 2], b[..., 5] - b[..., 4]
    return 2.0 * (dx * dy + dy * dz + dz * dx)


def meets(o, inv, t_end, box, use_t_end=True):
    """bool per segment: the segment [0, t_end] of the ray o + t d (inv = 1 / d) meets the box (xmin xmax ymin ymax zmin zmax), float32"""
    f = np.float32
    e = np.zeros(len(o), f)
    m = t_end.copy() if use_t_end else np.full(len(o), np.inf, f)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo = ((f(box[2 * a]) - o[:, a]) * inv[:, a]).astype(f)
            hi = ((f(box[2 * a + 1]) - o[:, a]) * inv[:, a]).astype(f)
            first = lo < hi
            near, far = np.where(first, lo, hi), np.where(first, hi, lo)
            e = np.where(near > e, near, e)
            m = np.where(far < m, far, m)
        return ~(m <= e)


def tree_ray_cost(left, right, prim, boxes, segments, use_t_end=True, fringe_weight=FRINGE_WEIGHT):
    """the objective for a tree as srt_scene_get_bvh returns it and an (n, 7) float32 sample"""
    left, right, prim = (np.asarray(a, np.int64) for a in (left, right, prim))
    boxes = np.asarray(boxes, np.float32)
    if len(prim) == 0:
        return 0.0
    s = np.ascontiguousarray(segments, np.float32).reshape(-1, 7)
    s = s[usable(s)]
    o, t_end = s[:, 0:3], s[:, 6]
    with np.errstate(all="ignore"):
        inv = (np.float32(1.0) / s[:, 3:6]).astype(np.float32)
    mu = RAY_WEIGHT * float(box_area(boxes[0])) / len(s) if len(s) else 0.0
    area = box_area(boxes)
    met = {0: meets(o, inv, t_end, boxes[0], use_t_end)}
    total = 0.0
    for k in range(len(prim)):                       # pre-order: a node's mask exists before the node is reached
        mine = met.pop(k)
        if prim[k] >= 0:
            continue
        l, r = left[k], right[k]
        assert l > k and r > k
        leaf_child = prim[l] >= 0 or prim[r] >= 0
        total += (area[k] + mu * int(mine.sum())) * (fringe_weight if leaf_child else 1.0)
        for ch in (l, r):
            met[int(ch)] = mine & meets(o, inv, t_end, boxes[ch], use_t_end)
    return total


def scene_ray_cost(scene, segments, **kw):
    return tree_ray_cost(*scene.bvh(), segments, **kw)
