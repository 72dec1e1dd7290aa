"""Inputs that drive the traversal stack to its last slot, and restatements of how that stack is sized and used.  Host side only (no GPU):
tests/test_traversal_limits_reference.py holds this file to the CPU oracle and to tests/ground_truth.py, tests/test_traversal_limits.py
holds the device to it.

The scene is a pile of n SHELVES: triangles that each fill the lower-left half of the square [-1, 1]^2 (x + y <= about 0) at distinct z.
A ray through the upper-right half, nearly parallel to z, meets every node's box and no triangle: nothing is pruned, every internal node is
visited, and the stack fills as far as the topology allows.  The traversal descends left and pushes right (bvh.cu:154-160), so that ray
reaches the occupancy

    E(k) = max([k is INNER] + E(left), E(right)),   E(leaf) = 0,   INNER = both children internal,

while flatten_scene sizes the stack by the largest number of INNER nodes on ANY root-to-leaf path (loose_bound): E <= loose_bound, with
equality on every tight case of CASES, where the ray therefore uses the last slot the kernels allocate."""
import collections

import numpy as np

import ground_truth as G
from helpers import custom_scene

BVH_REFERENCE, BVH_SAH = 0, 1
MAT_LAMBERTIAN = 0
SENTINELS = 2              # kStackSentinels (srt_device.h): slots 0 and 1 hold -1, entry k lives in slot k + 2
# The shelves' edges move outwards by up to this much, so that no two centroids or boxes coincide and the builders' sorts have no ties; the
# hypotenuse stays below x + y = 0.001.  Small against the shelves on purpose: with 0.05 the SAH builder's splits follow the jitter instead of
# z, its trees lose their balance, and E falls one or two short of the library's bound (measured: 64 shelves 5 / 6, 32 768 shelves 15 / 17).
JITTER = 1e-3
TILT = 1e-3                # the rays' directions are (+-TILT, +-TILT, +-1) at most
STANDOFF = 1.0             # the rays start this far in front of the first shelf
N_RAYS = 4096
FAR = 200.0                # distance of the far, narrow cameras
DEFAULT_GAP = 0.01


# ---- the shelves -----------------------------------------------------------------------------------------------------------------
def shelf_vertices(n, seed, jitter=True, duplicates=False, gap=DEFAULT_GAP):
    """(n, 3, 3) float32 in a shuffled order: (-1 - j0, -1 - j0, z_k), (1 + j1, -1 - j0, z_k), (-1 - j0, 1 + j2, z_k) with z_k = (k - (n - 1) / 2)
    gap.  jitter=False: j = 0, every centroid has the same x and y.  duplicates: j = 0 and every z_k = 0 -- n exact copies, every t ties."""
    rng = np.random.default_rng(9000 + seed)
    j = rng.uniform(0.0, JITTER, (n, 3)) if jitter and not duplicates else np.zeros((n, 3))
    z = np.zeros(n) if duplicates else (np.arange(n) - (n - 1) / 2.0) * gap
    V = np.zeros((n, 3, 3))
    V[:, 0] = np.stack([-1 - j[:, 0], -1 - j[:, 0], z], axis=1)
    V[:, 1] = np.stack([1 + j[:, 1], -1 - j[:, 0], z], axis=1)
    V[:, 2] = np.stack([-1 - j[:, 0], 1 + j[:, 2], z], axis=1)
    return np.ascontiguousarray(V[rng.permutation(n)], np.float32)


def shelves(srt, n, seed, jitter=True, duplicates=False, gap=DEFAULT_GAP):
    """the product scene of the shelves (no tree yet): one Lambertian material, a grey background"""
    V = shelf_vertices(n, seed, jitter, duplicates, gap).astype(np.float64)
    tris = [(tuple(v[0]), tuple(v[1]), tuple(v[2]), 0, 0) for v in V.tolist()]
    return custom_scene(srt, tris, [(MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0.0)], (0.5, 0.5, 0.5))


def top_of(V):
    """the largest |z| of the pile"""
    return float(np.abs(np.asarray(V)[:, :, 2]).max())


# ---- the stack's size, restated ------------------------------------------------------------------------------------------------------
def _topology(scene):
    left, right, prim, _ = scene.bvh()
    internal = prim < 0
    inner = np.zeros(left.size, bool)
    inner[internal] = internal[left[internal]] & internal[right[internal]]
    return left.tolist(), right.tolist(), internal.tolist(), inner.tolist()


def loose_bound(scene):
    """flatten_scene, "Entries the traversal stack can hold at once": the largest number of INNER nodes on a root-to-leaf path, at least 1
    (srt_scene_get_bvh's order is a pre-order: children follow their parent, one reverse sweep)"""
    left, right, internal, inner = _topology(scene)
    path = [0] * len(left)
    for k in range(len(left) - 1, -1, -1):
        if internal[k]:
            path[k] = (1 if inner[k] else 0) + max(path[left[k]], path[right[k]])
    return max(1, path[0])


def exact_occupancy(scene):
    """E(root): the most entries any ray can have on the stack at once -- only the way to a LEFT child keeps an entry (the pushed right
    sibling) alive; the way to a right child starts after that entry was popped"""
    left, right, internal, inner = _topology(scene)
    E = [0] * len(left)
    for k in range(len(left) - 1, -1, -1):
        if internal[k]:
            E[k] = max((1 if inner[k] else 0) + E[left[k]], E[right[k]])
    return E[0]


class StackModel:
    """The device's stack protocol (srt_device.h, "Branch-free ...") walked over the topology alone for the ray that hits every box and no
    triangle: slots 0 and 1 are sentinels holding -1, entry k lives in slot k + 2, the newest entry lives in the register `top`; every step
    reads slot sp (`below`) and writes `top` to slot sp + 1, then pops (no child internal: node = top, top = below, sp - 1), pushes (both
    internal: node = left, top = right, sp + 1) or descends into the one internal child.  slots: the slots the lane owns.  Records the
    highest slot read and written, the writes that fell outside the lane's slots, and the visit order."""

    def __init__(self, scene, slots):
        left, right, internal, _ = _topology(scene)
        self.slots, self.max_read, self.max_written, self.out_of_range, self.order = slots, -1, -1, [], []
        mem = {0: -1, 1: -1}                     # stack_init
        node, top, sp = (0 if internal[0] else -1), -1, 0
        while node != -1:
            below = mem[sp]                      # (a KeyError would be a read of a slot nothing wrote: the protocol never does that)
            self.max_read = max(self.max_read, sp)
            mem[sp + 1] = top
            self.max_written = max(self.max_written, sp + 1)
            if sp + 1 >= slots:
                self.out_of_range.append((len(self.order), sp + 1))
            self.order.append(node)
            l, r = left[node], right[node]
            if internal[l] and internal[r]:
                node, top, sp = l, r, sp + 1
            elif not internal[l] and not internal[r]:
                node, top, sp = top, below, sp - 1
            else:
                node = l if internal[l] else r
        assert sp == -1 and top == -1, "the walk ends with the pop from the empty stack"
        self.visits = len(self.order)


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def _rays(n_rays, top, sign, lo, hi, seed):
    rng = np.random.default_rng(seed)
    o = np.empty((n_rays, 3))
    o[:, :2] = rng.uniform(lo, hi, (n_rays, 2))
    o[:, 2] = -sign * (top + STANDOFF)
    d = np.empty((n_rays, 3))
    d[:, :2] = rng.uniform(-TILT, TILT, (n_rays, 2))
    d[:4, :2] = 0.0                              # a few exactly axis-aligned: 1 / d is infinite on two axes
    d[:, 2] = sign
    return np.concatenate([o, d], axis=1).astype(np.float32)


def grazing_rays(n_rays, top, sign, seed=31):
    """rays that travel towards sign * z through x, y in (0.15, 0.85) from STANDOFF in front of the pile: over the pile's 2 top + STANDOFF they
    drift sideways by at most TILT times that (0.05 for the deepest pile, top = 24), so that they stay inside every box ([-1, 1]^2 at the
    least) and above every hypotenuse (x + y <= 0.001)"""
    return _rays(n_rays, top, sign, 0.15, 0.85, seed + (0 if sign > 0 else 1))


def striking_rays(n_rays, top, sign, seed=41):
    """the same through x, y in (-0.85, -0.15): inside every shelf, so that they hit the nearest one"""
    return _rays(n_rays, top, sign, -0.85, -0.15, seed + (0 if sign > 0 else 1))


def interleaved_rays(top, n_rays=N_RAYS):
    """lane by lane: grazing towards +z, striking towards +z, grazing towards -z, striking towards -z -- every wave holds lanes at full
    occupancy next to lanes that finish after one descent.  Returns rays (n_rays, 6) float32 and the boolean row `grazing`."""
    q = n_rays // 4
    rays = np.empty((4 * q, 6), np.float32)
    rays[0::4], rays[1::4] = grazing_rays(q, top, +1), striking_rays(q, top, +1)
    rays[2::4], rays[3::4] = grazing_rays(q, top, -1), striking_rays(q, top, -1)
    return rays, (np.arange(4 * q) % 2) == 0


def far_camera(srt, W, H, sign, centre=(0.5, 0.5), vfov=0.35):
    """a narrow camera FAR in front of the pile that looks towards sign * z at (centre, 0).  (0.5, 0.5) with 0.35 degrees sees the grazing
    half and, in its corners, a little of the other; (0, 0) sees both halves; 0.1 degrees at W = H is a square of half-width 0.175: about
    (0.5, 0.5) every ray grazes, about (-0.5, -0.5) every ray strikes."""
    return srt.camera_init(W, H, vfov, (centre[0], centre[1], -sign * FAR), (centre[0], centre[1], 0.0))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# shape = (narrow_refs, all_cached, paired) of the launch without test knobs; paired_tree = scene.is_paired.  The launcher runs the PAIRED
# variant only where narrow == all_cached (render_paired_variant): the 32 768 shelves' SAH tree IS paired, but its 16 383 INNER records
# do not fit LDS, and <., NARROW, !ALL_CACHED> has the general variant alone.
# loose: the allocation exceeds the need (E < loose_bound): exempt from "last slot used", results must hold all the same.
Case = collections.namedtuple("Case", "name n builder optimise jitter duplicates gap shape paired_tree loose")


def _case(name, n, builder, shape, paired_tree, optimise=False, jitter=True, duplicates=False, gap=DEFAULT_GAP, loose=False):
    return Case(name, n, builder, optimise, jitter, duplicates, gap, shape, paired_tree, loose)


CASES = [
    _case("8_reference", 8, BVH_REFERENCE, (1, 1, 1), True),
    _case("8_sah", 8, BVH_SAH, (1, 1, 1), True),
    _case("64_reference", 64, BVH_REFERENCE, (1, 1, 1), True),
    _case("64_sah", 64, BVH_SAH, (1, 1, 1), True),
    _case("257_reference", 257, BVH_REFERENCE, (1, 1, 0), False),
    _case("257_sah", 257, BVH_SAH, (1, 1, 0), False),
    _case("33_duplicates_reference", 33, BVH_REFERENCE, (1, 1, 0), False, duplicates=True),
    _case("33_duplicates_sah", 33, BVH_SAH, (1, 1, 0), False, duplicates=True),
    _case("64_no_jitter_reference", 64, BVH_REFERENCE, (1, 1, 1), True, jitter=False),
    _case("64_no_jitter_sah", 64, BVH_SAH, (1, 1, 1), True, jitter=False),
    _case("4802_reference", 4802, BVH_REFERENCE, (1, 1, 0), False),                 # scene 100's size: its bound is reached
    _case("32768_reference", 32768, BVH_REFERENCE, (1, 0, 0), True, gap=0.001),    # 32 767 records: the last tree with 16-bit references
    _case("32768_sah", 32768, BVH_SAH, (1, 0, 0), True, gap=0.001),
    _case("32769_reference", 32769, BVH_REFERENCE, (0, 0, 0), False, gap=0.001),   # the first tree with 32-bit references
    _case("32769_sah", 32769, BVH_SAH, (0, 0, 0), False, gap=0.001),
    _case("600_optimised", 600, BVH_REFERENCE, (1, 1, 0), False, optimise=True, loose=True),
    # (its 33 slots per lane leave room for 1 815 of its INNER records: the slack of the bound is what keeps this tree out of LDS)
    _case("4802_optimised", 4802, BVH_REFERENCE, (1, 0, 0), False, optimise=True, loose=True),
]
CASE = {c.name: c for c in CASES}
TIGHT = [c.name for c in CASES if not c.loose]
LOOSE = [c.name for c in CASES if c.loose]
PAIRED = ["8_sah", "64_sah"]                    # the PAIRED cases of the render tests (SAH trees: the headline's builder)
SEED = 5


def vertices_of(case):
    case = CASE[case] if isinstance(case, str) else case
    return G.cached(("shelf vertices", case.n, case.jitter, case.duplicates, case.gap),
                    lambda: shelf_vertices(case.n, SEED, case.jitter, case.duplicates, case.gap))


def built(srt, case):
    """the case's scene with its tree, built once per session (nothing mutates it)"""
    case = CASE[case] if isinstance(case, str) else case

    def make():
        scene = shelves(srt, case.n, SEED, case.jitter, case.duplicates, case.gap).build_bvh(case.builder, 1984)
        if case.optimise:
            scene.optimise_bvh(2)
        assert np.array_equal(scene.vertices(), vertices_of(case))
        return scene
    return G.cached(("shelf scene", case.name), make)


TRUTH_CHUNK = 1024
BIG_PILE, BIG_PILE_TRUTH_RAYS = 4802, 512


def truth_rays(case):
    """how many of the case's rays, from the first on, the truth is computed for: all 4 096, but on the piles of 32 768 and 32 769 shelves the
    first 512 (128 of each kind; the rays are independent draws).  ground_truth.closest_hit visits one triangle per Python step: 4 096
    rays cost 16 s per such pile, 512 cost 3 s.  ALL 4 096 answers of the device are still held to the oracle's bit for bit."""
    case = CASE[case] if isinstance(case, str) else case
    return N_RAYS if case.n <= BIG_PILE else BIG_PILE_TRUTH_RAYS


def closest_hit_in_chunks(V, o, d):
    """ground_truth.closest_hit over all triangles, TRUTH_CHUNK at a time (its scratch array has one float64 per ray and triangle): the
    earliest chunk wins a tie in t, as the earliest triangle does inside closest_hit.  Returns t, tri, near."""
    t, tri, near = np.full(len(o), np.inf), np.full(len(o), -1, np.int64), np.full(len(o), np.inf)
    for lo in range(0, len(V), TRUTH_CHUNK):
        tc, kc, _, nc = G.closest_hit(V[lo:lo + TRUTH_CHUNK], o, d)
        better = tc < t
        t, tri, near = np.where(better, tc, t), np.where(better, kc + lo, tri), np.minimum(near, nc)
    return t, tri, near


def rays_and_truth(case):
    """the case's 4 096 interleaved rays, the row `grazing`, and the float64 truth (t, tri, near) over ALL triangles, no tree, for the first
    truth_rays(case) of them: computed once per pile (the builders share it)"""
    case = CASE[case] if isinstance(case, str) else case

    def make():
        V = vertices_of(case)
        rays, grazing = interleaved_rays(top_of(V))
        r = rays[:truth_rays(case)]
        t, tri, near = closest_hit_in_chunks(G.f64(V), G.f64(r[:, :3]), G.f64(r[:, 3:]))
        return rays, grazing, t, tri, near
    return G.cached(("shelf rays", case.n, case.jitter, case.duplicates, case.gap), make)


def assert_truth_of_the_rays(case):
    """what ground_truth.closest_hit says about the case's rays: every grazing ray misses; every striking ray hits the NEAREST shelf (for
    the duplicates: one of the tied copies, at the t they all share), far from every edge"""
    case = CASE[case] if isinstance(case, str) else case
    V = vertices_of(case).astype(np.float64)
    rays, grazing, t, tri, near = rays_and_truth(case)
    rays, grazing = rays[:len(t)], grazing[:len(t)]
    assert (tri[grazing] == -1).all() and np.isinf(t[grazing]).all(), "%s: a grazing ray hits a shelf in the truth" % case.name
    s = ~grazing
    assert (tri[s] >= 0).all() and (near[s] >= 1e-3).all(), "%s: a striking ray misses, or passes near an edge" % case.name
    towards_plus = rays[s, 5] > 0
    z_hit = V[tri[s], 0, 2]
    zs = V[:, 0, 2]
    assert (z_hit[towards_plus] == zs.min()).all() and (z_hit[~towards_plus] == zs.max()).all(), "%s: not the nearest shelf" % case.name
    if case.duplicates:
        assert (zs == 0).all() and ((tri[s] >= 0) & (tri[s] < case.n)).all()
        assert np.array_equal(V, np.broadcast_to(V[0], V.shape)), "the duplicates are exact copies: every one ties"
    return rays, grazing, t, tri
