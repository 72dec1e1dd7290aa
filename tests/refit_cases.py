"""Shared by the refit suites (test_refit_host.py, test_refit_api.py, test_refit.py): value equality of scene images, the scenes
and motions of the cases, and a numpy restatement of the node boxes.  Host side only."""
import ctypes as C

import numpy as np

import helpers as H

IMAGES = ("nodes", "nodes_sw", "fringe", "tris", "shade")


def values_equal(a, b):
    """the refit's buffer contract, word by word: two float32 words are equal when their bits are equal, or both are NaN, or both are
    zero (srt_c_api.h, srt_refit_vertices).  a, b: uint32 or float32 arrays of one shape -> bool array"""
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    fa, fb = ua.view(np.float32), ub.view(np.float32)
    return (ua == ub) | (np.isnan(fa) & np.isnan(fb)) | ((fa == 0) & (fb == 0))


def assert_values_equal(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = values_equal(a, b)
    if not ok.all():
        bad = np.nonzero(~ok.reshape(-1))[0]
        raise AssertionError("%s: %d of %d words differ as values, first at word %d: %#x vs %#x" %
                             (what, bad.size, ok.size, bad[0], a.reshape(-1).view(np.uint32)[bad[0]], b.reshape(-1).view(np.uint32)[bad[0]]))


def moved(srt, scene, vertices):
    """a fresh scene (no BVH) made of `scene`'s triangles with the vertices replaced: materials, aa_plane and background as they are"""
    t0 = scene.triangles()
    T = (srt.binding.TriIn * len(t0))()
    C.memmove(T, t0, C.sizeof(T))
    for k in range(len(t0)):
        T[k].v0[:] = vertices[k, 0]; T[k].v1[:] = vertices[k, 1]; T[k].v2[:] = vertices[k, 2]
    return srt.Scene.from_arrays(T, scene.materials(), scene.background())


def restated_boxes(scene):
    """the node boxes of the scene's tree in srt_scene_get_bvh's pre-order, restated: a leaf's is its triangle record's box, an internal
    node's the float32 fmin / fmax of its children's (children follow their parent in pre-order: one reverse sweep)"""
    left, right, prim, _ = scene.bvh()
    rec = scene.tri_records()
    out = np.zeros((left.size, 6), np.float32)
    for k in range(left.size - 1, -1, -1):
        if prim[k] >= 0:
            out[k] = rec[prim[k], 6:12]
        else:
            l, r = out[left[k]], out[right[k]]
            out[k, 0::2] = np.fmin(l[0::2], r[0::2])
            out[k, 1::2] = np.fmax(l[1::2], r[1::2])
    return out


def leaf_plus_inner_nodes(scene):
    """the nodes with one leaf child whose other child has two internal children: a FRINGE record that references an INNER record, which
    lies in FRONT of it in the record order (only unpaired trees have them)"""
    left, right, prim, _ = scene.bvh()
    internal = prim < 0
    inner = np.zeros(left.size, bool)
    inner[internal] = internal[left[internal]] & internal[right[internal]]
    k = np.nonzero(internal)[0]
    return int(np.sum((~internal[left[k]] & inner[right[k]]) | (~internal[right[k]] & inner[left[k]])))


def restated_schedule(scene):
    """records per height of the scene's tree, restated from srt_scene_get_bvh's pre-order: every internal node is a record, its height
    1 + the largest height of an internal child (a leaf child counts 0) -> counts of heights 1, 2, .."""
    left, right, prim, _ = scene.bvh()
    height = np.zeros(left.size, np.int64)
    for k in range(left.size - 1, -1, -1):
        if prim[k] < 0:
            height[k] = 1 + max(height[left[k]], height[right[k]])
    return np.bincount(height[prim < 0], minlength=1)[1:].astype(np.uint32) if (prim < 0).any() else np.zeros(0, np.uint32)


UNPAIRED = ("sah_odd_outlier", "sah_fuzz_13", "sah_optimised")


def unpaired_scene(srt, which):
    """SAH trees with at least one leaf + INNER node -> (scene, cam, W, H, spp, depth).  sah_odd_outlier: 13 triangles, one far from the
    rest, so an odd span splits 1 | rest; sah_fuzz_13: the fuzz case of that seed as it is built; sah_optimised: fuzz case 41 after
    srt_scene_optimise_bvh, whose reinsertions leave such nodes."""
    if which == "sah_odd_outlier":
        rng = np.random.default_rng(0)
        tris = []
        for k in range(13):
            c = np.array([40.0, 0.0, 0.0]) if k == 0 else rng.uniform(-3, 3, 3)
            v = [tuple(float(x) for x in c + rng.normal(0, 0.5, 3)) for _ in range(3)]
            tris.append((v[0], v[1], v[2], k % 2, 0))
        mats = [(srt.binding.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0.0), (srt.binding.MAT_METALLIC, (1.0, 1.0, 1.0), 0.2, 0.0)]
        scene = H.custom_scene(srt, tris, mats).build_bvh(srt.BVH_SAH, 1984)
        W, H_, spp, depth = 45, 37, 3, 5
        return scene, srt.camera_init(W, H_, 60.0, (6.0, 2.0, 30.0), (10.0, 0.0, 0.0)), W, H_, spp, depth
    scene, cam, W, H_, spp, depth, mode, n = H.fuzz_case(srt, 13 if which == "sah_fuzz_13" else 41)
    assert mode == srt.BVH_SAH
    if which == "sah_optimised":
        scene.optimise_bvh(3)
    else:
        assert which == "sah_fuzz_13", which
    return scene, cam, min(W, 64), min(H_, 48), min(spp, 3), depth


def scene_state(scene):
    """everything of a scene a refit may touch or must keep, as bytes and arrays that compare exactly"""
    left, right, prim, boxes = scene.bvh()
    return dict(tris=bytes(scene.triangles()), rec=scene.tri_records().view(np.uint32).copy(), left=left, right=right, prim=prim,
                boxes=boxes.view(np.uint32).copy(), depth=scene.bvh_depth, nodes=scene.n_nodes, paired=scene.is_paired)


def assert_state_equal(a, b, what):
    for k in a:
        same = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]
        assert same, "%s: %s changed" % (what, k)


def jitter(v0, seed, scale=0.25):
    """every vertex moved by a random float32 offset: shared vertices move apart, axis-aligned triangles stop being so"""
    rng = np.random.default_rng(7000 + seed)
    return (v0 + rng.normal(0, scale, v0.shape).astype(np.float32)).astype(np.float32)


def smooth(v0, phase=0.7, amp=0.35):
    """a smooth deformation: a sine wave along x displaces y and z, so that neighbouring triangles keep their shared vertices"""
    v = v0.copy()
    v[..., 1] = (v0[..., 1] + np.float32(amp) * np.sin(np.float32(phase) * v0[..., 0] + np.float32(0.3))).astype(np.float32)
    v[..., 2] = (v0[..., 2] + np.float32(amp) * np.cos(np.float32(phase) * v0[..., 0])).astype(np.float32)
    return np.ascontiguousarray(v, np.float32)


def motion_scene(srt, case):
    """Scenes that come in through srt_scene_set_*, each with two motions -> (scene with a reference BVH, cam, W, H, spp, depth, v1, v2).
    axis_aligned: v1 turns a slanted triangle into an axis-aligned one (its projection axes, and with them its record layout, change) and
    an axis-aligned one into a slanted one; v2 moves them again.  thin: an extent on one axis falls below 1e-4, so the box is padded.
    signed_zero: vertices holding +0 and -0 on the same axis, so fminf and a compare-and-select may pick zeros of either sign.
    degenerate: helpers' degenerate_and_odd_materials; v1 makes a proper triangle degenerate and the point and the needle proper, v2
    undoes part of it."""
    NONE, XY, YZ, XZ = 0, 1, 2, 3
    f = np.float32
    if case == "degenerate":
        scene, cam, W, H_, spp, depth = H.edge_case_scene(srt, "degenerate_and_odd_materials")
        v0 = scene.vertices()
        v1 = v0.copy()
        v1[0] = [[1, 1, 0], [1, 1, 0], [1, 1, 0]]                       # a wall triangle collapses to a point
        v1[4] = [[-1, -1, 1], [1, -1, 1], [0, 1, 1.5]]                  # the point becomes a triangle
        v1[5] = [[-1, 0, 2], [0, 0.8, 2], [1, 0, 2]]                    # the needle opens
        v2 = v1.copy()
        v2[0] = v0[0]                                                   # ... and the wall triangle is back
        v2[5] = [[-1, 0, 2], [0, 0, 2], [1, 0, 2]]                      # the needle closes again
        return scene, cam, W, H_, spp, depth, v1.astype(f), v2.astype(f)
    mats = [(srt.binding.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0.0), (srt.binding.MAT_METALLIC, (1.0, 1.0, 1.0), 0.2, 0.0),
            (srt.binding.MAT_EMISSIVE, (1.0, 1.0, 1.0), 0.0, 3.0)]
    floor = [((-4, -2, -4), (4, -2, -4), (4, -2, 4), 0, NONE), ((-4, -2, -4), (4, -2, 4), (-4, -2, 4), 0, NONE)]
    if case == "axis_aligned":
        tris = floor + [((-2, -1, 0), (0, -1, 1), (-1, 2, 0.5), 1, NONE),       # slanted, plane NONE
                        ((1, -1, 0), (3, -1, 0), (2, 2, 0), 2, YZ),             # in a z plane although its stored plane says YZ
                        ((-3, 0, -1), (-3, 2, -1), (-3, 1, 1), 1, XY),          # in an x plane
                        ((0, 1, -2), (2, 1, -2), (1, 1, -1), 0, XZ)]            # in a y plane
        v0 = np.array([t[:3] for t in tris], f)
        v1 = v0.copy()
        v1[2, :, 2] = 0.25                                              # slanted -> in a z plane
        v1[3, 2, 2] = 1.0                                               # z plane -> slanted: the stored YZ plane applies again
        v1[4, 2, 0] = -2.0                                              # x plane -> slanted: XY
        v1[5, :, 1] = [1.0, 1.5, 1.0]                                   # y plane -> slanted: XZ
        v2 = v1.copy()
        v2[2, :, 2] = [0.0, 1.0, 0.5]                                   # ... and back to the slanted triangle
        v2[2, :, 0] = 1.5                                               # now in an x plane
        v2[5, :, 1] = 1.0
    elif case == "thin":
        tris = floor + [((-1, 0, 0), (1, 0, 0), (0, 1.5, 0.5), 1, NONE), ((-2, 0, 1), (0, 0, 1), (-1, 1, 1.5), 2, NONE)]
        v0 = np.array([t[:3] for t in tris], f)
        v1 = v0.copy()
        v1[2, :, 2] = [0.0, 0.00003, 0.00006]                           # z extent 6e-5 < 1e-4: padded, and not axis aligned
        v1[3, :, 0] = [-1.0, -1.00005, -1.00002]                        # x extent 5e-5
        v2 = v1.copy()
        v2[2, :, 2] = [0.0, 0.0001, 0.0002]                             # extent 2e-4: no padding any more
        v2[3, :, 1] = [0.5, 0.50002, 0.50001]                           # two thin axes at once
    else:
        assert case == "signed_zero", case
        tris = floor + [((0.0, 0, 0), (1, 0, 0.0), (0, 1, 1), 1, NONE), ((-1, 0.0, 0), (0, 1, 0), (0.0, 0, 1), 2, NONE),
                        ((0.0, -1, 0.0), (2, -1, 0.0), (1, -1, 2), 1, NONE)]
        v0 = np.array([t[:3] for t in tris], f)
        v1 = v0.copy()
        v1[2, 0, 0] = -0.0; v1[2, 2, 0] = 0.0; v1[2, 0, 2] = 0.0; v1[2, 1, 2] = -0.0       # min over {-0, 1, +0}, {+0, -0, 1}
        v1[3, 1, 0] = -0.0; v1[3, 2, 0] = 0.0; v1[3, 0, 1] = -0.0; v1[3, 2, 1] = 0.0       # max over {-1, -0, +0}; min over {-0, 1, +0}
        v1[4, 0, 0] = 0.0; v1[4, 0, 2] = -0.0; v1[4, 1, 2] = 0.0                           # boxes of siblings meet in zeros of both signs
        v2 = v1.copy()
        v2[2, 0, 0] = 0.0; v2[2, 2, 0] = -0.0
        v2[3, :, 2] = [-0.0, 0.0, 1.0]
    scene = H.custom_scene(srt, tris, mats).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H_, spp, depth = 45, 37, 4, 5
    cam = srt.camera_init(W, H_, 60.0, (0.3, 0.2, 9.0), (0.0, 0.0, 0.0))
    return scene, cam, W, H_, spp, depth, np.ascontiguousarray(v1, f), np.ascontiguousarray(v2, f)
