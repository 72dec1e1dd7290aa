"""The ray-weighted reinsertion (srt_scene_optimise_bvh_for_rays) on the host: no GPU.

The segments are synthetic and seeded: camera rays of the scene's default camera cut at a random t_end (structure, determinism, the
objective), or camera-plus-bounce rays cut at their closest hit on the CPU oracle (the work comparison)."""
import hashlib

import numpy as np
import pytest

import refit_cases as R
import tree_cost_reference as T
from helpers import oracle_scene_for

SCENES = {"random spheres (4802 triangles)": 100, "42 triangles": 0, "20 triangles": 1}
W, H = 480, 270


def _built(srt, sid):
    return srt.Scene.builtin(sid, 0).build_bvh(srt.BVH_SAH, 1984)


def _sha(scene):
    h = hashlib.sha256()
    for a in scene.bvh():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _camera(scene):
    cam = scene.default_camera(W, H)
    return tuple(np.array(list(getattr(cam, k)), np.float64) for k in ("pixel_delta_u", "pixel_delta_v", "pixel00_loc", "camera_center"))


def _camera_segments(scene, n, seed):
    """n rays of the default camera through uniformly random image points, each cut at a random t_end between 0.2 and 3 times the
    distance to the middle of the scene's box (the direction is the camera's unnormalised one: t = 1 is the image plane)"""
    rng = np.random.default_rng(seed)
    du, dv, p00, c = _camera(scene)
    d = p00[None, :] + rng.uniform(0, W, n)[:, None] * du[None, :] + rng.uniform(0, H, n)[:, None] * dv[None, :] - c[None, :]
    boxes = scene.bvh()[3]
    mid = 0.5 * (boxes[0, 0::2] + boxes[0, 1::2])
    t_mid = np.linalg.norm(mid - c) / np.linalg.norm(d, axis=1)
    seg = np.zeros((n, 7), np.float32)
    seg[:, 0:3] = c; seg[:, 3:6] = d; seg[:, 6] = t_mid * rng.uniform(0.2, 3.0, n)
    return seg


def _bounce_segments(orc, scene, n_cam, seed, bounces=3):
    """camera rays and up to three diffuse bounces each, cut at their closest hit on the oracle (a miss: the query's upper limit)"""
    rng = np.random.default_rng(seed)
    du, dv, p00, c = _camera(scene)
    osc = oracle_scene_for(orc, scene, 1)
    segs = []
    for _ in range(n_cam):
        o, d = c.copy(), p00 + rng.uniform(0, W) * du + rng.uniform(0, H) * dv - c
        for _ in range(bounces + 1):
            hit, out = osc.trace(o, d)
            segs.append(list(o) + list(d) + [float(out[0]) if hit else float(np.finfo(np.float32).max)])
            if not hit:
                break
            n = out[4:7].astype(np.float64)
            n = -n if np.dot(n, d) > 0 else n
            v = rng.normal(size=3)
            o, d = out[1:4].astype(np.float64) + 1e-3 * n, n + v / np.linalg.norm(v)
    return np.array(segs, np.float32)


def _useless_rows(scene):
    """eight segments the objective leaves out: zero length (two), negative length, NaN direction, all-zero direction, NaN origin, infinite
    origin, NaN length"""
    useless = _camera_segments(scene, 8, seed=3)
    useless[0:2, 6] = 0.0; useless[2, 6] = -1.0; useless[3, 3] = np.nan; useless[4, 3:6] = 0.0; useless[5, 0] = np.nan; useless[6, 1] = np.inf; useless[7, 6] = np.nan
    return useless


def _edge_segments(scene, n=200, seed=23):
    """n segments whose origin lies exactly on the x-min plane of a node's box (within the box's y and z extent) and whose direction runs
    along one axis: 0 x inf, a NaN, turns up in the slabs of that box and of every box that shares the plane.  t_end is FLT_MAX for a
    third of them; every fifth carries -0.0 in its zero components, every seventh + infinity as its one non-zero component."""
    rng = np.random.default_rng(seed)
    boxes = scene.bvh()[3]
    seg = np.zeros((n, 7), np.float32)
    for k in range(n):
        b = boxes[rng.integers(len(boxes))]
        seg[k, 0:3] = (b[0], rng.uniform(b[2], b[3]), rng.uniform(b[4], b[5]))
        if k % 5 == 1:
            seg[k, 3:6] = -0.0
        seg[k, 3 + rng.integers(3)] = np.inf if k % 7 == 2 else rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
        seg[k, 6] = np.finfo(np.float32).max if k % 3 == 0 else rng.uniform(0.1, 20.0)
    return seg


def _depths(left, right, prim):
    """depth of every node (the root's is 0: edges from the root), recomputed from left / right in pre-order"""
    depth = np.zeros(len(prim), np.int64)
    for k in np.nonzero(prim < 0)[0]:
        depth[left[k]] = depth[right[k]] = depth[k] + 1
    return depth


def _check_structure(scene, n_tris):
    left, right, prim, boxes = scene.bvh()
    leaves = prim[prim >= 0]
    assert sorted(leaves.tolist()) == list(range(n_tris)), "every triangle exactly once"
    assert len(prim) == 2 * n_tris - 1
    for k in np.nonzero(prim < 0)[0]:
        for ch in (left[k], right[k]):
            assert ch > k, ("child", ch, "does not follow its parent", k)
            assert (boxes[k, 0::2] <= boxes[ch, 0::2]).all() and (boxes[k, 1::2] >= boxes[ch, 1::2]).all(), ("box", k, "child", ch)
    # a leaf's box contains its own triangle (the vertices the scene holds, not the record the box was made from) ...
    leaf = np.nonzero(prim >= 0)[0]
    V = scene.vertices()[prim[leaf]]
    lo, hi = boxes[leaf, 0::2][:, None, :], boxes[leaf, 1::2][:, None, :]
    inside = ((lo <= V) & (V <= hi)).all(axis=(1, 2))
    assert inside.all(), ("leaf", leaf[~inside][0], "triangle", prim[leaf[~inside][0]], "lies outside its box")
    # ... every box is the one a rebuild over this topology gives, and the depth is the deepest node's
    R.assert_values_equal(boxes, R.restated_boxes(scene), "node boxes against their restatement")
    assert scene.bvh_depth == _depths(left, right, prim).max()


@pytest.mark.parametrize("sid", list(SCENES.values()), ids=list(SCENES.keys()))
def test_structure_pairing_and_determinism(srt, sid):
    """The tree that comes back holds every triangle exactly once, every box contains its children, a paired tree is still paired, and the
    same segments give the same tree in a second call on a fresh copy.  (Whether a deeper tree still fits LDS is a property of a context's
    launch plan: tests/test_tree_rays_gpu.py holds the recipe to it.)  The ray-weighted tree differs from the area-based one on the large
    scene: the sample is not ignored."""
    segs = _camera_segments(_built(srt, sid), 512 if sid == 100 else 64, seed=11)
    a, b = _built(srt, sid), _built(srt, sid)
    paired = a.is_paired
    a.optimise_bvh_for_rays(segs, 3)
    b.optimise_bvh_for_rays(segs.copy(), 3)
    _check_structure(a, a.n_tris)
    assert a.is_paired == paired
    assert a.bvh_depth <= 64
    assert _sha(a) == _sha(b)
    if sid == 100:
        assert _sha(a) != _sha(_built(srt, sid).optimise_bvh(3))


@pytest.mark.parametrize("sid", list(SCENES.values()), ids=list(SCENES.keys()))
def test_prior_alone_is_the_area_optimiser(srt, sid):
    """No usable segment -- an empty array, or segments the call leaves out: zero length, NaN direction, all-zero direction, NaN origin --
    and the entry point returns srt_scene_optimise_bvh's tree, array for array."""
    want = _sha(_built(srt, sid).optimise_bvh(3))
    assert _sha(_built(srt, sid).optimise_bvh_for_rays(np.zeros((0, 7), np.float32), 3)) == want
    useless = _useless_rows(_built(srt, sid))
    assert _sha(_built(srt, sid).optimise_bvh_for_rays(useless, 3)) == want
    assert _built(srt, sid).bvh_ray_cost(useless) == _built(srt, sid).bvh_ray_cost(np.zeros((0, 7), np.float32)) > 0


@pytest.mark.parametrize("sid,n,seed", [(100, 512, 11), (100, 300, 5), (0, 64, 11), (1, 64, 11), (1, 7, 2)])
def test_objective_never_rises(srt, sid, n, seed):
    """The old position of every subtree is in the search space, and a result whose objective for the sample came out higher is put back:
    srt_scene_bvh_ray_cost of the returned tree is at most that of the tree that walked in -- and lower on the large scene."""
    segs = _camera_segments(_built(srt, sid), n, seed)
    s = _built(srt, sid)
    before = s.bvh_ray_cost(segs)
    s.optimise_bvh_for_rays(segs, 3)
    after = s.bvh_ray_cost(segs)
    print("scene %d, %d segments: objective %.6g -> %.6g" % (sid, n, before, after))
    assert 0 < after <= before
    if sid == 100:
        assert after < before


def test_less_work_for_the_rays_it_was_given(srt, orc):
    """Scene 100 at 480 x 270 x 4 spp, depth 16, counted by the CPU oracle (the setting DESIGN.md 5.4 quotes): node visits + 2 x triangle
    tests per ray on the tree tuned against 2 074 camera-plus-bounce segments are fewer than on the area-based tree of the recipe before
    (srt_scene_optimise_bvh, 3 passes).  The oracle walks the whole tree for a NaN-direction ray: the same count on every
    tree of the scene, so it raises both figures by the same amount.  Recorded: profiles/tree_rays/cpu_counts.txt."""
    built = _built(srt, 100)
    segs = _bounce_segments(orc, built, 900, seed=7)
    area = _built(srt, 100).optimise_bvh(3)
    rays = _built(srt, 100).optimise_bvh_for_rays(segs, 3)
    cam = built.default_camera(W, H)
    work = {}
    for name, scene in (("area", area), ("rays", rays)):
        st = oracle_scene_for(orc, scene, 1).render(cam, W, H, 4, 16, threads=16)["stats"]
        work[name] = (st["trav_iters"] + 2 * st["tri_tests"]) / st["rays"]
        print("%s: node visits %.4f + 2 x triangle tests %.4f per ray = %.4f (%d rays, %d segments)"
              % (name, st["trav_iters"] / st["rays"], st["tri_tests"] / st["rays"], work[name], st["rays"], len(segs)))
    assert work["rays"] < work["area"]


# ---- the objective against its restatement (tests/tree_cost_reference.py) ------------------------------------------------------------
def _samples(scene, sid):
    cam, edge = _camera_segments(scene, 512 if sid == 100 else 64, seed=11), _edge_segments(scene)
    return {"camera": cam, "edge": edge, "camera + edge + unusable": np.concatenate([cam, edge, _useless_rows(scene)])}


@pytest.mark.parametrize("sid", list(SCENES.values()), ids=list(SCENES.keys()))
def test_objective_equals_its_restatement(srt, sid):
    """srt_scene_bvh_ray_cost == the numpy restatement written from the header's text, to 1e-12 relative (the order of a float64 sum is
    not part of the contract), on the built tree and on the tree after the ray-weighted reinsertion, for camera segments, for 200 edge
    segments (origin on a box's x-min plane, direction along an axis: NaN slabs; FLT_MAX lengths, -0.0 and +inf components), for both
    with the unusable rows mixed in, and for the unusable rows and an empty array alone.  Measured: the two agree to 2.1e-14 relative or
    better in all 30 cases (this restatement sums in pre-order, the library in its stack's order); scene 100, built tree: 806020901.365294
    for the 512 camera segments, 1033317097.707426 for the edge segments, 869868147.528819 for the mixed sample."""
    built = _built(srt, sid)
    samples = _samples(built, sid)
    tuned = _built(srt, sid).optimise_bvh_for_rays(samples["camera"], 3)
    for tree_name, scene in (("built", built), ("ray-tuned", tuned)):
        for name, segs in list(samples.items()) + [("unusable", _useless_rows(built)), ("empty", np.zeros((0, 7), np.float32))]:
            got, want = scene.bvh_ray_cost(segs), T.scene_ray_cost(scene, segs)
            print("scene %d, %s tree, %s (%d rows, %d usable): library %.17g restatement %.17g" %
                  (sid, tree_name, name, len(segs), T.usable(segs).sum(), got, want))
            assert want > 0 and abs(got - want) <= 1e-12 * want
    assert T.usable(samples["edge"]).all() and not T.usable(_useless_rows(built)).any()
    edge = samples["edge"]
    assert (np.signbit(edge[:, 3:6]) & (edge[:, 3:6] == 0)).any() and np.isposinf(edge[:, 3:6]).any()
    share = (edge[:, 6] == np.finfo(np.float32).max).mean()
    assert 0.3 < share < 0.37


def test_a_wrong_restatement_disagrees(srt):
    """The comparison above discriminates: the restatement with t_end ignored (m starts at +inf: a box beyond the hit is charged) and the
    one with the FRINGE weight at 1 each differ from the library on scene 100 by far more than the 1e-12 the right one is held to."""
    scene = _built(srt, 100)
    segs = _samples(scene, 100)["camera + edge + unusable"]
    got = scene.bvh_ray_cost(segs)
    assert abs(T.scene_ray_cost(scene, segs) - got) <= 1e-12 * got
    for name, kw in (("t_end ignored", dict(use_t_end=False)), ("FRINGE weight 1", dict(fringe_weight=1.0))):
        wrong = T.scene_ray_cost(scene, segs, **kw)
        print("%s: %.17g against the library's %.17g (%.3g relative)" % (name, wrong, got, abs(wrong - got) / got))
        assert abs(wrong - got) > 1e-6 * got


@pytest.mark.parametrize("sid", list(SCENES.values()), ids=list(SCENES.keys()))
def test_structure_of_the_area_tuned_tree(srt, sid):
    """_check_structure on srt_scene_optimise_bvh's trees (3 passes; test_structure_pairing_and_determinism applies it to the ray-tuned
    ones).  Measured depths after area / ray tuning with this file's camera segments (no LDS limit on the host call): 17 / 20 (scene 100),
    10 / 10 (scene 0), 7 / 7 (scene 1)."""
    s = _built(srt, sid).optimise_bvh(3)
    _check_structure(s, s.n_tris)
    r = _built(srt, sid).optimise_bvh_for_rays(_camera_segments(_built(srt, sid), 512 if sid == 100 else 64, seed=11), 3)
    print("scene %d: depth %d after area tuning, %d after ray tuning" % (sid, s.bvh_depth, r.bvh_depth))


@pytest.mark.parametrize("which", R.UNPAIRED)
def test_structure_of_the_unpaired_trees(srt, which):
    """_check_structure on the three SAH trees with a leaf + INNER node (refit_cases.UNPAIRED), as built and after the ray-weighted
    reinsertion against their own camera's segments"""
    scene = R.unpaired_scene(srt, which)[0]
    _check_structure(scene, scene.n_tris)
    scene.optimise_bvh_for_rays(_camera_segments(scene, 64, seed=11), 3)
    _check_structure(scene, scene.n_tris)
