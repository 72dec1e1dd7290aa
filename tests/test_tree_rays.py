"""The ray-weighted reinsertion (srt_scene_optimise_bvh_for_rays) on the host: no GPU.

The segments are synthetic and seeded: camera rays of the scene's default camera cut at a random t_end (structure, determinism, the
objective), or camera-plus-bounce rays cut at their closest hit on the CPU oracle (the work comparison)."""
import hashlib

import numpy as np
import pytest

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


def _check_structure(scene, n_tris):
    left, right, prim, boxes = scene.bvh()
    leaves = prim[prim >= 0]
    assert sorted(leaves.tolist()) == list(range(n_tris)), "every triangle exactly once"
    assert len(prim) == 2 * n_tris - 1
    for k in np.nonzero(prim < 0)[0]:
        for ch in (left[k], right[k]):
            assert ch > 0
            assert (boxes[k, 0::2] <= boxes[ch, 0::2]).all() and (boxes[k, 1::2] >= boxes[ch, 1::2]).all(), ("box", k, "child", ch)


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
    useless = _camera_segments(_built(srt, sid), 8, seed=3)
    useless[0:2, 6] = 0.0; useless[2, 6] = -1.0; useless[3, 3] = np.nan; useless[4, 3:6] = 0.0; useless[5, 0] = np.nan; useless[6, 1] = np.inf; useless[7, 6] = np.nan
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
