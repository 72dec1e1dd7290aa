"""The device with its traversal stack driven to the LAST slot, in every kernel that owns one: srt_trace_rays, render_kernel (both builds,
every launch shape, an accumulating mode) and the surface-motion kernel, on fresh uploads and after the refit on the device.

The inputs are the shelves of tests/traversal_limit_cases.py: a grazing ray meets every box and no triangle, so its lane holds
exact_occupancy(tree) entries at once, which on every tight case is the number the library allocates -- the lane writes slot
loose_bound + 1 of its loose_bound + 2.  One slot further lies the next wave's stack or the end of the workgroup's LDS.  Grazing and
striking rays alternate lane by lane, from both sides of the pile, so that every wave holds lanes at full occupancy next to lanes that are
done after one descent.  tests/test_traversal_limits_reference.py holds the same inputs to the oracle and to the truth on the CPU.

No kernel is ever run with fewer slots than it needs: what the model of the protocol catches with a shortened stack, it catches on the
CPU (test_the_model_has_teeth)."""
import concurrent.futures
import ctypes as C
import os

import numpy as np
import pytest

import ground_truth as G
import surface_motion_reference as M
import traversal_limit_cases as L
from accum_helpers import EVERY_SHAPE_CASES, assert_same_image
from helpers import assert_planes_equal, bits, oracle_scene_for

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
# no knob, and the knob sets of tests/test_gpu_parity.py and accum_helpers.EVERY_SHAPE_CASES: the other stack width and every fetch path
KNOBS = [dict(), dict(wide_refs=True), dict(lds_cache_max=0), dict(lds_cache_max=3), dict(wide_refs=True, lds_cache_max=0),
         dict(wide_refs=True, lds_cache_max=3)]
assert all(k in KNOBS for k, _, _ in EVERY_SHAPE_CASES)
W, H, SPP, DEPTH = 48, 32, 2, 4


def _knob_id(k):
    return ",".join("%s=%s" % kv for kv in sorted(k.items())) or "no knob"


def _n_inner(scene):
    left, right, prim, _ = scene.bvh()
    internal = prim < 0
    k = np.nonzero(internal)[0]
    return int((internal[left[k]] & internal[right[k]]).sum())


def _expected_shape(scene, case, knobs):
    """(narrow_refs, all_cached, paired) the launcher must report for the case's tree under the knobs: 16-bit references up to 32 767
    records unless wide_refs; the whole inner tree in LDS unless the cap is below it (the trees up to 4 802 shelves fit without a knob, the
    two largest do not); the PAIRED variant for a paired tree where narrow == all_cached (render_paired_variant)"""
    narrow = case.shape[0] == 1 and not knobs.get("wide_refs", False)
    cap = knobs.get("lds_cache_max", -1)
    cached = case.shape[1] == 1 and (cap < 0 or cap >= _n_inner(scene))
    if cached and knobs.get("wide_refs", False) and case.n > 600:
        cached = None                        # (56-byte records and 4-byte slots: whether the tree still fits is the launcher's business)
    return narrow, cached, None if cached is None else (case.paired_tree and narrow == cached)


def _assert_shape(gpu, scene, case, knobs):
    plan = gpu.launch_plan()
    want = _expected_shape(scene, case, knobs)
    got = (plan["narrow_refs"], plan["all_cached"], plan["paired"])
    assert all(w is None or bool(w) == g for w, g in zip(want, got)), (case.name, knobs, plan, want)
    return plan


class _knobs:
    """the body runs under the test knobs; they are reset and the scene uploaded again whatever the body did"""
    def __init__(self, gpu, scene, knobs):
        self.gpu, self.scene, self.knobs = gpu, scene, knobs

    def __enter__(self):
        self.gpu.set_test_knobs(**self.knobs)
        self.gpu.upload_scene(self.scene)

    def __exit__(self, *exc):
        self.gpu.set_test_knobs()
        self.gpu.upload_scene(self.scene)
        return False


def _oracle_trace(orc, osc, rays):
    """orc_trace_ray on every ray (the words of the row itself) -> (n, 4) float32 in srt_trace_rays' layout but for column 1, which is 0 for
    a hit (the oracle does not name the triangle) and -1 for a miss: t, 0 / -1, front_face, mat_index.  A grazing ray of the largest piles
    costs the oracle 32 768 node visits: the rays are shared out to a few threads (the call releases the interpreter's lock)."""
    orc.lib()
    fn = C.CDLL(orc.ORACLE_SO).orc_trace_ray
    fn.argtypes, fn.restype = [C.c_void_p] * 4, C.c_int
    rays = np.ascontiguousarray(rays, np.float32)
    out = np.zeros((len(rays), 4), np.float32)
    out[:, 1] = -1
    base = rays.ctypes.data

    def work(ks):
        out9 = np.zeros(9, np.float32)
        po = out9.ctypes.data
        for k in ks:
            if fn(osc.h, base + 24 * k, base + 24 * k + 12, po):
                out[k] = (out9[0], 0.0, out9[7], out9[8])
    threads = max(1, min(os.cpu_count() or 1, 8))
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        list(pool.map(work, [range(j, len(rays), threads) for j in range(threads)]))
    return out


def _oracle_hits(srt, orc, name):
    def make():
        osc = oracle_scene_for(orc, L.built(srt, name), 1)
        out = _oracle_trace(orc, osc, L.rays_and_truth(name)[0])
        osc.close()
        return out
    return G.cached(("shelf oracle hits", name), make)


def _assert_trace_equals_oracle(got, want, what):
    """bit for bit in t, front_face and the material, equal in hit / miss; the device also names the triangle"""
    hit = want[:, 1] >= 0
    assert np.array_equal(got[:, 1] >= 0, hit), "%s: %d rays differ from the oracle in hit / miss" % (what, ((got[:, 1] >= 0) != hit).sum())
    for col, which in ((0, "t"), (2, "front_face"), (3, "material")):
        same = bits(got[:, col]) == bits(want[:, col])
        assert same.all(), "%s: %s of %d rays differs from the oracle's, first ray %d: %r vs %r" % (
            what, which, (~same).sum(), np.nonzero(~same)[0][0], got[~same][0], want[~same][0])


def _hold(name, V, rays, got, what, mat_of_tri=None):
    """ground_truth.assert_hits_hold with the project's thresholds (tests/tree_truth_cases.hold applies the same call to its populations):
    0 rays may differ in hit / miss.  One material for all shelves: the material names no triangle, so column 1 of the device's answer does
    -- on a pile without ties it must be the truth's triangle.  (mat_of_tri: the refitted soups have one material per triangle.)"""
    case = L.CASE[name]
    r, s = G.assert_hits_hold(G.f64(V), rays, got, what, mat_of_tri=np.zeros(len(V), np.int64) if mat_of_tri is None else mat_of_tri)
    assert s["differ"] == 0 and s["excluded"] == 0, (what, s)
    hit = r["want_hit"]
    tri = got[:, 1].astype(np.int64)
    if case.duplicates:
        assert ((tri[hit] >= 0) & (tri[hit] < case.n)).all(), what
    else:
        assert np.array_equal(tri[hit], r["tri"][hit]), "%s: %d rays hit another shelf than the truth's" % (what, (tri[hit] != r["tri"][hit]).sum())
    return s


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_trace_rays_at_full_occupancy(srt, gpu, orc, name):
    """srt_trace_rays on the case's 4 096 interleaved rays, without a knob and under every knob set: every answer equals the oracle's trace
    of the same ray bit for bit, and the rays the truth is computed for (all; the first 512 on the two largest piles) hold to
    ground_truth.closest_hit with 0 rays differing.  Half of the lanes of every wave reach exact_occupancy(tree) entries -- on a tight case
    the last slot of trace_rays_kernel's 32-bit stack."""
    case, scene = L.CASE[name], L.built(srt, name)
    rays, grazing, t, tri, near = L.rays_and_truth(name)
    want = _oracle_hits(srt, orc, name)
    assert np.array_equal(want[:, 1] >= 0, ~grazing)
    V = L.vertices_of(name)
    first = None
    for knobs in KNOBS:
        with _knobs(gpu, scene, knobs):
            plan = _assert_shape(gpu, scene, case, knobs)
            got = gpu.trace_rays(rays)
        what = "%s, %s" % (name, _knob_id(knobs))
        _assert_trace_equals_oracle(got, want, what)
        if first is not None:      # (the truth is walked once per case: under a knob the whole answer, triangle included, is the first one's)
            assert np.array_equal(bits(got), bits(first)), "%s: %d words differ from the answer without a knob" % (what, (bits(got) != bits(first)).sum())
        else:
            first = got
            s = _hold(name, V, rays[:len(t)], got[:len(t)], what)
            print("%-26s occupancy %2d of %2d slots in use  shape (narrow %d, all_cached %d, paired %d)  %s" % (
                name, L.exact_occupancy(scene), L.loose_bound(scene), plan["narrow_refs"], plan["all_cached"], plan["paired"], s))


def _far_render_camera(srt, sign):
    return L.far_camera(srt, W, H, sign, centre=(0.0, 0.0))       # both halves of the shelves in view


def _assert_render_matches(out, ref, what, count_traversal, n_tris):
    """tests/test_gpu_parity.py's reconciliation: planes bit for bit, rays and paths equal, the instrumented build's work counters equal to
    the oracle's up to the NaN-direction queries"""
    assert_planes_equal(out["xyz"], ref["xyz"], what + " XYZ")
    assert_planes_equal(out["lin"], ref["lin"], what + " unquantised sRGB")
    assert_planes_equal(out["fb"], ref["fb"], what + " fb")
    st, rs = out["stats"], ref["stats"]
    assert st["rays"] == rs["rays"] and st["paths"] == rs["paths"], (what, st, rs)
    if count_traversal:
        n_nan = st["util"][2]
        assert st["node_visits"] + n_nan * (n_tris - 1) == rs["trav_iters"] and st["tri_tests"] + n_nan * n_tris == rs["tri_tests"], (what, st, rs)


def _oracle_frames(srt, orc, name):
    """the oracle's renders of the case through the far camera from either side, once per session; each reaches E"""
    def make():
        scene = L.built(srt, name)
        osc = oracle_scene_for(orc, scene, 1)
        out = {sign: osc.render(_far_render_camera(srt, sign), W, H, SPP, DEPTH) for sign in (+1, -1)}
        osc.close()
        for ref in out.values():
            assert ref["stats"]["max_stack"] == L.exact_occupancy(scene), "the frame holds a ray at full occupancy"
            assert W * H * SPP < ref["stats"]["rays"], "... and paths that hit a shelf and go on"
        return out
    return G.cached(("shelf oracle frames", name), make)


@pytest.mark.parametrize("count_traversal", [False, True], ids=["production", "instrumented"])
@pytest.mark.parametrize("knobs", KNOBS, ids=_knob_id)
@pytest.mark.parametrize("name", L.PAIRED)
def test_render_at_full_occupancy_in_every_shape(srt, gpu, orc, name, knobs, count_traversal):
    """render_kernel on the two PAIRED cases through a far narrow camera that sees both halves of the shelves (48 x 32 x 2 spp, depth 4),
    from either side, both kernel builds, without a knob and under every knob set: <1,1,paired> (the headline's shape, its INNER bursts in
    assembly), <0,0,paired>, <1,0>, <0,1> and what the caps make of them.  Planes equal to the oracle's bit for bit, counters reconciled,
    the launch plan the intended one; the oracle's frame reaches max_stack == E == the library's bound."""
    case, scene = L.CASE[name], L.built(srt, name)
    refs = _oracle_frames(srt, orc, name)
    with _knobs(gpu, scene, knobs):
        for sign in (+1, -1):
            out = srt.render_image(scene, _far_render_camera(srt, sign), W, H, SPP, DEPTH, renderer=gpu, count_traversal=count_traversal)
            _assert_shape(gpu, scene, case, knobs)
            _assert_render_matches(out, refs[sign], "%s, %s, towards %+d z" % (name, _knob_id(knobs), sign), count_traversal, case.n)


@pytest.mark.parametrize("count_traversal", [False, True], ids=["production", "instrumented"])
@pytest.mark.parametrize("name", ["32768_sah", "32769_sah", "32768_reference", "4802_reference", "257_sah", "33_duplicates_sah"])
def test_render_at_full_occupancy_as_planned(srt, gpu, orc, name, count_traversal):
    """the shapes the plan picks by itself: 32 768 shelves (32 767 records, the last tree with 16-bit references; its record 32 766 is a
    stack entry) launch narrow_refs, not all_cached -- the tree is PAIRED (scene.is_paired), and the launcher has no PAIRED variant for
    that shape (render_paired_variant), so launch_plan reports the general one; 32 769 shelves launch 32-bit references; the unpaired
    LDS-resident trees <1,1> general.  Bit for bit the oracle's frame, from either side."""
    case, scene = L.CASE[name], L.built(srt, name)
    refs = _oracle_frames(srt, orc, name)
    assert scene.is_paired == case.paired_tree
    for sign in (+1, -1):
        out = srt.render_image(scene, _far_render_camera(srt, sign), W, H, SPP, DEPTH, renderer=gpu, count_traversal=count_traversal)
        plan = gpu.launch_plan()
        assert (plan["narrow_refs"], plan["all_cached"], plan["paired"]) == tuple(bool(x) for x in case.shape), (name, plan)
        _assert_render_matches(out, refs[sign], "%s, towards %+d z" % (name, sign), count_traversal, case.n)
    if case.n == 32768:
        assert scene.n_nodes == 65535 and plan["narrow_refs"] and not plan["all_cached"]
    if case.n == 32769:
        assert not plan["narrow_refs"]


@pytest.mark.parametrize("knobs", KNOBS, ids=_knob_id)
def test_progressive_accumulation_at_full_occupancy(srt, gpu, orc, knobs):
    """render_kernel MODE 3 on the 64-shelf PAIRED case: 2 spp in two passes of 1 through every launch shape equal the oracle's single
    render of 2 spp, bit for bit, after the last pass"""
    name = "64_sah"
    case, scene = L.CASE[name], L.built(srt, name)
    ref = _oracle_frames(srt, orc, name)[+1]
    with _knobs(gpu, scene, knobs):
        steps = list(srt.render_progressive(scene, _far_render_camera(srt, +1), W, H, [1, 1], DEPTH, renderer=gpu))
        _assert_shape(gpu, scene, case, knobs)
    assert [s[0] for s in steps] == [1, 2]
    assert_same_image(steps[-1][1], ref, "%s progressive, %s" % (name, _knob_id(knobs)), rowmajor=False)
    assert steps[-1][1]["stats"]["rays"] > 0


@pytest.mark.parametrize("name", ["64_sah", "64_reference", "257_sah", "257_reference"])
def test_surface_motion_at_full_occupancy(srt, gpu, orc, name):
    """The surface-motion kernel with tracking on.  A far camera whose every pixel-centre ray grazes: tri == -1 everywhere, every output
    word zero, although every lane walked the whole tree at full occupancy.  The same camera over the striking half: the nearest shelf, and
    point and barycentrics equal to tests/surface_motion_reference.py bit for bit, fed the truth's triangle and the oracle's t."""
    scene, V = L.built(srt, name), L.vertices_of(name)
    w = h = 24
    osc = oracle_scene_for(orc, scene, 1)
    gpu.track_motion(True)
    try:
        gpu.upload_scene(scene)
        for sign in (+1, -1):
            cam = L.far_camera(srt, w, h, sign, centre=(0.5, 0.5), vfov=0.1)
            gpu.set_camera(cam)
            got = gpu.surface_motion(w, h)
            assert (got["tri"] == -1).all() and not bits(got["point"]).any() and not bits(got["bary"]).any(), (name, sign)
            assert got["stats"] == dict(hit=0, miss=w * h, moved=0, degenerate=0)
            cam = L.far_camera(srt, w, h, sign, centre=(-0.5, -0.5), vfov=0.1)
            gpu.set_camera(cam)
            got = gpu.surface_motion(w, h)
            rays = M.trace_inputs(cam, w, h)
            t64, k, _, near = G.closest_hit(G.f64(V), G.f64(rays[:, :3]), G.f64(rays[:, 3:]))
            assert (k >= 0).all() and (near >= 1e-3).all()
            zs = V[:, 0, 2]
            assert (V[k, 0, 2] == (zs.min() if sign > 0 else zs.max())).all(), "the truth's triangle is the nearest shelf"
            t = _oracle_trace(orc, osc, rays)
            assert (t[:, 1] >= 0).all() and np.abs(t[:, 0] - t64).max() <= 1e-5      # (t in units of |d| = 200: the next shelf is 5e-5 away)
            want = M.surface_motion(cam, t[:, 0].reshape(h, w), k.reshape(h, w), V)
            assert np.array_equal(got["tri"], want["tri"]), "%s: %d pixels see another shelf" % (name, (got["tri"] != want["tri"]).sum())
            for key in ("point", "bary"):
                same = bits(got[key]) == bits(want[key])
                assert same.all(), "%s towards %+d z, %s: %d of %d words differ" % (name, sign, key, (~same).sum(), same.size)
            assert got["stats"] == want["stats"] == dict(hit=w * h, miss=0, moved=0, degenerate=0)
    finally:
        gpu.track_motion(False)
        osc.close()


REFITS = [(64, L.BVH_REFERENCE, False), (64, L.BVH_SAH, False), (64, L.BVH_SAH, True), (257, L.BVH_REFERENCE, False), (257, L.BVH_SAH, False),
          (257, L.BVH_REFERENCE, True)]


@pytest.mark.parametrize("n,builder,optimise", REFITS, ids=["%d-builder%d%s" % (n, b, "-optimised" if o else "") for n, b, o in REFITS])
def test_refit_to_the_shelves_and_back(srt, gpu, orc, n, builder, optimise):
    """ground_truth.soup(seed, n, 2.0) built and uploaded, its vertices then refitted ON THE DEVICE to the shelves of the same n: a topology no
    shelf builder would make, every box of it hit by the grazing rays.  The trace holds to the truth of the new vertices and equals,
    bit for bit, the oracle walking the same topology over the same vertices, whose far render reaches exact_occupancy(topology).  Then
    back to the soup, held to its truth on the soup's own random rays, and to the shelves once more."""
    name = "%d_sah" % n
    soup = G.soup(300 + n, n, 2.0)
    v_soup, v_shelves = np.ascontiguousarray(soup["V"], np.float32), L.vertices_of(name)
    scene = G.product_scene(srt, soup, builder)
    if optimise:
        scene.optimise_bvh(2)
    E, loose = L.exact_occupancy(scene), L.loose_bound(scene)
    rays, grazing, t, tri, near = L.rays_and_truth(name)
    soup_rays = G.random_rays(400 + n, 4096)
    gpu.upload_scene(scene)
    for step, (v, r) in enumerate(((v_shelves, rays), (v_soup, soup_rays), (v_shelves, rays))):
        gpu.refit(v)
        got = gpu.trace_rays(r)
        scene.refit(v)                          # the host's refit of the same topology: what the oracle is given
        assert L.exact_occupancy(scene) == E and L.loose_bound(scene) == loose, "a refit keeps the topology"
        osc = oracle_scene_for(orc, scene, 1)
        what = "soup of %d, builder %d%s, refit %d" % (n, builder, ", optimised" if optimise else "", step)
        _assert_trace_equals_oracle(got, _oracle_trace(orc, osc, r), what)
        if v is v_shelves:
            _hold(name, v, r, got, what, mat_of_tri=np.arange(n))
            for sign in (+1, -1):
                st = osc.render(L.far_camera(srt, 24, 16, sign), 24, 16, 1, 2)["stats"]
                assert st["max_stack"] == E, (what, st, E)
        else:
            G.assert_hits_hold(G.f64(v), r, got, what, mat_of_tri=np.arange(n))
        osc.close()
    print("soup of %d, builder %d%s: occupancy %d reached on the refitted shelves, library's bound %d" % (n, builder, ", optimised" if optimise else "", E, loose))


def test_the_ray_sample_of_a_grazing_frame(srt, gpu, orc):
    """srt_collect_ray_segments on the 64-shelf PAIRED case through the far camera over the grazing half: every segment is a camera ray, and
    every one has the t_end of a miss (FLT_MAX); through the camera over both halves the row checks of tests/test_tree_rays_gpu.py pass:
    canonical order, every row the oracle's closest hit or miss bit for bit, the misses counted."""
    name = "64_sah"
    scene = L.built(srt, name)
    osc = oracle_scene_for(orc, scene, 1)
    w = h = 24
    cam = L.far_camera(srt, w, h, +1, centre=(0.5, 0.5), vfov=0.1)
    gpu.upload_scene(scene); gpu.set_camera(cam)
    segs, queries = gpu.collect_ray_segments(w, h, SPP, DEPTH, stride=1)
    st = gpu.stats()
    assert len(segs) == queries == st["rays"] - st["util"][2] == w * h * SPP and st["hits"] == 0
    assert (segs[:, 6] == FLT_MAX).all(), "%d segments of grazing pixels do not have the t_end of a miss" % (segs[:, 6] != FLT_MAX).sum()
    assert (segs[:, 0:3] == np.array(list(cam.camera_center), np.float32)).all()
    cam = _far_render_camera(srt, -1)
    gpu.upload_scene(scene); gpu.set_camera(cam)
    segs, queries = gpu.collect_ray_segments(W, H, SPP, DEPTH, stride=1)
    st = gpu.stats()
    assert len(segs) == queries == st["rays"] - st["util"][2] > W * H * SPP
    words = np.ascontiguousarray(segs).view(np.uint32)
    assert np.array_equal(np.lexsort(words.T[::-1]), np.arange(len(words))), "the rows are not in canonical order"
    want = _oracle_trace(orc, osc, np.ascontiguousarray(segs[:, :6]))
    missed = segs[:, 6] == FLT_MAX
    differ = ((want[:, 1] >= 0) == missed) | (~missed & (bits(want[:, 0]) != bits(segs[:, 6])))
    assert not differ.any(), ("first differing row", int(np.nonzero(differ)[0][0]), segs[np.nonzero(differ)[0][0]])
    assert int(missed.sum()) == queries - st["hits"] and 0 < missed.sum() < len(segs)
    osc.close()
    # ... and its camera rows against the truth over all triangles, with the project's thresholds
    rows = segs[(segs[:, 0:3] == np.array(list(cam.camera_center), np.float32)).all(axis=1)]
    assert len(rows) == W * H * SPP
    V, o, d = G.f64(L.vertices_of(name)), G.f64(rows[:, 0:3]), G.f64(rows[:, 3:6])
    t64, tri, _, near = G.closest_hit(V, o, d)
    held, want_hit, got_hit, k = near >= G.EDGE_MARGIN, tri >= 0, rows[:, 6] < FLT_MAX, np.maximum(tri, 0)
    with np.errstate(all="ignore"):
        ratio = np.where(got_hit & want_hit, np.abs(rows[:, 6].astype(np.float64) - t64) / G.t_bound(G.normals(V)[1][k], V[k, 0], o, d, t64), 0.0)
    bad = held & (got_hit != want_hit)
    print("%s: %d camera rows, %d hit in the truth, %d inside the margin, %d differ, largest |dt| / t_bound %.3f" % (
        name, len(rows), want_hit.sum(), (~held).sum(), bad.sum(), ratio[held].max()))
    assert not bad.any() and ratio[held].max() <= G.C_T and (~held).mean() <= G.MAX_EXCLUDED and 0 < want_hit.sum() < len(rows)


def _lds_bytes(srt, gpu):
    n = C.c_size_t()
    srt.binding.check(srt.binding.lib().srt_launch_lds_bytes(gpu._h, C.byref(n)), gpu._h)
    return n.value


def test_the_allocation_is_the_bound_plus_two_slots(srt, gpu):
    """srt_launch_lds_bytes with the LDS cache capped at 0 is tables + waves x slots x 64 x (2 | 4) bytes: under 16-bit and under 32-bit
    references the difference is waves x slots x 128.  On the trees up to 4 802 shelves but the deepest the workgroup has 16 waves (the
    stacks leave room for the cache), so slots = difference / 2 048 -- and that is loose_bound + 2 on every one of them, with one and the same table size."""
    tables = set()
    for case in L.CASES:
        scene = L.built(srt, case.name)
        # (render_launch_shape halves the workgroup once 16 stacks and a 16 KB cache pass the 160 KB budget: 4802_optimised under 32-bit slots)
        if case.n > 4802 or 16 * (L.loose_bound(scene) + L.SENTINELS) * 256 + 32 * 1024 > 160 * 1024:
            continue
        size = {}
        for wide in (False, True):
            with _knobs(gpu, scene, dict(wide_refs=wide, lds_cache_max=0)):
                assert gpu.launch_plan()["n_cached"] == 0 and gpu.launch_plan()["narrow_refs"] == (not wide)
                size[wide] = _lds_bytes(srt, gpu)
        slots, rest = divmod(size[True] - size[False], 16 * 64 * 2)
        assert rest == 0 and slots == L.loose_bound(scene) + L.SENTINELS, (case.name, size, slots, L.loose_bound(scene))
        tables.add(size[False] - 16 * slots * 64 * 2)
    assert len(tables) == 1, tables


DEVICE_FIGURES = """Measured on one MI355X.  Entries a grazing lane holds at once / entries the library allocates, and the shape (narrow_refs, all_cached,
paired) the launch plan picks without a knob; every answer equals the oracle's bit for bit, 0 rays differ from the truth, none excluded:

  8_reference, 8_sah                    2 /  2   (1, 1, 1)        4802_reference                      11 / 11   (1, 1, 0)
  64_*, 64_no_jitter_* (both builders)  5 /  5   (1, 1, 1)        32768_reference, 32768_sah          14 / 14   (1, 0, 0)   truth: 512 rays
  257_reference, 257_sah                7 /  7   (1, 1, 0)        32769_reference, 32769_sah          14 / 14   (0, 0, 0)   truth: 512 rays
  33_duplicates_reference, _sah         4 /  4   (1, 1, 0)        600_optimised (loose)               12 / 17   (1, 1, 0)
                                                                  4802_optimised (loose)              25 / 31   (1, 0, 0)
  refitted soups (occupancy / bound)    64: reference 5 / 5, SAH 6 / 7, SAH optimised 6 / 7;  257: reference 7 / 7, SAH 7 / 9, reference optimised 9 / 11

With their last slot in use now run: trace_rays_kernel (32-bit slots; LDS, partly cached and L2 fetch paths, 16- and 32-bit references) on
every tight case; render_kernel MODE 0 and MODE 1 in <1,1,paired>, <0,0,paired>, <1,1>, <1,0>, <0,1> and <0,0> (the PAIRED cases under the
knobs, 257 / 33 / 4 802 / 32 768 / 32 769 shelves as planned), MODE 3 in the same six shapes, the segment dump's frame; the surface-motion
kernel (64 and 257 shelves, both builders).  <., NARROW = false, ALL_CACHED = true> runs only under the wide_refs knob, here as elsewhere.
Not run at full occupancy: render_kernel's MODE 2 and MODEs 4 - 11 (cost probe, adaptive, spectral, streamed and featured accumulations).

  the ray sample of 64_sah       grazing camera: 1 152 segments, all with the t_end of a miss; camera over both halves: 3 072 camera rows, 1 533
                                 hit in the truth, 0 inside the margin, 0 differ, largest |dt| / t_bound 0.058
  the 71 tests of this file      23.3 s together, the slowest 4.0 s (32768_reference: 3 s of it the truth's walk over 32 768 triangles)"""
