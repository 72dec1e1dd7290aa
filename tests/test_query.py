"""The batched ray queries on the device (srt_intersect_rays*, srt_occluded_rays*; include/srt_c_api.h "Ray queries").

Populations (tests/query_reference.py): 4 096 random rays with random intervals into a soup, the bumpy sheet, the axis-aligned set and the
degenerate walls, and 4 000 camera rays of scene 0 (CORNELL).  Each runs under every knob set of tests/test_traversal_limits.KNOBS, so that
every instantiated shape of query_kernel meets it, and:
  * anchor: over [0, FLT_MAX] and [0, +inf] the closest query is srt_trace_rays word for word;
  * exact contracts on every ray: occluded == (hit.tri >= 0), every hit has tmin <= t <= tmax, and the answers are the same words under
    every knob set (a ray's answer depends on the ray and the tree alone);
  * truth on the held rays (not on the degenerate walls, which the product answers by its projected test, as the reference does): hit or
    miss, triangle, |t - t_truth| <= C_T t_bound, front_face; at most MAX_EXCLUDED of the rays left out.  Where triangles overlap in one
    plane the truth has several triangles at one t (query_reference, `tie`: scene 0's floor under its tall box, which an interval that
    starts inside the box reaches): the named triangle must be one of them, and t and front_face are held to the triangle named.
query_last() reports the plan's shape: narrow_refs, all_cached, paired and n_cached of launch_plan()."""
import ctypes as C

import numpy as np
import pytest

import ground_truth as G
import query_reference as Q
from helpers import bits
from test_traversal_limits import KNOBS, _knob_id, _knobs

pytestmark = pytest.mark.gpu

FLT_MAX = Q.FLT_MAX


def _scene(srt, name):
    """the product scene of a population, built once per session"""
    def make():
        kind, src = Q.population(name, srt)["source"]
        return src if kind == "builtin" else G.product_scene(srt, src, srt.BVH_SAH)
    return G.cached(("query scene", name), make)


def _assert_plan_shape(gpu, any_query, what):
    plan, q = gpu.launch_plan(), gpu.query_last()
    got = (q["narrow_refs"], q["all_cached"], q["paired"], q["n_cached"], q["any"])
    want = (plan["narrow_refs"], plan["all_cached"], plan["paired"], plan["n_cached"], any_query)
    assert got == want, (what, q, plan)
    assert q["waves"] >= 1 and q["ms"] >= 0.0
    return q


def _assert_exact(rays, hits, occ, what):
    hit = hits[:, 1] >= 0
    assert np.array_equal(occ, hit), "%s: %d rays where occluded differs from the closest query's hit" % (what, (occ != hit).sum())
    t = hits[hit, 0]
    inside = (rays[hit, 3] <= t) & (t <= rays[hit, 7])
    assert inside.all(), "%s: %d hits outside [tmin, tmax], first %r" % (what, (~inside).sum(), (rays[hit][~inside][:1], hits[hit][~inside][:1]))
    miss = hits[~hit]
    assert (bits(miss[:, 0]) == 0).all() and (miss[:, 1] == -1).all() and (bits(miss[:, 2:]) == 0).all(), what


def _assert_truth(pop, hits, what):
    V, rays, t = G.f64(pop["V"]), pop["rays"], pop["truth"]
    held = t["held"]
    got_hit = hits[:, 1] >= 0
    bad = held & (got_hit != t["hit"])
    assert not bad.any(), "%s: %d held rays differ from the truth in hit / miss, first %d" % (what, bad.sum(), np.nonzero(bad)[0][0])
    both = held & got_hit & t["hit"]
    m = np.arange(len(rays))
    k = np.clip(hits[:, 1].astype(np.int64), 0, len(V) - 1)
    # the truth's triangle, or one that crosses the ray at the same t within the error bounds (overlapping coplanar triangles: query_reference)
    same_tri = ~both | t["tie"][k, m]
    assert same_tri.all(), "%s: %d held rays hit another triangle than the truth's, first %d (%d, truth %d)" % (
        what, (~same_tri).sum(), np.nonzero(~same_tri)[0][0], k[~same_tri][0], t["tri"][~same_tri][0])
    print("%s: %d held hits, %d of them on a tie (%d named another tied triangle than the truth's first)" % (
        what, both.sum(), (both & (t["tie"].sum(0) > 1)).sum(), (both & (k != t["tri"])).sum()))
    o, d = G.f64(rays[:, 0:3]), G.f64(rays[:, 4:7])
    _, nu = G.normals(V)
    tk = np.where(both, t["all_t"][k, m], 0.0)      # the named triangle's crossing: the truth's t unless the ray hit a tie
    with np.errstate(all="ignore"):
        ratio = np.where(both, np.abs(hits[:, 0].astype(np.float64) - tk) / G.t_bound(nu[k], V[k, 0], o, d, tk), 0.0)
    assert ratio.max() <= G.C_T, "%s: |dt| / t_bound = %.3g at ray %d" % (what, ratio.max(), ratio.argmax())
    ff = G.front_face(V, k, d)
    assert ((hits[both, 2] != 0) == ff[both]).all(), "%s: front_face differs from the truth's" % what
    excluded = (~held).mean()
    assert excluded <= G.MAX_EXCLUDED, (what, excluded)
    return dict(held=int(held.sum()), hits=int(both.sum()), max_ratio=float(ratio.max()), excluded=int((~held).sum()))


def _anchor(pop):
    base = pop["base"]
    return Q.rows(base[:, 0:3], base[:, 3:6], 0.0, FLT_MAX), Q.rows(base[:, 0:3], base[:, 3:6], 0.0, np.inf)


@pytest.mark.parametrize("knobs", KNOBS, ids=_knob_id)
@pytest.mark.parametrize("name", Q.POPULATIONS)
def test_population_in_every_shape(srt, gpu, name, knobs):
    pop = Q.population(name, srt)
    scene = _scene(srt, name)
    rays = pop["rays"]
    what = "%s, %s" % (name, _knob_id(knobs))
    with _knobs(gpu, scene, knobs):
        trace = gpu.trace_rays(Q.six(rays))
        for anchor in _anchor(pop):
            got = gpu.intersect(anchor)
            _assert_plan_shape(gpu, False, what)
            assert np.array_equal(bits(got), bits(trace)), "%s: %d words differ from srt_trace_rays over [0, %g]" % (what, (bits(got) != bits(trace)).sum(), anchor[0, 7])
        hits = gpu.intersect(rays)
        _assert_plan_shape(gpu, False, what)
        occ = gpu.occluded(rays)
        _assert_plan_shape(gpu, True, what)
    assert occ.dtype == bool and hits.dtype == np.float32 and hits.shape == (len(rays), 4)
    _assert_exact(rays, hits, occ, what)
    first = G.cached(("query answers", name), lambda: (hits, occ))
    assert np.array_equal(bits(first[0]), bits(hits)) and np.array_equal(first[1], occ), "%s: the answers depend on the shape" % what
    if name in Q.TRUTH_POPULATIONS:
        print(what, _assert_truth(pop, hits, what))


@pytest.mark.parametrize("n", Q.SIZES)
def test_sizes(srt, gpu, n):
    """the first n rays of the soup's population alone: the same words as in the launch of all 4 096 (one partial wave, one wave, one lane
    past a wave, many waves)"""
    pop = Q.population("soup", srt)
    gpu.upload_scene(_scene(srt, "soup"))
    full_h, full_o = gpu.intersect(pop["rays"]), gpu.occluded(pop["rays"])
    r = np.ascontiguousarray(pop["rays"][:n])
    h, o = gpu.intersect(r), gpu.occluded(r)
    assert np.array_equal(bits(h), bits(full_h[:n])) and np.array_equal(o, full_o[:n])
    assert gpu.query_last()["waves"] == (n + 63) // 64      # (never more waves than rays need: whole workgroups of at most 16)


def test_leaf_root(srt, gpu):
    """one triangle: the root is a leaf.  Rays straight down from z = 5 onto it (t = 4.5) and beside it, intervals on either side of 4.5
    and around it"""
    sc = G.scene([[[-1, -1, 0.5], [1, -1, 0.5], [-1, 1, 0.5]]], [G.GREY])
    scene = G.product_scene(srt, sc, srt.BVH_REFERENCE)
    gpu.upload_scene(scene)
    o = np.array([[-0.5, -0.5, 5.0]] * 5 + [[0.9, 0.9, 5.0]], np.float32)
    d = np.array([[0.0, 0.0, -1.0]] * 6, np.float32)
    tmin = np.array([0.0, 0.0, 4.6, 4.0, 0.0, 0.0], np.float32)
    tmax = np.array([FLT_MAX, 4.4, 9.0, 5.0, np.inf, FLT_MAX], np.float32)
    r = Q.rows(o, d, tmin, tmax)
    hits, occ = gpu.intersect(r), gpu.occluded(r)
    assert (hits[:, 1] >= 0).tolist() == [True, False, False, True, True, False] and occ.tolist() == [True, False, False, True, True, False]
    assert (hits[[0, 3, 4], 0] == 4.5).all() and (hits[[0, 3, 4], 1] == 0).all()
    trace = gpu.trace_rays(Q.six(r))
    assert np.array_equal(bits(hits[[0, 4, 5]]), bits(trace[[0, 4, 5]]))
    _assert_exact(r, hits, occ, "leaf root")
    assert gpu.query_last()["any"]


def test_special_inputs(srt, gpu):
    """a NaN direction is a miss; a NaN tmin or tmax, or tmin > tmax, accepts nothing -- on rays that hit over [0, FLT_MAX]"""
    pop = Q.population("soup", srt)
    gpu.upload_scene(_scene(srt, "soup"))
    base = pop["base"]
    full = gpu.intersect(Q.rows(base[:, 0:3], base[:, 3:6], 0.0, FLT_MAX))
    k = np.nonzero(full[:, 1] >= 0)[0][:64]
    nan = np.float32(np.nan)
    r = np.concatenate([
        Q.rows(base[k, 0:3], np.where(np.arange(3) == 1, nan, base[k, 3:6]), 0.0, FLT_MAX),     # NaN direction component
        Q.rows(base[k, 0:3], base[k, 3:6], nan, FLT_MAX),
        Q.rows(base[k, 0:3], base[k, 3:6], 0.0, nan),
        Q.rows(base[k, 0:3], base[k, 3:6], nan, nan),
        Q.rows(base[k, 0:3], base[k, 3:6], full[k, 0] + 1.0, full[k, 0] - 1e-3),                # tmin > tmax around the hit
        Q.rows(base[k, 0:3], base[k, 3:6], FLT_MAX, 0.0),
    ])
    hits, occ = gpu.intersect(r), gpu.occluded(r)
    assert (hits[:, 1] == -1).all() and not occ.any()
    assert (bits(hits[:, [0, 2, 3]]) == 0).all()
    assert np.array_equal(bits(hits[:len(k)]), bits(gpu.trace_rays(Q.six(r[:len(k)]))))


@pytest.mark.parametrize("max_waves", [1, 3])
def test_refill(srt, gpu, max_waves):
    """5 000 rays through one wave and through three: every wave refills many times; the answers are the full grid's"""
    pop = Q.population("soup", srt)
    gpu.upload_scene(_scene(srt, "soup"))
    r = np.concatenate([pop["rays"], pop["rays"][:5000 - len(pop["rays"])]])
    assert len(r) == 5000
    full_h, full_o = gpu.intersect(r), gpu.occluded(r)
    try:
        gpu.set_query_test_grid(max_waves)
        h = gpu.intersect(r)
        assert gpu.query_last()["waves"] == max_waves
        o = gpu.occluded(r)
        assert gpu.query_last()["waves"] == max_waves
    finally:
        gpu.set_query_test_grid(0)
    assert np.array_equal(bits(h), bits(full_h)) and np.array_equal(o, full_o)


def _refit_pair(srt):
    """the soup and a second soup of the same size: the vertices a refit moves the first one's tree to"""
    sc = Q.population("soup", srt)["source"][1]
    v_new = np.ascontiguousarray(G.soup(105, len(sc["V"]), 2.0)["V"], np.float32)
    return sc, v_new


def test_refit(srt, gpu):
    """after a device refit, both queries answer as a context that uploaded the host-refitted scene"""
    torch = pytest.importorskip("torch")
    pop = Q.population("soup", srt)
    sc, v_new = _refit_pair(srt)
    scene = G.product_scene(srt, sc, srt.BVH_SAH)
    gpu.upload_scene(scene)
    gpu.refit(torch.from_numpy(v_new).to("cuda:%d" % gpu.device))
    h, o = gpu.intersect(pop["rays"]), gpu.occluded(pop["rays"])
    scene.refit(v_new)
    other = srt.Renderer(gpu.device)
    try:
        other.upload_scene(scene)
        want_h, want_o = other.intersect(pop["rays"]), other.occluded(pop["rays"])
    finally:
        other.close()
    assert np.array_equal(bits(h), bits(want_h)) and np.array_equal(o, want_o)
    assert (h[:, 1] >= 0).any()


def test_torch_entries(srt, gpu):
    """the device entries equal the host entries; on a non-blocking stream without a synchronisation a query issued after a refit sees the
    refit, and one issued before a refit sees the old tree"""
    torch = pytest.importorskip("torch")
    pop = Q.population("soup", srt)
    sc, v_new = _refit_pair(srt)
    dev = torch.device("cuda:%d" % gpu.device)
    gpu.upload_scene(G.product_scene(srt, sc, srt.BVH_SAH))
    rays = pop["rays"]
    old_h, old_o = gpu.intersect(rays), gpu.occluded(rays)
    rt = torch.from_numpy(rays).to(dev)
    torch.cuda.synchronize(dev)
    h, o = gpu.intersect(rt), gpu.occluded(rt)
    assert isinstance(h, torch.Tensor) and h.dtype == torch.float32 and o.dtype == torch.bool
    assert np.array_equal(bits(h.cpu().numpy()), bits(old_h)) and np.array_equal(o.cpu().numpy(), old_o)
    # before a refit: enqueued on a non-blocking stream, then the refit on the NULL stream, then the stream is waited for
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        h_before, o_before = gpu.intersect(rt), gpu.occluded(rt)
    gpu.refit(v_new)
    s.synchronize()
    assert np.array_equal(bits(h_before.cpu().numpy()), bits(old_h)) and np.array_equal(o_before.cpu().numpy(), old_o)
    # after the refit: the new tree's answers
    new_h, new_o = gpu.intersect(rays), gpu.occluded(rays)
    assert not np.array_equal(bits(new_h), bits(old_h))
    with torch.cuda.stream(s):
        h_after, o_after = gpu.intersect(rt), gpu.occluded(rt)
    s.synchronize()
    assert np.array_equal(bits(h_after.cpu().numpy()), bits(new_h)) and np.array_equal(o_after.cpu().numpy(), new_o)


def test_capi_refusals_write_nothing(srt, gpu):
    """every refusal of the C-ABI returns SRT_ERR_INVALID and leaves the output as it was; n = 0 succeeds and touches nothing"""
    torch = pytest.importorskip("torch")
    B = srt.binding
    L = B.lib()
    u8p = C.POINTER(C.c_uint8)
    pop = Q.population("soup", srt)
    rays = np.ascontiguousarray(pop["rays"][:64])
    sentinel_h = np.full((64, 4), 7.0, np.float32)
    sentinel_o = np.full(64, 7, np.uint8)

    def host(ctx, r, n, h, o):
        return (L.srt_intersect_rays(ctx, r, n, h), L.srt_occluded_rays(ctx, r, n, o))

    fresh = srt.Renderer(gpu.device)      # no scene uploaded
    try:
        h, o = sentinel_h.copy(), sentinel_o.copy()
        assert host(fresh._h, B.fptr(rays), 64, B.fptr(h), o.ctypes.data_as(u8p)) == (-1, -1)
        assert (h == 7.0).all() and (o == 7).all()
    finally:
        fresh.close()
    gpu.upload_scene(_scene(srt, "soup"))
    h, o = sentinel_h.copy(), sentinel_o.copy()
    assert host(gpu._h, None, 64, B.fptr(h), o.ctypes.data_as(u8p)) == (-1, -1)          # null rays
    assert host(gpu._h, B.fptr(rays), 64, None, None) == (-1, -1)                        # null outputs
    assert host(gpu._h, B.fptr(rays), B.QUERY_MAX_RAYS + 1, B.fptr(h), o.ctypes.data_as(u8p)) == (-1, -1)
    assert host(gpu._h, B.fptr(rays), 0, B.fptr(h), o.ctypes.data_as(u8p)) == (0, 0)
    assert host(gpu._h, None, 0, None, None) == (0, 0)
    assert (h == 7.0).all() and (o == 7).all()
    # device entries: misaligned rays, misaligned hits, null pointers, too many rays, n = 0
    dev = torch.device("cuda:%d" % gpu.device)
    rbuf = torch.zeros(64 * 8 + 4, dtype=torch.float32, device=dev)
    rbuf[:64 * 8] = torch.from_numpy(rays.reshape(-1)).to(dev)
    hbuf = torch.full((64 * 4 + 4,), 7.0, dtype=torch.float32, device=dev)
    obuf = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    torch.cuda.synchronize(dev)
    calls = [
        L.srt_intersect_rays_dev(gpu._h, p(rbuf, 4), 64, p(hbuf), None),
        L.srt_intersect_rays_dev(gpu._h, p(rbuf), 64, p(hbuf, 4), None),
        L.srt_occluded_rays_dev(gpu._h, p(rbuf, 8), 64, p(obuf), None),
        L.srt_intersect_rays_dev(gpu._h, None, 64, p(hbuf), None),
        L.srt_occluded_rays_dev(gpu._h, p(rbuf), 64, None, None),
        L.srt_intersect_rays_dev(gpu._h, p(rbuf), B.QUERY_MAX_RAYS + 1, p(hbuf), None),
    ]
    assert calls == [-1] * len(calls)
    assert L.srt_intersect_rays_dev(gpu._h, p(rbuf), 0, p(hbuf), None) == 0 and L.srt_occluded_rays_dev(gpu._h, None, 0, None, None) == 0
    gpu.synchronize()
    assert (hbuf.cpu() == 7.0).all() and (obuf.cpu() == 7).all()
    # (the occluded output needs no alignment: one byte per ray)
    assert L.srt_occluded_rays_dev(gpu._h, p(rbuf), 63, p(obuf, 1), None) == 0      # 63 rays: bytes 1 .. 63 of the 64
    gpu.synchronize()
    ob = obuf.cpu().numpy()
    assert ob[0] == 7 and np.array_equal(ob[1:].astype(bool), gpu.occluded(rays)[:63])
