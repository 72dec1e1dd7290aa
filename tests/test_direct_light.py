"""The deferred direct-light pass on the device (srt_direct_light*; include/srt_c_api.h "Direct lighting").

Bit identity: the device equals tests/direct_light_reference.py in every bit of sum and m2, in every counter and, through the KAT entry, in
every intermediate row; the restatement's two queries are Renderer.intersect / occluded on its own rows.  On the truth scenes of
tests/direct_light_cases.py, scene 0 (CORNELL), scene TRIS and RANDOM_SPHERES (a lens, a sky, metals and glass together); rectangles 1 x 1,
67 x 35 and an offset chunk; under every knob set of tests/test_query.py; with rounds forced small; with first_sample; with single parts.
The light table with its slots, on 37 lights with pinned ones (many_lights) and on two emitters whose slot order is not their material order.
Truth: the conditions of tests/direct_light_cases.py on the device's output, no restatement in between.  test_fixed_draw: the two committed
draws of many_lights, a pinned light's single value and a wide light's first value, through the KAT entry.  test_black_sky: SKY asked for
under a black background.  test_lens_rows_hold_to_geometry: the device's own camera rows under a thin lens, held to the disk and the footprint.
State: a call between two passes of a bound accumulation changes nothing; after a refit SKY follows the refitted geometry and LIGHTS is
refused; every other refusal.
End to end: CORNELL against the product's own path tracer at bounce_limit = 2 (test_path_tracer_agrees)."""
import ctypes as C

import numpy as np
import pytest

import direct_light_cases as DC
import direct_light_reference as R
import ground_truth as G
from helpers import bits
from test_traversal_limits import KNOBS, _knob_id, _knobs

pytestmark = pytest.mark.gpu

SEED = 0x5eed0123456789ab
BUILTIN = {"cornell": "SCENE_CORNELL", "tris": "SCENE_TRIS", "random_spheres": "SCENE_RANDOM_SPHERES"}
IDENTITY_SCENES = DC.NAMES + tuple(BUILTIN)


def _case(srt, name, W=64, H=48):
    """dict(scene, desc, cam, W, H) of a truth scene or a built-in scene at its default view"""
    if name in DC.NAMES:
        return DC.case(srt, name)

    def make():
        scene = srt.Scene.builtin(getattr(srt, BUILTIN[name])).build_bvh(srt.BVH_REFERENCE, 1984)
        return dict(scene=scene, desc=R.describe(srt, scene), cam=scene.default_camera(W, H), W=W, H=H)
    return G.cached(("direct light builtin", name, W, H), make)


def _lit_sky_case(srt):
    """the occluded light under a grey sky: LIGHTS and SKY both have work"""
    def make():
        sc, camera, W, H = DC._scene("occluded_light")
        sc["background"] = DC.GREY_SKY
        scene = G.product_scene(srt, sc, srt.BVH_SAH)
        return dict(scene=scene, desc=R.describe(srt, scene), cam=G.camera(srt, camera, W, H), W=W, H=H)
    return G.cached(("direct light case", "lit sky"), make)


def _setup(gpu, c):
    gpu.upload_scene(c["scene"])
    gpu.set_camera(c["cam"])


def _restate(gpu, c, w, h, ox=0, oy=0, **kw):
    return R.run(c["desc"], c["cam"], w, h, ox, oy, gpu.intersect, gpu.occluded, **kw)


def _assert_same(got, want, what):
    for k in ("sum", "m2"):
        a, b = bits(got[k]), bits(want[k])
        assert np.array_equal(a, b), "%s: %d words of %s differ, first at %r: %r / %r" % (
            what, (a != b).sum(), k, tuple(np.argwhere(a != b)[0]), got[k][tuple(np.argwhere(a != b)[0])], want[k][tuple(np.argwhere(a != b)[0])])
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_bit_identity(srt, gpu, name):
    c = _case(srt, name)
    _setup(gpu, c)
    got = gpu.direct_light(c["W"], c["H"], samples=4, seed=SEED)
    want = _restate(gpu, c, c["W"], c["H"], samples=4, seed=SEED)
    _assert_same(got, want, name)
    st = got["stats"]
    assert st["miss"] + st["emitted"] + st["specular"] + st["shaded"] == 4 * c["W"] * c["H"]
    assert (st["shaded"] > 0) != (name == "emitters_in_view")          # (that one looks up from under the floor's lights: nothing is shaded)
    assert np.array_equal(bits(got["mean"]), bits(got["sum"] / np.float32(4)))
    # the light table, bit for bit
    tab, dev = want["tab"], gpu.light_table()
    assert np.array_equal(dev["thresholds"], tab["thresholds"]) and st["lights"] == len(tab["area"])
    for k in ("v0", "e1", "e2", "normal", "area"):
        assert np.array_equal(bits(dev[k]), bits(tab[k])), (name, k)
    assert np.array_equal(dev["mat"], tab["mat"]) and np.array_equal(dev["tri"], tab["tri"])
    first = list(dict.fromkeys(tab["mat"].tolist()))          # slots number the emissive materials by their first light
    assert dev["slot"].tolist() == [first.index(m) for m in tab["mat"].tolist()], (name, dev["slot"])
    # one round of sample 2 through the KAT entry: every intermediate row
    kat = gpu.direct_light_kat(c["W"], c["H"], sample=2, seed=SEED)
    ref = _restate(gpu, c, c["W"], c["H"], samples=1, first_sample=2, seed=SEED, keep=True)
    _assert_same(kat, ref, name + " (kat)")
    for k in ("cam_rows", "hit_rows", "light_rows", "sky_rows"):
        assert np.array_equal(bits(kat[k]), bits(ref["rounds"][0][k])), (name, k, int((bits(kat[k]) != bits(ref["rounds"][0][k])).sum()))
    assert np.array_equal(kat["records"], ref["rounds"][0]["records"]), (name, "records")
    assert np.array_equal(kat["occ_light"], ref["rounds"][0]["occ_light"]) and np.array_equal(kat["occ_sky"], ref["rounds"][0]["occ_sky"])
    print(name, st, gpu.direct_light_last())


@pytest.mark.parametrize("rect", [(1, 1, 40, 30), (67, 35, 0, 0), (67, 35, 29, 29), (23, 17, 70, 41)], ids=lambda r: "%dx%d+%d+%d" % r)
def test_rectangles(srt, gpu, rect):
    """any rectangle of the 96 x 64 image: the restatement's, and the same pixels' words of the whole image"""
    c = _case(srt, "cornell", 96, 64)
    _setup(gpu, c)
    w, h, ox, oy = rect
    got = gpu.direct_light(w, h, ox, oy, samples=3, seed=SEED)
    _assert_same(got, _restate(gpu, c, w, h, ox, oy, samples=3, seed=SEED), str(rect))
    whole = G.cached(("direct light whole image",), lambda: gpu.direct_light(96, 64, samples=3, seed=SEED))
    assert np.array_equal(bits(got["sum"]), bits(whole["sum"][oy:oy + h, ox:ox + w])) and np.array_equal(bits(got["m2"]), bits(whole["m2"][oy:oy + h, ox:ox + w]))


@pytest.mark.parametrize("knobs", KNOBS, ids=_knob_id)
@pytest.mark.parametrize("name", ["cornell", "occluded_light"])
def test_every_knob_set(srt, gpu, name, knobs):
    c = _case(srt, name)
    with _knobs(gpu, c["scene"], knobs):
        gpu.set_camera(c["cam"])
        got = gpu.direct_light(c["W"], c["H"], samples=2, seed=SEED)
        _assert_same(got, _restate(gpu, c, c["W"], c["H"], samples=2, seed=SEED), "%s, %s" % (name, _knob_id(knobs)))
        plan, q = gpu.launch_plan(), gpu.query_last()
        assert (q["narrow_refs"], q["all_cached"], q["paired"]) == (plan["narrow_refs"], plan["all_cached"], plan["paired"])
    first = G.cached(("direct light knobs", name), lambda: got)
    _assert_same(got, first, "%s: the answers depend on the shape (%s)" % (name, _knob_id(knobs)))


@pytest.mark.parametrize("max_rows,rounds,per_round", [(64, 5, 1), (4097, 5, 1), (5000, 3, 2)])
def test_round_size(srt, gpu, max_rows, rounds, per_round):
    """67 x 35 = 2 345 pixels, 5 samples: rounds of one sample (64 and 4 097 rows allowed) and of two (5 000) against one round of five"""
    c = _case(srt, "cornell", 96, 64)
    _setup(gpu, c)
    free = gpu.direct_light(67, 35, 13, 7, samples=5, seed=SEED)
    assert gpu.direct_light_last()["rounds"] == 1
    try:
        gpu.set_light_test_batch(max_rows)
        forced = gpu.direct_light(67, 35, 13, 7, samples=5, seed=SEED)
        info = gpu.direct_light_last()
    finally:
        gpu.set_light_test_batch(0)
    assert info["rounds"] == rounds and info["rows_per_round"] == 2345 * per_round
    _assert_same(forced, free, "rounds of %d rows" % max_rows)


def test_first_sample_halves(srt, gpu):
    c = _lit_sky_case(srt)
    _setup(gpu, c)
    for first in (0, 3):
        got = gpu.direct_light(c["W"], c["H"], samples=3, first_sample=first, seed=SEED)
        _assert_same(got, _restate(gpu, c, c["W"], c["H"], samples=3, first_sample=first, seed=SEED), "first_sample %d" % first)
    a, b = gpu.direct_light(c["W"], c["H"], samples=3, seed=SEED), gpu.direct_light(c["W"], c["H"], samples=3, first_sample=3, seed=SEED)
    assert not np.array_equal(a["sum"], b["sum"])
    whole = gpu.direct_light(c["W"], c["H"], samples=6, seed=SEED)
    assert all(a["stats"][k] + b["stats"][k] == whole["stats"][k] for k in R.COUNTERS)


def test_parts_alone_draw_the_combined_call_s_numbers(srt, gpu):
    c = _lit_sky_case(srt)
    _setup(gpu, c)
    both = gpu.direct_light_kat(c["W"], c["H"], sample=1, seed=SEED)
    assert both["stats"]["light_rows"] > 0 and both["stats"]["sky_rows"] > 0 and 0 < both["stats"]["light_unoccluded"] < both["stats"]["light_rows"]
    for part, rows, occ in (("lights", "light_rows", "occ_light"), ("sky", "sky_rows", "occ_sky")):
        alone = gpu.direct_light_kat(c["W"], c["H"], sample=1, seed=SEED, parts=(part,))
        assert np.array_equal(bits(alone[rows]), bits(both[rows])) and np.array_equal(alone[occ], both[occ]), part
        other = "sky_rows" if part == "lights" else "light_rows"
        assert not alone[other].any()
        _assert_same(alone, _restate(gpu, c, c["W"], c["H"], samples=1, first_sample=1, seed=SEED, parts=(part,)), part + " alone")
    emitted = gpu.direct_light(c["W"], c["H"], samples=2, seed=SEED, parts=("emitted",))
    _assert_same(emitted, _restate(gpu, c, c["W"], c["H"], samples=2, seed=SEED, parts=("emitted",)), "emitted alone")
    assert emitted["stats"]["light_rows"] == 0 and emitted["stats"]["sky_rows"] == 0


@pytest.mark.parametrize("name", DC.NAMES)
def test_truth_on_the_device(srt, gpu, name):
    """tests/direct_light_cases.py's conditions on the device's own sums"""
    c = DC.case(srt, name)
    _setup(gpu, c)
    out = gpu.direct_light(c["W"], c["H"], samples=c["samples"], seed=SEED, parts=c["parts"])
    if name in DC.ALL_HELD:          # every camera ray meets the floor, under a lens too, and nothing stands between the floor and its lights
        n = c["W"] * c["H"] * c["samples"]
        assert out["stats"]["shaded"] == out["stats"]["light_rows"] == out["stats"]["light_unoccluded"] == n, (name, out["stats"])
    print(name, out["stats"], DC.assert_holds(name, DC.expectation(srt, name), out["sum"], out["m2"], c["samples"], c["W"], c["H"], "device"),
          gpu.direct_light_last())


@pytest.mark.parametrize("which", ["pinned", "edge"])
def test_fixed_draw(srt, gpu, which):
    """many_lights' two committed draws (tests/test_direct_light_reference.py re-derives them) through the KAT entry on their 1 x 1
    rectangle: "pinned" draws thresholds[a] of a light of width 1, "edge" thresholds[m] of a wider one.  The device picks that light,
    traces the row, equals the restatement in every bit, and its weight is the float64 one within DC.assert_weight_holds' bound."""
    c = DC.case(srt, "many_lights")
    _setup(gpu, c)
    (x, y), s = DC.DRAW_PIXEL, DC.DRAW_S[which]
    kat = gpu.direct_light_kat(1, 1, x, y, sample=s, seed=DC.DRAW_SEED, parts=("lights",))
    ref = _restate(gpu, c, 1, 1, x, y, samples=1, first_sample=s, seed=DC.DRAW_SEED, parts=("lights",), keep=True)
    tab = ref["tab"]
    k = int(R.philox(np.array([y * c["W"] + x], np.uint32), np.uint32(s), 2, 0, *R.seed_key(DC.DRAW_SEED))[0][0] >> np.uint32(8))
    a = int(np.nonzero(tab["thresholds"] == k)[0][0])
    width = int(tab["thresholds"][a + 1]) - int(tab["thresholds"][a])
    assert width == 1 if which == "pinned" else (width > 1 and a > 0), (which, a, width)
    assert np.array_equal(gpu.light_table()["thresholds"], tab["thresholds"])
    _assert_same(kat, ref, which + " draw")
    assert np.array_equal(kat["records"], ref["rounds"][0]["records"]) and np.array_equal(bits(kat["light_rows"]), bits(ref["rounds"][0]["light_rows"]))
    assert kat["stats"]["light_rows"] == 1
    print(which, "light %d of width %d, draw %d; weight off by %.3g, allowed %.3g" % (
        (a, width, k) + DC.assert_weight_holds(tab, kat["records"][0], kat["light_rows"][0], a, which + " on the device")))


def test_black_sky(srt, gpu):
    """cosine_law's background is black.  SKY alone: the sums are 0, no sky row is made and every round launches the closest query alone;
    LIGHTS with SKY is LIGHTS alone in every bit and counter.  All of it is the restatement's as well."""
    c = DC.case(srt, "cosine_law")
    _setup(gpu, c)
    W, H = c["W"], c["H"]
    try:
        gpu.set_light_test_batch(W * H)          # rounds of one sample: three rounds
        sky = gpu.direct_light(W, H, samples=3, seed=SEED, parts=("sky",))
        info = gpu.direct_light_last()
    finally:
        gpu.set_light_test_batch(0)
    assert not sky["sum"].any() and not sky["m2"].any() and sky["stats"]["sky_rows"] == 0 and sky["stats"]["shaded"] == 3 * W * H
    assert info["rounds"] == 3 and info["query_launches"] == info["rounds"], info
    _assert_same(sky, _restate(gpu, c, W, H, samples=3, seed=SEED, parts=("sky",)), "sky alone under a black sky")
    kat = gpu.direct_light_kat(W, H, sample=1, seed=SEED, parts=("sky",))
    assert not kat["sky_rows"].any() and not kat["occ_sky"].any() and not (kat["records"][:, 3] & R.ROW_SKY).any()
    both, lights = gpu.direct_light(W, H, samples=3, seed=SEED, parts=("lights", "sky")), gpu.direct_light(W, H, samples=3, seed=SEED, parts=("lights",))
    assert gpu.direct_light_last()["query_launches"] == 2 * gpu.direct_light_last()["rounds"]
    _assert_same(both, lights, "lights with a black sky")
    _assert_same(both, _restate(gpu, c, W, H, samples=3, seed=SEED, parts=("lights", "sky")), "lights and sky under a black sky")
    assert lights["stats"]["light_unoccluded"] > 0 and lights["sum"].any()


@pytest.mark.parametrize("name", DC.LENS_CAMERAS)
def test_lens_rows_hold_to_geometry(srt, gpu, name):
    """the device's own camera rows of samples 0 .. 3 under a thin lens, through the KAT entry, held to the geometry
    DC.assert_lens_rows_hold states: no restatement in between"""
    c = _case(srt, name)
    _setup(gpu, c)
    assert c["cam"].defocus_angle > 0
    rows = np.stack([gpu.direct_light_kat(c["W"], c["H"], sample=s, seed=SEED, parts=("emitted",))["cam_rows"] for s in range(4)])
    print(name, DC.assert_lens_rows_hold(c["cam"], c["W"], c["H"], rows, name + " on the device"))


def test_a_call_moves_no_state(srt, gpu):
    """two passes of a bound accumulation with a direct-light call between them: the second pass is the one without the call"""
    c = _case(srt, "cornell")
    W, H = c["W"], c["H"]

    def passes(with_call):
        _setup(gpu, c)
        gpu.init_device_params(W, H, 4, 4, 77)
        gpu.set_partition(0, 1)
        gpu.accum_reset()
        gpu.render_chunk_accum(W, H, 2)
        if with_call:
            gpu.direct_light(W, H, samples=2, seed=SEED)
            gpu.direct_light_kat(W - 3, H - 5, 1, 2, sample=1, seed=SEED)
        gpu.render_chunk_accum(W, H, 2)
        gpu.scatter_tiles()
        return [np.array(p) for p in gpu.read_fb_aux(2)] + [np.array(p) for p in gpu.read_fb()], gpu.accum_samples

    plain, with_call = passes(False), passes(True)
    assert plain[1] == with_call[1] == 4
    for k, (a, b) in enumerate(zip(plain[0], with_call[0])):
        assert np.array_equal(bits(a), bits(b)), "plane %d differs after a direct-light call" % k


def test_refit(srt, gpu):
    """after a device refit SKY and EMITTED follow the refitted geometry, LIGHTS is refused with SRT_ERR_UNSUPPORTED; a new upload lifts it"""
    sc, camera, W, H = DC._scene("occluded_light")
    sc["background"] = DC.GREY_SKY
    scene = G.product_scene(srt, sc, srt.BVH_SAH)
    cam = G.camera(srt, camera, W, H)
    gpu.upload_scene(scene)
    gpu.set_camera(cam)
    before = gpu.direct_light(W, H, samples=2, seed=SEED)
    v_new = scene.vertices().copy()
    v_new[3:5, :, 1] -= np.float32(0.25)          # the blocker comes down
    v_new[3:5, :, 0] += np.float32(0.5)
    gpu.refit(v_new)
    with pytest.raises(srt.SrtError) as e:
        gpu.direct_light(W, H, samples=2, seed=SEED)
    assert e.value.code == -5 and "refitted" in str(e.value)
    with pytest.raises(srt.SrtError) as e:
        gpu.direct_light(W, H, samples=2, seed=SEED, parts=("lights",))
    assert e.value.code == -5
    got = gpu.direct_light(W, H, samples=2, seed=SEED, parts=("emitted", "sky"))
    scene.refit(v_new)
    c = dict(desc=R.describe(srt, scene), cam=cam)
    _assert_same(got, _restate(gpu, c, W, H, samples=2, seed=SEED, parts=("emitted", "sky")), "sky after a refit")
    gpu.upload_scene(scene)
    after = gpu.direct_light(W, H, samples=2, seed=SEED)
    _assert_same(after, _restate(gpu, c, W, H, samples=2, seed=SEED), "a new upload of the refitted scene")
    assert not np.array_equal(after["sum"], before["sum"])


def test_refusals_write_nothing(srt, gpu):
    B = srt.binding
    L = B.lib()
    c = _case(srt, "cornell")
    W, H = c["W"], c["H"]
    out, m2, res = np.full((H, W, 3), 7.0, np.float32), np.full((H, W, 3), 7.0, np.float32), B.LightResult()
    res.shaded = 99

    def call(ctx, cfg, w=W, h=H, ox=0, oy=0, s=out):
        return L.srt_direct_light(ctx, C.byref(cfg) if cfg is not None else None, B.fptr(s) if s is not None else None, B.fptr(m2), C.byref(res), w, h, ox, oy)

    good = srt.direct_light_config(samples=2)
    fresh = srt.Renderer(gpu.device)
    try:
        assert call(fresh._h, good) == -1 and b"no scene" in L.srt_last_error(fresh._h)
        fresh.upload_scene(c["scene"])
        assert call(fresh._h, good) == -1 and b"no camera" in L.srt_last_error(fresh._h)
        n = C.c_uint32(0)
        assert L.srt_direct_light_last(fresh._h, C.byref(B.LightInfo())) == -1
    finally:
        fresh.close()
    _setup(gpu, c)
    bad_cfgs = [B.Light(samples=0, parts=7), B.Light(samples=65537, parts=7), B.Light(samples=2, parts=0), B.Light(samples=2, parts=8),
                B.Light(samples=2, parts=7, first_sample=2 ** 32 - 1)]
    assert [call(gpu._h, cfg) for cfg in bad_cfgs] == [-1] * len(bad_cfgs)
    assert call(gpu._h, None) == -1 and call(gpu._h, good, s=None) == -1
    assert [call(gpu._h, good, *r) for r in ((0, H), (W, 0), (W + 1, H), (W, H + 1), (W, H, 1, 0), (W, H, 0, 1), (1, 1, W, 0))] == [-1] * 7
    kat = lambda cfg: L.srt_direct_light_kat(gpu._h, C.byref(cfg), B.fptr(out), B.fptr(m2), C.byref(res), W, H, 0, 0, None, None, None, None, None, None, None)
    assert kat(good) == -1 and kat(srt.direct_light_config(samples=1)) == 0
    assert (m2 == 7.0).sum() == 0          # (the one call that ran wrote its outputs)
    out[:] = 7.0; m2[:] = 7.0; res.shaded = 99
    assert call(gpu._h, bad_cfgs[2]) == -1 and (out == 7.0).all() and (m2 == 7.0).all() and res.shaded == 99
    n = C.c_uint32(0)
    assert L.srt_read_light_table(gpu._h, C.byref(n), None, None, 0) == 0 and n.value >= 1
    th = np.zeros(n.value + 1, np.uint32)
    assert L.srt_read_light_table(gpu._h, C.byref(n), th.ctypes.data_as(C.POINTER(C.c_uint32)), None, n.value - 1) == -1 and not th.any()


def test_path_tracer_agrees(srt, gpu):
    """CORNELL, 64 x 48: the product's path tracer at bounce_limit = 2 -- an adaptive accumulation with rel_tol = 0, which keeps S2 -- at
    1 024 spp against the pass at S = 64.  Per 8 x 8 tile without a specular sample: z = (Y_pt - Y_direct) / sqrt(Var_pt + Var_direct), the
    tile's Y the sum of its pixels' mean luminance, the variances from S2 and m2.  |z| <= Z_IMG_MAX in every tile, and the rms of the N
    scores within 1 +- 4 / sqrt(2 N): four standard deviations of the rms of N unit normals, not a measurement.

    One mend of the statistic, so that every tile stays in: S2 knows only the paths that arrived.  On the ceiling beside the light, which
    lies one unit under it, a path reaches the light with probability 6e-6; a tile's 65 536 paths then bring 0 or 1 arrivals, S2 says
    "variance 0", and z is a division by the direct pass's small variance alone (measured before the mend: z = -48.7 and -44.6 in two such
    tiles, PT 0.1228 / 0 against direct 0.1413 / 0.0028).  A count that came out k has the variance of k + 1 arrivals at least, so the path
    tracer's variance gets one more arrival of the largest expected size, (max T_light.y / spp)^2 per tile: a 1 / k of the variance where
    k arrivals came, all of it where none did."""
    c = _case(srt, "cornell")
    W, H, S, SPP = c["W"], c["H"], 64, 1024
    _setup(gpu, c)
    direct = gpu.direct_light(W, H, samples=S, seed=SEED)
    specular = np.zeros((H, W), bool)
    if direct["stats"]["specular"]:
        for s in range(8):
            specular |= ((gpu.direct_light_kat(W, H, sample=s, seed=SEED)["records"][:, 3] & 3) == R.SPECULAR).reshape(H, W)
    gpu.init_device_params(W, H, SPP, 2, 4242)
    gpu.set_partition(0, 1)
    gpu.accum_reset_adaptive(0.0, 1e-30, SPP)      # rel_tol = 0 (abs_tol^2 underflows to 0: the two must not both be 0): no pixel stops early
    gpu.render_chunk_accum(W, H, SPP)
    st = gpu.accum_stats(W, H)
    n = st["samples"].reshape(H, W).astype(np.float64)
    assert n.min() == n.max() == SPP
    y_pt = st["sum_y"].reshape(H, W).astype(np.float64) / n
    var_pt = np.maximum(st["sum_y2"].reshape(H, W).astype(np.float64) / n - y_pt ** 2, 0.0) * n / (n - 1) / n
    y_d = direct["sum"][:, :, 1].astype(np.float64) / S
    var_d = np.maximum(direct["m2"][:, :, 1].astype(np.float64) / S - y_d ** 2, 0.0) * S / (S - 1) / S
    tiles = lambda a: a.reshape(H // 8, 8, W // 8, 8).sum((1, 3)).ravel()
    one_arrival = (float(R.tables(c["desc"])["t_light"][:, :, 1].max()) / SPP) ** 2
    keep = (tiles(specular.astype(np.float64)) == 0) & (tiles(var_pt) + tiles(var_d) > 0)
    z = (tiles(y_pt) - tiles(y_d))[keep] / np.sqrt((tiles(var_pt) + one_arrival + tiles(var_d))[keep])
    N = int(keep.sum())
    rms = float(np.sqrt((z * z).mean()))
    print("path tracer vs direct: %d tiles, max |z| %.2f, rms %.3f (allowed 1 +- %.3f); relative noise per tile pt %.3g direct %.3g" % (
        N, np.abs(z).max(), rms, 4 / np.sqrt(2 * N), np.median(np.sqrt(tiles(var_pt)[keep]) / np.maximum(tiles(y_pt)[keep], 1e-30)),
        np.median(np.sqrt(tiles(var_d)[keep]) / tiles(y_d)[keep])))
    assert N >= 24
    assert np.abs(z).max() <= G.Z_IMG_MAX, (N, float(np.abs(z).max()))
    assert abs(rms - 1.0) <= 4 / np.sqrt(2 * N), (N, rms)
