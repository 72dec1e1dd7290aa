"""Predictions from the state of every path at its end (oracle/srt_oracle.c orc_render_path_ends: the seven wavelengths, the seven
powers and valid_wavelengths that dev_spectrum_to_XYZ receives), shared by test_path_ends.py, test_spectral.py, test_adaptive.py and
test_accum_edge_scenes.py.  The spectral film (render_kernel MODE 5), the XYZ conversion and S2 of adaptive sampling (MODE 4) are
fixed functions of that state, spelled out in include/srt_c_api.h; they are restated here in numpy float32, operation by operation,
from the oracle's words alone -- nothing of the product is used.  Every set of path ends passes a self-check before it is returned:
the X, Y and Z built from it in sample order are the xyz planes of a plain oracle render of the same chunk, bit for bit."""
import ctypes as C

import numpy as np

from accum_helpers import N_GRID, SEED, lane_of, named_workload, shape_case
from helpers import bits, fuzz_with_lens, oracle_scene_for

F = np.float32
N_WL = 7
LAMBDA_MIN, LAMBDA_MAX = F(360.0), F(830.0)


def bits_equal_or_both_nan(a, b):
    """elementwise: same bits, or both NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same_floats(got, want, what):
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~bits_equal_or_both_nan(got, want))
    assert len(bad) == 0, "%s: %d of %d values differ, first at %r: got %r want %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _sample_xyz(orc, wl, power, valid):
    """orc_spectrum_to_XYZ of every path end: (n_pix, n, 3) float32"""
    fn = orc.lib().orc_spectrum_to_XYZ
    n_pix, n = valid.shape
    out = np.zeros((n_pix, n, 3), F)
    wl, power = np.ascontiguousarray(wl, F), np.ascontiguousarray(power, F)
    fp = C.POINTER(C.c_float)
    a, b, o, v = wl.ctypes.data, power.ctypes.data, out.ctypes.data, valid.ravel().tolist()
    for q in range(n_pix * n):
        fn(C.cast(a + 28 * q, fp), C.cast(b + 28 * q, fp), v[q], C.cast(o + 12 * q, fp))
    return out


def path_ends(orc, osc, cam, W, H, n, depth, offx=0, offy=0, seed=SEED, states=None, threads=8):
    """The ends of the n paths of every pixel of a W x H chunk at (offx, offy), row-major:
    dict(W, H, n, wl (W*H, n, 7) float32, power (W*H, n, 7) float32, valid (W*H, n) uint32, xyz (W*H, n, 3) float32: each end through
    orc_spectrum_to_XYZ, render: the oracle's frame of the chunk, lane: block-linear lane of every pixel).  states: (n_lanes, 6) uint32
    XORWOW states to continue from (left untouched) instead of seeding with `seed`.  Self-checked against a plain orc_render."""
    st = lambda: None if states is None else np.ascontiguousarray(states, np.uint32).copy()
    res = osc.render(cam, W, H, n, depth, offx=offx, offy=offy, seed=seed, states=st(), threads=threads, path_ends=True)
    plain = osc.render(cam, W, H, n, depth, offx=offx, offy=offy, seed=seed, states=st(), threads=threads)
    lane = lane_of(res["geom"], W, H)
    words = res.pop("ends")
    outside = np.ones(words.shape[0], bool)
    outside[lane] = False
    assert not words[outside].any(), "lanes outside the chunk were written"
    words = np.ascontiguousarray(words[lane])
    ends = dict(W=W, H=H, n=n, wl=np.ascontiguousarray(words[..., 0:N_WL]).view(F), power=np.ascontiguousarray(words[..., N_WL:2 * N_WL]).view(F),
                valid=np.ascontiguousarray(words[..., 2 * N_WL]), render=res, lane=lane)
    assert ends["valid"].max(initial=0) <= N_WL
    ends["xyz"] = _sample_xyz(orc, ends["wl"], ends["power"], ends["valid"])
    # the self-check: pixel_color = pixel_color + dev_spectrum_to_XYZ(...), sample after sample (render_block_row)
    total = np.zeros((W * H, 3), F)
    for s in range(n):
        total = total + ends["xyz"][:, s]
    assert total.dtype == F
    for k in ("fb", "lin", "xyz"):
        for c in range(3):
            assert np.array_equal(bits(res[k][c]), bits(plain[k][c])), "orc_render_path_ends and orc_render differ in %s plane %d" % (k, c)
    for c in range(3):
        assert_same_floats(total[:, c], plain["xyz"][c][lane], "XYZ plane %d rebuilt from the path ends" % c)
    assert res["stats"] == plain["stats"]
    return ends


def interp_coords(wl):
    """spectrum_interp's coordinates (spectrum.cu:11-22): x = (wl - 360) * (94 / 470); off = clip((int)x, 0, 93); w = x - off"""
    wl = np.asarray(wl, F)
    x = (wl - LAMBDA_MIN) * (F(N_GRID - 1) / (LAMBDA_MAX - LAMBDA_MIN))
    off = np.clip(x.astype(np.int32), 0, N_GRID - 2)
    w = x - off.astype(F)
    assert x.dtype == F and w.dtype == F
    return off, w


def deposit(film, wl, power, valid=None):
    """One sample of every pixel into film (n_pix, 95) float32, in place -- the one statement of the deposit rule of srt_c_api.h:
    p_k = power[k] if k < valid else +0; nothing at all when valid == 0; F[off] = F[off] + (1 - w) * p_k and F[off + 1] = F[off + 1] +
    w * p_k, each product rounded once, k = 0 .. 6 in order.  wl, power: (n_pix, 7); valid: (n_pix,), or None for 7 everywhere."""
    assert film.dtype == F and film.shape[1] == N_GRID
    wl, power = np.asarray(wl, F), np.asarray(power, F)
    n_pix = film.shape[0]
    valid = np.full(n_pix, N_WL, np.uint32) if valid is None else np.asarray(valid)
    rows = np.nonzero(valid > 0)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(N_WL):
            off, w = interp_coords(wl[rows, k])
            p = np.where(k < valid[rows], power[rows, k], F(0.0)).astype(F)
            film[rows, off] = film[rows, off] + (F(1.0) - w) * p
            film[rows, off + 1] = film[rows, off + 1] + w * p
    return film


def predict_film(ends, first=0, count=None):
    """(H, W, 95) float32: the film after samples [first, first + count) of every pixel, added in sample order"""
    W, H, n = ends["W"], ends["H"], ends["n"]
    film = np.zeros((W * H, N_GRID), F)
    for s in range(first, n if count is None else first + count):
        deposit(film, ends["wl"][:, s], ends["power"][:, s], ends["valid"][:, s])
    return film.reshape(H, W, N_GRID)


def predict_y_sums(orc, ends, n=None):
    """(S1, S2) after the first n samples (all of them by default), (W*H,) float32 each: per sample y = orc_spectrum_to_XYZ(...)[1],
    S1 = S1 + y and S2 = S2 + y * y, sequentially in float32 (srt_read_accum_stats' sum_y and sum_y2)"""
    xyz = ends["xyz"] if "xyz" in ends else _sample_xyz(orc, ends["wl"], ends["power"], ends["valid"])
    n = ends["n"] if n is None else n
    assert 0 <= n <= ends["n"]
    s1, s2 = np.zeros(xyz.shape[0], F), np.zeros(xyz.shape[0], F)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            y = xyz[:, s, 1]
            s1 = s1 + y
            s2 = s2 + y * y
    assert s1.dtype == F and s2.dtype == F
    return s1, s2


def boundary_sums(orc, ends, sched):
    """per pass boundary of the schedule: dict(total, stats = dict(sum_y, sum_y2)) from the path ends alone -- the layout
    accum_helpers.predict_stops and pick_tolerance take in place of a GPU run that never stops"""
    out = []
    for t in np.cumsum(sched):
        s1, s2 = predict_y_sums(orc, ends, int(t))
        out.append(dict(total=int(t), stats=dict(sum_y=s1, sum_y2=s2)))
    return out


def assert_sums_at_counts(stats, oracle, what):
    """every pixel's S1 and S2 (srt_read_accum_stats) are the oracle's after as many samples as the pixel has taken; oracle: boundary_sums"""
    counts = stats["samples"]
    assert np.isin(counts, [o["total"] for o in oracle]).all(), np.unique(counts)
    for key in ("sum_y", "sum_y2"):
        want = np.zeros(counts.size, F)
        for o in oracle:
            at = counts == o["total"]
            want[at] = o["stats"][key][at]
        assert_same_floats(stats[key], want, "%s %s" % (what, key))


# ---- what a set of path ends covers (asserted from the oracle alone, before any GPU run) ---------------------------------------------
def coverage(ends, background):
    """dict of the path ends' kinds.  Under an all-zero background a miss leaves +0 in every valid power, so there a path end with a
    non-zero valid power ended on a hit without a scattered ray (an emitter); `hit_off` are the grid offsets such ends deposit to with
    a non-zero power (empty under any other background, where a miss cannot be told from a hit by the end's words)."""
    valid, power = ends["valid"], ends["power"]
    live = np.arange(N_WL) < valid[..., None]
    nonzero = live & (power != 0)
    off, _ = interp_coords(ends["wl"])
    black = not np.asarray(background).any()
    hit_ended = nonzero.any(axis=-1) if black else np.zeros(valid.shape, bool)
    return dict(valid=set(np.unique(valid).tolist()), hit_ended=int(hit_ended.sum()),
                powers_other_than_one=int((live & (power != 1)).sum()),
                hit_off=set(np.unique(off[nonzero & hit_ended[..., None]]).tolist()),
                bins=predict_film(ends).reshape(-1, N_GRID).max(axis=0) > 0)


# ---- one prediction per workload --------------------------------------------------------------------------------------------------
_cache = {}


def cached_ends(orc, key, osc_of, cam, W, H, n, depth, **kw):
    """path_ends computed once per key, with its film after all n samples as ends["film"]; osc_of() makes the oracle scene"""
    if key not in _cache:
        osc = osc_of()
        ends = path_ends(orc, osc, cam, W, H, n, depth, **kw)
        osc.close()
        ends["film"] = predict_film(ends)
        _cache[key] = ends
    return _cache[key]


# ---- the workloads of the film tests ---------------------------------------------------------------------------------------------------
FILM_WORKLOADS = ("prism", "cornell", "dielectric", "random_spheres", "fuzz_with_lens", "prism_depth_1")
FILM_SPP = 6


def film_workload(srt, name):
    """(scene, cam, W, H, n, depth, builder mode): named_workload's sizes at FILM_SPP samples, the lens fuzz case at its own size and
    count, and prism with bounce_limit 1 (every path that scatters once ends at the limit, valid == 0)"""
    if name == "fuzz_with_lens":
        scene, cam, W, H, spp, depth, mode = fuzz_with_lens(srt)
        return scene, cam, W, H, min(spp, FILM_SPP), depth, mode
    scene, cam, W, H, depth, mode = named_workload(srt, "prism" if name == "prism_depth_1" else name)
    return scene, cam, W, H, FILM_SPP, (1 if name == "prism_depth_1" else depth), mode


def workload_ends(srt, orc, name):
    """(workload, its path ends with ends["film"]), computed once per name"""
    wl = film_workload(srt, name)
    scene, cam, W, H, n, depth, mode = wl
    return wl, cached_ends(orc, ("workload", name), lambda: oracle_scene_for(orc, scene, mode), cam, W, H, n, depth)


def shape_ends(srt, orc, paired, n):
    """(shape_case(paired), its path ends) computed once per (paired, n)"""
    case = shape_case(srt, paired)
    scene, cam, W, H, depth = case
    return case, cached_ends(orc, ("shape", paired, n), lambda: oracle_scene_for(orc, scene, 1), cam, W, H, n, depth)


def assert_film_coverage(srt, orc):
    """What the film tests rely on, from the oracle alone: over FILM_WORKLOADS together there are path ends with valid == 7, == 1 and
    == 0, paths that ended on a hit without a scattered ray with non-zero power, powers other than 1, deposits of such hit-ended
    paths into the first bin pair (off == 0) and the clamped last one (off == 93), and on one workload a non-zero sum in every bin."""
    seen = dict(valid=set(), hit_ended=0, powers_other_than_one=0, hit_off=set(), every_bin=[])
    for name in FILM_WORKLOADS:
        (scene, *_), ends = workload_ends(srt, orc, name)
        if "coverage" not in ends:
            ends["coverage"] = coverage(ends, scene.background())
        c = ends["coverage"]
        seen["valid"] |= c["valid"]; seen["hit_off"] |= c["hit_off"]
        seen["hit_ended"] += c["hit_ended"]; seen["powers_other_than_one"] += c["powers_other_than_one"]
        if c["bins"].all():
            seen["every_bin"].append(name)
    assert {0, 1, 7} <= seen["valid"], seen["valid"]
    assert seen["hit_ended"] > 0 and seen["powers_other_than_one"] > 0, seen
    assert 0 in seen["hit_off"] and N_GRID - 2 in seen["hit_off"], sorted(seen["hit_off"])
    assert seen["every_bin"], "no workload with a non-zero sum in every bin"
    return seen
