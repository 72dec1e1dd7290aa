"""The adversarial scenes of the parity suite -- a leaf root, a two-leaf tree, NaN normals, unknown material types, forty materials
(helpers.edge_case_scene) -- and the fuzz scenes 0 to 5 through the accumulating instantiations of render_kernel, which have their own
register allocation and their own use of the LDS uniform block (MODE 7 reuses the pointer slots of the film and of the S2 plane):
plain accumulation (MODE 3), adaptive (MODE 4), the spectral film (MODE 5), two streams (MODE 6) and the feature buffers (MODE 7),
each bit for bit against the CPU oracle or a prediction built from it."""
import numpy as np
import pytest

from accum_helpers import (SEED, adaptive_run, assert_same_image, fresh_context, lane_of, predict_stops, read_frame, spectral_run,
                           stream_prediction)
from features_reference import predict_features, stack_features
from helpers import EDGE_CASES, assert_planes_equal, bits, edge_case_scene, fuzz_case, oracle_scene_for
from path_ends_reference import assert_same_floats, assert_sums_at_counts, boundary_sums, cached_ends

CASES = EDGE_CASES + ["fuzz_seed_%d" % s for s in range(6)]
SEES_SOMETHING = [c for c in EDGE_CASES if c != "degenerate_and_odd_materials"]      # (the degenerate scene may be all dark)
_cases = {}


def _case(srt, orc, name):
    """(scene, cam, W, H, n, depth, builder mode) and the oracle's path ends of the n samples; an edge case at 45 x 37 x 6 spp, a fuzz
    case at its own size, depth and sample count (two at the least: every run here is split into passes)"""
    if name not in _cases:
        if name in EDGE_CASES:
            scene, cam, W, H, n, depth = edge_case_scene(srt, name)
            mode = 0
        else:
            scene, cam, W, H, spp, depth, mode, _ = fuzz_case(srt, int(name.rsplit("_", 1)[1]))
            n = max(spp, 2)
        assert n <= 6
        _cases[name] = (scene, cam, W, H, n, depth, mode)
    wl = _cases[name]
    scene, cam, W, H, n, depth, mode = wl
    return wl, cached_ends(orc, ("edge", name), lambda: oracle_scene_for(orc, scene, mode), cam, W, H, n, depth)


def _assert_sees_something(name, frame):
    if name in SEES_SOMETHING:
        assert max(float(p.max()) for p in frame["xyz"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_plain_accumulation_in_two_passes_equals_the_oracle_frame(srt, gpu, orc, name):
    (scene, cam, W, H, n, depth, _), ends = _case(srt, orc, name)
    fresh_context(gpu, scene, cam, W, H, depth, spp=n)
    gpu.accum_reset()
    for s in (1, n - 1):
        gpu.render_chunk_accum(W, H, s)
    got = read_frame(gpu, W, H)
    for k in ("xyz", "lin", "fb"):
        assert_planes_equal(got[k], ends["render"][k], "%s %s" % (name, k))
    assert gpu.accum_samples == n
    _assert_sees_something(name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_adaptive_equals_the_oracle_frame_of_each_pixels_count(srt, gpu, orc, name):
    """the stop map is the criterion on the oracle's S1 and S2, S1 and S2 are the oracle's at every pixel's count, and the pixels that
    took c samples hold the oracle's c-spp frame"""
    (scene, cam, W, H, n, depth, mode), ends = _case(srt, orc, name)
    sched, rel, ab = [2] + [1] * (n - 2), 0.3, 1e-3
    oracle = boundary_sums(orc, ends, sched)
    maps, _, actives = predict_stops(oracle, rel, ab, min_spp=2)
    run = adaptive_run(gpu, scene, cam, W, H, depth, rel, sched=sched, min_spp=2, abs_tol=ab)
    for p, want, act in zip(run, maps, actives):
        assert np.array_equal(p["stats"]["samples"], want), "%s after %d: %d pixels differ" % (name, p["total"], int((p["stats"]["samples"] != want).sum()))
        assert p["active"] == act, (name, p["total"], p["active"], act)
    last = run[-1]
    assert_sums_at_counts(last["stats"], oracle, name)
    counts, lane = last["stats"]["samples"], lane_of(gpu.geom, W, H)
    osc = oracle_scene_for(orc, scene, mode)
    for c in np.unique(counts):
        ref = ends["render"] if c == n else osc.render(cam, W, H, int(c), depth)
        at = lane[counts == c]
        for k in ("xyz", "lin", "fb"):
            for q in range(3):
                assert np.array_equal(bits(last["frame"][k][q])[at], bits(ref[k][q])[at]), (name, int(c), k, q)
    osc.close()
    _assert_sees_something(name, last["frame"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_film_equals_the_deposits_of_the_oracles_path_ends(srt, gpu, orc, name):
    (scene, cam, W, H, n, depth, _), ends = _case(srt, orc, name)
    frame, film = spectral_run(gpu, scene, cam, W, H, depth, [1, n - 1])
    assert_same_floats(film, ends["film"], name + " film")
    assert_planes_equal(frame["xyz"], ends["render"]["xyz"], name + " XYZ sums")
    _assert_sees_something(name, frame)
    if name in SEES_SOMETHING:
        assert ends["film"].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_two_streams_equal_the_stream_prediction(srt, gpu, orc, name):
    """... whose plain sub-frames are the oracle's frames of the seeds 1984 and 1984 + n_lanes"""
    (scene, cam, W, H, n, depth, mode), _ = _case(srt, orc, name)
    n += n % 2                   # (n / 2 samples in each of the two streams)
    want = stream_prediction(srt, gpu, orc, "edge " + name, (scene, cam, W, H, depth), n, 2, must_differ=False)
    osc = oracle_scene_for(orc, scene, mode)
    for k, sub in enumerate(want["subs"]):
        ref = osc.render(cam, W, H, n // 2, depth, seed=SEED + k * sub["geom"]["n_lanes"])
        assert_planes_equal(sub["xyz"], ref["xyz"], "%s sub-frame %d XYZ" % (name, k))
    osc.close()
    (total, got), = srt.render_streams(scene, cam, W, H, [n], depth, 2, renderer=gpu)
    assert total == n
    assert_same_image(got, want, name + " K = 2")
    _assert_sees_something(name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_features_equal_the_cpu_prediction(srt, gpu, orc, name):
    """(forty_materials: the colour table beyond 32 entries; the unknown material id of the degenerate scene)"""
    (scene, cam, W, H, _, depth, mode), _ = _case(srt, orc, name)
    n = 2
    want = predict_features(orc, scene, cam, W, H, n, depth, mode)["rows"]
    fresh_context(gpu, scene, cam, W, H, depth, spp=n)
    gpu.accum_reset_features()
    for s in (1, 1):
        gpu.render_chunk_accum(W, H, s)
    got = stack_features(gpu.read_features(W, H))
    for c in range(8):
        assert_same_floats(got[..., c], want[..., c], "%s channel %d" % (name, c))
    if name in SEES_SOMETHING:
        assert want[..., 7].max() > 0
        if name == "forty_materials":
            assert want[..., 3:6].max() > 0
