"""The path ends of the CPU oracle (orc_render_path_ends) and the float32 predictions built on them (tests/path_ends_reference.py): CPU
only.  Every set of path ends rebuilds the oracle's own XYZ planes bit for bit (the self-check inside path_ends), the predicted film
contracts to the oracle's XYZ sums, and the workloads of the GPU film tests cover, by the oracle alone, the kinds of path end those
tests rely on."""
import ctypes as C

import numpy as np
import pytest

from accum_helpers import N_GRID, named_workload
from helpers import bits, oracle_scene_for
from path_ends_reference import (FILM_SPP, FILM_WORKLOADS, assert_film_coverage, deposit, interp_coords, path_ends, predict_film,
                                 predict_y_sums, workload_ends)

F = np.float32


@pytest.mark.parametrize("name", ["prism", "dielectric", "fuzz_with_lens"])
def test_path_ends_rebuild_the_oracles_xyz_planes(srt, orc, name):
    """path_ends asserts it: X, Y and Z summed from the ends in sample order == a plain orc_render, lanes outside the chunk stay zero"""
    _, ends = workload_ends(srt, orc, name)
    assert ends["valid"].shape == (ends["W"] * ends["H"], ends["n"]) and ends["n"] >= 3
    assert ((ends["wl"] >= 360) & (ends["wl"] <= 830)).all()
    s1, _ = predict_y_sums(orc, ends)
    assert np.array_equal(bits(s1), bits(ends["render"]["xyz"][1][ends["lane"]]))


def test_offset_chunk_and_continued_states(srt, orc):
    """a 30 x 21 chunk at (17, 9) of a 64 x 40 image; and samples 3 .. 5 continued from the states after 3 are the last three of 6"""
    scene, _, _, _, depth, mode = named_workload(srt, "random_spheres")
    osc = oracle_scene_for(orc, scene, mode)
    cam = scene.default_camera(64, 40)
    ends = path_ends(orc, osc, cam, 30, 21, 4, depth, offx=17, offy=9)
    moved = path_ends(orc, osc, cam, 30, 21, 4, depth)
    assert not np.array_equal(ends["power"], moved["power"])          # the camera ray follows the image coordinates ...
    assert np.array_equal(ends["wl"][:, 0], moved["wl"][:, 0])        # ... the RNG stream (the first hero wavelength) the lane of the chunk's grid
    scene, cam, W, H, depth, mode = named_workload(srt, "dielectric")
    osc = oracle_scene_for(orc, scene, mode)
    whole = path_ends(orc, osc, cam, W, H, 6, depth)
    states = np.zeros((whole["render"]["geom"]["n_lanes"], 6), np.uint32)
    rs = orc.Rng()
    for idx in range(states.shape[0]):
        orc.lib().orc_rng_init(1984 + idx, C.byref(rs))
        states[idx, 0] = rs.d
        states[idx, 1:] = rs.v[:]
    osc.render(cam, W, H, 3, depth, states=states)
    rest = path_ends(orc, osc, cam, W, H, 3, depth, states=states)
    for k in ("wl", "power", "valid"):
        assert np.array_equal(whole[k][:, 3:].view(np.uint32), rest[k].view(np.uint32)), k
    assert np.array_equal(bits(predict_film(whole, 3, 3)), bits(predict_film(rest)))


@pytest.mark.parametrize("name", FILM_WORKLOADS)
def test_predicted_film_contracts_to_the_oracles_xyz_sums(srt, orc, name):
    """the tolerance of test_spectral.test_film_contracts_to_the_xyz_sums: the contraction reassociates the sum"""
    _, ends = workload_ends(srt, orc, name)
    W, H = ends["W"], ends["H"]
    want = np.stack([ends["render"]["xyz"][c][ends["lane"]] for c in range(3)], axis=-1).reshape(H, W, 3).astype(np.float64)
    got = srt.film_to_xyz(ends["film"])
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    ok = ~np.isnan(want)
    assert np.abs(want[ok]).max() > 0, name
    np.testing.assert_allclose(got[ok], want[ok], rtol=2e-4, atol=1e-9, err_msg=name)


def test_deposit_rule_on_hand_made_ends():
    """the select, the valid == 0 rule, the clamped last bin pair and the order of the sum, on values worked out by hand"""
    wl = np.array([[360.0, 362.5, 830.0, 827.5, 500.0, 600.0, 700.0]] * 3, F)
    power = np.array([[2.0, 4.0, 8.0, 16.0, 1.0, 1.0, np.inf]] * 3, F)
    film = np.zeros((3, N_GRID), F)
    deposit(film, wl, power, np.array([4, 0, 1], np.uint32))
    off, w = interp_coords(wl[0])
    assert off.tolist() == [0, 0, 93, 93, 28, 48, 68] and w.tolist() == [0.0, 0.5, 1.0, 0.5, 0.0, 0.0, 0.0]
    want = np.zeros(N_GRID, F)
    want[0], want[1], want[93], want[94] = 2.0 + 2.0, 2.0, 8.0, 8.0 + 8.0
    assert np.array_equal(bits(film[0]), bits(want))           # k >= valid (the infinite power among them) deposits +0
    assert not bits(film[1]).any()                             # valid == 0: nothing
    want = np.zeros(N_GRID, F); want[0] = 2.0
    assert np.array_equal(bits(film[2]), bits(want))


def test_film_workloads_cover_every_kind_of_path_end(srt, orc):
    seen = assert_film_coverage(srt, orc)
    print(seen)
    for name in FILM_WORKLOADS:
        (_, _, W, H, n, _, _), ends = workload_ends(srt, orc, name)
        assert n <= FILM_SPP and ends["film"].shape == (H, W, N_GRID)
    # prism at depth 1: every end is a miss, an emitter or the bounce limit
    _, ends = workload_ends(srt, orc, "prism_depth_1")
    assert set(np.unique(ends["valid"]).tolist()) == {0, 7}
