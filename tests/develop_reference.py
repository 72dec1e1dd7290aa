"""The developed film (srt_develop_spectral, include/srt_c_api.h) restated in numpy float32: one rounded operation per line, the loop
over the 95 grid samples in the kernel's order, vectorised over the pixels.  tests/test_develop_reference.py holds this restatement to
exact rational arithmetic; tests/test_develop.py holds the device to it bit for bit."""
import numpy as np

F = np.float32
N_GRID = 95
MAX_CHANNELS = 16
CIE_SCALE = F(470.0) / F(7.0)      # the kernel's fp32 470/7 (srt_device.h, hero_expand's step)


def develop(film, response, scale=1.0, order=None):
    """out[..., k] = (sum over j of film[..., j] * response[k][j]) * scale in float32: a_k = +0; for j = 0 .. 94 ascending:
    t = F_j * R[k][j] (rounded), a_k = a_k + t (rounded); out_k = a_k * scale.  film (..., 95) -- a 96th word, if given, never enters --
    response (K, 95).  order: another order of the 95 samples, for the test that shows the order is pinned."""
    film = np.asarray(film, F)
    resp = np.asarray(response, F).reshape(-1, N_GRID)
    assert film.shape[-1] >= N_GRID
    acc = np.zeros(film.shape[:-1] + (resp.shape[0],), F)
    with np.errstate(all="ignore"):
        for j in (range(N_GRID) if order is None else order):
            t = (film[..., j, None] * resp[:, j]).astype(F)
            acc = (acc + t).astype(F)
        return (acc * F(scale)).astype(F)


def normalise(xyz_sums, samples):
    """the render kernel's normalising step on developed XYZ sums: inv = 1.0f / (float)samples; c = inv * sum (float32, one rounding each);
    the conversion to sRGB that follows is xyz_mean_to_srgb (the oracle's orc_XYZ_to_sRGB in the tests)"""
    inv = F(1) / F(samples)
    with np.errstate(all="ignore"):
        return (inv * np.asarray(xyz_sums, F)).astype(F)


def one_hot(first, count):
    """`count` response curves, curve k being 1 at grid sample first + k and 0 elsewhere: at scale 1 they reproduce the film"""
    r = np.zeros((count, N_GRID), F)
    r[np.arange(count), first + np.arange(count)] = 1
    return r
