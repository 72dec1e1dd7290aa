"""Spectral film without a GPU: the new entry points are declared, bound and exported, the library's gfx950 code object holds the
spectral render kernel (render_kernel<5, ...>) for every shape the launcher picks, the host-side helpers (grid, estimator with its edge
factor, film -> XYZ contraction) give the right numbers on synthetic arrays, and the C-ABI refuses null contexts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from accum_helpers import ERR_INVALID, ROOT, SHAPES, kernel_id

NEW_SYMBOLS = ("srt_accum_reset_spectral", "srt_read_spectral", "srt_comm_accum_reset_spectral")
SPECTRAL_SYM = re.compile(r"^_ZN3srt13render_kernelILi5ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, fp = C.c_uint32, C.POINTER(C.c_float)
    assert srt.binding.PROTOTYPES["srt_accum_reset_spectral"] == (C.c_int, [C.c_void_p])
    assert srt.binding.PROTOTYPES["srt_read_spectral"] == (C.c_int, [C.c_void_p, u32, u32, fp, u32, u32])
    assert srt.binding.PROTOTYPES["srt_comm_accum_reset_spectral"] == (C.c_int, [C.c_void_p])
    lib = srt.binding.lib()
    assert lib.srt_read_spectral.argtypes == [C.c_void_p, u32, u32, fp, u32, u32]
    for name in ("render_spectral", "spectral_wavelengths", "spectral_radiance", "film_to_xyz"):
        assert name in srt.__all__ and callable(getattr(srt, name)), name
    for attr in ("accum_reset_spectral", "read_spectral"):
        assert hasattr(srt.Renderer, attr), attr
        assert hasattr(srt.Comm, attr), attr
    # the deposit rule and the estimator are part of the contract the header states
    for phrase in ("F[off_k] += (1 - w_k) * p_k", "F[off_k + 1] += w_k * p_k", "F_j * 470 / (35 n)", "adaptive + spectral is not supported"):
        assert phrase in header, phrase


def test_code_object_holds_every_spectral_variant(srt):
    found = set()
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        m = SPECTRAL_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)


def test_wavelength_grid(srt):
    lam = srt.spectral_wavelengths()
    assert lam.dtype == np.float32 and lam.shape == (95,)
    assert lam[0] == 360.0 and lam[-1] == 830.0 and np.all(np.diff(lam) == 5.0)


def test_spectral_radiance_and_its_edge_factor(srt):
    n = 7
    film = np.full((2, 3, 95), 35.0 * n / 470.0, np.float32)       # a constant spectrum of 1: interior samples
    film[..., 0] /= 2.0
    film[..., 94] /= 2.0                                           # half-width hats at the grid's ends collect half as much
    L = srt.spectral_radiance(film, n)
    assert L.shape == film.shape and L.dtype == np.float64
    np.testing.assert_allclose(L, 1.0, rtol=1e-6)
    # a sub-range keeps the grid's edge factors where they are: [90, 95) has j = 94, [0, 3) has j = 0
    np.testing.assert_allclose(srt.spectral_radiance(film[..., 90:], n, first=90), 1.0, rtol=1e-6)
    np.testing.assert_allclose(srt.spectral_radiance(film[..., :3], n, first=0), 1.0, rtol=1e-6)
    mid = srt.spectral_radiance(film[..., 10:20], n, first=10)
    np.testing.assert_allclose(mid, 1.0, rtol=1e-6)
    # a per-pixel sample map
    samples = np.array([[1, 2, 4], [8, 16, 32]])
    f = np.ones((2, 3, 95), np.float32) * samples[..., None].astype(np.float32)
    L = srt.spectral_radiance(f, samples)
    np.testing.assert_allclose(L[..., 5], 470.0 / 35.0)
    np.testing.assert_allclose(L[..., 0], 2 * 470.0 / 35.0)
    with pytest.raises(ValueError):
        srt.spectral_radiance(film[..., :10], n, first=90)


def test_film_to_xyz_contracts_with_the_colour_matching_rows(srt):
    cmf = np.zeros(95 * 4, np.float32)
    m = np.zeros(9, np.float32)
    assert srt.binding.lib().srt_color_tables(srt.binding.fptr(cmf), srt.binding.fptr(m)) == 0
    cmf = cmf.reshape(95, 4)[:, :3].astype(np.float64)
    d = float(np.float32(470.0) / np.float32(7.0))
    # a unit impulse at sample j gives d times row j
    for j in (0, 17, 56, 94):
        f = np.zeros(95, np.float32)
        f[j] = 1.0
        np.testing.assert_array_equal(srt.film_to_xyz(f), d * cmf[j])
    rng = np.random.default_rng(5)
    film = rng.random((4, 5, 95)).astype(np.float32)
    want = np.einsum("hwj,jc->hwc", film.astype(np.float64), cmf) * d
    np.testing.assert_allclose(srt.film_to_xyz(film), want, rtol=1e-12)
    # the deposit of one path at one wavelength reproduces the kernel's XYZ term (1 - w) * x[off] + w * x[off + 1], times power * d
    off, w, p = 40, np.float32(0.25), np.float32(3.0)
    f = np.zeros(95, np.float32)
    f[off] += (np.float32(1) - w) * p
    f[off + 1] += w * p
    term = ((1 - w) * cmf[off] + w * cmf[off + 1]) * p * d
    np.testing.assert_allclose(srt.film_to_xyz(f), term, rtol=1e-6)
    with pytest.raises(ValueError):
        srt.film_to_xyz(film[..., :94])


@pytest.mark.parametrize("kw", [dict(passes=[]), dict(passes=[0]), dict(passes=[4, -1]), dict(passes=[65535, 1]), dict(first=-1),
                                dict(count=0), dict(first=90, count=6), dict(first=1.5)],
                         ids=lambda kw: ",".join("%s=%r" % i for i in sorted(kw.items())))
def test_render_spectral_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_spectral created a device context for arguments it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    args = dict(passes=[4], first=0, count=95)
    args.update(kw)
    with pytest.raises(ValueError):
        srt.render_spectral(None, None, 16, 16, bounce_limit=8, **args)


def test_null_context_refusals(srt):
    lib = srt.binding.lib()
    out = np.zeros(95, np.float32)
    assert lib.srt_accum_reset_spectral(None) == ERR_INVALID
    assert lib.srt_read_spectral(None, 0, 95, srt.binding.fptr(out), 1, 1) == ERR_INVALID
    assert lib.srt_comm_accum_reset_spectral(None) == ERR_INVALID
