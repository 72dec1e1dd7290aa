"""The developed film, the interface, without a GPU: the entry points are declared, bound and exported, the code object holds the kernels,
and sensor_response / render_developed check their arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from accum_helpers import ERR_INVALID, ROOT, kernel_id
from helpers import bits

NEW_SYMBOLS = ("srt_develop_spectral", "srt_develop_spectral_srgb", "srt_develop_kat", "srt_develop_last_ms")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    u32, f, fp, vp = C.c_uint32, C.c_float, C.POINTER(C.c_float), C.c_void_p
    assert srt.binding.PROTOTYPES["srt_develop_spectral"] == (C.c_int, [vp, fp, u32, f, fp, u32, u32])
    assert srt.binding.PROTOTYPES["srt_develop_spectral_srgb"] == (C.c_int, [vp, fp, f, fp, fp, fp, u32, u32])
    assert srt.binding.PROTOTYPES["srt_develop_kat"] == (C.c_int, [vp, fp, u32, fp, u32, f, fp])
    assert srt.binding.PROTOTYPES["srt_develop_last_ms"] == (C.c_int, [vp, fp, fp])
    for name in ("sensor_response", "render_developed"):
        assert name in srt.__all__ and callable(getattr(srt, name)), name
    for attr in ("develop_spectral", "develop_spectral_srgb", "develop_kat", "develop_last_ms"):
        assert hasattr(srt.Renderer, attr), attr
    assert hasattr(srt.Comm, "develop_spectral")
    assert srt.renderer.MAX_DEVELOP_CHANNELS == 16 and "#define SRT_MAX_DEVELOP_CHANNELS 16" in header
    # the operation is part of the contract the header states
    for phrase in ("a_k = +0.0f", "t = F_j * R[k][j];   a_k = a_k + t", "out_k = a_k * scale", "inv = 1.0f / (float)n"):
        assert phrase in header, phrase


def test_code_object_holds_the_develop_kernels(srt):
    names = [n for n, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH) if "develop" in n]
    for want in ["develop_kernelILi%dE" % k for k in (1, 2, 3, 4, 8, 16)] + ["develop_srgb_kernel"]:
        assert sum(want in n for n in names) == 1, (want, names)


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    assert lib.srt_develop_spectral(None, None, 1, 1.0, None, 1, 1) == ERR_INVALID
    assert lib.srt_develop_spectral_srgb(None, None, 1.0, None, None, None, 1, 1) == ERR_INVALID
    assert lib.srt_develop_kat(None, None, 1, None, 1, 1.0, None) == ERR_INVALID
    assert lib.srt_develop_last_ms(None, None, None) == ERR_INVALID


def test_sensor_response_shapes_and_filter(srt):
    rng = np.random.default_rng(3)
    one = srt.sensor_response(rng.random(95))
    assert one.shape == (1, 95) and one.dtype == np.float32 and one.flags.c_contiguous
    curves = (rng.random((16, 95)) - 0.5).astype(np.float32)
    r = srt.sensor_response(curves)
    assert r.shape == (16, 95) and np.array_equal(bits(r), bits(curves))
    t = rng.random(95).astype(np.float32)
    folded = srt.sensor_response(curves, t)
    assert np.array_equal(bits(folded), bits((curves * t[None, :]).astype(np.float32)))      # one float32 product per entry
    assert np.array_equal(bits(srt.sensor_response(curves[:3].tolist(), [0.5] * 95)), bits(curves[:3] * np.float32(0.5)))
    cie = srt.renderer.cie_response()
    assert cie.shape == (3, 95) and cie.dtype == np.float32 and (cie >= 0).all() and cie[1].max() > 0.9
    assert srt.renderer.CIE_SCALE == float(np.float32(470.0) / np.float32(7.0))


BAD_RESPONSES = [
    ("no curve", dict(curves=np.zeros((0, 95)))),
    ("seventeen curves", dict(curves=np.zeros((17, 95)))),
    ("94 samples", dict(curves=np.zeros((3, 94)))),
    ("96 samples", dict(curves=np.zeros(96))),
    ("three dimensions", dict(curves=np.zeros((1, 3, 95)))),
    ("a NaN", dict(curves=np.where(np.arange(95) == 7, np.nan, 1.0))),
    ("an inf", dict(curves=np.where(np.arange(95) == 94, np.inf, 1.0))),
    ("beyond float32", dict(curves=np.full(95, 1e39))),
    ("words", dict(curves=["wide"] * 95)),
    ("a short filter", dict(curves=np.ones(95), filter=np.ones(94))),
    ("a filter per curve", dict(curves=np.ones((2, 95)), filter=np.ones((2, 95)))),
    ("a NaN filter", dict(curves=np.ones(95), filter=np.full(95, np.nan))),
    ("an overflowing product", dict(curves=np.full(95, 1e30), filter=np.full(95, 1e30))),
]


@pytest.mark.parametrize("kw", [kw for _, kw in BAD_RESPONSES], ids=[n for n, _ in BAD_RESPONSES])
def test_sensor_response_rejects(srt, kw):
    with pytest.raises(ValueError):
        srt.sensor_response(**kw)


@pytest.mark.parametrize("kw", [dict(passes=[]), dict(passes=[0]), dict(passes=[4, -1]), dict(passes=[65535, 1]),
                                dict(passes=[4], response=np.zeros((17, 95))), dict(passes=[4], response=np.full(95, np.nan)),
                                dict(passes=[4], filter=np.ones(3)), dict(passes=[4], response=np.ones(95), filter=np.full(95, np.inf)),
                                dict(passes=[4], scale=float("nan")), dict(passes=[4], response=np.ones(95), scale="big")],
                         ids=lambda kw: ",".join(sorted(kw)) + "-%d" % len(repr(kw)))
def test_render_developed_rejects_bad_arguments_before_touching_a_device(srt, kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_developed created a device context for arguments it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_developed(None, None, 16, 16, bounce_limit=8, **kw)


def test_renderer_methods_check_their_arguments_before_the_library(srt):
    r = object.__new__(srt.Renderer)      # no device context: a checked argument never reaches the handle
    r._h = None
    with pytest.raises(ValueError):
        r.develop_spectral(4, 4, np.zeros((17, 95)))
    with pytest.raises(ValueError):
        r.develop_spectral(4, 4, np.ones(95), scale=float("inf"))
    with pytest.raises(ValueError):
        r.develop_spectral_srgb(4, 4, np.ones((2, 95)))
    with pytest.raises(ValueError):
        r.develop_spectral_srgb(4, 4, filter=np.ones(5))
    with pytest.raises(ValueError):
        r.develop_kat(np.zeros((4, 96)), np.ones(95))
    with pytest.raises(ValueError):
        r.develop_kat(np.zeros((0, 95)), np.ones(95))
