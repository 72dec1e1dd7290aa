"""The firefly filter's surface without a GPU: symbols, prototypes and struct sizes, the header's statement of the operation, and every bad
keyword and value refused before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("srt_despeckle_accum", "srt_despeckle_kat", "srt_despeckle_last_ms", "srt_denoise_features_ds", "srt_present_despeckled")


def header():
    return open(os.path.join(ROOT, "include", "srt_c_api.h")).read()


def test_symbols_prototypes_and_struct_sizes(srt):
    B = srt.binding
    L = C.CDLL(B.LIB_PATH)
    src = header()
    for name in SYMBOLS:
        assert name in B.PROTOTYPES, name
        assert getattr(L, name) is not None
        assert re.search(r"SRT_API int %s\(" % name, src), name
    vp, u32, fp = C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
    ds, dres, u8p = C.POINTER(B.Despeckle), C.POINTER(B.DespeckleResult), C.POINTER(C.c_uint8)
    assert B.PROTOTYPES["srt_despeckle_accum"] == (C.c_int, [vp, ds, fp, fp, fp, fp, dres, u32, u32])
    assert B.PROTOTYPES["srt_despeckle_kat"] == (C.c_int, [vp, ds, fp, u32, u32, fp, fp, dres])
    assert B.PROTOTYPES["srt_despeckle_last_ms"] == (C.c_int, [vp, fp])
    assert B.PROTOTYPES["srt_denoise_features_ds"] == (C.c_int, [vp, ds, C.POINTER(B.Denoise), fp, fp, fp, u32, u32])
    assert B.PROTOTYPES["srt_present_despeckled"] == (C.c_int, [vp, C.POINTER(B.PresentCfg), ds, u8p, C.c_size_t, u32, u32, C.POINTER(B.PresentResult), dres])
    assert C.sizeof(B.Despeckle) == 32 and C.sizeof(B.DespeckleResult) == 24
    assert [f[0] for f in B.Despeckle._fields_] == ["radius", "rank_ppm", "gain", "floor", "reserved"]
    assert (B.Despeckle.radius.offset, B.Despeckle.rank_ppm.offset, B.Despeckle.gain.offset, B.Despeckle.floor.offset, B.Despeckle.reserved.offset) == (0, 4, 8, 12, 16)
    assert [f[0] for f in B.DespeckleResult._fields_] == ["clamped", "nonfinite", "alone"]
    assert C.sizeof(B.PresentCfg) == 184          # srt_present_cfg is what it was: the stage has a struct of its own
    assert "typedef struct srt_despeckle { uint32_t radius, rank_ppm; float gain, floor; uint32_t reserved[4]; } srt_despeckle;" in src
    assert "typedef struct srt_despeckle_result { uint64_t clamped, nonfinite, alone; } srt_despeckle_result;" in src
    for name in ("despeckle_config", "render_despeckled"):
        assert name in srt.__all__ and callable(getattr(srt, name)), name
    for name in ("despeckle", "despeckle_kat", "despeckle_last_ms", "denoise_despeckled", "present_despeckled"):
        assert callable(getattr(srt.Renderer, name)), name


def test_the_header_states_the_operation():
    text = " ".join(header().replace("*", " ").split())
    for phrase in ("valid(q) := q inside the rectangle && (Y_q - Y_q) == 0",
                   "v_q = Y_q > 0 ? Y_q : +0.0f",
                   "m = number of valid q; u_0 <= u_1 <= .. <= u_{m-1} the v_q in ascending order",
                   "k = (uint64)(m - 1) rank_ppm / 1000000; ref = u_k",
                   "limit = gain ref; limit = limit + floor",
                   "1. nonfinite: (v - v) == 0 is false for a component v of c_p -> o = c_p, s = 1.0f",
                   "2. alone: m == 0 -> o = c_p, s = 1.0f",
                   "3. clamped: Y_p > limit -> s = limit / Y_p; o = (s c_p.x, s c_p.y, s c_p.z)",
                   "4. kept: otherwise -> o = c_p (its bits), s = 1.0f",
                   "inv = 1.0f / (float)n",
                   "0 counts as 1",
                   "A non-finite pixel is neither repaired nor used as a neighbour",
                   "radius 1 or 2; rank_ppm <= 1000000; gain finite and >= 0",
                   "floor >= 0 and not NaN (+inf allowed",
                   "colour[1] = Despeckle(colour[0])",
                   "At floor = +inf it equals srt_denoise_features, bit for bit"):
        assert phrase in text, phrase


def test_despeckle_config_values(srt):
    d = srt.despeckle_config()
    assert (d.radius, d.rank_ppm, d.gain, d.floor, list(d.reserved)) == (2, 875000, 4.0, 0.0, [0, 0, 0, 0])       # floor None: metered later, 0 here
    d = srt.despeckle_config(radius=1, rank_ppm=0, gain=0, floor=float("inf"))
    assert (d.radius, d.rank_ppm, d.gain, d.floor) == (1, 0, 0.0, float("inf"))
    assert srt.despeckle_config(gain=np.float32(1.5), floor=1e300).floor == float("inf")      # beyond float32: inf, which is allowed
    assert srt.despeckle_config(rank_ppm=np.int64(1000000)).rank_ppm == 1000000
    inf, nan = float("inf"), float("nan")
    for bad in (dict(radius=0), dict(radius=3), dict(radius=1.0), dict(radius=True), dict(radius="2"), dict(rank_ppm=-1), dict(rank_ppm=1000001),
                dict(rank_ppm=0.5), dict(rank_ppm=True), dict(gain=-1.0), dict(gain=inf), dict(gain=nan), dict(gain=1e39), dict(gain="four"), dict(gain=None),
                dict(gain=True), dict(floor=-1e-3), dict(floor=nan), dict(floor=-inf), dict(floor="none"), dict(floor=False)):
        with pytest.raises(ValueError):
            srt.despeckle_config(**bad)
    with pytest.raises(TypeError):
        srt.despeckle_config(sigma=1.0)
    assert "untuned" in srt.despeckle_config.__doc__


def test_bad_arguments_are_refused_before_a_device_is_touched(srt):
    """scene and camera are None: anything that got as far as a device would fail on them with another exception"""
    args = (None, None, 8, 8, [2], 4)
    for kw, exc in ((dict(despeckle=dict(radius=3)), ValueError), (dict(despeckle=dict(gain=-1.0)), ValueError), (dict(despeckle=dict(floor=float("nan"))), ValueError),
                    (dict(despeckle=dict(rank=5)), TypeError), (dict(despeckle=dict(sigma_color=1.0)), TypeError), (dict(levels=9), ValueError),
                    (dict(sigma_color=0.0), ValueError), (dict(denoise=False, levels=2), TypeError)):
        with pytest.raises(exc):
            srt.render_despeckled(*args, **kw)
    with pytest.raises(TypeError):
        srt.render_despeckled(*args, white=4.0)
    with pytest.raises(ValueError):
        srt.render_despeckled(None, None, 8, 8, [], 4)
    # the Renderer's methods check their keywords before their first library call: a Renderer that holds no context shows it
    r = object.__new__(srt.Renderer)
    r._h = None
    for call, exc in ((lambda: r.despeckle(8, 8, radius=0), ValueError), (lambda: r.despeckle(8, 8, rank=1), TypeError),
                      (lambda: r.despeckle_kat(np.ones((2, 2, 3), np.float32), gain=float("inf")), ValueError),
                      (lambda: r.despeckle_kat(np.ones((2, 2), np.float32), floor=0.0), ValueError),
                      (lambda: r.denoise_despeckled(8, 8, despeckle=dict(radius=5)), ValueError), (lambda: r.denoise_despeckled(8, 8, levels=9), ValueError),
                      (lambda: r.denoise_despeckled(8, 8, despeckle=dict(levels=1)), TypeError),
                      (lambda: r.present_despeckled(8, 8, source="develop", despeckle=dict(floor=0.0)), ValueError),
                      (lambda: r.present_despeckled(8, 8, source="denoise_vg", despeckle=dict(floor=0.0)), ValueError),
                      (lambda: r.present_despeckled(8, 8, despeckle=dict(floor=-1.0)), ValueError),
                      (lambda: r.present_despeckled(8, 8, gain=0.0, despeckle=dict(floor=0.0)), ValueError),
                      (lambda: r.present_despeckled(8, 8, sigma=1.0), TypeError)):
        with pytest.raises(exc):
            call()
    r._h = None      # (nothing to close)
