"""The presented picture, the part that needs no GPU: the entry points are declared, bound and exported; present_config routes its
keywords by name and refuses what it must before a device is touched; the packing rule of tests/present_reference.py; and the
precondition of the cast -- the quantised sRGB behind the tone curve is a whole number in 0 .. 255 for every input."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import expose_reference as R
import present_reference as P
from accum_helpers import ROOT, convert_xyz

F = np.float32
NEW_SYMBOLS = ("srt_present", "srt_present_kat", "srt_present_last_ms")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    B = srt.binding
    u32, u8p = C.c_uint32, C.POINTER(C.c_uint8)
    assert B.PROTOTYPES["srt_present"] == (C.c_int, [C.c_void_p, C.POINTER(B.PresentCfg), u8p, C.c_size_t, u32, u32, C.POINTER(B.PresentResult)])
    assert B.PROTOTYPES["srt_present_kat"] == (C.c_int, [C.c_void_p, C.POINTER(B.Tone), C.POINTER(C.c_float), u32, u32, u8p, C.POINTER(B.ToneResult)])
    for name in ("present_config", "render_presented"):
        assert name in srt.__all__ and callable(getattr(srt, name)), name
    for attr in ("present", "present_kat", "present_last_ms"):
        assert hasattr(srt.Renderer, attr), attr
    assert not hasattr(srt.Comm, "present")      # a gathered present is out of scope
    # the struct is the header's: the sources' numbers, the field order, the sizes
    for name, value in B.PRESENT_SOURCES.items():
        assert re.search(r"#define SRT_PRESENT_%s %d\b" % (name.upper(), value), header), name
    m = re.search(r"typedef struct srt_present_cfg \{(.*?)\} srt_present_cfg;", header, re.S)
    fields = re.findall(r"(\w+)(?:\[\d+\])?;", m.group(1))
    assert fields == [f[0] for f in B.PresentCfg._fields_]
    assert C.sizeof(B.PresentCfg) == 184 and B.PresentCfg.response3.offset == 152 and C.sizeof(B.PresentResult) == 64
    for phrase in ("(uint32)q.r | (uint32)q.g << 8 | (uint32)q.b << 16 | 255 << 24", "pitch_bytes < 4 * image_width", "and no other byte of the caller's buffer"):
        assert phrase in header, phrase


def test_present_config_routes_keywords_by_name(srt):
    B = srt.binding
    p = srt.present_config()
    assert (p.source, p.metered, p.tone.curve, p.tone.gain, bool(p.response3)) == (0, 1, 1, 1.0, False)
    assert bytes(p.meter) == bytes(srt.meter_config()) and bytes(p.denoise) == bytes(srt.denoise_config()) and bytes(p.denoise_vg) == bytes(srt.denoise_vg_config())
    assert not any(p.reserved) and p.scale == F(470.0) / F(7.0)
    p = srt.present_config("accum", gain=0.5, curve="linear", white=2.0)
    assert (p.metered, p.tone.gain, p.tone.curve, p.tone.white) == (0, 0.5, 0, 2.0)
    p = srt.present_config("accum", percentile_ppm=900000, key=0.3, rect=(1, 2, 3, 4), curve=0)
    assert (p.metered, p.meter.percentile_ppm, p.meter.key, p.meter.x0, p.meter.h, p.tone.curve) == (1, 900000, float(F(0.3)), 1, 4, 0)
    p = srt.present_config("denoise", gain=2.0, levels=2, sigma_color=0.5)
    assert (p.source, p.denoise.levels, p.denoise.sigma_color) == (B.PRESENT_SOURCES["denoise"], 2, 0.5)
    for src in ("denoise_vg", "denoise_mv"):
        p = srt.present_config(src, levels=3, sigma_variance=1.5, variance_floor=1e-6, white=float("inf"))
        assert (p.source, p.denoise_vg.levels, p.denoise_vg.sigma_variance, p.denoise_vg.variance_floor) == (B.PRESENT_SOURCES[src], 3, 1.5, float(F(1e-6)))
        assert p.metered == 1 and p.tone.white == float("inf")
    p = srt.present_config("develop")
    assert p.source == 4 and not p.response3 and p.scale == F(470.0) / F(7.0)
    curves = np.random.default_rng(3).random((3, 95)).astype(F)
    t = np.linspace(0.25, 1.0, 95).astype(F)
    p = srt.present_config("develop", response=curves, filter=t, scale=2.0, gain=1.0)
    got = np.ctypeslib.as_array(p.response3, (3, 95))
    assert np.array_equal(got, (curves * t).astype(F)) and p.scale == 2.0
    p = srt.present_config("develop", filter=t)      # the filter alone folds into the colour-matching rows
    assert np.array_equal(np.ctypeslib.as_array(p.response3, (3, 95)), srt.sensor_response(srt.renderer.cie_response(), t))


def test_present_config_refuses_before_the_device_is_touched(srt):
    bad_values = [dict(source="film"), dict(source=None), dict(source=0), dict(source="accum", gain=1.0, key=0.2), dict(source="accum", gain=1.0, rect=(0, 0, 1, 1)),
                  dict(source="accum", levels=2), dict(source="accum", sigma_variance=1.0), dict(source="develop", sigma_depth=1.0),
                  dict(source="denoise", sigma_variance=1.0), dict(source="denoise", variance_floor=1.0), dict(source="denoise_vg", sigma_color=1.0),
                  dict(source="denoise_mv", sigma_color=1.0), dict(source="denoise", response=np.ones((3, 95))), dict(source="accum", scale=2.0),
                  dict(source="denoise_vg", filter=np.ones(95)),
                  # ... and what the stage's own config function refuses
                  dict(source="accum", gain=0.0), dict(source="accum", gain=float("nan")), dict(source="accum", curve=2), dict(source="accum", white=0.0),
                  dict(source="accum", percentile_ppm=0), dict(source="accum", key=-1.0), dict(source="denoise", levels=9), dict(source="denoise_vg", sigma_variance=float("inf")),
                  dict(source="develop", response=np.ones((2, 95))), dict(source="develop", response=np.full((3, 95), np.nan)), dict(source="develop", scale=float("inf")),
                  dict(source="develop", filter=np.ones(94))]
    for kw in bad_values:
        with pytest.raises(ValueError):
            srt.present_config(**kw)
    for kw in (dict(sigma=1.0), dict(source="develop", channels=3)):
        with pytest.raises(TypeError):
            srt.present_config(**kw)
    # the generator checks the same things, and its schedule, when it is called
    scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    cam = scene.default_camera(16, 16)
    for kw in (dict(source="film"), dict(gain=1.0, key=0.2), dict(source="accum", levels=2), dict(source="denoise_mv", min_spp=0)):
        with pytest.raises(ValueError):
            srt.render_presented(scene, cam, 16, 16, [2], 4, **kw)
    with pytest.raises(ValueError):
        srt.render_presented(scene, cam, 16, 16, [], 4)


def test_pack_is_a_cast_and_an_alpha_byte():
    q = np.array([[[0, 1, 2], [255, 254, 128]], [[7, 0, 255], [31, 32, 33]]], F)
    rgba = P.pack(q)
    assert rgba.dtype == np.uint8 and rgba.shape == (2, 2, 4)
    assert np.array_equal(rgba[..., :3], q.astype(np.uint8)) and (rgba[..., 3] == 255).all()
    assert P.words(rgba)[0, 1] == 255 | 254 << 8 | 128 << 16 | 255 << 24 and P.words(rgba)[1, 0] == 7 | 0 << 8 | 255 << 16 | 255 << 24
    for bad in ([[0.5, 0, 0]], [[256, 0, 0]], [[-1, 0, 0]], [[np.nan, 0, 0]]):
        with pytest.raises(AssertionError):
            P.pack(np.array(bad, F))


def test_quantised_values_are_whole_numbers_in_0_255_for_every_input(orc):
    """what the cast to bytes rests on: behind either tone curve, at any gain, the quantised sRGB of NaN, +-inf, negative, denormal, zero
    and huge XYZ is a whole number in 0 .. 255 (a NaN channel fails every compare of the transfer function and comes out 255)"""
    specials = np.array([np.nan, np.inf, -np.inf, -1.0, 1e-41, -1e-41, 1e30, -1e30, 3.4e38, 0.0, -0.0, 0.18, 1.0, 1e-6], F)
    grid = np.stack(np.meshgrid(specials, specials, specials, indexing="ij"), axis=-1).reshape(-1, 3)
    assert grid.shape[0] == specials.size ** 3
    saw_nan_255 = False
    for curve in (0, 1):
        for gain, white in ((1.0, 4.0), (2.0 ** -20, np.inf), (3e5, 0.5)):
            o = R.tone(grid, gain, curve, white)
            _, q = convert_xyz(orc, [o[:, c] for c in range(3)], 1)
            q = np.stack(q, axis=1)
            assert ((q >= 0) & (q <= 255) & (q == np.floor(q))).all(), (curve, gain, white)
            rgba = P.pack(q)
            all_nan = np.isnan(o).all(axis=1)
            assert all_nan.any() and (rgba[all_nan] == 255).all()
            saw_nan_255 = True
    assert saw_nan_255
