"""CPU: the Python face and the C-ABI's argument checks of the direct-light pass -- direct_light_config, every refusal of
Renderer.direct_light / direct_light_kat raised before any device is touched (the library is replaced by a trap for the duration), the
struct layouts, and the C entries' refusal of a null context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("srt_direct_light", "srt_direct_light_kat", "srt_read_light_table", "srt_direct_light_last", "srt_set_light_test_batch")


@pytest.fixture
def trapped(srt, monkeypatch):
    """a Renderer without a context whose library calls all fail the test: a check that ran after a call would not be a check"""
    def trap():
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(srt.binding, "lib", trap)
    r = object.__new__(srt.Renderer)
    r._h, r._owned, r.device = None, False, 0
    return r


def test_config_defaults_and_layout(srt):
    B = srt.binding
    cfg = srt.direct_light_config()
    assert (cfg.samples, cfg.first_sample, cfg.parts, cfg.seed) == (16, 0, 7, 0)
    assert C.sizeof(B.Light) == 24 and B.Light.seed.offset == 16 and C.sizeof(B.LightResult) == 72 and C.sizeof(B.LightInfo) == 32
    cfg = srt.direct_light_config(samples=65536, seed=2 ** 64 - 1, first_sample=2 ** 32 - 65536, parts=("sky",))
    assert (cfg.samples, cfg.first_sample, cfg.parts, cfg.seed) == (65536, 2 ** 32 - 65536, 4, 2 ** 64 - 1)
    assert srt.direct_light_config(parts="lights").parts == 2 and srt.direct_light_config(parts=["emitted", "lights"]).parts == 3
    assert B.LIGHT_PARTS == {"emitted": 1, "lights": 2, "sky": 4}


@pytest.mark.parametrize("bad", [dict(samples=0), dict(samples=65537), dict(samples=1.5), dict(samples=True), dict(seed=-1), dict(seed=2 ** 64),
                                 dict(first_sample=2 ** 32), dict(first_sample=2 ** 32 - 1, samples=2), dict(parts=()), dict(parts=("shadow",)),
                                 dict(parts=("sky", "moon"))],
                         ids=lambda b: ",".join("%s=%r" % kv for kv in b.items()))
def test_config_refusals(srt, trapped, bad):
    with pytest.raises(ValueError):
        srt.direct_light_config(**bad)
    with pytest.raises(ValueError):
        trapped.direct_light(8, 8, **bad)
    kat = {k: v for k, v in bad.items() if k not in ("samples", "first_sample")}
    if kat:
        with pytest.raises(ValueError):
            trapped.direct_light_kat(8, 8, **kat)


@pytest.mark.parametrize("rect", [(0, 4, 0, 0), (4, 0, 0, 0), (-1, 4, 0, 0), (4, 4, -1, 0), (4.0, 4, 0, 0), (1 << 16, 1 << 15, 0, 0)])
def test_rectangle_refusals(trapped, rect):
    with pytest.raises(ValueError):
        trapped.direct_light(*rect)
    with pytest.raises(ValueError):
        trapped.direct_light_kat(*rect)


def test_render_direct_checks_before_any_device(srt, monkeypatch):
    def trap(*a, **k):
        raise AssertionError("a renderer was made before the arguments were checked")
    monkeypatch.setattr(srt.renderer, "Renderer", trap)
    for bad in (dict(passes=0), dict(passes=1.5), dict(passes=2, samples=0), dict(passes=2, parts=()), dict(passes=2, samples=40000, first_sample=2 ** 32 - 50000)):
        kw = dict(passes=2, samples=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            srt.render_direct(None, None, 8, 8, **kw)
    gen = srt.render_direct(None, None, 8, 8, 2, samples=4)      # a generator: nothing runs until it is advanced
    assert hasattr(gen, "__next__")


def test_header_declares_and_library_exports(srt):
    src = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    declared = set(re.findall(r"SRT_API\s+[\w\s\*]+?\b(srt_\w+)\s*\(", src))
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in srt.binding.PROTOTYPES and getattr(L, name) is not None
    for word in ("Philox4x32-10", "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "largest remainder", "SRT_LIGHT_EMITTED", "SRT_LIGHT_LIGHTS", "SRT_LIGHT_SKY"):
        assert word in src, word


def test_null_context_is_refused(srt):
    """no GPU needed: every entry answers SRT_ERR_INVALID for a null context and writes nothing"""
    B = srt.binding
    L = B.lib()
    cfg, res, info = srt.direct_light_config(), B.LightResult(), B.LightInfo()
    out = np.full((4, 4, 3), 7.0, np.float32)
    n = C.c_uint32(9)
    assert L.srt_direct_light(None, C.byref(cfg), B.fptr(out), None, C.byref(res), 4, 4, 0, 0) == -1
    assert L.srt_direct_light_kat(None, C.byref(cfg), B.fptr(out), None, C.byref(res), 4, 4, 0, 0, None, None, None, None, None, None, None) == -1
    assert L.srt_read_light_table(None, C.byref(n), None, None, 0) == -1
    assert L.srt_direct_light_last(None, C.byref(info)) == -1
    assert L.srt_set_light_test_batch(None, 64) == -1
    assert (out == 7.0).all() and n.value == 9 and res.shaded == 0
    assert b"null" in L.srt_last_error(None)
