"""Gathering an accumulation, the interface.  Without a GPU: the entry points are declared, bound and exported, the code object holds
both directions of the copy kernel, the Python signatures, and gather_parts' refusals (which come before any device is touched)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from accum_helpers import ERR_INVALID, ROOT, kernel_id

NEW_SYMBOLS = ("srt_accum_exchange_size", "srt_pack_accum", "srt_unpack_accum", "srt_accum_gathered", "srt_accum_whole", "srt_gather_last_ms", "srt_comm_gather_accum",
               "srt_comm_last_accum_gather_ms")
GATHER_SYM = re.compile(r"^_ZN3srt12_GLOBAL__N_113gather_kernelILb([01])EEEvNS_12GatherParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    vp, u32, fp, sz = C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.c_size_t
    P = srt.binding.PROTOTYPES
    assert P["srt_accum_exchange_size"] == (C.c_int, [vp, u32, C.POINTER(sz)])
    assert P["srt_pack_accum"] == (C.c_int, [vp, u32, vp, vp]) and P["srt_unpack_accum"] == (C.c_int, [vp, u32, vp, vp])
    assert P["srt_accum_gathered"] == (C.c_int, [vp, C.POINTER(u32)]) and P["srt_gather_last_ms"] == (C.c_int, [vp, fp, fp])
    assert P["srt_comm_gather_accum"] == (C.c_int, [vp, u32]) and P["srt_comm_last_accum_gather_ms"] == (C.c_int, [vp, fp, fp, fp])
    for bit, name in ((1, "SUMS"), (2, "COUNTS"), (4, "FEATURES"), (8, "FILM")):
        assert re.search(r"#define\s+SRT_GATHER_%s\s+%du" % (name, bit), header), name
        assert srt.GATHER_PARTS[name.lower()] == bit
    # the contract the header states: what clears the mark, what the stale records mean, the refusals' hint
    for phrase in ("Gather before you look", "STALE until the next gather", "srt_pack_accum and srt_unpack_accum; every other"):
        assert phrase in header, phrase
    for name in ("render_interactive_multi", "gather_parts", "GATHER_PARTS"):
        assert name in srt.__all__ and hasattr(srt, name), name


def test_code_object_holds_both_directions(srt):
    found = {m.group(1) for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH) for m in [GATHER_SYM.match(name)] if m}
    assert found == {"0", "1"}, found


def test_python_signatures(srt):
    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(srt.Renderer.accum_exchange_size) == ["self", "parts"]
    assert params(srt.Renderer.pack_accum) == ["self", "dst_ptr", "parts", "hip_stream"]
    assert params(srt.Renderer.unpack_accum) == ["self", "gathered_ptr", "parts", "hip_stream"]
    assert params(srt.Renderer.accum_whole) == ["self", "parts"] and params(srt.Renderer.accum_gathered) == ["self"] and params(srt.Renderer.gather_last_ms) == ["self"]
    assert params(srt.Comm.gather_accum) == ["self", "parts"] and inspect.signature(srt.Comm.gather_accum).parameters["parts"].default is None
    assert params(srt.Comm.last_accum_gather_ms) == ["self"]
    sig = inspect.signature(srt.render_interactive_multi)
    assert list(sig.parameters)[:6] == ["scene", "cameras", "width", "height", "spp", "bounce_limit"]
    want = dict(devices=None, comm=None, denoise=True, despeckle=None, temporal=None, variance_guided=False)
    for name, default in want.items():
        assert sig.parameters[name].default is default, name
    assert sig.parameters["cfg"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.isgeneratorfunction(srt.renderer._interactive_frames_multi)


def test_the_stream_handle_of_pack_and_unpack_reaches_the_library(srt, monkeypatch):
    """tests/test_stream_order_api.py holds the four older calls that take a stream to this; the two new ones name theirs hip_stream"""
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    assert set(re.findall(r"SRT_API\s+int\s+(srt_\w+)\s*\([^;]*?void \*hip_stream\)", header)) == {"srt_pack_accum", "srt_unpack_accum"}
    calls = []

    class Recorder:      # stands in for the loaded library: every function returns SRT_OK and notes its arguments
        def __getattr__(self, name):
            return lambda *args: calls.append((name, args)) or 0
    monkeypatch.setattr(srt.binding, "lib", lambda: Recorder())
    r = srt.Renderer.__new__(srt.Renderer)
    r._h, r._owned = C.c_void_p(0x1000), False
    try:
        for method, symbol in ((srt.Renderer.pack_accum, "srt_pack_accum"), (srt.Renderer.unpack_accum, "srt_unpack_accum")):
            assert inspect.signature(method).parameters["hip_stream"].default is None
            for handle, want in ((0x7f12345678, 0x7f12345678), (None, None)):      # (None: the null stream, a NULL pointer)
                del calls[:]
                method(r, 0x2000, ["sums", "features"], hip_stream=handle)
                assert len(calls) == 1 and calls[0][0] == symbol, calls
                args = calls[0][1]
                assert args[0] is r._h and args[1] == 5 and args[2].value == 0x2000
                assert isinstance(args[-1], C.c_void_p) and args[-1].value == want, (symbol, args[-1])
    finally:
        r._h = None


def test_gather_parts_turns_names_into_the_mask(srt):
    g = srt.gather_parts
    assert g() == 0 and g(None) == 0 and g(0) == 0 and g([]) == 0
    assert g("film") == 8 and g(["sums", "counts"]) == 3 and g(("features", "film", "sums", "counts")) == 15 and g({"features"}) == 4
    assert g(13) == 13 and g(np.uint32(5)) == 5


@pytest.mark.parametrize("bad,exc", [("Film", ValueError), (["sums", "rng"], ValueError), (16, ValueError), (-1, ValueError), (True, TypeError),
                                     ([4], ValueError), ([None], ValueError), (31, ValueError)])
def test_gather_parts_refuses_what_it_does_not_know(srt, bad, exc):
    with pytest.raises(exc, match="gather_parts"):
        srt.gather_parts(bad)


def test_refusals_come_before_any_device_is_touched(srt):
    """a renderer without a handle would fault in the library: the names are checked first"""
    class NoDevice(srt.Renderer):
        def __init__(self):
            self._h = None
    r = NoDevice()
    for call in (lambda: r.accum_exchange_size("flim"), lambda: r.pack_accum(0, ["sums", "x"]), lambda: r.unpack_accum(0, 64)):
        with pytest.raises(ValueError, match="gather_parts"):
            call()
    cam = srt.camera_init(16, 16, 40.0, (0, 0, 5), (0, 0, 0))
    with pytest.raises(ValueError, match="no camera"):
        srt.render_interactive_multi(None, [], 16, 16, 4, 4)
    with pytest.raises(TypeError, match="CameraData"):
        srt.render_interactive_multi(None, [cam, 3], 16, 16, 4, 4)
    with pytest.raises(ValueError, match="not both"):
        srt.render_interactive_multi(None, [cam], 16, 16, 4, 4, devices=[0], comm=object())
    with pytest.raises(TypeError, match="single-process Comm"):
        srt.render_interactive_multi(None, [cam], 16, 16, 4, 4, comm=object())
    with pytest.raises(ValueError, match="variance_guided=True with denoise=False"):
        srt.render_interactive_multi(None, [cam], 16, 16, 4, 4, denoise=False, variance_guided=True)


def test_null_arguments_are_refused(srt):
    lib = srt.binding.lib()
    n, m, a = C.c_size_t(), C.c_uint32(), C.c_float()
    assert lib.srt_accum_exchange_size(None, 0, C.byref(n)) == ERR_INVALID
    assert lib.srt_pack_accum(None, 0, None, None) == ERR_INVALID and lib.srt_unpack_accum(None, 0, None, None) == ERR_INVALID
    assert lib.srt_accum_gathered(None, C.byref(m)) == ERR_INVALID and lib.srt_gather_last_ms(None, C.byref(a), C.byref(a)) == ERR_INVALID
    assert lib.srt_comm_gather_accum(None, 0) == ERR_INVALID and lib.srt_accum_whole(None, 0, C.byref(C.c_int())) == ERR_INVALID
    assert lib.srt_comm_last_accum_gather_ms(None, C.byref(a), C.byref(a), C.byref(a)) == ERR_INVALID
