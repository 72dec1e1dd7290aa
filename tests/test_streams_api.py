"""Sample-parallel pixels without a GPU: the streamed entry points are declared, bound and exported, the library's gfx950 code object
holds the streamed render kernel (render_kernel<6, ...>) for every shape the launcher picks, and render_streams checks its schedule
before any device is touched."""
import ctypes as C
import os
import re

import pytest

from accum_helpers import ROOT, SHAPES, kernel_id

NEW_SYMBOLS = ("srt_accum_reset_streams", "srt_accum_streams", "srt_comm_accum_reset_streams")
# render_kernel<6, NARROW, ALL_CACHED, PAIRED>
STREAMS_SYM = re.compile(r"^_ZN3srt13render_kernelILi6ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    assert re.search(r"#define\s+SRT_MAX_STREAMS\s+16\b", header)
    assert srt.renderer.MAX_STREAMS == 16
    assert srt.binding.PROTOTYPES["srt_accum_reset_streams"][1][1] is C.c_uint32      # K
    assert "render_streams" in srt.__all__ and callable(srt.render_streams)
    for attr in ("accum_reset_streams", "accum_streams"):
        assert hasattr(srt.Renderer, attr), attr
    assert hasattr(srt.Comm, "accum_reset_streams")


def test_code_object_holds_every_streamed_variant(srt):
    found = set()
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        m = STREAMS_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)
    # ... and the tool that compares two builds kernel by kernel sees them
    assert {k[1:] for k in kernel_id().render_code_hashes(srt.binding.LIB_PATH) if k[0] == 6} == SHAPES


def test_production_kernels_are_still_found_by_kernel_id(srt):
    """the streamed variant is a separate instantiation: the six MODE 0 kernels are all still there for bench.py's hash tie"""
    hs = kernel_id().code_hashes(srt.binding.LIB_PATH)
    assert set(hs) == {(1, 1, 1), (0, 0, 1), (1, 1), (1, 0), (0, 1), (0, 0)}, sorted(hs)


@pytest.mark.parametrize("passes,streams", [
    ([], 4), ([0], 1), ([4, 0, 4], 2), ([-2, 6], 2), ([2.5], 1),      # what render_progressive rejects
    ([6], 4), ([8, 12, 6], 4), ([3], 2), ([15], 16),                   # a pass that K does not divide
    ([4], 0), ([34], 17), ([4], -1), ([4], 2.0), ([4], True), ([4], None),      # K out of range / no whole number
    ([65536], 1), ([40000, 25536], 2), ([65534, 2], 2),                # a total above 65535
])
def test_render_streams_rejects_bad_schedules_before_touching_a_device(srt, passes, streams, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_streams created a device context for a schedule it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_streams(None, None, 16, 16, passes, 8, streams)


def test_render_streams_accepts_the_largest_schedules(srt):
    assert srt.renderer.streams_schedule([65520], 16) == [65520]
    assert srt.renderer.streams_schedule((4, 8, 12), 4) == [4, 8, 12]
    assert srt.renderer.streams_schedule([5, 7], 1) == [5, 7]
