"""Progressive rendering without a GPU: the accumulating entry points are declared, bound and exported, the library's gfx950 code
object holds the accumulating render kernel (render_kernel<3, ...>) for every shape the launcher picks, and render_progressive
checks its schedule before any device is touched."""
import ctypes as C
import os
import re

import pytest

from accum_helpers import ROOT, SHAPES, kernel_id

NEW_SYMBOLS = ("srt_accum_reset", "srt_render_chunk_accum", "srt_accum_samples", "srt_comm_accum_reset", "srt_render_frame_multi_accum")
# render_kernel<3, NARROW, ALL_CACHED, PAIRED>
ACCUM_SYM = re.compile(r"^_ZN3srt13render_kernelILi3ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")


def test_new_symbols_are_declared_bound_and_exported(srt):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    L = C.CDLL(srt.binding.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"SRT_API\s+int\s+%s\s*\(" % name, header), name
        assert name in srt.binding.PROTOTYPES, name
        assert getattr(L, name) is not None
    assert srt.binding.PROTOTYPES["srt_render_chunk_accum"][1][5] is C.c_uint32      # spp_add
    assert "render_progressive" in srt.__all__ and callable(srt.render_progressive)
    for attr in ("accum_reset", "render_chunk_accum", "accum_samples"):
        assert hasattr(srt.Renderer, attr), attr
    for attr in ("accum_reset", "render_frame_accum"):
        assert hasattr(srt.Comm, attr), attr


def test_code_object_holds_every_accumulating_variant(srt):
    found = set()
    for name, _ in kernel_id().gfx950_functions(srt.binding.LIB_PATH):
        m = ACCUM_SYM.match(name)
        if m:
            found.add(tuple(int(g) for g in m.groups()))
    assert found == SHAPES, sorted(found)


def test_production_kernels_are_still_found_by_kernel_id(srt):
    """the accumulating variant is a separate instantiation: the six MODE 0 kernels are all still there for bench.py's hash tie"""
    hs = kernel_id().code_hashes(srt.binding.LIB_PATH)
    assert set(hs) == {(1, 1, 1), (0, 0, 1), (1, 1), (1, 0), (0, 1), (0, 0)}, sorted(hs)


@pytest.mark.parametrize("passes", [[], (), [0], [4, 0, 4], [-1, 5], [2.5], [65536], [40000, 25536], [1] * 65535 + [1]])
def test_render_progressive_rejects_bad_schedules_before_touching_a_device(srt, passes, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("render_progressive created a device context for a schedule it must reject")
    monkeypatch.setattr(srt.renderer, "Renderer", no_device)
    with pytest.raises(ValueError):
        srt.render_progressive(None, None, 16, 16, passes, 8)


def test_render_progressive_accepts_the_largest_total(srt):
    assert srt.renderer.progressive_schedule([65000, 535]) == [65000, 535]
    assert srt.renderer.progressive_schedule((1, 1, 10)) == [1, 1, 10]
