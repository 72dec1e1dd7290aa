"""The ray queries with their traversal stacks driven to the last slot: the shelves of tests/traversal_limit_cases.py, whose grazing rays meet
every box and no triangle, so a lane holds exact_occupancy(tree) entries at once -- on the tight cases the last of the stack_depth + 2 slots
query_kernel gives every lane (one LDS stack per wave, as render_kernel's).  Grazing and striking rays alternate lane by lane.

Both query kinds, over [0, FLT_MAX] (the striking rays hit; the grazing ones walk the whole tree and miss), without a knob and under every
knob set of tests/test_traversal_limits.py: the closest query equals srt_trace_rays word for word -- which tests/test_traversal_limits.py
holds to the oracle on the same rays -- and occluded equals its hit / miss.  Every case of the file: no truth is walked here, so even the
piles of 32 768 and 32 769 shelves (the plan's own <1,0> and <0,0> shapes, 14 slots) take seconds."""
import numpy as np
import pytest

import query_reference as Q
import traversal_limit_cases as L
from helpers import bits
from test_traversal_limits import KNOBS, _assert_shape, _knob_id, _knobs

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_queries_at_full_occupancy(srt, gpu, name):
    case, scene = L.CASE[name], L.built(srt, name)
    six, grazing = L.interleaved_rays(L.top_of(L.vertices_of(name)))
    rays = Q.rows(six[:, 0:3], six[:, 3:6], 0.0, Q.FLT_MAX)
    for knobs in KNOBS:
        with _knobs(gpu, scene, knobs):
            plan = _assert_shape(gpu, scene, case, knobs)
            trace = gpu.trace_rays(six)
            hits = gpu.intersect(rays)
            q = gpu.query_last()
            occ = gpu.occluded(rays)
            qa = gpu.query_last()
        what = "%s, %s" % (name, _knob_id(knobs))
        for info, any_query in ((q, False), (qa, True)):
            assert (info["narrow_refs"], info["all_cached"], info["paired"], info["n_cached"], info["any"]) == (
                plan["narrow_refs"], plan["all_cached"], plan["paired"], plan["n_cached"], any_query), (what, info, plan)
        assert np.array_equal(bits(hits), bits(trace)), "%s: %d words differ from srt_trace_rays" % (what, (bits(hits) != bits(trace)).sum())
        assert np.array_equal(occ, trace[:, 1] >= 0), what
        if not case.duplicates:
            assert np.array_equal(trace[:, 1] >= 0, ~grazing), what
    print("%-26s occupancy %2d of %2d slots in use, both queries equal srt_trace_rays under %d knob sets" % (
        name, L.exact_occupancy(scene), L.loose_bound(scene), len(KNOBS)))
