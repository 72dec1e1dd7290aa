"""The device on TRANSFORMED trees against tests/ground_truth.py: trees that went through srt_scene_optimise_bvh, the ray-weighted
reinsertion, srt_scene_order_children, the tuning recipe and the refit on the device are walked by srt_trace_rays and held to the
brute-force float64 hits over every triangle.  No oracle call and no tree on the truth's side: a triangle a reinsertion unhooked, or a
refit that gave a record another triangle's vertex on host and device alike, fails here and nowhere else.  The matrix, the inputs and the
thresholds are those tests/test_ground_truth_reference.py holds the CPU oracle to (tests/tree_truth_cases.py); the oracle's own figures
on every input: 0 rays differ, at most 2 of 20 000 inside the margin, largest |dt| / t_bound 2.02 (3.44 on the axis-aligned set)."""
import numpy as np
import pytest

import ground_truth as G
import tree_truth_cases as TC
from ground_truth import cached, population

pytestmark = pytest.mark.gpu

SRT_ERR_INVALID = -1
FRAME = (1920, 1080)


def _device_hits(gpu, scene, name):
    gpu.upload_scene(scene)
    return gpu.trace_rays(population(name)[1])


@pytest.mark.parametrize("tuning", TC.TUNINGS)
@pytest.mark.parametrize("name", TC.TUNED_POPULATIONS)
def test_tuned_trees_hold(srt, gpu, name, tuning):
    """SAH trees after 3 area-based reinsertion passes, after 3 passes against the first 2 048 rays cut at the truth's t (the tree's hash
    changed in both) and after srt_scene_order_children for an eye on the far side: all 20 000 rays hold.
    Measured on the device: see DEVICE_FIGURES at the end of this file."""
    scene = TC.tuned_scene(srt, name, tuning)
    print(name, tuning, TC.hold(name, population(name)[0]["V"], _device_hits(gpu, scene, name), "%s after %s tuning" % (name, tuning)))


def _device_refits(gpu, name, what, via=None):
    for motion in TC.REFIT_POPULATIONS[name]:
        v = TC.moved_vertices(name, motion)
        gpu.refit(v if via is None else via(v))
        print(name, what, motion, TC.hold(name, v, gpu.trace_rays(population(name)[1]), "%s %s after the device's refit(%s)" % (name, what, motion)))


@pytest.mark.parametrize("mode", TC.BUILDERS)
@pytest.mark.parametrize("name", list(TC.REFIT_POPULATIONS))
def test_device_refit_holds(srt, gpu, name, mode):
    """The built scene is uploaded ONCE; srt_refit_vertices then moves every vertex by N(0, 0.1), applies the smooth sine deformation and
    returns to the first vertices, and after each the 20 000 rays hold to the truth of the vertices the device was given.  (The smooth
    motion of the axis-aligned set is left out: the oracle itself exceeds C_T there, test_oracle_holds_on_refitted_trees.)
    Measured on the device: see DEVICE_FIGURES."""
    gpu.upload_scene(G.product_scene(srt, population(name)[0], mode))
    _device_refits(gpu, name, "mode %d" % mode)


def test_device_refit_through_the_device_pointer_holds(srt, gpu):
    """soup_200_spread_2.0 (98 % of the rays hit), SAH tree: the same three motions through srt_refit_vertices_dev with torch tensors"""
    import torch
    name = "soup_200_spread_2.0"
    gpu.upload_scene(G.product_scene(srt, population(name)[0], TC.BVH_SAH))
    dev = torch.device("cuda", 0)
    _device_refits(gpu, name, "device pointer", via=lambda v: torch.from_numpy(v).to(dev))


def test_tuned_then_device_refit_holds(srt, gpu):
    """soup_200_spread_0.5: the ray-weighted reinsertion, the upload, then the jitter refit on the device"""
    name = "soup_200_spread_0.5"
    gpu.upload_scene(TC.tuned_scene(srt, name, "rays"))
    v = TC.moved_vertices(name, "jitter")
    gpu.refit(v)
    print(name, TC.hold(name, v, gpu.trace_rays(population(name)[1]), "%s, ray tuned then refitted on the device" % name))


@pytest.mark.parametrize("name", ["soup_200_spread_2.0", "sheet_12x12"])
def test_the_recipe_holds(srt, gpu, name):
    """srt_tune_tree_for_throughput, gated, for a 1920 x 1080 frame at depth 16, as the front ends call it: whichever branch it reports
    (reinsertion undone, kept, vetoed or without a usable segment; child order profiled or refused), the tree it leaves holds all 20 000
    rays.  These scenes keep the library's default camera, which has them in a corner of its frame: should srt_order_children_by_profile
    refuse because its probe frame records no sample (first item), the printed line says so, and the hits are checked all the same.
    Measured on the device: see DEVICE_FIGURES."""
    scene = G.product_scene(srt, population(name)[0], TC.BVH_SAH)
    before = TC.tree_sha(scene)
    gpu.upload_scene(scene)
    t = srt.tree_tuning(gpu, scene, FRAME[0], FRAME[1], 16, gate=True)
    message = (srt.binding.lib().srt_last_error(gpu._h) or b"").decode()
    refused = t["order_status"] != 0
    print("%s: tree tuning %r; tree %s; child order %s" % (name, t, "changed" if TC.tree_sha(scene) != before else "as built",
          ("REFUSED (%s)" % message) if refused else "profiled, %d nodes swapped" % t["nodes_swapped"]))
    assert t["throughput_bound"] == 1 and t["reinsertion"] in (2, 3, 4, 5)
    if refused:         # the one refusal that is no fault: nothing was there to profile
        assert t["order_status"] == SRT_ERR_INVALID and "recorded no samples" in message and t["nodes_swapped"] == 0
    if t["reinsertion"] != 3 and not t["nodes_swapped"]:
        assert TC.tree_sha(scene) == before, "the report says that the tree is as it walked in"
    print(name, TC.hold(name, population(name)[0]["V"], _device_hits(gpu, scene, name), "%s after the recipe" % name))


def test_edge_aimed_rays_hold_on_the_refitted_sheet(srt, gpu):
    """The 10 712 rays aimed at vertices and edges of the sheet, on the device after refit(jittered vertices), refit(first vertices): the
    triangle records are rebuilt from the vertices twice, and every ray still hits a triangle adjacent to its target, within the t bound,
    or leaks -- none hits another triangle.  Measured on the device: see DEVICE_FIGURES (a fresh upload: 9.3 % leak)."""
    sc = G.bumpy_sheet()[0]
    rays, adjacent = cached("edge_rays", G.edge_aimed_rays)
    v0 = np.ascontiguousarray(sc["V"], np.float32)
    gpu.upload_scene(G.product_scene(srt, sc, TC.BVH_SAH))
    gpu.refit(TC.moved_vertices("sheet_12x12", "jitter"))
    gpu.refit(v0)
    s = G.assert_edge_aimed_hold(G.f64(v0), rays, adjacent, gpu.trace_rays(rays), "edge-aimed rays after two device refits")
    print("edge-aimed rays after two device refits: %d of %d leak (%.2f %%)" % (s["leaks"], s["rays"], 100 * s["leak_share"]), s)


DEVICE_FIGURES = """Measured on one MI355X (20 000 rays per line; `in` = rays inside the edge margin, `c` = largest |dt| / t_bound).  Every figure equals the
oracle's on the same input (tests/test_ground_truth_reference.py), digit for digit:

  tuned trees, area / rays / order alike     soup_200_spread_0.5  0 differ, in 1, c 1.643      sheet_12x12         0 differ, in 0, c 1.818
                                             axis_aligned_and_sticky 0 differ, in 0, c 3.441   soup_30_spread_2.0  0 differ, in 0, c 1.802
  device refit, both builders alike          jitter                  smooth                  return
    soup_200_spread_0.5                      0 differ, in 0, c 2.017  0 differ, in 0, c 1.673  0 differ, in 1, c 1.643
    soup_200_spread_2.0 (and device pointer) 0 differ, in 1, c 1.792  0 differ, in 1, c 1.898  0 differ, in 2, c 1.986
    sheet_12x12                              0 differ, in 0, c 1.715  0 differ, in 1, c 1.685  0 differ, in 0, c 1.818
    soup_30_spread_0.5                       0 differ, in 0, c 1.266  0 differ, in 0, c 1.340  0 differ, in 0, c 1.430
    axis_aligned_and_sticky                  0 differ, in 0, c 1.637  --                      0 differ, in 0, c 3.441
  ray tuned, then device refit (jitter)      soup_200_spread_0.5  0 differ, in 0, c 2.017
  the recipe, 1920 x 1080, depth 16, gated   soup_200_spread_2.0  7.91 pixels per lane, reinsertion 3 (kept, 2 048 segments), probe 480 x 270 x 8,
                                                                  3 nodes swapped, order_status 0; tree changed; 0 differ, in 2, c 1.986
                                             sheet_12x12          reinsertion 4 (vetoed), 0 nodes swapped, order_status 0; tree as built;
                                                                  0 differ, in 0, c 1.818
                                             (the default camera sees both scenes in a corner of its frame: no refusal occurred)
  edge-aimed rays after refit(jitter), refit(first vertices)     999 of 10 712 leak (9.33 %, a fresh upload's share), c 1.708, none hits a
                                                                  triangle that is not adjacent to its target
  the 39 tests of this file and of tests/test_tree_rays_gpu.py   9.4 s together, the slowest 0.7 s"""
