"""The transformed trees both truth suites walk: the CPU oracle in tests/test_ground_truth_reference.py, the device in
tests/test_tree_truth.py -- the same populations, the same transforms, the same moved vertices, so that what the reference alone
achieves against tests/ground_truth.py is measured on exactly the inputs the device is held to.  Host side only."""
import hashlib

import numpy as np

import ground_truth as G
import refit_cases as R
from ground_truth import cached, population

FLT_MAX = float(np.finfo(np.float32).max)
BVH_SAH = 1
N_SEGMENTS = 2048

TUNED_POPULATIONS = ("soup_200_spread_0.5", "sheet_12x12", "axis_aligned_and_sticky", "soup_30_spread_2.0")
TUNINGS = ("area", "rays", "order")            # optimise_bvh(3), optimise_bvh_for_rays(truth segments, 3), order_children(FAR_EYE)
# A scene that comes in through the raw-array boundary keeps the library's default camera, whose eye (278, 278, -800) the SAH builder
# orders every node's children for; the populations lie about the origin: this eye looks at them from the opposite side.
FAR_EYE = (-278.0, -278.0, 800.0)

MOTIONS = ("jitter", "smooth", "return")       # applied one after the other to ONE scene: refit(jitter), refit(smooth), refit(v0)
# the smooth motion is left out for the axis-aligned set: see test_oracle_holds_on_refitted_trees' docstring
REFIT_POPULATIONS = {"soup_200_spread_0.5": MOTIONS, "soup_200_spread_2.0": MOTIONS, "sheet_12x12": MOTIONS, "soup_30_spread_0.5": MOTIONS,
                     "axis_aligned_and_sticky": ("jitter", "return")}
BUILDERS = (0, 1)                              # BVH_REFERENCE, BVH_SAH


def tree_sha(scene):
    h = hashlib.sha256()
    for a in scene.bvh():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def truth_segments(name):
    """the population's first 2 048 rays cut at the truth's closest hit (FLT_MAX on a miss), (2048, 7) float32"""
    def make():
        sc, rays = population(name)
        r = rays[:N_SEGMENTS]
        t = G.closest_hit(G.f64(sc["V"]), G.f64(r[:, :3]), G.f64(r[:, 3:]))[0]
        with np.errstate(over="ignore"):
            return np.concatenate([r, np.where(np.isfinite(t), t, FLT_MAX).astype(np.float32)[:, None]], axis=1).astype(np.float32)
    return cached(("segments", name), make)


def tuned_scene(srt, name, tuning):
    """the population's SAH tree through one tuning step; the hash of the tree must have changed for the two reinsertions"""
    scene = G.product_scene(srt, population(name)[0], BVH_SAH)
    before = tree_sha(scene)
    if tuning == "area":
        scene.optimise_bvh(3)
    elif tuning == "rays":
        segs = truth_segments(name)
        assert (segs[:, 6] > 0).all() and 0 < (segs[:, 6] < FLT_MAX).sum() < len(segs)
        scene.optimise_bvh_for_rays(segs, 3)
    else:
        assert tuning == "order", tuning
        scene.order_children(FAR_EYE)
    if tuning != "order":
        assert tree_sha(scene) != before, "%s: %s tuning left the tree as it was" % (name, tuning)
    return scene


def moved_vertices(name, motion):
    """(n, 3, 3) float32: the population's vertices after `motion`"""
    v0 = np.ascontiguousarray(population(name)[0]["V"], np.float32)
    return {"jitter": lambda: R.jitter(v0, 3, 0.1), "smooth": lambda: R.smooth(v0), "return": lambda: v0.copy()}[motion]()


def hold(name, V, got, what):
    """G.assert_hits_hold for the population's 20 000 rays against the truth of the vertices V -> summary"""
    return G.assert_hits_hold(G.f64(V), population(name)[1], got, what)[1]
