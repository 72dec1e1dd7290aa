"""The skeleton of the accumulation cost tools (progressive_cost.py, adaptive_cost.py, spectral_cost.py, streams_cost.py): the headline workload
(random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16) on one device context, the framebuffer checksum as bench.py
prints it, the best of --reps measurements, and the report (printed, and written with --out)."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
srt = importlib.import_module("cuda-spectral-ray-tracer_amd")

W, H, DEPTH = 1920, 1080, 16


def parse_args(more=None):
    """--reps and --out; more(parser) adds a tool's own arguments"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    if more:
        more(ap)
    return ap.parse_args()


def headline_renderer():
    """(device context with the headline scene, camera and the whole frame as its partition; the tree tuning's note)"""
    r = srt.Renderer(0)
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    note = srt.tune_tree_for_throughput(r, scene, W, H, DEPTH)
    r.upload_scene(scene)
    r.set_camera(scene.default_camera(W, H))
    r.set_partition(0, 1)
    return r, note


def timed(r, fn):
    """wall ms of fn() on an idle device, its work waited for"""
    r.synchronize()
    t0 = time.perf_counter()
    fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def checksum(r):
    r.scatter_tiles()
    return int(sum(int(p.astype("int64").sum()) for p in r.read_fb()))


def best_of(reps, fn):
    """the measurement with the least wall ms (a number, or a tuple that starts with it) of `reps` calls of fn; the first of equals"""
    return min((fn() for _ in range(reps)), key=lambda v: v[0] if isinstance(v, tuple) else v)


def write_report(lines, out):
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
