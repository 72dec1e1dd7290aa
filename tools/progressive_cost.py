#!/usr/bin/env python3
"""Cost of progressive rendering on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16,
1024 spp): one frame rendered as a plain launch (srt_render_chunk, 1 x 1024) and as accumulations (srt_render_chunk_accum) of
1 x 1024, 4 x 256, 16 x 64 and 64 x 16 samples.  For each schedule: wall ms per frame (first pass enqueued .. last pass done, cost
probe and header writes included), ms per pass, and the render kernels' own ms (HIP events, summed over the passes); the best of
--reps frames.  Every schedule must end on the same framebuffer (checksum of the quantised planes, as bench.py prints it): the
accumulation is exact, so a differing checksum is an error, not noise.  Prints one line per schedule and a JSON line.

Usage: python tools/progressive_cost.py [--reps 3] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
srt = importlib.import_module("cuda-spectral-ray-tracer_amd")

W, H, DEPTH, SPP = 1920, 1080, 16, 1024
SCHEDULES = [("plain", 1, 1024), ("accum", 1, 1024), ("accum", 4, 256), ("accum", 16, 64), ("accum", 64, 16)]


def frame(r, kind, n_pass, spp):
    """one frame of the schedule from a freshly seeded grid; returns (wall ms, summed kernel ms)"""
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.synchronize()
    kms = 0.0
    t0 = time.perf_counter()
    if kind == "plain":
        r.render_chunk(W, H)
        kms += r.last_kernel_ms()          # (waits for the launch's end event)
    else:
        r.accum_reset()
        for _ in range(n_pass):
            r.render_chunk_accum(W, H, spp)
            kms += r.last_kernel_ms()      # one pass in flight at a time: the event pair brackets this pass's kernel
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3, kms


def checksum(r):
    r.scatter_tiles()
    return int(sum(int(p.astype("int64").sum()) for p in r.read_fb()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    r = srt.Renderer(0)
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    note = srt.tune_tree_for_throughput(r, scene, W, H, DEPTH)
    r.upload_scene(scene)
    r.set_camera(scene.default_camera(W, H))
    r.set_partition(0, 1)
    lines = ["progressive_cost: random spheres %dx%d, depth %d, %d spp; tree: %s" % (W, H, DEPTH, SPP, note),
             "plan: %r" % (r.launch_plan(),)]
    frame(r, "plain", 1, SPP)          # warm-up (code objects, clocks)
    rows, ref_sum = [], None
    for kind, n_pass, spp in SCHEDULES:
        best = None
        for _ in range(args.reps):
            wall, kms = frame(r, kind, n_pass, spp)
            if best is None or wall < best[0]:
                best = (wall, kms)
        cs = checksum(r)
        ref_sum = cs if ref_sum is None else ref_sum
        row = dict(schedule="%s %dx%d" % (kind, n_pass, spp), frame_ms=round(best[0], 2), ms_per_pass=round(best[0] / n_pass, 3),
                   kernel_ms=round(best[1], 2), kernel_ms_per_pass=round(best[1] / n_pass, 3), fb_checksum=cs)
        rows.append(row)
        if cs != ref_sum:
            raise SystemExit("progressive_cost: %s ends on checksum %d, the plain frame on %d: the accumulation is not exact" % (row["schedule"], cs, ref_sum))
    base = rows[0]["frame_ms"]
    for row in rows:
        row["frame_vs_plain_pct"] = round(100.0 * (row["frame_ms"] / base - 1.0), 2)
        lines.append("%-16s frame %9.2f ms (%+6.2f %% vs plain)  per pass %8.3f ms  kernel %9.2f ms (%8.3f per pass)  checksum %d" %
                     (row["schedule"], row["frame_ms"], row["frame_vs_plain_pct"], row["ms_per_pass"], row["kernel_ms"], row["kernel_ms_per_pass"], row["fb_checksum"]))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "rows": rows}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    r.close()


if __name__ == "__main__":
    main()
