#!/usr/bin/env python3
"""Cost and quality of sample-parallel pixels (srt_accum_reset_streams): every case renders one frame as a plain accumulation
(srt_accum_reset, one pass) and as streamed accumulations of K streams per pixel, all in this run, on the random-spheres scene at
depth 16:

  cfg2       1280x720 x 256 spp (BASELINE cfg 2: 3.5 pixels per lane), K = 1, 2, 4, 8, 16
  headline   1920x1080 x 1024 spp, K = 1, 4, 8
  pass64     one 64-spp pass at 1920x1080, K = 1, 4, 8
  pass16     one 16-spp pass at 1920x1080, K = 1, 4, 8
  w8-rank0   rank 0's share of the 8-rank headline frame (as tools/world_emulation.py renders it), K = 1, 8
  quality    RMSE of the quantised planes of the plain and the K = 8 1024-spp headline frames against one plain 4096-spp frame of
             another seed (independent of both)

Per row: the best of --reps frames (wall ms from the reset's end to the pass's end: header write, cost probe, render kernel and, when
streamed, the combine kernel), the spread of the repetitions (max - min, the noise of the row), the render kernel's own ms (HIP
events), and the frame against the plain accumulation of the same case.  K = 1 must end on the plain frame's checksum.

Usage: python tools/streams_cost.py [--reps 3] [--out FILE] [--cases cfg2,headline,pass64,pass16,w8-rank0,quality]"""
import json
import time

import numpy as np

from _cost_common import DEPTH, H, W, checksum, parse_args, srt, write_report

CASES = {      # name: (width, height, spp, world, the K's)
    "cfg2": (1280, 720, 256, 1, (1, 2, 4, 8, 16)),
    "headline": (W, H, 1024, 1, (1, 4, 8)),
    "pass64": (W, H, 64, 1, (1, 4, 8)),
    "pass16": (W, H, 16, 1, (1, 4, 8)),
    "w8-rank0": (W, H, 1024, 8, (1, 8)),
}


def frame(r, w, h, spp, k, seed=1984):
    """one single-pass frame from a freshly seeded grid: k = 0 a plain accumulation, k > 0 one of k streams; (wall ms, kernel ms)"""
    r.init_device_params(w, h, spp, DEPTH, seed)
    if k:
        r.accum_reset_streams(k)
    else:
        r.accum_reset()
    r.synchronize()
    t0 = time.perf_counter()
    r.render_chunk_accum(w, h, spp)
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3, r.last_kernel_ms()


def tree_for(r, w, h, world):
    """the tree bench.py renders the frame with: tuned for throughput unless the launch is chain-bound (world_emulation.py)"""
    s = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    note = srt.tune_tree_for_throughput(r, s, w, h, DEPTH, world=world, gate=True)
    return s, note


def quantised(r, w, h):
    r.scatter_tiles()
    return np.stack(r.read_fb_rowmajor(w, h)).astype(np.float64)


def main():
    args = parse_args(lambda ap: ap.add_argument("--cases", default=",".join(list(CASES) + ["quality"])))
    cases = args.cases.split(",")
    r = srt.Renderer(0)
    lines, rows = ["streams_cost: random spheres, depth %d, best of %d" % (DEPTH, args.reps)], []
    for name in cases:
        if name == "quality":
            continue
        w, h, spp, world, ks = CASES[name]
        scene, note = tree_for(r, w, h, world)
        r.upload_scene(scene); r.set_camera(scene.default_camera(w, h)); r.set_partition(0, world)
        lines.append("%s: %dx%d x %d spp, rank 0 of %d; tree: %s; %.2f pixels per lane" % (name, w, h, spp, world, note, srt.pixels_per_lane(r, w, h, world)))
        frame(r, w, h, min(spp, 16), 0)          # warm-up (code objects, clocks)
        base, base_sum = None, None
        for k in (0,) + tuple(ks):
            reps = [frame(r, w, h, spp, k) for _ in range(args.reps)]
            best = min(reps)
            cs = checksum(r) if world == 1 else None
            row = dict(case=name, schedule="plain accum" if k == 0 else "K = %d" % k, frame_ms=round(best[0], 2), kernel_ms=round(best[1], 2),
                       spread_ms=round(max(x[0] for x in reps) - min(x[0] for x in reps), 2), fb_checksum=cs)
            if k == 0:
                base, base_sum = best[0], cs
            if k == 1 and cs != base_sum:
                raise SystemExit("streams_cost: K = 1 ends on checksum %r, the plain accumulation on %r: not exact" % (cs, base_sum))
            row["vs_plain_pct"] = round(100.0 * (best[0] / base - 1.0), 2)
            rows.append(row)
            lines.append("  %-12s frame %9.2f ms (%+7.2f %% vs plain accum)  spread %6.2f ms  kernel %9.2f ms  checksum %s" %
                         (row["schedule"], row["frame_ms"], row["vs_plain_pct"], row["spread_ms"], row["kernel_ms"], cs))
    if "quality" in cases:
        scene, note = tree_for(r, W, H, 1)
        r.upload_scene(scene); r.set_camera(scene.default_camera(W, H)); r.set_partition(0, 1)
        frame(r, W, H, 4096, 0, seed=1984 + 500000000)      # (seeds beyond every stream of the two frames: an independent reference)
        ref = quantised(r, W, H)
        q = {}
        for label, k in (("plain accum", 0), ("K = 8", 8)):
            frame(r, W, H, 1024, k)
            q[label] = float(np.sqrt(np.mean((quantised(r, W, H) - ref) ** 2)))
        rows.append(dict(case="quality", rmse_vs_4096spp=q))
        lines.append("quality: RMSE of the quantised 1920x1080 x 1024 spp planes against one plain 4096-spp frame (0 .. 255 scale): " +
                     ", ".join("%s %.4f" % kv for kv in q.items()))
    lines.append(json.dumps({"reps": args.reps, "rows": rows}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
