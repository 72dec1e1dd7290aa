#!/usr/bin/env python3
"""Cost of the first-hit feature buffers on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16): a
plain accumulation (srt_accum_reset, render_kernel MODE 3) against a featured one (srt_accum_reset_features, MODE 7), each as 1 x 1024
samples and as a single 64-spp pass, in the same run.  The MODE 3 kernels are byte for byte those of the commit before the features
(tools/accum_kernel_id.py compares two builds), so the plain rows are that commit's kernels.  For each: wall ms per frame (first pass
enqueued .. last pass done, cost probe and header writes included) and the render kernels' own ms (HIP events), the best of --reps
frames; both kinds must end on the same framebuffer checksum (the deposit touches neither the image nor the RNG streams).  Then the time
and bytes of a full-frame srt_read_features (device un-swizzle + copy to the host), the best of --reps reads.  Prints one line per row
and a JSON line.

Usage: python tools/features_cost.py [--reps 3] [--out profiles/features/features_cost_headline.txt]"""
import json
import time

import numpy as np

from _cost_common import DEPTH, H, W, best_of, checksum, headline_renderer, parse_args, srt, write_report

SCHEDULES = [("accum", 1, 1024), ("features", 1, 1024), ("accum", 1, 64), ("features", 1, 64)]


def frame(r, kind, n_pass, spp):
    """one frame of the schedule from a freshly seeded grid; returns (wall ms, summed kernel ms)"""
    r.init_device_params(W, H, n_pass * spp, DEPTH, 1984)
    r.synchronize()
    kms = 0.0
    t0 = time.perf_counter()
    if kind == "features":
        r.accum_reset_features()
    else:
        r.accum_reset()
    for _ in range(n_pass):
        r.render_chunk_accum(W, H, spp)
        kms += r.last_kernel_ms()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3, kms


def main():
    args = parse_args()
    r, note = headline_renderer()
    lines = ["features_cost: random spheres %dx%d, depth %d; tree: %s" % (W, H, DEPTH, note), "plan: %r" % (r.launch_plan(),)]
    frame(r, "features", 1, 16)          # warm-up (code objects, clocks, the rows' first allocation)
    rows, sums = [], {}
    for kind, n_pass, spp in SCHEDULES:
        best = best_of(args.reps, lambda: frame(r, kind, n_pass, spp))
        cs = checksum(r)
        key = n_pass * spp
        sums.setdefault(key, cs)
        if cs != sums[key]:
            raise SystemExit("features_cost: %s %dx%d ends on checksum %d, the plain accumulation on %d" % (kind, n_pass, spp, cs, sums[key]))
        rows.append(dict(schedule="%s %dx%d" % (kind, n_pass, spp), frame_ms=round(best[0], 2), kernel_ms=round(best[1], 2), fb_checksum=cs))
    for row in rows:
        base = next(x for x in rows if x["schedule"] == row["schedule"].replace("features", "accum"))
        row["frame_vs_mode3_pct"] = round(100.0 * (row["frame_ms"] / base["frame_ms"] - 1.0), 2)
        row["kernel_vs_mode3_pct"] = round(100.0 * (row["kernel_ms"] / base["kernel_ms"] - 1.0), 2)
        lines.append("%-18s frame %9.2f ms (%+6.2f %% vs MODE 3)  kernel %9.2f ms (%+6.2f %%)  checksum %d" %
                     (row["schedule"], row["frame_ms"], row["frame_vs_mode3_pct"], row["kernel_ms"], row["kernel_vs_mode3_pct"], row["fb_checksum"]))
    # the last frame is a featured one: read all its rows
    def read():
        t0 = time.perf_counter()
        read.out = r.read_features(W, H)
        return (time.perf_counter() - t0) * 1e3
    best = best_of(args.reps, read)
    nbytes = W * H * 8 * 4
    means = srt.feature_means(read.out, 64)
    cover = float(means["coverage"].mean())
    rd = dict(ms=round(best, 2), bytes=nbytes, gb_per_s=round(nbytes / (best * 1e-3) / 1e9, 2), mean_coverage=round(cover, 6))
    lines.append("srt_read_features full frame: %.2f ms for %d bytes (%.2f GB/s to host memory, the split into four arrays included); mean coverage %.4f"
                 % (rd["ms"], nbytes, rd["gb_per_s"], cover))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d" % (W, H, DEPTH), "reps": args.reps, "rows": rows, "read_features": rd}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
