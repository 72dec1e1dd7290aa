#!/usr/bin/env python3
"""Cost of progressive rendering on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16,
1024 spp): one frame rendered as a plain launch (srt_render_chunk, 1 x 1024) and as accumulations (srt_render_chunk_accum) of
1 x 1024, 4 x 256, 16 x 64 and 64 x 16 samples.  For each schedule: wall ms per frame (first pass enqueued .. last pass done, cost
probe and header writes included), ms per pass, and the render kernels' own ms (HIP events, summed over the passes); the best of
--reps frames.  Every schedule must end on the same framebuffer (checksum of the quantised planes, as bench.py prints it): the
accumulation is exact, so a differing checksum is an error, not noise.  Prints one line per schedule and a JSON line.

Usage: python tools/progressive_cost.py [--reps 3] [--out FILE]"""
import json
import time

from _cost_common import DEPTH, H, W, best_of, checksum, headline_renderer, parse_args, write_report

SPP = 1024
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


def main():
    args = parse_args()
    r, note = headline_renderer()
    lines = ["progressive_cost: random spheres %dx%d, depth %d, %d spp; tree: %s" % (W, H, DEPTH, SPP, note),
             "plan: %r" % (r.launch_plan(),)]
    frame(r, "plain", 1, SPP)          # warm-up (code objects, clocks)
    rows, ref_sum = [], None
    for kind, n_pass, spp in SCHEDULES:
        best = best_of(args.reps, lambda: frame(r, kind, n_pass, spp))
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
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
