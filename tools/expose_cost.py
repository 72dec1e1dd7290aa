#!/usr/bin/env python3
"""Cost of metering and tone mapping on the device, on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080,
depth 16) with a 16-spp accumulation: the meter kernel and the tone kernel (HIP events, srt_expose_last_ms), the whole calls
srt_meter_accum and srt_expose_accum as wall ms (kernel, copies to host memory, synchronise), and the path they replace -- the XYZ sum
planes read to the host, then a numpy histogram, decision and tone curve there (tests/expose_reference.py's operations; the conversion to
sRGB is left out of the host path, which flatters it).  Every figure is the best of --reps (default 5) from this one run.  The host
path's histogram and gain are compared with the device's.  Nothing here is gated.  Prints one line per row and a JSON line.

Usage: python tools/expose_cost.py [--reps 5] [--out FILE]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from _cost_common import DEPTH, H, ROOT, W, best_of, headline_renderer, parse_args, srt, timed, write_report

sys.path.insert(0, os.path.join(ROOT, "tests"))
import expose_reference as R  # noqa: E402

SPP = 16


def main():
    args = parse_args(lambda ap: ap.set_defaults(reps=5))
    r, note = headline_renderer()
    lines = ["expose_cost: random spheres %dx%d, depth %d, %d-spp accumulation; tree: %s" % (W, H, DEPTH, SPP, note)]
    r.set_gather_planes(9)
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    rows = []

    def measure(name, call, which, out_bytes):
        call()          # warm-up (code object, the working blocks' allocation)
        def once():
            wall = timed(r, call)
            return wall, r.expose_last_ms()[which]
        runs = [once() for _ in range(args.reps)]
        row = dict(call=name, kernel_ms=round(min(v[1] for v in runs), 4), call_ms=round(min(v[0] for v in runs), 3), out_bytes=out_bytes)
        rows.append(row)
        lines.append("%-36s kernel %7.4f ms  whole call %8.3f ms  %9d bytes to the host" % (name, row["kernel_ms"], row["call_ms"], out_bytes))

    measure("srt_meter_accum", lambda: r.meter(with_hist=True), "meter", 4096 * 4 + 24)
    dev = r.meter(with_hist=True)
    measure("srt_expose_accum (all three images)", lambda: r.expose(W, H, gain=dev["gain"]), "tone", 9 * W * H * 4)
    tone = srt.tone_config(gain=dev["gain"])
    fb = np.zeros((H, W, 3), np.float32)
    measure("srt_expose_accum (out_q alone)", lambda: r._ck(srt.binding.lib().srt_expose_accum(r._h, C.byref(tone), None, None, srt.binding.fptr(fb), None, W, H)), "tone", 3 * W * H * 4)

    # the path this replaces: the XYZ sums to the host, histogram, decision and tone curve there
    lane = None
    host = {}
    def host_path():
        nonlocal lane
        t0 = time.perf_counter()
        planes = r.read_fb_aux(2)
        t1 = time.perf_counter()
        if lane is None:
            g = r.geom
            j, i = np.divmod(np.arange(W * H), W)
            gbx, gby = i // g["tx"], j // g["ty"]
            lane = (j - gby * g["ty"]) * g["tx"] + (i - gbx * g["tx"]) + g["tx"] * g["ty"] * (gby * g["bx"] + gbx)
        mean = R.mean_xyz(np.stack([p[lane] for p in planes], axis=-1), SPP)
        host["meter"] = R.meter(mean[..., 1])
        t2 = time.perf_counter()
        host["xyz"] = R.tone(mean, host["meter"]["gain"])
        t3 = time.perf_counter()
        return (t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
    r.scatter_tiles()
    host_path()
    best = best_of(args.reps, host_path)
    same = bool(np.array_equal(host["meter"]["hist"], dev["hist"].astype(np.uint64)) and float(host["meter"]["gain"]) == dev["gain"])
    replaced = dict(total_ms=round(best[0], 2), read_ms=round(best[1], 2), meter_ms=round(best[2], 2), tone_ms=round(best[3], 2), plane_bytes=3 * r.geom["n_lanes"] * 4,
                    histogram_and_gain_equal_the_devices=same)
    lines.append("read XYZ planes + numpy (host)        %8.2f ms = %.2f ms read of %d bytes + %.2f ms un-swizzle, histogram and decision + %.2f ms tone curve; "
                 "histogram and gain equal the device's: %s" % (replaced["total_ms"], replaced["read_ms"], replaced["plane_bytes"], replaced["meter_ms"], replaced["tone_ms"], same))
    lines.append("metered: %d pixels, %d dark, %d non-finite; bin %d, y_ref %.6g, gain %.6g" % (dev["metered"], dev["dark"], dev["nonfinite"], dev["bin_ref"], dev["y_ref"], dev["gain"]))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d, %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "rows": rows, "replaced": replaced}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
