#!/usr/bin/env python3
"""Cost of developing the spectral film on the device, on the headline workload (random spheres, the throughput-tuned SAH tree,
1920x1080, depth 16) with a 16-spp spectral accumulation: srt_develop_spectral at K = 1, 3 and 16 channels and the sRGB variant, each as
the kernels' own ms (HIP events, srt_develop_last_ms) and the whole call's wall ms (upload of the curves, kernel, copy of the K planes
to host memory), and the path they replace -- a full srt_read_spectral plus film_to_xyz's float64 contraction on the host.  Every figure
is the best of --reps (default 5) from this one run.  The K = 3 planes developed with the colour-matching rows are compared with the
host path's.  Prints one line per row and a JSON line.

Usage: python tools/develop_cost.py [--reps 5] [--out FILE]"""
import json
import time

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, timed, write_report

SPP = 16
FILM_BYTES = W * H * 96 * 4      # what the kernel reads: 384 B per pixel


def main():
    args = parse_args(lambda ap: ap.set_defaults(reps=5))
    r, note = headline_renderer()
    lines = ["develop_cost: random spheres %dx%d, depth %d, %d-spp spectral accumulation; tree: %s" % (W, H, DEPTH, SPP, note)]
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_spectral()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    cie = srt.renderer.cie_response()
    rng = np.random.default_rng(1)
    rows = []

    def measure(name, call, planes):
        call()          # warm-up (code object, the working blocks' allocation)
        def once():
            wall = timed(r, call)
            ms = r.develop_last_ms()
            return wall, ms["contract"], ms["epilogue"]
        runs = [once() for _ in range(args.reps)]
        wall, kern = min(v[0] for v in runs), (min(v[1] for v in runs), min(v[2] for v in runs))      # each figure's own best
        row = dict(call=name, kernel_ms=round(kern[0], 4), epilogue_ms=round(kern[1], 4), call_ms=round(wall, 3), out_bytes=planes * W * H * 4,
                   film_gb_per_s=round(FILM_BYTES / (kern[0] * 1e-3) / 1e9, 1))
        rows.append(row)
        lines.append("%-34s kernel %7.4f ms (film read at %7.1f GB/s)  epilogue %7.4f ms  whole call %8.3f ms  %9d bytes out"
                     % (name, row["kernel_ms"], row["film_gb_per_s"], row["epilogue_ms"], row["call_ms"], row["out_bytes"]))

    for k in (1, 3, 16):
        resp = cie if k == 3 else rng.random((k, 95)).astype(np.float32)
        measure("srt_develop_spectral K = %d" % k, lambda resp=resp: r.develop_spectral(W, H, resp, srt.renderer.CIE_SCALE), k)
    measure("srt_develop_spectral_srgb", lambda: r.develop_spectral_srgb(W, H), 9)

    # the path this replaces: the whole film to the host, contracted there in float64
    film = np.zeros((H, W, 95), np.float32)
    host = {}
    def host_path():
        t0 = time.perf_counter()
        r.read_spectral(W, H, into=film)
        t1 = time.perf_counter()
        host["xyz"] = srt.film_to_xyz(film)
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3
    best = best_of(args.reps, host_path)
    dev = r.develop_spectral(W, H, cie, srt.renderer.CIE_SCALE).astype(np.float64)
    ok = np.isfinite(host["xyz"]) & np.isfinite(dev)
    rel = float(np.abs(dev[ok] - host["xyz"][ok]).max() / np.abs(host["xyz"][ok]).max())
    replaced = dict(total_ms=round(best[0], 2), read_ms=round(best[1], 2), contract_ms=round(best[0] - best[1], 2), film_bytes=film.nbytes, max_diff_rel_to_peak=rel)
    lines.append("read_spectral + film_to_xyz (host)   %8.2f ms = %.2f ms read of %d bytes + %.2f ms float64 contraction; device K = 3 vs host: %.1e of the peak"
                 % (replaced["total_ms"], replaced["read_ms"], film.nbytes, replaced["contract_ms"], rel))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d, %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "rows": rows, "replaced": replaced}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
