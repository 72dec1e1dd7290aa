#!/usr/bin/env python3
"""Cost of spectral featured accumulations (srt_accum_reset_spectral_features, render_kernel MODE 9) and of the denoised developed film
(srt_denoise_developed) on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16).  Every figure
comes from this one run:

 * the render kernel's ms of a 16-spp pass of a spectral featured accumulation (MODE 9) next to the same pass of a spectral (MODE 5) and
   of a featured (MODE 7) accumulation, the best of --reps each;
 * on one 16-spp spectral featured accumulation, the kernel-only ms of srt_denoise_developed at K = 1, 3 and 16 (HIP events around each
   kernel, the best of --reps): both prepasses, the five payload levels, both output kernels and the develop contraction, next to the
   plain srt_denoise_features' prepass, levels and epilogue;
 * the whole call's wall ms (the copy of the results to the host included) for the same K, next to srt_denoise_features'.

Nothing is gated.  Prints one line per row and a JSON line.

Usage: python tools/denoise_developed_cost.py [--reps 5] [--out profiles/denoise_developed/denoise_developed_cost_headline.txt]"""
import json
import sys

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, timed, write_report

SPP = 16
CHANNELS = (1, 3, 16)


def pass_kernel_ms(r, reset, reps):
    """the render kernel's ms of a 16-spp first pass after reset()"""
    def once():
        r.init_device_params(W, H, SPP, DEPTH, 1984)
        reset()
        r.render_chunk_accum(W, H, SPP)
        r.synchronize()
        return r.last_kernel_ms()
    once()      # warm-up
    return best_of(reps, once)


def main():
    args = parse_args()
    r, note = headline_renderer()
    lines = ["denoise_developed_cost: random spheres %dx%d, depth %d; tree: %s" % (W, H, DEPTH, note)]

    # ---- the pass: MODE 9 next to its two parents
    k9 = pass_kernel_ms(r, r.accum_reset_spectral_features, args.reps)
    k5 = pass_kernel_ms(r, r.accum_reset_spectral, args.reps)
    k7 = pass_kernel_ms(r, r.accum_reset_features, args.reps)
    lines.append("%d-spp pass, render kernel ms (best of %d): spectral + features (MODE 9) %.3f, spectral (MODE 5) %.3f, features (MODE 7) %.3f; "
                 "MODE 9 / MODE 5 = %.4f, MODE 9 / MODE 7 = %.4f" % (SPP, args.reps, k9, k5, k7, k9 / k5, k9 / k7))

    # ---- the denoisers' kernels on one spectral featured accumulation
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_spectral_features()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    rng = np.random.default_rng(1)

    def kernel_times(call, develop):
        call()      # warm-up (working images)
        runs, wall = [], []
        for _ in range(args.reps):
            wall.append(timed(r, call))
            runs.append((r.denoise_last_ms(), r.develop_last_ms()["contract"] if develop else 0.0))
        return dict(prepass_ms=round(min(k["prepass"] for k, _ in runs), 4), level_ms=[round(min(k["levels"][i] for k, _ in runs), 4) for i in range(5)],
                    epilogue_ms=round(min(k["epilogue"] for k, _ in runs), 4), develop_ms=round(min(d for _, d in runs), 4), call_wall_ms=round(min(wall), 3))
    t = {"plain": kernel_times(lambda: r.denoise(W, H), False)}
    for k in CHANNELS:
        resp = rng.uniform(0.0, 1.0, (k, 95)).astype(np.float32)
        t["K=%d" % k] = kernel_times(lambda: r.denoise_developed(W, H, resp), True)
    for name, v in t.items():
        lines.append("%-5s kernel ms (best of %d): prepass %.4f, levels %r (sum %.4f), output kernels %.4f, develop %.4f; whole call %.3f ms wall"
                     % (name, args.reps, v["prepass_ms"], v["level_ms"], sum(v["level_ms"]), v["epilogue_ms"], v["develop_ms"], v["call_wall_ms"]))
    p = sum(t["plain"]["level_ms"])
    lines.append("payload levels / plain levels: " + ", ".join("K = %d: %.3f" % (k, sum(t["K=%d" % k]["level_ms"]) / p) for k in CHANNELS))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d" % (W, H, DEPTH), "reps": args.reps, "spp": SPP,
                             "pass_kernel_ms": dict(mode9=round(k9, 3), mode5=round(k5, 3), mode7=round(k7, 3)), "denoise_ms": t}))
    write_report(lines, args.out)
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
