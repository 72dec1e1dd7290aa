#!/usr/bin/env python3
"""Cost and quality of adaptive featured accumulations (srt_accum_reset_adaptive_features, render_kernel MODE 8) and of the
measured-variance denoise (srt_denoise_features_mv) on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080,
depth 16).  Every figure comes from this one run:

 * the render kernel's ms of an all-active 16-spp first pass of an adaptive featured accumulation (MODE 8) next to the same pass of an
   adaptive (MODE 4) and of a featured (MODE 7) accumulation, the best of --reps each;
 * the kernel-only ms of the per-pixel-count prepass, of the measured estimator, of the five levels and of the epilogue of
   srt_denoise_features_mv (HIP events around each kernel, the best of --reps), next to the spatial estimator's;
 * the RMSE in unquantised sRGB against a --ref-spp frame of the same seed, on ONE adaptive featured run at --rel-tol (min_spp 16, passes
   of 16, at most --max-spp samples): the noisy adaptive frame, the plain denoise, the spatial-variance denoise and the measured-variance
   denoise, all at the shipped defaults of denoise_config / denoise_vg_config.

Nothing is gated: whether the measured variance beats the spatial one on this frame is reported either way.  Prints one line per row and a
JSON line.

Usage: python tools/adaptive_features_cost.py [--reps 5] [--ref-spp 1024] [--rel-tol 0.05] [--max-spp 64]
                                              [--out profiles/adaptive_features/adaptive_features_cost_headline.txt]"""
import json
import sys

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, write_report
from denoise_cost import rmse, rowmajor_lin

SPP = 16
NEVER = 1e-30      # a relative tolerance no pixel with any variance meets


def first_pass_kernel_ms(r, reset, reps):
    """the render kernel's ms of a 16-spp first pass after reset(): every pixel is active in it"""
    def once():
        r.init_device_params(W, H, SPP, DEPTH, 1984)
        reset()
        r.render_chunk_accum(W, H, SPP)
        r.synchronize()
        return r.last_kernel_ms()
    once()      # warm-up
    return best_of(reps, once)


def main():
    args = parse_args(lambda ap: (ap.add_argument("--ref-spp", type=int, default=1024), ap.add_argument("--rel-tol", type=float, default=0.05),
                                  ap.add_argument("--max-spp", type=int, default=64)))
    r, note = headline_renderer()
    r.set_gather_planes(9)
    lines = ["adaptive_features_cost: random spheres %dx%d, depth %d; tree: %s" % (W, H, DEPTH, note)]

    r.init_device_params(W, H, args.ref_spp, DEPTH, 1984)
    r.render_chunk(W, H)
    r.scatter_tiles()
    ref = rowmajor_lin(r)

    # ---- the all-active pass: MODE 8 next to its two parents
    k8 = first_pass_kernel_ms(r, lambda: r.accum_reset_adaptive_features(NEVER, 0.0, SPP), args.reps)
    k4 = first_pass_kernel_ms(r, lambda: r.accum_reset_adaptive(NEVER, 0.0, SPP), args.reps)
    k7 = first_pass_kernel_ms(r, r.accum_reset_features, args.reps)
    lines.append("all-active %d-spp pass, render kernel ms (best of %d): adaptive + features (MODE 8) %.3f, adaptive (MODE 4) %.3f, features (MODE 7) %.3f; "
                 "MODE 8 / MODE 4 = %.4f, MODE 8 / MODE 7 = %.4f" % (SPP, args.reps, k8, k4, k7, k8 / k4, k8 / k7))

    # ---- one adaptive featured run at the stated tolerance
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_adaptive_features(args.rel_tol, 0.0, SPP)
    passes = []
    while r.accum_samples < args.max_spp:
        r.render_chunk_accum(W, H, min(SPP, args.max_spp - r.accum_samples))
        passes.append(dict(total=r.accum_samples, active=r.accum_active, kernel_ms=round(r.last_kernel_ms(), 3)))
        if passes[-1]["active"] == 0:
            break
    r.scatter_tiles()
    noisy = rowmajor_lin(r)
    samples = r.accum_stats(W, H)["samples"]
    counts = {int(c): int(n) for c, n in zip(*np.unique(samples, return_counts=True))}
    lines.append("adaptive featured run at rel_tol %g, min_spp %d, passes of %d up to %d: %r" % (args.rel_tol, SPP, SPP, args.max_spp, passes))
    lines.append("samples per pixel: mean %.2f; pixels by count %r" % (samples.mean(dtype=np.float64), counts))

    # ---- the denoisers' kernels on that accumulation
    def kernel_times(call, estimator):
        call()      # warm-up (working images)
        runs = []
        for _ in range(args.reps):
            call()
            runs.append((r.denoise_last_ms(), r.denoise_estimate_last_ms() if estimator else 0.0))
        return dict(prepass_ms=round(min(k["prepass"] for k, _ in runs), 4), estimator_ms=round(min(e for _, e in runs), 4),
                    level_ms=[round(min(k["levels"][i] for k, _ in runs), 4) for i in range(5)], epilogue_ms=round(min(k["epilogue"] for k, _ in runs), 4))
    t_mv = kernel_times(lambda: r.denoise_mv(W, H), True)
    t_vg = kernel_times(lambda: r.denoise_vg(W, H), True)
    t_plain = kernel_times(lambda: r.denoise(W, H), False)
    for name, t in (("measured variance", t_mv), ("spatial variance", t_vg), ("plain", t_plain)):
        lines.append("%s denoise, kernel ms (best of %d): per-pixel-count prepass %.4f, estimator %.4f, levels %r, epilogue %.4f"
                     % (name, args.reps, t["prepass_ms"], t["estimator_ms"], t["level_ms"], t["epilogue_ms"]))

    # ---- quality on that run
    q = dict(ref_spp=args.ref_spp, rmse_noisy=round(rmse(noisy, ref), 6), rmse_plain=round(rmse(r.denoise(W, H)["lin"], ref), 6),
             rmse_spatial=round(rmse(r.denoise_vg(W, H)["lin"], ref), 6))
    mv = r.denoise_mv(W, H)
    q["rmse_measured"] = round(rmse(mv["lin"], ref), 6)
    lines.append("quality (unquantised sRGB against %d spp): RMSE noisy adaptive frame %.6f, plain denoise %.6f, spatial-variance denoise %.6f, measured-variance denoise %.6f: %s"
                 % (args.ref_spp, q["rmse_noisy"], q["rmse_plain"], q["rmse_spatial"], q["rmse_measured"],
                    "the measured variance is closer than the spatial one" if q["rmse_measured"] < q["rmse_spatial"] else "THE MEASURED VARIANCE IS NOT CLOSER THAN THE SPATIAL ONE at these starting values"))
    lines.append("measured variance of the mean of Y: median %.3e, mean %.3e; after the last level: median %.3e, mean %.3e"
                 % (np.median(mv["var"][..., 0]), mv["var"][..., 0].mean(dtype=np.float64), np.median(mv["var"][..., 1]), mv["var"][..., 1].mean(dtype=np.float64)))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d" % (W, H, DEPTH), "reps": args.reps,
                             "all_active_pass_kernel_ms": dict(mode8=round(k8, 3), mode4=round(k4, 3), mode7=round(k7, 3)),
                             "adaptive_run": dict(rel_tol=args.rel_tol, min_spp=SPP, step=SPP, max_spp=args.max_spp, passes=passes, counts=counts),
                             "denoise_kernels_ms": dict(measured=t_mv, spatial=t_vg, plain=t_plain), "quality": q}))
    write_report(lines, args.out)
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
