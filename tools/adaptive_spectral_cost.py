#!/usr/bin/env python3
"""Cost of adaptive spectral accumulations (srt_accum_reset_adaptive_spectral / _features, render_kernel MODE 10 / 11) on the headline
workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16).  Every figure comes from this one run, the best of --reps:

 * the render kernel's ms of an all-active 16-spp first pass of an adaptive spectral (MODE 10) and an adaptive spectral featured (MODE 11)
   accumulation next to the same pass of an adaptive (MODE 4), a spectral (MODE 5) and a spectral featured (MODE 9) accumulation.  MODE 10
   against MODE 5 is what S2 through memory and the adaptive bookkeeping cost on top of the film in the headline shape;
 * one adaptive spectral run at --rel-tol (min_spp 16, passes of 16, at most --max-spp samples): the render kernels' ms summed over its
   passes, against ONE plain spectral pass (MODE 5) of the run's mean sample count, rounded to a whole number;
 * the per-pixel-count sRGB epilogue of srt_develop_spectral_srgb, timed on that run's accumulation while it is still bound, against the
   scalar epilogue on a spectral featured (non-adaptive) one, and both prepasses of srt_denoise_developed (colour + payload, K = 3: one event pair brackets the two kernels) on an
   adaptive spectral featured accumulation against the scalar pair on a spectral featured one.

Nothing is gated.  Prints one line per row and a JSON line.

Usage: python tools/adaptive_spectral_cost.py [--reps 5] [--rel-tol 0.05] [--max-spp 64]
                                              [--out profiles/adaptive_spectral/adaptive_spectral_cost_headline.txt]"""
import json
import sys

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, write_report

SPP = 16
NEVER = 1e-30      # a relative tolerance no pixel with any variance meets


def first_pass_kernel_ms(r, reset, reps, spp=SPP):
    """the render kernel's ms of a first pass of `spp` samples after reset(): every pixel is active in it"""
    def once():
        r.init_device_params(W, H, spp, DEPTH, 1984)
        reset()
        r.render_chunk_accum(W, H, spp)
        r.synchronize()
        return r.last_kernel_ms()
    once()      # warm-up
    return best_of(reps, once)


def develop_epilogue_ms(r, reps):
    """kernel ms of srt_develop_spectral_srgb's sRGB epilogue on the context's accumulation, the best of reps"""
    r.develop_spectral_srgb(W, H)      # warm-up (working images)
    return best_of(reps, lambda: (r.develop_spectral_srgb(W, H), r.develop_last_ms()["epilogue"])[1])


def adaptive_run(r, reset, max_spp):
    """(sum of the passes' render kernel ms, the passes) of one adaptive run from a fresh seed"""
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    reset()
    passes = []
    while r.accum_samples < max_spp:
        r.render_chunk_accum(W, H, min(SPP, max_spp - r.accum_samples))
        active = r.accum_active      # (synchronises)
        passes.append(dict(total=r.accum_samples, active=active, kernel_ms=round(r.last_kernel_ms(), 3)))
        if active == 0:
            break
    return sum(p["kernel_ms"] for p in passes), passes


def main():
    args = parse_args(lambda ap: (ap.add_argument("--rel-tol", type=float, default=0.05), ap.add_argument("--max-spp", type=int, default=64)))
    r, note = headline_renderer()
    lines = ["adaptive_spectral_cost: random spheres %dx%d, depth %d; tree: %s" % (W, H, DEPTH, note)]

    # ---- the all-active pass: MODE 10 and 11 next to MODE 4, 5 and 9
    k = {"mode10": first_pass_kernel_ms(r, lambda: r.accum_reset_adaptive_spectral(NEVER, 0.0, SPP), args.reps),
         "mode11": first_pass_kernel_ms(r, lambda: r.accum_reset_adaptive_spectral_features(NEVER, 0.0, SPP), args.reps),
         "mode4": first_pass_kernel_ms(r, lambda: r.accum_reset_adaptive(NEVER, 0.0, SPP), args.reps),
         "mode5": first_pass_kernel_ms(r, r.accum_reset_spectral, args.reps),
         "mode9": first_pass_kernel_ms(r, r.accum_reset_spectral_features, args.reps)}
    lines.append("all-active %d-spp pass, render kernel ms (best of %d): adaptive + spectral (MODE 10) %.3f, adaptive + spectral + features (MODE 11) %.3f, "
                 "adaptive (MODE 4) %.3f, spectral (MODE 5) %.3f, spectral + features (MODE 9) %.3f; MODE 10 / MODE 5 = %.4f, MODE 10 / MODE 4 = %.4f, "
                 "MODE 11 / MODE 9 = %.4f" % (SPP, args.reps, k["mode10"], k["mode11"], k["mode4"], k["mode5"], k["mode9"],
                                              k["mode10"] / k["mode5"], k["mode10"] / k["mode4"], k["mode11"] / k["mode9"]))

    # ---- one adaptive spectral run against the plain spectral frame of the same mean sample count
    reset = lambda: r.accum_reset_adaptive_spectral(args.rel_tol, 0.0, SPP)
    adaptive_run(r, reset, args.max_spp)      # warm-up
    run_ms, passes = best_of(args.reps, lambda: adaptive_run(r, reset, args.max_spp))
    samples = r.accum_stats(W, H)["samples"]
    counts = {int(c): int(n) for c, n in zip(*np.unique(samples, return_counts=True))}
    mean = float(samples.mean(dtype=np.float64))
    same = max(1, int(round(mean)))
    # (the per-pixel-count epilogue is timed here, while the adaptive spectral accumulation of the run is still the context's own)
    assert r.accum_active >= 0 and len(counts) >= 2      # refused unless the accumulation is adaptive; a map of one count would hide a scalar divide
    e_counts = develop_epilogue_ms(r, args.reps)
    plain_ms = first_pass_kernel_ms(r, r.accum_reset_spectral, args.reps, spp=same)
    lines.append("adaptive spectral run at rel_tol %g, min_spp %d, passes of %d up to %d: %r" % (args.rel_tol, SPP, SPP, args.max_spp, passes))
    lines.append("samples per pixel: mean %.2f; pixels by count %r" % (mean, counts))
    lines.append("render kernels, ms (best of %d): the adaptive spectral run %.3f in %d passes; one plain spectral pass (MODE 5) of %d spp %.3f; ratio %.4f"
                 % (args.reps, run_ms, len(passes), same, plain_ms, run_ms / plain_ms))

    # ---- the per-pixel-count epilogue and prepasses against their scalar siblings
    def prepass_ms(resp):
        r.denoise_developed(W, H, resp)
        return best_of(args.reps, lambda: (r.denoise_developed(W, H, resp), r.denoise_last_ms()["prepass"])[1])
    resp = np.random.default_rng(1).uniform(0.0, 1.0, (3, 95)).astype(np.float32)
    adaptive_run(r, lambda: r.accum_reset_adaptive_spectral_features(args.rel_tol, 0.0, SPP), args.max_spp)
    assert r.accum_active >= 0      # (adaptive, or refused)
    p_counts = prepass_ms(resp)
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_spectral_features()
    r.render_chunk_accum(W, H, SPP)
    try:      # the scalar siblings run on an accumulation that is NOT adaptive
        r.accum_active
        raise AssertionError("the scalar kernels would be timed on an adaptive accumulation")
    except srt.SrtError:
        pass
    e_scalar, p_scalar = develop_epilogue_ms(r, args.reps), prepass_ms(resp)
    lines.append("kernel ms (best of %d): sRGB epilogue per-pixel count %.4f, scalar %.4f; srt_denoise_developed's two prepasses (K = 3) per-pixel count %.4f, scalar %.4f"
                 % (args.reps, e_counts, e_scalar, p_counts, p_scalar))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d" % (W, H, DEPTH), "reps": args.reps,
                             "all_active_pass_kernel_ms": {m: round(v, 3) for m, v in k.items()},
                             "adaptive_run": dict(rel_tol=args.rel_tol, min_spp=SPP, step=SPP, max_spp=args.max_spp, passes=passes, counts=counts,
                                                  mean_spp=round(mean, 3), kernel_ms=round(run_ms, 3)),
                             "plain_spectral_pass": dict(spp=same, kernel_ms=round(plain_ms, 3)),
                             "epilogue_ms": dict(per_pixel=round(e_counts, 4), scalar=round(e_scalar, 4)),
                             "prepasses_ms": dict(per_pixel=round(p_counts, 4), scalar=round(p_scalar, 4))}))
    write_report(lines, args.out)
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
