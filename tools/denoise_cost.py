#!/usr/bin/env python3
"""Cost and quality of the a-trous denoiser (srt_denoise_features) on the headline workload (random spheres, the throughput-tuned SAH
tree, 1920x1080, depth 16), at the shipped defaults of denoise_config.

Cost: a 16-spp featured pass (srt_accum_reset_features + srt_render_chunk_accum: wall ms and the render kernel's own ms) and, in the
same run, srt_denoise_features on that accumulation at 1 .. 5 levels -- wall ms of the call with one output (kernels + one 24.9 MB copy
to the host) and with all three, the best of --reps calls -- and the kernel-only ms of the prepass, of every level and of the epilogue
(srt_denoise_last_ms: HIP events around each kernel, the best of --reps).  For every level the bandwidth it achieves against its
compulsory traffic: 48 B read + 16 B written per pixel.

Quality: the RMSE in unquantised sRGB, over all pixels and channels, of the noisy 16-spp frame and of the denoised 16-spp frame against
a 1024-spp frame of the same seed.  The requirement is denoised < noisy at the defaults; the tool exits with status 1 otherwise.
Prints one line per row and a JSON line.

Usage: python tools/denoise_cost.py [--reps 5] [--ref-spp 1024] [--out profiles/denoise/denoise_cost_headline.txt]"""
import json
import sys
import time

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, write_report

SPP = 16
COMPULSORY = 48 + 16      # bytes per pixel per level: guides + colour read once, colour written once


def rowmajor_lin(r):
    """the unquantised sRGB of the scattered frame as (H, W, 3)"""
    from_lane = lane_index(r.geom)
    return np.stack([np.asarray(p, np.float32)[from_lane].reshape(H, W) for p in r.read_fb_aux(1)], axis=-1)


def lane_index(geom):
    tx, ty, bx = geom["tx"], geom["ty"], geom["bx"]
    j, i = np.divmod(np.arange(W * H), W)
    gbx, gby = i // tx, j // ty
    return (j - gby * ty) * tx + (i - gbx * tx) + tx * ty * (gby * bx + gbx)


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def main():
    args = parse_args(lambda ap: ap.add_argument("--ref-spp", type=int, default=1024))
    cfg = dict(levels=5, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1)
    shipped = srt.denoise_config()
    assert all(abs(getattr(shipped, k) - v) < 1e-6 for k, v in cfg.items()), "the tool's configuration is not denoise_config's defaults"
    r, note = headline_renderer()
    r.set_gather_planes(9)
    lines = ["denoise_cost: random spheres %dx%d, depth %d, %d spp; tree: %s" % (W, H, DEPTH, SPP, note), "defaults: %r" % (cfg,)]

    # the reference frame
    r.init_device_params(W, H, args.ref_spp, DEPTH, 1984)
    r.render_chunk(W, H)
    r.scatter_tiles()
    ref = rowmajor_lin(r)

    def featured_pass():
        r.init_device_params(W, H, SPP, DEPTH, 1984)
        r.synchronize()
        t0 = time.perf_counter()
        r.accum_reset_features()
        r.render_chunk_accum(W, H, SPP)
        kms = r.last_kernel_ms()
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3, kms
    featured_pass()      # warm-up
    pass_ms, pass_kms = best_of(args.reps, featured_pass)
    r.scatter_tiles()
    noisy = rowmajor_lin(r)
    lines.append("featured pass %d spp: frame %.2f ms, render kernel %.2f ms" % (SPP, pass_ms, pass_kms))

    lib, B = srt.binding.lib(), srt.binding
    out = [np.zeros((H, W, 3), np.float32) for _ in range(3)]
    rows = []
    for levels in range(1, 6):
        c = srt.denoise_config(**dict(cfg, levels=levels))

        def call(n_out):
            ptrs = [B.fptr(o) if k < n_out else None for k, o in enumerate(out)]
            t0 = time.perf_counter()
            r._ck(lib.srt_denoise_features(r._h, c, ptrs[0], ptrs[1], ptrs[2], W, H))
            return (time.perf_counter() - t0) * 1e3, r.denoise_last_ms()
        call(3)      # warm-up (working images, code objects)
        one = best_of(args.reps, lambda: call(1))
        three = best_of(args.reps, lambda: call(3))
        kern = [call(1)[1] for _ in range(args.reps)]
        level_ms = [min(k["levels"][i] for k in kern) for i in range(levels)]
        row = dict(levels=levels, call_ms_one_output=round(one[0], 3), call_ms_three_outputs=round(three[0], 3),
                   prepass_ms=round(min(k["prepass"] for k in kern), 4), epilogue_ms=round(min(k["epilogue"] for k in kern), 4),
                   level_ms=[round(v, 4) for v in level_ms],
                   level_gb_per_s=[round(W * H * COMPULSORY / (v * 1e-3) / 1e9, 1) for v in level_ms])
        row["kernels_ms"] = round(row["prepass_ms"] + row["epilogue_ms"] + sum(level_ms), 4)
        row["kernels_vs_pass_kernel_pct"] = round(100.0 * row["kernels_ms"] / pass_kms, 2)
        rows.append(row)
        lines.append("levels %d: call %.3f ms (one output) / %.3f ms (three); kernels %.4f ms = %.2f %% of the pass's render kernel; prepass %.4f, epilogue %.4f"
                     % (levels, row["call_ms_one_output"], row["call_ms_three_outputs"], row["kernels_ms"], row["kernels_vs_pass_kernel_pct"],
                        row["prepass_ms"], row["epilogue_ms"]))
        lines.append("          per level ms %r; GB/s of compulsory traffic (%d B/pixel) %r" % (row["level_ms"], COMPULSORY, row["level_gb_per_s"]))

    den = r.denoise(W, H, **cfg)["lin"]
    q = dict(ref_spp=args.ref_spp, rmse_noisy=round(rmse(noisy, ref), 6), rmse_denoised=round(rmse(den, ref), 6))
    q["ratio"] = round(q["rmse_denoised"] / q["rmse_noisy"], 4)
    ok = q["rmse_denoised"] < q["rmse_noisy"]
    lines.append("quality (unquantised sRGB against %d spp): RMSE noisy %d spp %.6f, denoised %.6f (x %.4f): %s"
                 % (args.ref_spp, SPP, q["rmse_noisy"], q["rmse_denoised"], q["ratio"], "denoised is closer" if ok else "DENOISED IS NOT CLOSER"))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "config": cfg,
                             "featured_pass": dict(frame_ms=round(pass_ms, 2), kernel_ms=round(pass_kms, 2)), "rows": rows, "quality": q}))
    write_report(lines, args.out)
    r.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
