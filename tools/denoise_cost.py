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

The variance-guided mode (srt_denoise_features_vg, the defaults of denoise_vg_config) gets a table of its own from the same run, written
with --vg-out: the estimator kernel's ms beside the rest, every level's ms next to the plain level's and the spread of the plain
level over the repetitions, and the RMSE next to the plain denoiser's.  Both are then repeated through the KAT entry points on the
frame's XYZ sums scaled by 4 (the result scaled back by 1/4 before the sRGB conversion, here in numpy float64): the variance-guided
figure stays where it was -- exactly so with variance_floor scaled by 16 -- and the plain one moves.  Nothing of it is gated.

Usage: python tools/denoise_cost.py [--reps 5] [--ref-spp 1024] [--out profiles/denoise/denoise_cost_headline.txt]
                                    [--vg-out profiles/denoise/denoise_vg_cost_headline.txt]"""
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


def srgb_from_xyz(xyz):
    """unquantised sRGB of an (H, W, 3) XYZ image with the library's matrix and the render kernel's transfer curve, in float64"""
    cmf, m = np.zeros(4 * srt.binding.N_CIE, np.float32), np.zeros(9, np.float32)
    srt.binding.lib().srt_color_tables(srt.binding.fptr(cmf), srt.binding.fptr(m))
    with np.errstate(invalid="ignore"):
        v = xyz.astype(np.float64) @ m.astype(np.float64).reshape(3, 3).T
        return np.where(v < 0, 0.0, np.where(v < 0.0031308, 12.92 * v, np.where(v < 1.0, 1.055 * np.power(np.maximum(v, 0.0), 0.416666) - 0.055, 1.0)))


def variance_guided_report(r, args, plain_cfg, plain_rows, ref, noisy, plain_q, note):
    """the variance-guided table: times at 1 .. 5 levels beside the plain rows of this run, and the quality figures"""
    lib, B = srt.binding.lib(), srt.binding
    cfg = dict(levels=5, sigma_variance=2.0, sigma_normal=0.5, sigma_albedo=0.25, sigma_depth=0.1, variance_floor=1e-8)
    shipped = srt.denoise_vg_config()
    assert all(abs(getattr(shipped, k) - v) < 1e-6 * max(v, 1e-9) + 1e-12 for k, v in cfg.items()), "the tool's configuration is not denoise_vg_config's defaults"
    lines = ["denoise_cost, variance-guided: random spheres %dx%d, depth %d, %d spp; tree: %s" % (W, H, DEPTH, SPP, note), "defaults: %r" % (cfg,)]
    out = [np.zeros((H, W, 3), np.float32) for _ in range(3)] + [np.zeros((H, W, 2), np.float32)]
    rows = []
    for levels in range(1, 6):
        c = srt.denoise_vg_config(**dict(cfg, levels=levels))

        def call(n_out):
            ptrs = [B.fptr(o) if k < n_out else None for k, o in enumerate(out)]
            t0 = time.perf_counter()
            r._ck(lib.srt_denoise_features_vg(r._h, c, ptrs[0], ptrs[1], ptrs[2], ptrs[3], W, H))
            return (time.perf_counter() - t0) * 1e3, r.denoise_last_ms(), r.denoise_estimate_last_ms()
        call(4)      # warm-up (the working images grow by the variance output)
        one = best_of(args.reps, lambda: call(1))
        four = best_of(args.reps, lambda: call(4))
        kern = [call(1) for _ in range(args.reps)]
        level_ms = [min(k[1]["levels"][i] for k in kern) for i in range(levels)]
        plain = plain_rows[levels - 1]
        row = dict(levels=levels, call_ms_one_output=round(one[0], 3), call_ms_four_outputs=round(four[0], 3),
                   prepass_ms=round(min(k[1]["prepass"] for k in kern), 4), estimator_ms=round(min(k[2] for k in kern), 4),
                   epilogue_ms=round(min(k[1]["epilogue"] for k in kern), 4), level_ms=[round(v, 4) for v in level_ms],
                   plain_level_ms=plain["level_ms"], plain_level_spread_ms=plain["level_spread_ms"], plain_kernels_ms=plain["kernels_ms"])
        row["kernels_ms"] = round(row["prepass_ms"] + row["estimator_ms"] + row["epilogue_ms"] + sum(level_ms), 4)
        rows.append(row)
        lines.append("levels %d: call %.3f ms (one output) / %.3f ms (four); kernels %.4f ms (plain %.4f); prepass %.4f, estimator %.4f, epilogue + variance copy %.4f"
                     % (levels, row["call_ms_one_output"], row["call_ms_four_outputs"], row["kernels_ms"], plain["kernels_ms"], row["prepass_ms"],
                        row["estimator_ms"], row["epilogue_ms"]))
        lines.append("          per level ms %r; plain %r, plain max - min over %d calls %r" % (row["level_ms"], plain["level_ms"], args.reps, plain["level_spread_ms"]))

    # quality at the defaults, on the device's own conversion, beside the plain figures of this run
    den = r.denoise_vg(W, H, **cfg)
    q = dict(ref_spp=args.ref_spp, rmse_noisy=plain_q["rmse_noisy"], rmse_plain=plain_q["rmse_denoised"], rmse_variance_guided=round(rmse(den["lin"], ref), 6))
    lines.append("quality (unquantised sRGB against %d spp): RMSE noisy %d spp %.6f, plain %.6f, variance-guided %.6f: %s"
                 % (args.ref_spp, SPP, q["rmse_noisy"], q["rmse_plain"], q["rmse_variance_guided"],
                    "variance-guided is closer than plain" if q["rmse_variance_guided"] < q["rmse_plain"] else "VARIANCE-GUIDED IS NOT CLOSER THAN PLAIN at these starting values"))
    lines.append("estimated variance of Y: median %.3e, mean %.3e; after the last level: median %.3e, mean %.3e"
                 % (np.median(den["var"][..., 0]), den["var"][..., 0].mean(dtype=np.float64), np.median(den["var"][..., 1]), den["var"][..., 1].mean(dtype=np.float64)))

    # the same frame four times brighter, through the KAT entry points; the conversion in numpy for all of these figures
    f = r.read_features(W, H)
    feat = np.concatenate([f["normal"], f["albedo"], f["distance"][..., None], f["hits"][..., None]], axis=-1).astype(np.float32)
    sums = (np.float32(SPP) * r.denoise(W, H, levels=0)["xyz"]).astype(np.float32)      # (the mean times a power of two: the sums)
    quarter = np.float32(0.25)
    floor16 = float(np.float32(16) * np.float32(cfg["variance_floor"]))
    x4 = {}
    for scale in (1, 4):
        S = (np.float32(scale) * sums).astype(np.float32)
        back = np.float32(1.0 / scale)
        x4["plain_x%d" % scale] = round(rmse(srgb_from_xyz(back * r.denoise_kat(S, feat, SPP, **plain_cfg)), ref), 6)
        x4["variance_guided_x%d" % scale] = round(rmse(srgb_from_xyz(back * r.denoise_vg_kat(S, feat, SPP, **cfg)[0]), ref), 6)
    x4["variance_guided_x4_floor_x16"] = round(rmse(srgb_from_xyz(quarter * r.denoise_vg_kat((np.float32(4) * sums).astype(np.float32), feat, SPP,
                                                                                              **dict(cfg, variance_floor=floor16))[0]), ref), 6)
    lines.append("frame x 4 through the KAT entry points (result x 1/4, numpy conversion): RMSE plain %.6f -> %.6f; variance-guided %.6f -> %.6f, with variance_floor x 16 %.6f"
                 % (x4["plain_x1"], x4["plain_x4"], x4["variance_guided_x1"], x4["variance_guided_x4"], x4["variance_guided_x4_floor_x16"]))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "config": cfg, "rows": rows,
                             "quality": q, "exposure_x4": x4}))
    return lines


def main():
    args = parse_args(lambda ap: (ap.add_argument("--ref-spp", type=int, default=1024),
                                  ap.add_argument("--vg-out", default=None, help="also write the variance-guided report to this file")))
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
                   level_spread_ms=[round(max(k["levels"][i] for k in kern) - min(k["levels"][i] for k in kern), 4) for i in range(levels)],
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
    write_report(variance_guided_report(r, args, cfg, rows, ref, noisy, q, note), args.vg_out)
    r.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
