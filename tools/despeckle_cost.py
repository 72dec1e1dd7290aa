#!/usr/bin/env python3
"""Cost and quality of the firefly filter (srt_despeckle_accum and the calls that chain it), every figure from this one run, the best of
--reps (default 5) after a warm-up.  Nothing here is gated: the figures are findings.

Timing, on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16) with a 16-spp featured
accumulation: the despeckle kernel at both radii (HIP events, srt_despeckle_last_ms); the whole srt_despeckle_accum as wall ms with one
output and with all four; srt_denoise_features_ds against srt_denoise_features (five levels, one output); srt_present_despeckled against
srt_present (source accum, fixed gain); and the host path the filter replaces -- read the XYZ planes, run the numpy restatement
(tests/despeckle_reference.py) at radius 2.

Quality: RMSE in unquantised sRGB, over all pixels and channels, against a 1024-spp frame of the same seed, of four 16-spp pictures --
noisy, despeckled, denoised, despeckled then denoised -- at the shipped defaults (metered floor), on the headline scene, where the
defaults should clamp next to nothing (the count is reported), and on a 256x192 Cornell frame, where the bias the clamp introduces is the
number to look at.  Prints one line per row and a JSON line.

Usage: python tools/despeckle_cost.py [--reps 5] [--ref-spp 1024] [--out profiles/despeckle/despeckle_cost_headline.txt]"""
import ctypes as C
import json
import os
import sys

import numpy as np

from _cost_common import DEPTH, H, W, ROOT, best_of, headline_renderer, parse_args, srt, timed, write_report

sys.path.insert(0, os.path.join(ROOT, "tests"))
import despeckle_reference as R  # noqa: E402

SPP = 16
GAIN = 0.8
F = np.float32
INF = float("inf")


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def quality(r, w, h, depth, ref_spp, lines, label):
    """the four pictures of the context's scene at SPP against ref_spp samples of the same seed; returns the row"""
    r.init_device_params(w, h, SPP, depth, 1984)
    r.accum_reset()
    r.render_chunk_accum(w, h, ref_spp)
    ref = r.despeckle(w, h, floor=INF)["lin"]          # the filter switched off: the mean's own unquantised sRGB, row-major
    r.init_device_params(w, h, SPP, depth, 1984)
    r.accum_reset_features()
    r.render_chunk_accum(w, h, SPP)
    noisy = r.despeckle(w, h, floor=INF)["lin"]
    clean = r.despeckle(w, h)
    row = dict(scene=label, pixels=w * h, ref_spp=ref_spp, floor=clean["floor"], clamped=clean["clip"]["clamped"], nonfinite=clean["clip"]["nonfinite"],
               alone=clean["clip"]["alone"], rmse_noisy=rmse(noisy, ref), rmse_despeckled=rmse(clean["lin"], ref),
               rmse_denoised=rmse(r.denoise(w, h)["lin"], ref), rmse_despeckled_denoised=rmse(r.denoise_despeckled(w, h)["lin"], ref))
    lines.append("%-28s %dx%d, %d spp against %d spp, defaults, metered floor %.6g: clamped %d of %d pixels" % (label, w, h, SPP, ref_spp, row["floor"], row["clamped"], w * h))
    lines.append("%-28s RMSE (unquantised sRGB): noisy %.5f  despeckled %.5f  denoised %.5f  despeckled then denoised %.5f" % (
        "", row["rmse_noisy"], row["rmse_despeckled"], row["rmse_denoised"], row["rmse_despeckled_denoised"]))
    return row


def main():
    args = parse_args(lambda ap: (ap.set_defaults(reps=5), ap.add_argument("--ref-spp", type=int, default=1024)))
    r, note = headline_renderer()
    L, B = srt.binding.lib(), srt.binding
    lines = ["despeckle_cost: random spheres %dx%d, depth %d, %d-spp featured accumulation; tree: %s" % (W, H, DEPTH, SPP, note),
             "defaults: radius 2, rank_ppm 875000, gain 4, floor metered (starting values, untuned)"]
    r.set_gather_planes(9)
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_features()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    floor = r.meter(percentile_ppm=500000)["y_ref"]
    out = [np.zeros((H, W, 3), F) for _ in range(3)]
    scale = np.zeros((H, W), F)
    rgba = np.zeros((H, W, 4), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    rows = {}

    def despeckle(radius, n_out):
        d, res = srt.despeckle_config(radius=radius, floor=floor), B.DespeckleResult()
        ptrs = [B.fptr(o) if k < n_out else None for k, o in enumerate(out)] + [B.fptr(scale) if n_out == 4 else None]
        r._ck(L.srt_despeckle_accum(r._h, C.byref(d), ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.byref(res), W, H))
        return res.clamped

    for radius in (1, 2):
        for n_out in (1, 4):
            despeckle(radius, n_out)          # warm-up (code object, the working block's allocation)

            def once():
                wall = timed(r, lambda: despeckle(radius, n_out))
                return wall, r.despeckle_last_ms()
            wall, kernel = best_of(args.reps, once)
            rows["radius %d, %d output%s" % (radius, n_out, "" if n_out == 1 else "s")] = dict(kernel_ms=round(kernel, 4), call_ms=round(wall, 3))
            lines.append("radius %d, %d output%s: despeckle kernel %7.4f ms  srt_despeckle_accum %8.3f ms" % (radius, n_out, " " if n_out == 1 else "s", kernel, wall))

    dcfg, ds = srt.denoise_config(levels=5), srt.despeckle_config(floor=floor)

    def chained():
        r._ck(L.srt_denoise_features_ds(r._h, C.byref(ds), C.byref(dcfg), B.fptr(out[0]), None, None, W, H))

    def plain():
        r._ck(L.srt_denoise_features(r._h, C.byref(dcfg), B.fptr(out[0]), None, None, W, H))

    pcfg = srt.present_config("accum", GAIN)

    def present_ds():
        r._ck(L.srt_present_despeckled(r._h, C.byref(pcfg), C.byref(ds), rgba.ctypes.data_as(u8p), 4 * W, W, H, None, None))

    def present():
        r._ck(L.srt_present(r._h, C.byref(pcfg), rgba.ctypes.data_as(u8p), 4 * W, W, H, None))

    for name, a, b in (("denoise, 5 levels, one output", chained, plain), ("present, accum, gain %.1f" % GAIN, present_ds, present)):
        a(); b()
        with_stage = best_of(args.reps, lambda: timed(r, a))
        without = best_of(args.reps, lambda: timed(r, b))
        rows[name] = dict(with_stage_ms=round(with_stage, 3), without_ms=round(without, 3))
        lines.append("%-32s with the stage %8.3f ms  without %8.3f ms" % (name, with_stage, without))

    def host_path():
        r.scatter_tiles()
        planes = r.read_fb_aux(2)
        tx, ty, bx = r.geom["tx"], r.geom["ty"], r.geom["bx"]
        j, i = np.divmod(np.arange(W * H), W)
        lane = (j - (j // ty) * ty) * tx + (i - (i // tx) * tx) + tx * ty * ((j // ty) * bx + i // tx)
        mean = R.mean_xyz(np.stack([np.asarray(p, F)[lane] for p in planes], axis=-1).reshape(H, W, 3), SPP)
        return R.despeckle(mean, 2, 875000, 4.0, floor)

    host_path()
    host = best_of(args.reps, lambda: timed(r, host_path))
    want = host_path()
    despeckle(2, 4)
    same = bool(np.array_equal(out[0].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(scale.view(np.uint32), want["scale"].view(np.uint32)))
    rows["host path, radius 2"] = dict(ms=round(host, 1), same_bits=same)
    lines.append("host path (read the XYZ planes, numpy restatement, radius 2): %9.1f ms; the device's bits: %s" % (host, same))

    quality_rows = [quality(r, W, H, DEPTH, args.ref_spp, lines, "headline (random spheres)")]
    scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    cw, ch = 256, 192
    r.upload_scene(scene)
    r.set_camera(scene.default_camera(cw, ch))
    quality_rows.append(quality(r, cw, ch, 8, args.ref_spp, lines, "cornell"))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d, %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "floor": floor, "timing": rows,
                             "quality": quality_rows}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
