#!/usr/bin/env python3
"""Cost and quality of the variance measured across frames (srt_denoise_features_temporal_vg), every figure from this one run, the best of
--reps (default 5) after a warm-up.  Nothing here is gated: the figures are findings, whichever way they fall.

Timing, on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16) with a 16-spp featured accumulation
and a history in place (HIP events): the moments kernel (srt_temporal_last_ms behind srt_denoise_features_temporal_vg) against the static
kernel (behind srt_denoise_features_temporal); the choice kernel (srt_temporal_variance_last_ms); and the whole chained call as wall ms
against srt_denoise_features_temporal -- five levels, one output, no firefly filter in either.

Quality: the two 16-frame dollies of tools/temporal_cost.py (the camera moves along its view direction by 1 % of its focus distance per
frame, 16 spp per frame; the headline scene, and a 256x192 Cornell frame).  RMSE in unquantised sRGB, over all pixels and channels, of the
last frame against a 1024-spp frame of the last camera, for four pictures -- noisy; temporal then the plain filter; temporal then the
variance-guided filter on the spatial estimate alone (min_len > max_len); temporal then the variance-guided filter on the variance the
history measured -- at the shipped defaults (min_len 4, sigma_variance 2: starting values, untuned), and the share of pixels that took the
temporal variance in every frame.  Prints one line per row and a JSON line.

Usage: python tools/temporal_vg_cost.py [--reps 5] [--ref-spp 1024] [--frames 16] [--out profiles/temporal_vg/temporal_vg_cost.txt]"""
import ctypes as C
import json

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, timed, write_report
from temporal_cost import SPP, dolly, rmse

F = np.float32
INF = float("inf")
SPATIAL_ONLY = 64      # a min_len above the default max_len of 32: the variance is always the spatial estimate


def quality(r, cam, w, h, depth, ref_spp, frames, lines, label):
    """the dolly on the context's scene, once per chain; returns the row"""
    cams = dolly(cam, w, h, frames)
    r.set_camera(cams[-1])
    r.init_device_params(w, h, SPP, depth, 1984)
    r.accum_reset()
    r.render_chunk_accum(w, h, ref_spp)
    ref = r.despeckle(w, h, floor=INF)["lin"]          # the firefly filter switched off: the mean's own unquantised sRGB, row-major
    chains = {"temporal_plain": lambda: r.denoise_temporal(w, h), "temporal_vg_spatial": lambda: r.denoise_temporal_vg(w, h, min_len=SPATIAL_ONLY),
              "temporal_vg": lambda: r.denoise_temporal_vg(w, h)}
    pictures, shares = {}, []
    for name, call in chains.items():
        r.init_device_params(w, h, SPP, depth, 1984)      # the same frames in every run (and it drops the history)
        for k, c in enumerate(cams):
            r.set_camera(c)
            r.accum_reset_features()
            r.render_chunk_accum(w, h, SPP)
            if k == frames - 1 and "noisy" not in pictures:
                pictures["noisy"] = r.despeckle(w, h, floor=INF)["lin"]
            out = call()
            if name == "temporal_vg":
                shares.append(out["n_temporal"] / (w * h))
            elif name == "temporal_vg_spatial":
                assert out["n_temporal"] == 0
        pictures[name] = out["lin"]
    row = dict(scene=label, pixels=w * h, frames=frames, ref_spp=ref_spp, temporal_share=shares, **{"rmse_" + k: rmse(v, ref) for k, v in pictures.items()})
    lines.append("%-28s %dx%d, %d-frame dolly at %d spp, last frame against %d spp of the last camera" % (label, w, h, frames, SPP, ref_spp))
    lines.append("%-28s RMSE (unquantised sRGB): noisy %.5f  temporal then plain %.5f  temporal then spatial-only variance %.5f  temporal then measured variance %.5f" % (
        "", row["rmse_noisy"], row["rmse_temporal_plain"], row["rmse_temporal_vg_spatial"], row["rmse_temporal_vg"]))
    lines.append("%-28s share of pixels with the temporal variance, per frame: %s" % ("", " ".join("%.4f" % s for s in shares)))
    return row


def main():
    args = parse_args(lambda ap: (ap.set_defaults(reps=5), ap.add_argument("--ref-spp", type=int, default=1024), ap.add_argument("--frames", type=int, default=16)))
    r, note = headline_renderer()
    L, B = srt.binding.lib(), srt.binding
    lines = ["temporal_vg_cost: random spheres %dx%d, depth %d, %d-spp featured accumulation; tree: %s" % (W, H, DEPTH, SPP, note),
             "defaults: min_len 4, sigma_variance 2, variance_floor 1e-8, the temporal defaults of temporal_cost (starting values, untuned)"]
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    cam = scene.default_camera(W, H)
    r.set_gather_planes(9)
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_features()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    out = np.zeros((H, W, 3), F)
    tcfg, dcfg, vcfg, tv = srt.temporal_config(), srt.denoise_config(levels=5), srt.denoise_vg_config(levels=5), srt.temporal_vg_config()
    n = C.c_uint64()

    def chained_vg():
        r._ck(L.srt_denoise_features_temporal_vg(r._h, C.byref(tcfg), None, C.byref(vcfg), C.byref(tv), B.fptr(out), None, None, None, None, C.byref(n), None, W, H))

    def chained_plain():
        r._ck(L.srt_denoise_features_temporal(r._h, C.byref(tcfg), None, C.byref(dcfg), B.fptr(out), None, None, None, W, H))

    rows = {}
    for name, fn in (("srt_denoise_features_temporal_vg", chained_vg), ("srt_denoise_features_temporal", chained_plain)):
        for _ in range(tv.min_len + 1):      # warm-up: the code objects, the working blocks, and a history long enough for the choice to take it
            fn()

        def once():
            wall = timed(r, fn)
            return wall, r.temporal_last_ms(), (r.temporal_variance_last_ms() if fn is chained_vg else 0.0), (r.denoise_estimate_last_ms() if fn is chained_vg else 0.0)
        wall, stage, choice, estimate = best_of(args.reps, once)
        rows[name] = dict(call_ms=round(wall, 3), temporal_kernel_ms=round(stage, 4), choice_kernel_ms=round(choice, 4), estimator_kernel_ms=round(estimate, 4))
        if fn is chained_vg:
            rows[name]["n_temporal"] = int(n.value)
            lines.append("%-34s call %8.3f ms  moments kernel %7.4f ms  estimator %7.4f ms  choice kernel %7.4f ms  (%d of %d pixels took the temporal variance)" % (
                name, wall, stage, estimate, choice, n.value, W * H))
        else:
            lines.append("%-34s call %8.3f ms  static kernel  %7.4f ms" % (name, wall, stage))

    quality_rows = [quality(r, cam, W, H, DEPTH, args.ref_spp, args.frames, lines, "headline (random spheres)")]
    cornell = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    cw, ch = 256, 192
    r.upload_scene(cornell)
    quality_rows.append(quality(r, cornell.default_camera(cw, ch), cw, ch, 8, args.ref_spp, args.frames, lines, "cornell"))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d, %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "timing": rows, "quality": quality_rows}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
