#!/usr/bin/env python3
"""Cost and quality of the temporal reprojection (srt_temporal_accum and the calls that chain it), every figure from this one run, the best
of --reps (default 5) after a warm-up.  Nothing here is gated: the figures are findings.

Timing, on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16) with a 16-spp featured
accumulation and a history in place: the temporal kernel (HIP events, srt_temporal_last_ms); the whole srt_temporal_accum as wall ms with
one output and with all five; srt_denoise_features_temporal against srt_denoise_features_ds (five levels, one output, the same firefly
filter in both); srt_present_temporal against srt_present_despeckled (source accum, fixed gain); and the host path the stage replaces --
read the XYZ planes and the feature rows, run the numpy restatement (tests/temporal_reference.py).

Quality: a 16-frame dolly (the camera moves along its view direction by 1 % of its focus distance per frame) at 16 spp per frame, on the
headline scene and on a 256x192 Cornell frame.  RMSE in unquantised sRGB, over all pixels and channels, of the last frame against a
1024-spp frame of the last camera, for four pictures -- noisy, denoised, temporal, temporal then denoised -- at the shipped defaults,
and the blended / fresh / rejected shares of every frame.  Prints one line per row and a JSON line.

Usage: python tools/temporal_cost.py [--reps 5] [--ref-spp 1024] [--frames 16] [--out profiles/temporal/temporal_cost_headline.txt]"""
import ctypes as C
import json
import os
import sys

import numpy as np

from _cost_common import DEPTH, H, W, ROOT, best_of, headline_renderer, parse_args, srt, timed, write_report

sys.path.insert(0, os.path.join(ROOT, "tests"))
import temporal_reference as T  # noqa: E402

SPP = 16
GAIN = 0.8
F = np.float32
INF = float("inf")


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def dolly(cam, w, h, frames):
    """`frames` cameras, each 1 % of the focus distance further along the view direction than the one before"""
    du, dv, p00, ce = (np.asarray(v, np.float64) for v in T.camera_vectors(cam))
    forward = p00 + 0.5 * w * du + 0.5 * h * dv - ce
    step = 0.01 * forward
    return [T.move_camera(cam, tuple(k * step)) for k in range(frames)]


def lane_map(r, w, h):
    tx, ty, bx = r.geom["tx"], r.geom["ty"], r.geom["bx"]
    j, i = np.divmod(np.arange(w * h), w)
    return (j - (j // ty) * ty) * tx + (i - (i // tx) * tx) + tx * ty * ((j // ty) * bx + i // tx)


def host_inputs(r, w, h, n):
    """(c, guides) of the restatement from the planes and rows the device holds"""
    r.scatter_tiles()
    planes = r.read_fb_aux(2)
    lane = lane_map(r, w, h)
    sums = np.stack([np.asarray(p, F)[lane] for p in planes], axis=-1).reshape(h, w, 3)
    feat = r.read_features(w, h)
    rows = np.concatenate([feat["normal"], feat["albedo"], feat["distance"][..., None], feat["hits"][..., None]], axis=-1).astype(F)
    return T.mean_of(sums, n), T.guides_of(rows, n)


def quality(r, cam, w, h, depth, ref_spp, frames, lines, label):
    """the dolly on the context's scene; returns the row"""
    cams = dolly(cam, w, h, frames)
    r.set_camera(cams[-1])
    r.init_device_params(w, h, SPP, depth, 1984)
    r.accum_reset()
    r.render_chunk_accum(w, h, ref_spp)
    ref = r.despeckle(w, h, floor=INF)["lin"]          # the firefly filter switched off: the mean's own unquantised sRGB, row-major
    pictures, shares = {}, []
    for chained in (False, True):
        r.init_device_params(w, h, SPP, depth, 1984)      # the same frames in both runs (and it drops the history)
        for k, c in enumerate(cams):
            r.set_camera(c)
            r.accum_reset_features()
            r.render_chunk_accum(w, h, SPP)
            last = k == frames - 1
            if last and not chained:
                pictures["noisy"] = r.despeckle(w, h, floor=INF)["lin"]
                pictures["denoised"] = r.denoise(w, h)["lin"]
            out = r.denoise_temporal(w, h) if chained else r.temporal(w, h)
            if not chained:
                s = out["stats"]
                shares.append(dict(frame=k, blended=s["blended"] / (w * h), fresh=s["fresh"] / (w * h), rejected=s["rejected"] / (w * h),
                                   offscreen=s["offscreen"] / (w * h)))
            if last:
                pictures["temporal_denoised" if chained else "temporal"] = out["lin"]
                if not chained:
                    mean_len = float(out["len"].mean())
    row = dict(scene=label, pixels=w * h, frames=frames, ref_spp=ref_spp, mean_len_last=mean_len, shares=shares,
               **{"rmse_" + k: rmse(v, ref) for k, v in pictures.items()})
    lines.append("%-28s %dx%d, %d-frame dolly at %d spp, last frame against %d spp of the last camera; mean history length %.2f" % (
        label, w, h, frames, SPP, ref_spp, mean_len))
    lines.append("%-28s RMSE (unquantised sRGB): noisy %.5f  denoised %.5f  temporal %.5f  temporal then denoised %.5f" % (
        "", row["rmse_noisy"], row["rmse_denoised"], row["rmse_temporal"], row["rmse_temporal_denoised"]))
    for s in shares:
        lines.append("%-28s frame %2d: blended %.4f  fresh %.4f (rejected %.4f, offscreen %.4f)" % ("", s["frame"], s["blended"], s["fresh"], s["rejected"], s["offscreen"]))
    return row


def main():
    args = parse_args(lambda ap: (ap.set_defaults(reps=5), ap.add_argument("--ref-spp", type=int, default=1024), ap.add_argument("--frames", type=int, default=16)))
    r, note = headline_renderer()
    L, B = srt.binding.lib(), srt.binding
    lines = ["temporal_cost: random spheres %dx%d, depth %d, %d-spp featured accumulation; tree: %s" % (W, H, DEPTH, SPP, note),
             "defaults: alpha_min 0.1, max_len 32, sigma_normal 0.5, sigma_albedo 0.25, sigma_depth 0.1 (starting values, untuned)"]
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    cam = scene.default_camera(W, H)
    r.set_gather_planes(9)
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_features()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    floor = r.meter(percentile_ppm=500000)["y_ref"]
    out = [np.zeros((H, W, 3), F) for _ in range(3)]
    length, motion = np.zeros((H, W), F), np.zeros((H, W, 2), F)
    rgba = np.zeros((H, W, 4), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    rows = {}
    tcfg, tres = srt.temporal_config(), B.TemporalResult()

    def temporal(n_out):
        ptrs = [B.fptr(o) if k < n_out else None for k, o in enumerate(out)] + [B.fptr(length) if n_out == 5 else None, B.fptr(motion) if n_out == 5 else None]
        r._ck(L.srt_temporal_accum(r._h, C.byref(tcfg), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], C.byref(tres), W, H))
        return tres.blended

    for n_out in (1, 5):
        temporal(n_out)          # warm-up (code object, the working blocks, and a history to gather from)

        def once():
            wall = timed(r, lambda: temporal(n_out))
            return wall, r.temporal_last_ms()
        wall, kernel = best_of(args.reps, once)
        rows["%d output%s" % (n_out, "" if n_out == 1 else "s")] = dict(kernel_ms=round(kernel, 4), call_ms=round(wall, 3), blended=int(tres.blended))
        lines.append("%d output%s: temporal kernel %7.4f ms  srt_temporal_accum %8.3f ms  (blended %d of %d pixels)" % (
            n_out, " " if n_out == 1 else "s", kernel, wall, tres.blended, W * H))

    dcfg, ds = srt.denoise_config(levels=5), srt.despeckle_config(floor=floor)

    def chained():
        r._ck(L.srt_denoise_features_temporal(r._h, C.byref(tcfg), C.byref(ds), C.byref(dcfg), B.fptr(out[0]), None, None, None, W, H))

    def plain():
        r._ck(L.srt_denoise_features_ds(r._h, C.byref(ds), C.byref(dcfg), B.fptr(out[0]), None, None, W, H))

    pcfg = srt.present_config("accum", GAIN)

    def present_t():
        r._ck(L.srt_present_temporal(r._h, C.byref(pcfg), C.byref(tcfg), C.byref(ds), rgba.ctypes.data_as(u8p), 4 * W, W, H, None, None))

    def present_ds():
        r._ck(L.srt_present_despeckled(r._h, C.byref(pcfg), C.byref(ds), rgba.ctypes.data_as(u8p), 4 * W, W, H, None, None))

    for name, a, b in (("denoise, despeckled, 5 levels, one output", chained, plain), ("present, despeckled, accum, gain %.1f" % GAIN, present_t, present_ds)):
        a(); b()
        with_stage = best_of(args.reps, lambda: timed(r, a))
        without = best_of(args.reps, lambda: timed(r, b))
        rows[name] = dict(with_stage_ms=round(with_stage, 3), without_ms=round(without, 3))
        lines.append("%-44s with the stage %8.3f ms  without %8.3f ms" % (name, with_stage, without))

    # the host path: the same frame over a history the restatement made itself (a first frame of the same picture)
    c0, g0 = host_inputs(r, W, H, SPP)
    hist = T.temporal(c0, g0, cam, None, **T.DEFAULTS)

    def host_path():
        c, g = host_inputs(r, W, H, SPP)
        return T.temporal(c, g, cam, hist, **T.DEFAULTS)

    host = best_of(max(1, min(args.reps, 2)), lambda: timed(r, host_path))
    want = host_path()
    r.temporal_reset()
    temporal(1)
    temporal(5)
    same = bool(np.array_equal(out[0].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(length.view(np.uint32), want["len"].view(np.uint32)))
    rows["host path"] = dict(ms=round(host, 1), same_bits=same)
    lines.append("host path (read the XYZ planes and the rows, numpy restatement): %9.1f ms; the device's bits: %s" % (host, same))

    quality_rows = [quality(r, cam, W, H, DEPTH, args.ref_spp, args.frames, lines, "headline (random spheres)")]
    cornell = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    cw, ch = 256, 192
    r.upload_scene(cornell)
    quality_rows.append(quality(r, cornell.default_camera(cw, ch), cw, ch, 8, args.ref_spp, args.frames, lines, "cornell"))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d, %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "floor": floor, "timing": rows,
                             "quality": quality_rows}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
