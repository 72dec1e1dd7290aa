#!/usr/bin/env python3
"""Cost and worth of motion tracking (srt_surface_motion and the *_moving temporal calls), every figure from this one run, the best of
--reps (default 5) after a warm-up.  Nothing here is gated: the figures are findings.

Kernel time   the motion kernel (HIP events, srt_motion_last_ms) on the headline frame (random spheres, the throughput-tuned SAH tree,
              1920x1080, depth 16) and on SRT_SCENE_MESH100K at 960x540, next to the render kernel's time for a 16-spp featured pass of
              the same frame.
Chained call  the whole srt_present_temporal_moving against srt_present_temporal on the headline frame, wall ms.
Quality       a --frames (16) frame refit animation at 16 spp -- tools/refit_cost.py's sine deformation growing to amplitude --amp
              (0.35) on the headline scene at 960x540, and a rigid sideways move of the tall box of a 256x192 Cornell frame -- and the
              RMSE in unquantised sRGB, over all pixels and channels, of the last frame against a --ref-spp (1024) frame of the last
              pose, for: noisy, denoised (render_animated without tracking: every frame a first frame), temporal-moving, and
              temporal-moving then denoised; and the blended share of every frame.
Prints one line per row and a JSON line.

Usage: python tools/motion_cost.py [--reps 5] [--ref-spp 1024] [--frames 16] [--amp 0.35] [--out profiles/motion/motion_cost.txt]"""
import ctypes as C
import json

import numpy as np

from _cost_common import DEPTH, H, W, best_of, parse_args, srt, timed, write_report
from refit_cost import smooth

SPP = 16
GAIN = 0.8
F = np.float32
INF = float("inf")
CORNELL_BOX = slice(12, 24)      # the tall box's twelve triangles


def rmse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def kernel_times(r, label, w, h, depth, reps, lines):
    """the motion kernel and a 16-spp featured pass on the context's scene and camera; the vertices are known (tracking on, uploaded)"""
    r.init_device_params(w, h, SPP, depth, 1984)
    B, L = srt.binding, srt.binding.lib()
    res = B.MotionResult()

    def motion():
        r._ck(L.srt_surface_motion(r._h, w, h, 0, 0, None, None, None, C.byref(res)))      # (the counters only: no image crosses the bus)
        return r.motion_last_ms()

    def render():
        r.accum_reset_features()
        r.render_chunk_accum(w, h, SPP)
        r.synchronize()
        return r.last_kernel_ms()
    motion(); render()
    m, p = best_of(reps, motion), best_of(reps, render)
    lines.append("%-28s %dx%d: motion kernel %.4f ms, %d-spp featured pass %.3f ms: %.2f %% of the pass (hit %d of %d pixels)" % (
        label, w, h, m, SPP, p, 100.0 * m / p, res.hit, w * h))
    return dict(scene=label, width=w, height=h, motion_kernel_ms=round(m, 4), pass_kernel_ms=round(p, 3), share=round(m / p, 5), hit=int(res.hit))


def quality(r, scene, cam, w, h, depth, poses, ref_spp, lines, label):
    """the animation `poses` (vertex arrays) of `scene` on the tracking context r; returns the row"""
    frames = len(poses)
    r.upload_scene(scene)
    r.set_camera(cam)
    r.init_device_params(w, h, SPP, depth, 1984)
    r.refit(poses[-1])
    r.accum_reset()
    r.render_chunk_accum(w, h, ref_spp)
    ref = r.despeckle(w, h, floor=INF)["lin"]          # the firefly filter switched off: the mean's own unquantised sRGB, row-major
    pictures, shares = {}, []
    for chained in (False, True):
        r.upload_scene(scene)                             # the first pose's vertices; V_hist none; the history dropped
        r.init_device_params(w, h, SPP, depth, 1984)      # the same frames in both runs
        for k, v in enumerate(poses):
            r.refit(v)
            r.accum_reset_features()
            r.render_chunk_accum(w, h, SPP)
            last = k == frames - 1
            if last and not chained:
                pictures["noisy"] = r.despeckle(w, h, floor=INF)["lin"]
                pictures["denoised"] = r.denoise(w, h)["lin"]
            out = r.denoise_temporal_moving(w, h) if chained else r.temporal_moving(w, h)
            if not chained:
                s, m = out["stats"], out["surface"]
                shares.append(dict(frame=k, blended=s["blended"] / (w * h), fresh=s["fresh"] / (w * h), rejected=s["rejected"] / (w * h),
                                   offscreen=s["offscreen"] / (w * h), moved=m["moved"] / (w * h)))
            if last:
                pictures["temporal_moving_denoised" if chained else "temporal_moving"] = out["lin"]
                if not chained:
                    mean_len = float(out["len"].mean())
    row = dict(scene=label, pixels=w * h, frames=frames, ref_spp=ref_spp, mean_len_last=mean_len, shares=shares,
               **{"rmse_" + k: rmse(v, ref) for k, v in pictures.items()})
    lines.append("%-28s %dx%d, %d-frame refit animation at %d spp, last frame against %d spp of the last pose; mean history length %.2f" % (
        label, w, h, frames, SPP, ref_spp, mean_len))
    lines.append("%-28s RMSE (unquantised sRGB): noisy %.5f  denoised (no tracking) %.5f  temporal-moving %.5f  temporal-moving then denoised %.5f" % (
        "", row["rmse_noisy"], row["rmse_denoised"], row["rmse_temporal_moving"], row["rmse_temporal_moving_denoised"]))
    for s in shares:
        lines.append("%-28s frame %2d: blended %.4f  fresh %.4f (rejected %.4f, offscreen %.4f)  on moved triangles %.4f" % (
            "", s["frame"], s["blended"], s["fresh"], s["rejected"], s["offscreen"], s["moved"]))
    return row


def main():
    args = parse_args(lambda ap: (ap.set_defaults(reps=5), ap.add_argument("--ref-spp", type=int, default=1024), ap.add_argument("--frames", type=int, default=16),
                                  ap.add_argument("--amp", type=float, default=0.35)))
    r = srt.Renderer(0)
    L, B = srt.binding.lib(), srt.binding
    r.set_gather_planes(9)
    r.track_motion(True)      # (before the uploads: an upload is what makes the vertices known)
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    note = srt.tune_tree_for_throughput(r, scene, W, H, DEPTH)
    lines = ["motion_cost: best of %d; headline tree: %s" % (args.reps, note)]
    r.upload_scene(scene)
    r.set_camera(scene.default_camera(W, H))
    r.set_partition(0, 1)
    kernels = [kernel_times(r, "headline (random spheres)", W, H, DEPTH, args.reps, lines)]

    # the chained call on the headline frame: a history, a refit between the frames, the same accumulation presented both ways
    v0 = scene.vertices()
    v1 = smooth(v0, 0.7, args.amp / args.frames)
    rgba = np.zeros((H, W, 4), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    tcfg, pcfg = srt.temporal_config(), srt.present_config("accum", GAIN)
    tres, mres = B.TemporalResult(), B.MotionResult()

    def frame():
        r.accum_reset_features()
        r.render_chunk_accum(W, H, SPP)
        r.synchronize()

    def present_moving():
        r._ck(L.srt_present_temporal_moving(r._h, C.byref(pcfg), C.byref(tcfg), None, rgba.ctypes.data_as(u8p), 4 * W, W, H, None, C.byref(tres), C.byref(mres)))

    def present_static():
        r._ck(L.srt_present_temporal(r._h, C.byref(pcfg), C.byref(tcfg), None, rgba.ctypes.data_as(u8p), 4 * W, W, H, None, C.byref(tres)))
    frame(); present_moving(); r.refit(v1); frame(); present_moving()      # warm-up, and a history of the deformed pose
    moving = best_of(args.reps, lambda: timed(r, present_moving))
    blended_moving = int(tres.blended)
    present_static()
    static = best_of(args.reps, lambda: timed(r, present_static))
    chained = dict(moving_ms=round(moving, 3), static_ms=round(static, 3), blended_moving=blended_moving, blended_static=int(tres.blended))
    lines.append("present, accum, gain %.1f, %dx%d: srt_present_temporal_moving %.3f ms  srt_present_temporal %.3f ms  (+%.3f ms: the motion kernel and its counters)" % (
        GAIN, W, H, moving, static, moving - static))

    mesh = srt.Scene.builtin(srt.SCENE_MESH100K, 0).build_bvh(srt.BVH_SAH, 1984)
    r.upload_scene(mesh)
    r.set_camera(mesh.default_camera(960, 540))
    kernels.append(kernel_times(r, "mesh100k", 960, 540, DEPTH, args.reps, lines))

    qw, qh = 960, 540
    poses = [smooth(v0, 0.7, args.amp * (k + 1) / args.frames) for k in range(args.frames)]
    rows = [quality(r, scene, scene.default_camera(qw, qh), qw, qh, DEPTH, poses, args.ref_spp, lines, "random spheres, sine to %.2f" % args.amp)]
    cornell = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    c0 = cornell.vertices()
    assert c0.shape[0] == 42
    cposes = []
    for k in range(args.frames):
        v = c0.copy()
        v[CORNELL_BOX, :, 0] = (v[CORNELL_BOX, :, 0] - F(4.0 * (k + 1))).astype(F)      # 4 of the room's 555 units per frame
        cposes.append(v)
    cw, ch = 256, 192
    rows.append(quality(r, cornell, cornell.default_camera(cw, ch), cw, ch, 8, cposes, args.ref_spp, lines, "cornell, the tall box sideways"))
    lines.append(json.dumps({"reps": args.reps, "spp": SPP, "kernels": kernels, "chained": chained, "quality": rows}))
    write_report(lines, args.out)
    r.track_motion(False)
    r.close()


if __name__ == "__main__":
    main()
