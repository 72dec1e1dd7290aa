#!/usr/bin/env python3
"""Cost and quality of the deferred direct-light pass (srt_direct_light), every figure from this one run.  Nothing here is gated: the
figures are findings.

Part 1  the headline frame (random spheres, the throughput-tuned SAH tree, 1920x1080): one round of one sample -- the camera, shade and
        gather kernels and the query launches (srt_direct_light_last), the best of --reps by their sum -- next to the parent's kernels in the
        same run: the query kernel on the same camera rows (srt_intersect_rays_dev, srt_query_last) and render_kernel at 1 spp,
        bounce_limit 2 (srt_last_kernel_ms).
Part 2  CORNELL at 256x192: RMSE in unquantised sRGB (the library's XYZ -> sRGB matrix, the sRGB curve, clipped to [0, 1]) against a
        4 096-spp bounce_limit 2 frame, of the direct picture at --samples samples and of the path tracer at bounce_limit 2 with the spp
        whose kernel time is nearest the direct pass's.  Pixels whose first hit is specular are left out of both (the pass adds nothing
        there by design).  Not taken here: the path tracer behind the firefly filter and the denoiser.

Usage: python tools/direct_light_cost.py [--reps 5] [--samples 16] [--out profiles/direct_light/direct_light_cost.txt]"""
import json

import numpy as np

from _cost_common import H, W, best_of, headline_renderer, parse_args, srt, write_report

B = srt.binding


def srgb(xyz):
    cmf, m = np.zeros(95 * 4, np.float32), np.zeros(9, np.float32)
    B.check(B.lib().srt_color_tables(B.fptr(cmf), B.fptr(m)))
    lin = np.clip(xyz.astype(np.float64) @ m.reshape(3, 3).astype(np.float64).T, 0.0, 1.0)
    return np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * lin ** (1 / 2.4) - 0.055)


def path_traced(r, w, h, spp, seed):
    """(XYZ mean (h, w, 3), kernel ms) of the path tracer at bounce_limit 2"""
    r.init_device_params(w, h, spp, 2, seed)
    r.set_partition(0, 1)
    r.render_chunk(w, h)
    ms = r.last_kernel_ms()
    r.scatter_tiles()
    g = r.geom
    y, x = np.mgrid[0:h, 0:w]
    idx = ((y // g["ty"]) * g["bx"] + x // g["tx"]) * g["tx"] * g["ty"] + (y % g["ty"]) * g["tx"] + x % g["tx"]
    return np.stack([np.asarray(p)[idx] for p in r.read_fb_aux(2)], -1) / spp, ms


def main():
    args = parse_args(lambda ap: (ap.set_defaults(reps=5), ap.add_argument("--samples", type=int, default=16)))
    import torch
    r, note = headline_renderer()
    r.set_gather_planes(9)
    lines = ["direct_light_cost: best of %d; headline tree: %s" % (args.reps, note)]

    def one_round():
        r.direct_light(W, H, samples=1, seed=1)
        t = r.direct_light_last()
        return t["camera_ms"] + t["shade_ms"] + t["gather_ms"] + t["query_ms"], t
    total, t = best_of(args.reps, one_round)
    out = r.direct_light(W, H, samples=1, seed=1)
    lines.append("%dx%d, one round of one sample: camera %.3f ms, shade %.3f ms, gather %.3f ms, %d query launches %.3f ms; sum %.3f ms (%d rows); %r" % (
        W, H, t["camera_ms"], t["shade_ms"], t["gather_ms"], t["query_launches"], t["query_ms"], total, t["rows_per_round"], out["stats"]))
    # the parent's kernels in the same run: the query kernel on the pass's own camera rows ...
    rows = torch.from_numpy(r.direct_light_kat(W, H, seed=1)["cam_rows"]).to("cuda:%d" % r.device)
    torch.cuda.synchronize()

    def query():
        r.intersect(rows)
        return (r.query_last()["ms"],)
    q_ms = best_of(args.reps, query)[0]
    lines.append("parent's query kernel, closest hit of the same %d camera rows: %.3f ms (%.1f Mrays/s)" % (len(rows), q_ms, len(rows) / q_ms / 1e3))
    # ... and render_kernel at 1 spp, bounce_limit 2
    pt_ms = best_of(args.reps, lambda: (path_traced(r, W, H, 1, 1984)[1],))[0]
    lines.append("parent's render_kernel, 1 spp at bounce_limit 2: %.3f ms" % pt_ms)
    # Part 2
    w, h, S = 256, 192, args.samples
    scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_SAH, 1984)
    r.upload_scene(scene)
    r.set_camera(scene.default_camera(w, h))
    ref, _ = path_traced(r, w, h, 4096, 99)

    def direct():
        d = r.direct_light(w, h, samples=S, seed=2)
        t = r.direct_light_last()
        return t["camera_ms"] + t["shade_ms"] + t["gather_ms"] + t["query_ms"], d
    d_ms, d = best_of(args.reps, direct)
    per_spp = best_of(args.reps, lambda: (path_traced(r, w, h, 16, 7)[1] / 16,))[0]
    spp = max(1, int(round(d_ms / per_spp)))
    pt, ms = path_traced(r, w, h, spp, 7)
    held = np.ones((h, w), bool)
    for s in range(4):
        held &= ((r.direct_light_kat(w, h, sample=s, seed=2)["records"][:, 3] & 3) != 2).reshape(h, w)
    rmse = lambda a: float(np.sqrt(((srgb(a) - srgb(ref)) ** 2)[held].mean()))
    lines.append("CORNELL %dx%d against %d spp at bounce_limit 2, %d of %d pixels (no specular first hit), unquantised sRGB RMSE:" % (
        w, h, 4096, int(held.sum()), w * h))
    lines.append("  direct pass, %d samples, %.3f ms of kernels: %.4f" % (S, d_ms, rmse(d["mean"])))
    lines.append("  path tracer, bounce_limit 2, %d spp, %.3f ms of kernel (equal time; %.4f ms per spp): %.4f" % (spp, ms, per_spp, rmse(pt)))
    lines.append("  path tracer, bounce_limit 2, 16 spp: %.4f" % rmse(path_traced(r, w, h, 16, 7)[0]))
    lines.append(json.dumps(dict(reps=args.reps, round_1080p=t, round_1080p_ms=total, query_camera_ms=q_ms, render_1spp_depth2_ms=pt_ms,
                                 cornell=dict(samples=S, direct_ms=d_ms, equal_time_spp=spp, rmse_direct=rmse(d["mean"]), rmse_pt=rmse(pt)))))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
