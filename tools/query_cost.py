#!/usr/bin/env python3
"""Cost of the batched ray queries (srt_intersect_rays*, srt_occluded_rays*) against srt_trace_rays, every figure from this one run, the best
of --reps (default 5) after a warm-up.  Nothing here is gated: the figures are findings.

Setup   the headline scene on the tree bench.py times (random spheres, the throughput-tuned SAH tree), and the closest-hit queries of one
        1920x1080 frame at 1 spp, bounce limit 16, from srt_collect_ray_segments (origin, direction, t_end; t_end = FLT_MAX for a miss):
        the camera rays (origin on the camera's defocus disk; one per pixel) and all rays, separately.
Rows    srt_trace_rays, whole call (the parent's path: host rows in, blocking copies, one 64-lane workgroup per 64 rays);
        intersect over [0, FLT_MAX], host entry and device entry (a torch tensor, the current stream): kernel (HIP events, srt_query_last)
        and whole call (wall, the device waited for);
        occluded over [0, t_end] of the segments that hit (every query ends at its first accepted triangle);
        occluded over [0, 0.5 t_end] of the same segments (nothing is occluded: every query walks to its end).
ms and Mrays/s per row.  Prints one line per row and a JSON line.

Usage: python tools/query_cost.py [--reps 5] [--out profiles/query/query_cost.txt]"""
import json

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, timed, write_report

FLT_MAX = float(np.finfo(np.float32).max)


def main():
    args = parse_args(lambda ap: ap.set_defaults(reps=5))
    import torch
    r, note = headline_renderer()
    dev = torch.device("cuda:%d" % r.device)
    segs, queries = r.collect_ray_segments(W, H, 1, DEPTH, stride=1, capacity=8 * W * H)
    assert len(segs) == queries, (len(segs), queries)
    # camera rays: the headline camera has a lens (defocus), so its rays start on the defocus disk about the centre, not at the centre
    cam = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).default_camera(W, H)
    centre = np.array(list(cam.camera_center), np.float64)
    radius = np.linalg.norm(list(cam.defocus_disk_u)) + np.linalg.norm(list(cam.defocus_disk_v))
    camera = np.linalg.norm(segs[:, 0:3].astype(np.float64) - centre, axis=1) <= radius * (1 + 1e-5) + 1e-6
    plan = r.launch_plan()
    lines = ["query_cost: best of %d; headline tree: %s" % (args.reps, note),
             "%dx%d, 1 spp, bounce limit %d: %d closest-hit queries, %d of them camera rays; plan: narrow_refs %d, all_cached %d, paired %d, "
             "n_cached %d" % (W, H, DEPTH, len(segs), int(camera.sum()), plan["narrow_refs"], plan["all_cached"], plan["paired"], plan["n_cached"])]
    rows = []

    def row(label, n, kernel_ms, call_ms, extra=""):
        d = dict(rays=label[0], row=label[1], n=int(n), kernel_ms=None if kernel_ms is None else round(kernel_ms, 4), call_ms=round(call_ms, 3))
        rows.append(d)
        k = "kernel %8.3f ms %8.1f Mrays/s   " % (kernel_ms, n / kernel_ms / 1e3) if kernel_ms is not None else " " * 38
        lines.append("%-7s %-40s %9d rays  %swhole call %8.3f ms %8.1f Mrays/s%s" % (label[0], label[1], n, k, call_ms, n / call_ms / 1e3, extra))

    for name, sel in (("camera", camera), ("all", np.ones(len(segs), bool))):
        s = segs[sel]
        n = len(s)
        if n == 0:
            lines.append("%-7s no rays" % name)
            continue
        six = np.ascontiguousarray(s[:, 0:6])
        full = srt.ray_batch(s[:, 0:3], s[:, 3:6])
        trace = r.trace_rays(six)
        row((name, "srt_trace_rays (parent path)"), n, None, best_of(args.reps, lambda: timed(r, lambda: r.trace_rays(six))))

        def host(fn, rays):
            def once():
                ms = timed(r, lambda: fn(rays))
                return ms, r.query_last()["ms"]
            return once
        fn_i, fn_o = r.intersect, r.occluded
        got = r.intersect(full)
        assert np.array_equal(got.view(np.uint32), trace.view(np.uint32)), "%s: intersect over [0, FLT_MAX] differs from srt_trace_rays" % name
        call, kern = best_of(args.reps, host(fn_i, full))
        row((name, "intersect [0, FLT_MAX], host entry"), n, kern, call)
        full_t = torch.from_numpy(full).to(dev)
        torch.cuda.synchronize(dev)
        r.intersect(full_t)
        call, kern = best_of(args.reps, host(fn_i, full_t))
        row((name, "intersect [0, FLT_MAX], device entry"), n, kern, call, "   waves %d" % r.query_last()["waves"])
        hit = s[:, 6] < FLT_MAX
        for label, scale in (("occluded [0, t_end] of the hits", 1.0), ("occluded [0, 0.5 t_end] of the hits", 0.5)):
            q = srt.ray_batch(s[hit, 0:3], s[hit, 3:6], 0.0, (s[hit, 6] * np.float32(scale)).astype(np.float32))
            occ = r.occluded(q)
            want = scale == 1.0
            share = float(occ.mean())
            qt = torch.from_numpy(q).to(dev)
            torch.cuda.synchronize(dev)
            r.occluded(qt)
            call, kern = best_of(args.reps, host(fn_o, qt))
            row((name, label + ", device entry"), int(hit.sum()), kern, call, "   occluded share %.4f (%s expected)" % (share, "all" if want else "none"))
            rows[-1]["occluded_share"] = share
    lines.append(json.dumps({"reps": args.reps, "width": W, "height": H, "bounce_limit": DEPTH, "queries": int(len(segs)),
                             "camera_rays": int(camera.sum()), "plan": {k: plan[k] for k in ("narrow_refs", "all_cached", "paired", "n_cached")},
                             "rows": rows}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
