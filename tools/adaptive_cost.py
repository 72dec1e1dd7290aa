#!/usr/bin/env python3
"""Cost and pay-off of adaptive sampling on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16).

1. MODE 4 against MODE 3: one accumulation pass of 64 spp with every pixel active (adaptive, a tolerance nothing meets) against the
   same pass of a plain accumulation, first pass (cost probe included) and second pass; best of --reps, both in this run.  Wall ms
   (pass enqueued .. done, the queue compaction included) and the render kernel's own ms.
2. Per-pass ms against active pixels: adaptive runs with step = 64, max_spp = 1024, min_spp = 64 at two relative tolerances; the
   pass whose active share is nearest 1 %, and a pass with no active pixel at all (the fixed cost of a pass).
3. Equal-time quality: RMSE of the unquantised sRGB planes against a 4096-spp plain frame, for the adaptive frame and for a plain
   frame whose spp is chosen to take the adaptive run's wall time (measured, printed next to it).

Usage: python tools/adaptive_cost.py [--reps 3] [--out FILE]"""
import json
import time

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, timed, write_report

STEP, MAX_SPP, MIN_SPP = 64, 1024, 64
TOLERANCES = (0.05, 0.02)
NEVER = 1e-30


def pass_pair(r, adaptive):
    """(first pass, second pass) of 64 spp from a fresh grid: each (wall ms, kernel ms)"""
    r.init_device_params(W, H, 64, DEPTH, 1984)
    if adaptive:
        r.accum_reset_adaptive(NEVER, 0.0, 2)
    else:
        r.accum_reset()
    out = []
    for _ in range(2):
        wall = timed(r, lambda: r.render_chunk_accum(W, H, 64))
        out.append((wall, r.last_kernel_ms()))
    if adaptive:
        assert r.accum_active == W * H
    return out


def lin_image(r):
    r.scatter_tiles()
    return np.stack(r.read_fb_aux(1))


def adaptive_run(r, rel):
    """one adaptive run; returns (rows per pass, total wall ms, final unquantised sRGB planes, samples map)"""
    r.init_device_params(W, H, MAX_SPP, DEPTH, 1984)
    r.accum_reset_adaptive(rel, 0.0, MIN_SPP)
    sched = srt.renderer.adaptive_schedule(MIN_SPP, STEP, MAX_SPP)
    rows, total_ms, active = [], 0.0, W * H
    for s in sched:
        before = active
        wall = timed(r, lambda: r.render_chunk_accum(W, H, s))
        t0 = time.perf_counter()
        active = r.accum_active
        wall += (time.perf_counter() - t0) * 1e3
        total_ms += wall
        rows.append(dict(spp_total=r.accum_samples, active_before=before, active_before_pct=round(100.0 * before / (W * H), 3),
                         active_after=active, pass_ms=round(wall, 3), kernel_ms=round(r.last_kernel_ms(), 3), paths=r.stats()["paths"]))
        if active == 0:
            break
    return rows, total_ms, lin_image(r), r.accum_stats(W, H)["samples"]


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def main():
    args = parse_args()
    r, note = headline_renderer()
    r.set_gather_planes(9)
    lines = ["adaptive_cost: random spheres %dx%d, depth %d; tree: %s" % (W, H, DEPTH, note), "plan: %r" % (r.launch_plan(),)]
    report = {"workload": "random spheres %dx%d depth %d" % (W, H, DEPTH), "reps": args.reps}

    # 1. all-active MODE 4 pass against a MODE 3 pass of the same spp
    pass_pair(r, False)          # warm-up
    best = {}
    for _ in range(args.reps):
        for kind in ("mode3", "mode4"):
            pp = pass_pair(r, kind == "mode4")
            for k, (wall, kms) in enumerate(pp):
                key = (kind, k)
                if key not in best or wall < best[key][0]:
                    best[key] = (wall, kms)
    report["all_active_64spp"] = {}
    for k, what in ((0, "first pass (probe)"), (1, "second pass")):
        m3, m4 = best[("mode3", k)], best[("mode4", k)]
        lines.append("all-active 64-spp %-18s MODE 3 %8.3f ms (kernel %8.3f)  MODE 4 %8.3f ms (kernel %8.3f)  MODE 4 vs 3: wall %+.2f %%, kernel %+.2f %%" %
                     (what, m3[0], m3[1], m4[0], m4[1], 100.0 * (m4[0] / m3[0] - 1.0), 100.0 * (m4[1] / m3[1] - 1.0)))
        report["all_active_64spp"][what] = dict(mode3_ms=round(m3[0], 3), mode3_kernel_ms=round(m3[1], 3), mode4_ms=round(m4[0], 3),
                                                 mode4_kernel_ms=round(m4[1], 3))

    # 3 (reference first): the 4096-spp plain frame and the cost of a plain frame per sample
    r.init_device_params(W, H, 4096, DEPTH, 1984)
    r.render_chunk(W, H)
    ref = lin_image(r)
    r.init_device_params(W, H, 1024, DEPTH, 1984)
    plain_1024_ms = best_of(2, lambda: timed(r, lambda: r.render_chunk(W, H)))
    plain_1024 = lin_image(r)
    lines.append("plain 1024 spp: %.2f ms, RMSE vs 4096 spp %.6f" % (plain_1024_ms, rmse(plain_1024, ref)))
    report["plain_1024"] = dict(ms=round(plain_1024_ms, 2), rmse=rmse(plain_1024, ref))

    # 2. per-pass cost against active pixels, and 3. equal-time quality
    report["runs"] = []
    for rel in TOLERANCES:
        rows, total_ms, img, samples = adaptive_run(r, rel)
        lines.append("adaptive rel_tol %g (min_spp %d, step %d, max_spp %d): %d passes, %.2f ms in all, mean spp %.1f, "
                     "pixels at max_spp %.2f %%" % (rel, MIN_SPP, STEP, MAX_SPP, len(rows), total_ms, float(samples.mean()),
                                                     100.0 * float((samples == MAX_SPP).mean())))
        for row in rows:
            lines.append("  pass to %4d spp  active before %8d (%7.3f %%)  after %8d  pass %8.3f ms  kernel %8.3f ms" %
                         (row["spp_total"], row["active_before"], row["active_before_pct"], row["active_after"], row["pass_ms"], row["kernel_ms"]))
        later = rows[1:] or rows
        near1 = min(later, key=lambda x: abs(x["active_before_pct"] - 1.0))
        lines.append("  pass nearest 1 %% active: %.3f %% active, %.3f ms (kernel %.3f ms)" % (near1["active_before_pct"], near1["pass_ms"], near1["kernel_ms"]))
        spp_eq = max(1, int(round(1024.0 * total_ms / plain_1024_ms)))
        r.init_device_params(W, H, spp_eq, DEPTH, 1984)
        eq_ms = timed(r, lambda: r.render_chunk(W, H))
        eq_img = lin_image(r)
        e_ad, e_pl = rmse(img, ref), rmse(eq_img, ref)
        lines.append("  equal time: adaptive RMSE %.6f in %.2f ms; plain %d spp RMSE %.6f in %.2f ms  (adaptive / plain RMSE %.3f)" %
                     (e_ad, total_ms, spp_eq, e_pl, eq_ms, e_ad / e_pl))
        report["runs"].append(dict(rel_tol=rel, passes=rows, total_ms=round(total_ms, 2), mean_spp=float(samples.mean()),
                                   rmse_adaptive=e_ad, plain_equal_time_spp=spp_eq, plain_equal_time_ms=round(eq_ms, 2), rmse_plain_equal_time=e_pl,
                                   pass_nearest_1pct=near1))

    # the fixed cost of a pass: one in which no pixel is active (everything stopped after the first pass)
    r.init_device_params(W, H, 128, DEPTH, 1984)
    r.accum_reset_adaptive(1e3, 1e3, MIN_SPP)
    r.render_chunk_accum(W, H, MIN_SPP)
    assert r.accum_active == 0
    empty = best_of(args.reps, lambda: timed(r, lambda: r.render_chunk_accum(W, H, 1)))
    lines.append("pass with no active pixel: %.3f ms (kernel %.3f ms)" % (empty, r.last_kernel_ms()))
    report["empty_pass_ms"] = round(empty, 3)

    lines.append(json.dumps(report))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
