#!/usr/bin/env python3
"""Cost of the BVH refit on the device (srt_refit_vertices / srt_refit_vertices_dev) and what it costs in tree quality, every figure from
this one run, the best of --reps (default 5) after a warm-up.  Nothing here is gated: the figures are findings.

For the headline random-spheres scene and for SRT_SCENE_MESH100K (SAH trees), under a smooth deformation (smooth below:
a sine wave along x displaces y and z by `--amp` scene units):
  the refit's kernels   HIP events (srt_refit_last_ms): the triangle kernel, all level launches together, and their number
  the whole call        wall ms from a host array and from a device pointer (a torch tensor)
  the path it replaces  srt_scene_set_triangles + srt_scene_build_bvh + srt_upload_scene, wall ms, and its three parts
  the path in between   srt_scene_refit + srt_upload_scene
  tree quality          the render kernel's time for a 960x540 frame (16 spp, depth 16) on the refitted tree against
                        a tree freshly built from the deformed triangles, at the deformation above and at four times its amplitude
The fused top-level kernel the design mentions as an option was not built, so there is no figure for it.
Prints one line per row and a JSON line.

Usage: python tools/refit_cost.py [--reps 5] [--amp 0.35] [--out profiles/refit/refit_cost.txt]"""
import ctypes as C
import json
import time

import numpy as np

from _cost_common import best_of, parse_args, srt, timed, write_report

FW, FH, SPP, DEPTH = 960, 540, 16, 16


def smooth(v0, phase, amp):
    """a smooth deformation: a sine wave along x displaces y and z, so that neighbouring triangles keep their shared vertices"""
    v = v0.copy()
    v[..., 1] = v0[..., 1] + np.float32(amp) * np.sin(np.float32(phase) * v0[..., 0] + np.float32(0.3))
    v[..., 2] = v0[..., 2] + np.float32(amp) * np.cos(np.float32(phase) * v0[..., 0])
    return np.ascontiguousarray(v, np.float32)


def moved(scene, vertices):
    """a fresh scene (no BVH) of `scene`'s triangles with the vertices replaced: materials, aa_plane and background as they are"""
    t0 = scene.triangles()
    T = (srt.binding.TriIn * len(t0))()
    C.memmove(T, t0, C.sizeof(T))
    words = np.frombuffer(T, np.float32).reshape(len(t0), C.sizeof(srt.binding.TriIn) // 4)
    words[:, :9] = vertices.reshape(len(t0), 9)
    return srt.Scene.from_arrays(T, scene.materials(), scene.background())


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def frame_ms(r, cam, reps):
    """kernel ms of one frame of the uploaded scene from `cam`"""
    r.set_camera(cam); r.set_partition(0, 1)

    def once():
        r.init_device_params(FW, FH, SPP, DEPTH, 1984)
        r.render_chunk(FW, FH)
        r.synchronize()
        return r.last_kernel_ms()
    once()
    return best_of(reps, once)


def measure(r, label, scene_id, reps, amp, lines):
    import torch
    B, L = srt.binding, srt.binding.lib()
    scene = srt.Scene.builtin(scene_id, 0).build_bvh(srt.BVH_SAH, 1984)
    n = scene.n_tris
    v0 = scene.vertices()
    flat = v0.reshape(-1, 3)
    extent = (flat.max(0) - flat.min(0)).tolist()
    v1 = smooth(v0, 0.7, amp)
    r.upload_scene(scene)
    r.refit(v1)      # warm-up: the tables reach the device, scratch and staging are allocated
    row = dict(scene=label, triangles=n, extent=[round(float(e), 2) for e in extent], amplitude=amp)

    def host_entry():
        w = timed(r, lambda: r.refit(v1))
        return (w, r.refit_last_ms())
    w, ms = best_of(reps, host_entry)
    row.update(call_host_ms=round(w, 4), tri_kernel_ms=round(ms["triangles"], 4), level_kernels_ms=round(ms["levels"], 4), n_levels=ms["n_levels"])
    t1 = torch.from_numpy(v1).to(torch.device("cuda", r.device))
    r.refit(t1)
    w_dev, ms_dev = best_of(reps, lambda: (timed(r, lambda: r.refit(t1)), r.refit_last_ms()))
    row.update(call_dev_ms=round(w_dev, 4), tri_kernel_dev_ms=round(ms_dev["triangles"], 4), level_kernels_dev_ms=round(ms_dev["levels"], 4))
    lines.append("%-16s %7d triangles, extent %s, amplitude %.2f" % (label, n, row["extent"], amp))
    lines.append("%-16s refit kernels: triangles %.4f ms, %d level launches %.4f ms; whole call: host array %.3f ms, device pointer %.3f ms" % (
        "", ms["triangles"], ms["n_levels"], ms["levels"], w, w_dev))

    # the path the refit replaces, on a scene of its own
    tris = moved(scene, v1).triangles()
    other = moved(scene, v0)
    parts = {}

    def rebuild():
        parts["set"] = wall(lambda: B.check(L.srt_scene_set_triangles(other.handle, tris, len(tris))))
        parts["build"] = wall(lambda: other.build_bvh(srt.BVH_SAH, 1984))
        parts["upload"] = timed(r, lambda: r.upload_scene(other))
        return (parts["set"] + parts["build"] + parts["upload"], dict(parts))
    rebuild()
    w_re, p = best_of(reps, rebuild)
    row.update(rebuild_ms=round(w_re, 3), rebuild_parts_ms={k: round(v, 3) for k, v in p.items()})
    lines.append("%-16s the path it replaces: %.3f ms (set_triangles %.3f, build_bvh %.3f, upload_scene %.3f)" % ("", w_re, p["set"], p["build"], p["upload"]))

    def host_refit():
        a = wall(lambda: scene.refit(v1))
        b = timed(r, lambda: r.upload_scene(scene))
        return (a + b, a, b)
    host_refit()
    w_mid, a, b = best_of(reps, host_refit)
    row.update(host_refit_upload_ms=round(w_mid, 3), host_refit_ms=round(a, 3), upload_ms=round(b, 3))
    lines.append("%-16s the path in between: %.3f ms (srt_scene_refit %.3f, upload_scene %.3f)" % ("", w_mid, a, b))
    lines.append("%-16s per frame: rebuild / refit from a host array = %.0fx, rebuild / refit from a device pointer = %.0fx" % ("", w_re / w, w_re / w_dev))

    # tree quality: the same deformed geometry on the refitted tree and on a freshly built one
    quality, cam = [], scene.default_camera(FW, FH)      # (the built-in scene's camera for both trees)
    for scale in (1.0, 4.0):
        v = smooth(v0, 0.7, amp * scale)
        scene.refit(v0); r.upload_scene(scene); r.refit(v)
        refitted = frame_ms(r, cam, reps)
        fresh = moved(scene, v).build_bvh(srt.BVH_SAH, 1984)
        r.upload_scene(fresh)
        built = frame_ms(r, cam, reps)
        quality.append(dict(amplitude=amp * scale, refitted_ms=round(refitted, 3), rebuilt_ms=round(built, 3)))
        lines.append("%-16s frame %dx%d, %d spp, depth %d at amplitude %.2f: refitted tree %.3f ms, freshly built tree %.3f ms (%+.1f %%)" % (
            "", FW, FH, SPP, DEPTH, amp * scale, refitted, built, 100.0 * (refitted / built - 1.0)))
    row["quality"] = quality
    return row


def main():
    args = parse_args(lambda ap: (ap.set_defaults(reps=5), ap.add_argument("--amp", type=float, default=0.35)))
    r = srt.Renderer(0)
    lines = ["refit_cost: best of %d; the refit keeps the topology, the rebuild is the SAH builder on the moved triangles" % args.reps,
             "fused top-level kernel: not built, no figure"]
    rows = [measure(r, "random spheres", srt.SCENE_RANDOM_SPHERES, args.reps, args.amp, lines),
            measure(r, "mesh100k", srt.SCENE_MESH100K, args.reps, args.amp, lines)]
    lines.append(json.dumps({"reps": args.reps, "rows": rows}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
