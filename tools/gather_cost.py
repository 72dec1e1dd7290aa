#!/usr/bin/env python3
"""Cost of gathering an accumulation (srt_comm_gather_accum: srt_pack_accum on every rank, one gather, srt_unpack_accum on rank 0) on the
1080p headline frame (random spheres, SAH tree, 1920x1080, depth 16, one 16-spp pass), at W = 2, 4 and 8 ranks.

All ranks live on ONE device and the exchange goes over the test transport (tests/cpp/mock_rccl.cpp, built by __graft_entry__.build()):
the transport time reported here is a device-to-device copy and says NOTHING about xGMI -- RCCL has never carried this path.  What the
figures do say: the kernel times of pack and unpack (HIP events around each: srt_gather_last_ms on rank 0) and the bandwidth they achieve
-- every word is read once and written once, so 2 x the bytes moved -- next to the develop kernel's film read in the same run (384 B per
pixel read, 12 written) as the yardstick; the wall time of the whole call; and the 4-byte paths (test knob SRT_GATHER_SCALAR) against the
16-byte paths at W = 2.  The accumulations: featured (11 words per pixel) and spectral featured with its film (107) at every W, and at
W = 2 their adaptive siblings, which add the sample map and S2 (13 and 109).  Best of --reps from one run.  Nothing is gated.

Usage: python tools/gather_cost.py [--reps 5] [--out profiles/gather/gather_cost.txt]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "cpp", "_build", "libmock_rccl.so")
if not os.path.exists(MOCK):
    sys.exit("gather_cost: %s is missing (python -c 'import __graft_entry__ as g; g.build()')" % MOCK)
os.environ.update(SRT_RCCL_LIB=MOCK, SRT_COMM_TEST_SAME_DEVICE="1", SRT_TEST_KNOBS="1")      # (before the library looks for an RCCL)

from _cost_common import DEPTH, H, W, parse_args, srt, write_report  # noqa: E402

SPP = 16
KINDS = (("featured", lambda c: c.accum_reset_features(), ("sums", "features"), 11),
         ("adaptive featured", lambda c: c.accum_reset_adaptive_features(1e-30, 0.0, SPP), ("sums", "counts", "features"), 13),
         ("spectral featured + film", lambda c: c.accum_reset_spectral_features(), ("sums", "features", "film"), 107),
         ("adaptive spectral featured + film", lambda c: c.accum_reset_adaptive_spectral_features(1e-30, 0.0, SPP), ("sums", "counts", "features", "film"), 109))


def measure(scene, cam, world, reset, parts, reps, scalar=False):
    """dict of the best of `reps` gathers of one accumulation on a communicator of `world` ranks on device 0"""
    if scalar:
        os.environ["SRT_GATHER_SCALAR"] = "1"
    try:
        comm = srt.Comm.init_all([0] * world)      # (the contexts read the knob when they are made)
    finally:
        os.environ.pop("SRT_GATHER_SCALAR", None)
    try:
        comm.upload_scene(scene); comm.set_camera(cam)
        comm.init_device_params(W, H, SPP, DEPTH, 1984)
        reset(comm)
        comm.synchronize()
        t0 = time.perf_counter()
        comm.render_frame_accum(W, H, SPP)
        comm.synchronize()
        pass_ms = (time.perf_counter() - t0) * 1e3
        root = comm.root
        unit = root.accum_exchange_size(parts) * 4
        best = None
        for k in range(reps + 1):      # (the first call allocates: not counted)
            comm.synchronize()
            t0 = time.perf_counter()
            comm.gather_accum(parts)
            comm.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            pack, unpack = root.gather_last_ms()
            _, exchange, _ = comm.last_accum_gather_ms()
            row = dict(wall=wall, pack=pack, unpack=unpack, exchange=exchange)
            if k > 0:
                best = row if best is None else {key: min(best[key], row[key]) for key in row}
        develop = None
        if "film" in parts:
            root.develop_spectral(W, H, srt.renderer.cie_response())
            root.develop_spectral(W, H, srt.renderer.cie_response())
            develop = root.develop_last_ms()["contract"]
        return dict(best, unit_bytes=unit, pass_ms=pass_ms, develop=develop, world=world)
    finally:
        comm.close()


def gbps(n_bytes, ms):
    return n_bytes / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")


def main():
    args = parse_args()
    args.reps = max(args.reps, 1)
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    cam = scene.default_camera(W, H)
    lines = ["gather_cost: random spheres %dx%d, depth %d, one %d-spp pass; ranks on ONE device over the test transport; best of %d" % (W, H, DEPTH, SPP, args.reps),
             "the exchange column is a device-to-device copy on one GPU: it says nothing about xGMI, and RCCL has never carried this path",
             "pack / unpack: kernel ms on rank 0 (HIP events); GB/s = 2 x bytes moved / kernel time (every word read once, written once)",
             "%-34s %2s %6s %9s | %8s %7s | %8s %7s | %9s %8s | %9s" % ("accumulation", "W", "words", "unit MB", "pack ms", "GB/s", "unpack ms", "GB/s", "copy ms", "call ms", "pass ms")]
    rows = []
    for world in (2, 4, 8):
        for name, reset, parts, words in KINDS:
            if "adaptive" in name and world != 2:
                continue
            m = measure(scene, cam, world, reset, parts, args.reps)
            m.update(name=name, words=words)
            rows.append(m)
            lines.append("%-34s %2d %6d %9.1f | %8.3f %7.0f | %8.3f %7.0f | %9.3f %8.3f | %9.1f" % (
                name, world, words, m["unit_bytes"] / 1e6, m["pack"], gbps(2 * m["unit_bytes"], m["pack"]), m["unpack"],
                gbps(2 * (world - 1) * m["unit_bytes"], m["unpack"]), m["exchange"], m["wall"], m["pass_ms"]))
            if m["develop"]:
                n_pix = W * H
                lines.append("%-34s    the develop kernel's film read, same run: %.3f ms, %.0f GB/s (396 B per pixel)" % ("", m["develop"], gbps(396 * n_pix, m["develop"])))
    lines.append("the 4-byte paths alone (SRT_GATHER_SCALAR) against the 16-byte paths, W = 2:")
    for name, reset, parts, words in (KINDS[0], KINDS[2]):
        s = measure(scene, cam, 2, reset, parts, args.reps, scalar=True)
        v = next(r for r in rows if r["name"] == name and r["world"] == 2)
        s.update(name=name + " (scalar)", words=words)
        rows.append(s)
        lines.append("%-34s pack %.3f ms scalar / %.3f ms vector, unpack %.3f / %.3f" % (name, s["pack"], v["pack"], s["unpack"], v["unpack"]))
    lines.append(json.dumps(dict(tool="gather_cost", rows=rows)))
    write_report(lines, args.out)


if __name__ == "__main__":
    main()
