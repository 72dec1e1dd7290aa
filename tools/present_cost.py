#!/usr/bin/env python3
"""Cost of presenting on the device, on the headline workload (random spheres, the throughput-tuned SAH tree, 1920x1080, depth 16) with a
16-spp spectral featured accumulation, which every source can read: for the sources accum, denoise (five levels) and develop (the
colour-matching rows), at a fixed gain and metered, the present kernel (HIP events, srt_present_last_ms), the whole call srt_present as
wall ms (stage kernels, the 8.3 MB picture through pinned memory, synchronise, the row copy), and in the same run the path it replaces on
the entry points that existed before it -- the stage's call with its float XYZ output, (metered: srt_meter_kat,) then srt_expose_kat or
srt_expose_accum with out_q alone.  The replaced path is flattered: its developed sums are normalised with one numpy product, and
nothing packs its float32 out_q into bytes.  Both paths write into buffers allocated once.  Then present_kernel's 16-byte path against
its scalar path on the same 1920x1080 XYZ mean (a second context under the fenced test knob SRT_PRESENT_SCALAR).  Every figure is the
best of --reps (default 5) from this one run; the bytes of the two paths are compared.  Nothing here is gated.  Prints one line per row
and a JSON line.

Usage: python tools/present_cost.py [--reps 5] [--out FILE]"""
import ctypes as C
import json
import os

import numpy as np

from _cost_common import DEPTH, H, W, best_of, headline_renderer, parse_args, srt, timed, write_report

SPP = 16
GAIN = 0.8
F = np.float32


def main():
    args = parse_args(lambda ap: ap.set_defaults(reps=5))
    r, note = headline_renderer()
    L, B = srt.binding.lib(), srt.binding
    lines = ["present_cost: random spheres %dx%d, depth %d, %d-spp spectral featured accumulation; tree: %s" % (W, H, DEPTH, SPP, note)]
    r.set_gather_planes(9)
    r.init_device_params(W, H, SPP, DEPTH, 1984)
    r.accum_reset_spectral_features()
    r.render_chunk_accum(W, H, SPP)
    r.synchronize()
    rgba = np.zeros((H, W, 4), np.uint8)
    xyz, q = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    u8p = C.POINTER(C.c_uint8)
    inv = F(1) / F(SPP)
    rows = []

    def present(source, gain, **cfg):
        p, res = srt.present_config(source, gain, **cfg), B.PresentResult()
        r._ck(L.srt_present(r._h, C.byref(p), rgba.ctypes.data_as(u8p), 4 * W, W, H, C.byref(res)))
        return res

    def replaced(source, gain, **cfg):
        """the stage's float XYZ to the host, the exposure through the KAT doors, out_q alone; returns the gain used"""
        if source == "accum":
            if gain is None:
                gain = r.meter()["gain"]
            t = srt.tone_config(gain=gain)
            r._ck(L.srt_expose_accum(r._h, C.byref(t), None, None, B.fptr(q), None, W, H))
            return gain
        if source == "denoise":
            d = srt.denoise_config(**cfg)
            r._ck(L.srt_denoise_features(r._h, C.byref(d), B.fptr(xyz), None, None, W, H))
            mean = xyz
        else:
            r._ck(L.srt_develop_spectral_srgb(r._h, None, srt.renderer.CIE_SCALE, B.fptr(xyz), None, None, W, H))
            mean = (inv * xyz).astype(F)
        if gain is None:
            res = B.MeterResult()
            m = srt.meter_config()
            r._ck(L.srt_meter_kat(r._h, C.byref(m), B.fptr(mean), W, H, None, C.byref(res)))
            gain = res.gain
        t = srt.tone_config(gain=gain)
        r._ck(L.srt_expose_kat(r._h, C.byref(t), B.fptr(mean), W, H, None, None, B.fptr(q), None))
        return gain

    for source, cfg in (("accum", {}), ("denoise", dict(levels=5)), ("develop", {})):
        for gain in (GAIN, None):
            tag = "%s, %s" % (source, "metered" if gain is None else "gain %.1f" % gain)
            present(source, gain, **cfg)          # warm-up (code object, the working blocks' allocation)
            replaced(source, gain, **cfg)

            def once():
                wall = timed(r, lambda: present(source, gain, **cfg))
                return wall, r.present_last_ms()
            new = best_of(args.reps, once)
            old = best_of(args.reps, lambda: timed(r, lambda: replaced(source, gain, **cfg)))
            present(source, gain, **cfg)
            replaced(source, gain, **cfg)
            same = bool(np.array_equal(rgba[..., :3], q.astype(np.uint8)) and (rgba[..., 3] == 255).all())
            row = dict(source=source, metered=gain is None, present_kernel_ms=round(new[1], 4), present_call_ms=round(new[0], 3), replaced_path_ms=round(old, 3),
                       bytes_equal=same)
            rows.append(row)
            lines.append("%-22s present kernel %7.4f ms  srt_present %8.3f ms  replaced path %8.3f ms  same bytes: %s" % (tag, new[1], new[0], old, same))

    # the 16-byte path against the scalar path, the same picture through present_kernel's form b
    r._ck(L.srt_denoise_features(r._h, C.byref(srt.denoise_config(levels=5)), B.fptr(xyz), None, None, W, H))
    saved = {k: os.environ.get(k) for k in ("SRT_TEST_KNOBS", "SRT_PRESENT_SCALAR")}
    os.environ.update(SRT_TEST_KNOBS="1", SRT_PRESENT_SCALAR="1")
    try:
        scalar = srt.Renderer(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    paths = {}
    for name, ctx in (("16-byte path", r), ("scalar path", scalar)):
        out = ctx.present_kat(xyz, gain=GAIN)["rgba"]
        def once():
            ctx.present_kat(xyz, gain=GAIN)
            return ctx.present_last_ms()
        paths[name] = (round(best_of(args.reps, once), 4), out)
    scalar.close()
    same = bool(np.array_equal(paths["16-byte path"][1], paths["scalar path"][1]))
    lines.append("present_kernel on the denoised %dx%d XYZ mean: 16-byte path %.4f ms, scalar path %.4f ms; same bytes: %s" % (
        W, H, paths["16-byte path"][0], paths["scalar path"][0], same))
    lines.append(json.dumps({"workload": "random spheres %dx%d depth %d, %d spp" % (W, H, DEPTH, SPP), "reps": args.reps, "picture_bytes": 4 * W * H, "rows": rows,
                             "kernel_paths_ms": {k: v[0] for k, v in paths.items()}, "kernel_paths_same_bytes": same}))
    write_report(lines, args.out)
    r.close()


if __name__ == "__main__":
    main()
