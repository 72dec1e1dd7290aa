"""The CPU prediction of the first-hit feature buffers (srt_accum_reset_features, render_kernel MODE 7), shared by test_features.py and
test_features_api.py.  It uses the oracle and the scene's own material list and nothing of the product: per sample, every pixel's
XORWOW state is copied into an orc.Rng, the camera ray of get_ray (oracle/srt_oracle.c) is restated in numpy float32 operation by
operation from the oracle's own draws, orc_trace_ray gives t, the face-forwarded normal and the material, the eight increments are
added in float32, and a 1-spp render of the oracle advances all the states to the next sample."""
import ctypes as C

import numpy as np

from accum_helpers import SEED, lane_of, named_workload, shape_case
from helpers import oracle_scene_for

F = np.float32
CHANNELS = 8


def seeded_states(orc, geom, seed=SEED):
    """(n_lanes, 6) uint32: the oracle's XORWOW state (d, v[0..4]) of every lane of the grid, curand_init(seed + idx, 0, 0)"""
    states = np.zeros((geom["n_lanes"], 6), np.uint32)
    rs = orc.Rng()
    for idx in range(geom["n_lanes"]):
        orc.lib().orc_rng_init(seed + idx, C.byref(rs))
        states[idx, 0] = rs.d
        states[idx, 1:] = rs.v[:]
    return states


def grid_of(W, H, tx=28, ty=16):
    bx, by = W // tx + 1, H // ty + 1
    return dict(tx=tx, ty=ty, bx=bx, by=by, n_lanes=tx * ty * bx * by)


def camera_rays(orc, cam, states, lane, W, H, offx=0, offy=0):
    """get_ray restated for the row-major pixels of a W x H chunk at (offx, offy): the draws come from a copy of each pixel's state
    through the oracle's own orc_random_float (jitter x, jitter y, then the defocus-disk rejection loop when defocus_angle > 0, then
    the hero wavelength of ray_init); the arithmetic is numpy float32 in the oracle's order.  Returns (origins (n, 3), directions
    (n, 3), the states after the sample's camera-ray draws (n, 6))."""
    L = orc.lib()
    n = W * H
    lens = cam.defocus_angle > 0.0
    px, py, dx, dy = (np.zeros(n, F) for _ in range(4))
    after = np.zeros((n, 6), np.uint32)
    rs = orc.Rng()
    for k in range(n):
        st = states[lane[k]]
        rs.d = int(st[0])
        rs.v[:] = [int(v) for v in st[1:]]
        px[k] = F(-0.5) + F(L.orc_random_float(C.byref(rs)))              # pixel_sample_square
        py[k] = F(-0.5) + F(L.orc_random_float(C.byref(rs)))
        if lens:                                                          # random_in_unit_disk: random_float_range(-1, 1) twice per try
            while True:
                x = F(L.orc_random_float(C.byref(rs))) * F(2.0) + F(-1.0)
                y = F(L.orc_random_float(C.byref(rs))) * F(2.0) + F(-1.0)
                if (x * x + y * y) + F(0.0) * F(0.0) < F(1.0):
                    break
            dx[k], dy[k] = x, y
        L.orc_random_float(C.byref(rs))                                   # ray_init: the hero wavelength
        after[k, 0] = rs.d
        after[k, 1:] = rs.v[:]
    du, dv, p00 = (np.array(v[:], F) for v in (cam.pixel_delta_u, cam.pixel_delta_v, cam.pixel00_loc))
    center, disk_u, disk_v = (np.array(v[:], F) for v in (cam.camera_center, cam.defocus_disk_u, cam.defocus_disk_v))
    j, i = np.divmod(np.arange(n), W)
    fi, fj = (offx + i).astype(F)[:, None], (offy + j).astype(F)[:, None]
    pixel_center = (p00 + fi * du) + fj * dv
    pixel_sample = pixel_center + (px[:, None] * du + py[:, None] * dv)
    if lens:
        origin = (center + dx[:, None] * disk_u) + dy[:, None] * disk_v
    else:
        origin = np.broadcast_to(center, (n, 3)).astype(F)
    direction = pixel_sample - origin
    assert pixel_sample.dtype == F and origin.dtype == F and direction.dtype == F
    return np.ascontiguousarray(origin), np.ascontiguousarray(direction), after


def material_colours(scene):
    return np.array([[m.col[0], m.col[1], m.col[2]] for m in scene.materials()], F).reshape(-1, 3)


def predict_features(orc, scene, cam, W, H, n, depth, mode, seed=SEED, offx=0, offy=0):
    """dict(rows (H, W, 8) float32 raw sums after n samples, mats (n, H, W) int32: the material of every sample's first hit, -1 on a
    miss) for a W x H chunk at (offx, offy) of the camera's image, on the chunk's own reference grid"""
    osc = oracle_scene_for(orc, scene, mode)
    geom = grid_of(W, H)
    lane = lane_of(geom, W, H)
    states = seeded_states(orc, geom, seed)
    col = material_colours(scene)
    rows = np.zeros((W * H, CHANNELS), F)
    mats = np.full((n, W * H), -1, np.int32)
    out9 = np.zeros(9, F)
    p_out = orc.fptr(out9)
    trace = orc.lib().orc_trace_ray
    f3 = C.c_float * 3
    for s in range(n):
        origin, direction, _ = camera_rays(orc, cam, states, lane, W, H, offx, offy)
        inc = np.zeros((W * H, CHANNELS), F)
        if depth > 0:
            length = np.sqrt((direction[:, 0] * direction[:, 0] + direction[:, 1] * direction[:, 1]) + direction[:, 2] * direction[:, 2])
            assert length.dtype == F
            for k in range(W * H):
                if trace(osc.h, f3(*origin[k]), f3(*direction[k]), p_out):
                    m = int(out9[8])
                    mats[s, k] = m
                    inc[k, 0:3] = out9[4:7]
                    inc[k, 3:6] = col[m] if m < len(col) else 0.0
                    inc[k, 6] = out9[0] * length[k]
                    inc[k, 7] = 1.0
        rows = rows + inc
        assert rows.dtype == F
        osc.render(cam, W, H, 1, depth, offx=offx, offy=offy, seed=seed, states=states)      # every lane's state moves on by one sample
    osc.close()
    return dict(rows=rows.reshape(H, W, CHANNELS), mats=mats.reshape(n, H, W))


def stack_features(feat):
    """the dict of Renderer.read_features back as (H, W, 8) rows"""
    return np.concatenate([feat["normal"], feat["albedo"], feat["distance"][..., None], feat["hits"][..., None]], axis=-1).astype(F)


_cache = {}


def workload_prediction(srt, orc, name, n):
    """(workload tuple of named_workload, prediction) computed once per (name, n)"""
    key = (name, n)
    if key not in _cache:
        wl = named_workload(srt, name)
        scene, cam, W, H, depth, mode = wl
        _cache[key] = (wl, predict_features(orc, scene, cam, W, H, n, depth, mode))
    return _cache[key]


def shape_prediction(srt, orc, paired, n):
    key = ("shape", paired, n)
    if key not in _cache:
        case = shape_case(srt, paired)
        scene, cam, W, H, depth = case
        _cache[key] = (case, predict_features(orc, scene, cam, W, H, n, depth, 1))
    return _cache[key]
