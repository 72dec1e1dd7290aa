import os

import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_planes_equal(got, want, what):
    for c, (a, b) in enumerate(zip(got, want)):
        ba, bb = bits(a), bits(b)
        if not np.array_equal(ba, bb):
            bad = np.nonzero(ba != bb)[0]
            raise AssertionError("%s plane %d: %d of %d lanes differ, first idx %d: got %r want %r" %
                                 (what, c, bad.size, ba.size, bad[0], a[bad[0]], b[bad[0]]))


def oracle_scene_for(O, scene, mode, seed=1984):
    """Oracle scene fed with the product's raw inputs; reference topology is rebuilt by the oracle itself,
    any other tree is imported (boxes are always recomputed by the oracle)."""
    osc = O.OracleScene(scene.triangles(), scene.materials(), scene.background())
    if mode == 0:
        assert osc.build_reference(seed) == 1
    else:
        left, right, prim, _ = scene.bvh()
        assert osc.set_bvh(left, right, prim, 0) == 1
    return osc


def custom_scene(srt, tris, mats, bg_rgb=(0.5, 0.5, 0.5)):
    """Scene from raw arrays (the boundary's srt_scene_set_* path): tris = [(v0, v1, v2, mat, aa_plane)], mats = [(type, rgb, fuzz, power)]."""
    import ctypes as C
    B = srt.binding
    T = (B.TriIn * len(tris))()
    for k, (v0, v1, v2, mat, aap) in enumerate(tris):
        T[k].v0[:] = v0; T[k].v1[:] = v1; T[k].v2[:] = v2; T[k].mat_index = mat; T[k].aa_plane = aap
    M = (B.Material * len(mats))()
    for k, (mtype, rgb, fuzz, power) in enumerate(mats):
        M[k].col[:] = rgb; M[k].reflection_fuzz = fuzz; M[k].material_type = mtype; M[k].emission_power = power
        M[k].sellmeier_B[:] = (1.03961212, 0.231792344, 1.01046945); M[k].sellmeier_C[:] = (1.03961212, 0.231792344, 1.01046945)   # Q1: C := B
        B.check(B.lib().srt_material_bake(C.byref(M[k])))
    bg = np.zeros(B.N_CIE, np.float32)
    B.check(B.lib().srt_background_spectrum((C.c_float * 3)(*bg_rgb), B.fptr(bg)))
    return srt.Scene.from_arrays(T, M, bg)


def fuzz_case(srt, seed):
    """Random-scene case `seed` of the fuzz tests: a triangle soup with random materials, camera and builder (both BVH builders, lens
    on / off, thin and axis-aligned triangles, shared edges and vertices so that exact t ties occur -- Q11).  Host side only (no GPU).
    Returns scene (BVH built), camera, W, H, spp, depth, builder mode, number of triangles."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(3, 260))
    tris, mats = [], []
    n_mats = int(rng.integers(1, 12))
    for k in range(n_mats):
        mtype = int(rng.choice([0, 0, 0, 1, 1, 2, 4, 6]))
        grey = float(rng.choice([0.0, 0.3, 0.5, 0.73, 1.0]))
        mats.append((mtype, (grey, grey, grey), float(rng.uniform(0, 0.6)), float(rng.uniform(0.5, 3.0))))
    verts = rng.uniform(-5, 5, (max(4, n // 2), 3)).astype(np.float32)
    lattice = rng.random(verts.shape[0]) < 0.3
    verts[lattice] = np.round(verts[lattice])          # some vertices on lattice points: coplanar / axis-aligned coincidences
    for k in range(n):
        if rng.random() < 0.6:          # triangles that share vertices (a mesh-like soup: shared edges)
            i0, i1, i2 = rng.choice(verts.shape[0], 3, replace=False)
            v0, v1, v2 = verts[i0], verts[i1], verts[i2]
        else:
            c = rng.uniform(-5, 5, 3)
            v0, v1, v2 = (c + rng.normal(0, rng.choice([0.01, 0.5, 2.0]), 3) for _ in range(3))
        if rng.random() < 0.15:         # axis-aligned: exercises the aa_plane projection choice (tri.cu:66-77)
            ax = int(rng.integers(0, 3)); v0 = np.array(v0); v1 = np.array(v1); v2 = np.array(v2)
            v1[ax] = v0[ax]; v2[ax] = v0[ax]
        tris.append((tuple(float(x) for x in v0), tuple(float(x) for x in v1), tuple(float(x) for x in v2), int(rng.integers(0, n_mats)), int(rng.choice([0, 0, 1, 2, 3]))))
    bg = float(rng.choice([0.5, 1.0, 0.5, 0.0]))
    mode = int(rng.integers(0, 2))
    scene = custom_scene(srt, tris, mats, (bg, bg, bg)).build_bvh(mode, 1984)
    W, H, spp, depth = int(rng.integers(9, 70)), int(rng.integers(9, 50)), int(rng.integers(1, 7)), int(rng.integers(1, 17))
    cam = srt.camera_init(W, H, float(rng.uniform(20, 90)), tuple(rng.uniform(-12, 12, 3)), tuple(rng.uniform(-2, 2, 3)),
                          defocus_angle=float(rng.choice([0.0, 0.0, 1.5])), focus_dist=float(rng.uniform(5, 15)))
    return scene, cam, W, H, spp, depth, mode, n


EDGE_CASES = ["one_triangle", "two_triangles", "degenerate_and_odd_materials", "forty_materials"]


def edge_case_scene(srt, case):
    """Scenes that come in through srt_scene_set_* (not the built-ins): a BVH whose root is a leaf (bvh.cu:114-119), a two-leaf
    tree (one FRINGE record, no INNER record), zero-area / needle triangles (NaN normal: every test on them fails, as in the
    reference), material types the switch sends to its default branch (NO_MAT = 6, an unknown id), an emissive surface, and more
    than 32 materials (the reference would read its 32-entry shared copy out of bounds, Q16; the build indexes the real table).
    Returns scene (reference BVH built), camera, W, H, spp, depth."""
    XY, NONE = 1, 0
    wall = lambda z, m: [((-4, -4, z), (4, -4, z), (4, 4, z), m, NONE), ((-4, -4, z), (4, 4, z), (-4, 4, z), m, NONE)]
    if case == "one_triangle":
        tris = [((-3, -2, 0), (3, -2, 0), (0, 3, 0), 0, NONE)]
        mats = [(srt.binding.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 0.0)]
    elif case == "two_triangles":
        tris = wall(0.0, 0)
        mats = [(srt.binding.MAT_METALLIC, (1.0, 1.0, 1.0), 0.3, 0.0)]
    elif case == "degenerate_and_odd_materials":
        tris = wall(0.0, 0) + wall(-1.5, 1) + [((0, 0, 1), (0, 0, 1), (0, 0, 1), 2, NONE),          # a point
                                               ((-1, 0, 2), (0, 0, 2), (1, 0, 2), 3, NONE),          # a needle (collinear vertices)
                                               ((-2, -2, 3), (2, -2, 3), (0, 2, 3), 4, XY)]
        mats = [(srt.binding.MAT_NO_MAT, (1.0, 1.0, 1.0), 0.0, 0.0), (srt.binding.MAT_EMISSIVE, (1.0, 1.0, 1.0), 0.0, 3.0),
                (srt.binding.MAT_DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 0.0), (17, (0.5, 0.5, 0.5), 0.0, 0.0),
                (srt.binding.MAT_DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 0.0)]
    else:
        assert case == "forty_materials", case
        tris, mats = [], []
        for k in range(40):
            x = -3.9 + 0.2 * k
            tris.append(((x, -3, 0.1 * k), (x + 0.19, -3, 0.1 * k), (x + 0.1, 3, 0.1 * k), k, NONE))
            mats.append(((srt.binding.MAT_LAMBERTIAN, srt.binding.MAT_METALLIC, srt.binding.MAT_DIELECTRIC)[k % 3], (0.5, 0.5, 0.5) if k % 2 else (1.0, 1.0, 1.0), 0.1 * (k % 4), 0.0))
    scene = custom_scene(srt, tris, mats).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, spp, depth = 45, 37, 6, 6
    cam = srt.camera_init(W, H, 60.0, (0.3, 0.2, 9.0), (0.0, 0.0, 0.0))
    return scene, cam, W, H, spp, depth


def fuzz_with_lens(srt):
    """the first fuzz case with a defocus lens, at least three material types and a few bounces: scene, cam, W, H, spp, depth, mode"""
    for seed in range(200):
        scene, cam, W, H, spp, depth, mode, _ = fuzz_case(srt, seed)
        if (cam.defocus_angle > 0 and len({m.material_type for m in scene.materials()}) >= 3 and depth >= 3
                and scene.background().max() > 0):
            return scene, cam, W, H, max(spp, 3), depth, mode
    raise AssertionError("no fuzz case with a lens")


# ---- frozen outputs of the CPU oracle (tests/golden/oracle_digests.json) ---------------------------------------------------
DIGEST_PLANES = ("fb_r", "fb_g", "fb_b", "srgb_r", "srgb_g", "srgb_b", "xyz_x", "xyz_y", "xyz_z")


def digest_workloads(srt):
    """The frozen workloads: PRISM 64x64 x 16 spp depth 8, BASELINE cfg 1 (CORNELL 256x256 x 16 spp depth 8; the coloured walls use
    this build's own sigmoid fit, as every CORNELL render here does), six fuzz seeds.  name -> (scene, cam, W, H, spp, depth, mode)."""
    out = {}
    sc = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    out["prism_64x64_16spp_d8"] = (sc, sc.default_camera(64, 64), 64, 64, 16, 8, 0)
    sc = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    out["cfg1_cornell_256x256_16spp_d8"] = (sc, sc.default_camera(256, 256), 256, 256, 16, 8, 0)
    for seed in (0, 1, 2, 3, 4, 5):
        scene, cam, W, H, spp, depth, mode, _ = fuzz_case(srt, seed)
        out["fuzz_seed_%d" % seed] = (scene, cam, W, H, spp, depth, mode)
    return out


def digest_of_render(res):
    """sha256 of the bit patterns of the nine planes (quantised framebuffer, unquantised sRGB, XYZ sums: rendering/rendering.cu:205-234)
    + the ray / path counts of a render result (oracle or HIP path: same dict layout)"""
    import hashlib
    planes = list(res["fb"]) + list(res["lin"]) + list(res["xyz"])
    d = {name: hashlib.sha256(bits(p).tobytes()).hexdigest() for name, p in zip(DIGEST_PLANES, planes)}
    d["rays"] = int(res["stats"]["rays"]); d["paths"] = int(res["stats"]["paths"])
    return d


# ---- shared by the parity suite and the accumulation suites ------------------------------------------------------------------
def _xorwow_host(seeds):
    """cuRAND XORWOW (curand_init(seed, 0, 0) + curand()) on arrays of seeds: returns (state dict, next()) -- numpy restatement of srt_device.h's
    rng_seed / rng_next (the oracle restates the same published definition in C)."""
    u = np.uint32
    s0 = seeds.astype(u) ^ u(0xaad26b49); s1 = np.zeros_like(s0) ^ u(0xf7dcefdd)
    t0 = u(1099087573) * s0; t1 = u(2591861531) * s1
    st = {"d": u(6615241) + t1 + t0, "v": [u(123456789) + t0, u(362436069) ^ t0, u(521288629) + t1, u(88675123) ^ t1, u(5783321) + t0]}
    def nxt(mask):
        v = st["v"]
        t = v[0] ^ (v[0] >> u(2))
        n4 = (v[4] ^ (v[4] << u(4))) ^ (t ^ (t << u(1)))
        new = [v[1], v[2], v[3], v[4], n4]
        for k in range(5): v[k] = np.where(mask, new[k], v[k])
        st["d"] = np.where(mask, st["d"] + u(362437), st["d"])
        return v[4] + st["d"]
    return st, nxt


def _blocks_bit_exact(srt, gpu, orc, sid, mode, W, H, spp, depth, block_lo, stride, max_blocks):
    """a full-size frame of a built-in scene rendered on the GPU; its 28 x 16 blocks block_lo, block_lo + stride, .. against the oracle
    at full spp, bit for bit in the quantised and XYZ planes.  Returns the number of blocks compared (the frame stays in the context)."""
    scene = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
    cam = scene.default_camera(W, H)
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1)
    gpu.init_device_params(W, H, spp, depth, 1984)
    gpu.set_count_traversal(False)
    gpu.render_chunk(W, H)
    gpu.scatter_tiles()
    fb, xyz = gpu.read_fb(), gpu.read_fb_aux(2)
    g = gpu.geom
    n_blocks = g["bx"] * g["by"]
    osc = oracle_scene_for(orc, scene, mode)
    threads = min(os.cpu_count() or 1, 16)
    ref = osc.render(cam, W, H, spp, depth, block_lo=block_lo, block_stride=stride, threads=threads)
    checked = 0
    for b in range(block_lo, n_blocks, stride):
        sl = slice(b * 448, (b + 1) * 448)
        for c in range(3):
            assert np.array_equal(bits(xyz[c][sl]), bits(ref["xyz"][c][sl])), ("block", b, "plane", c)
            assert np.array_equal(fb[c][sl], ref["fb"][c][sl]), ("block", b, "plane", c)
        checked += 1
    assert 1 <= checked <= max_blocks
    rm = gpu.read_fb_rowmajor(W, H)
    assert all(np.isfinite(p).all() for p in rm)
    return checked
