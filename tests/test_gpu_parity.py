"""GPU parity tests proper: the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.
Bar: bit-exact fp32 (stronger than BASELINE's 1e-3 L-inf, which is asserted as well)."""
import importlib
import os
import numpy as np
import pytest

from accum_helpers import run_mock_transport_child
from helpers import _blocks_bit_exact, _xorwow_host, assert_planes_equal, bits, oracle_scene_for

pytestmark = pytest.mark.gpu


def _special_floats(rng, n):
    a = rng.standard_normal(n).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, 3.4028235e38, 1e-8, 0.5, 2.0,
                        255.99, 0.0031308, 360.0, 830.0], np.float32)
    a[: special.size] = special
    u = rng.integers(0, 2 ** 32, n // 4, dtype=np.uint64).astype(np.uint32).view(np.float32)   # raw bit patterns incl. denormals/NaNs
    a[special.size: special.size + u.size] = u
    return a


def _same(got, want):
    g, w = bits(got), bits(want)
    nan = np.isnan(got) & np.isnan(want)        # NaN payload/sign is not part of the contract
    return np.all((g == w) | nan)


def test_primitive_op_sweep(gpu, orc):
    """Device + - * / sqrt fmin fmax casts are bit-identical to the host's IEEE results (2^22 operand pairs incl.
    denormals, infinities, NaNs) and a*b+b is NOT contracted to an FMA."""
    rng = np.random.default_rng(7)
    n = 1 << 22
    a, b = _special_floats(rng, n), _special_floats(rng, n)[::-1].copy()
    with np.errstate(all="ignore"):
        host = {0: a + b, 1: a - b, 2: a * b, 3: a / b, 4: np.sqrt(a), 5: np.fmin(a, b), 6: np.fmax(a, b),
                9: np.float32(1.0) / a, 10: np.abs(a), 11: (a * b) + b, 13: ((a * a) + (b * b)) + (a * b)}
    for which, want in host.items():
        got = gpu.op_sweep(which, a, b)
        if which in (5, 6):     # fmin/fmax of (+0,-0) may return either zero
            ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)) | ((got == 0) & (want == 0))
            assert np.all(ok), which
        else:
            assert _same(got, want), "op %d differs on %d operands" % (which, int(np.sum(bits(got) != bits(want))))
    # packed fp32 (v_pk_mul_f32 / v_pk_add_f32) rounds each half like the scalar instruction
    with np.errstate(all="ignore"):
        odd = (np.arange(n) & 1).astype(bool)
        assert _same(gpu.op_sweep(14, a, b), a * b)
        assert _same(gpu.op_sweep(15, a, b), np.where(odd, b + a * np.float32(0.5), a + b))
        assert _same(gpu.op_sweep(16, a, b), np.where(odd, ((b - a) * a) - (b * a), ((a - b) * a) - (a * b)))
    # u32 -> f32 (RNG mapping) and the truncating cast used by spectrum_interp / expand_sRGB
    got = gpu.op_sweep(12, a, b)
    assert _same(got, a.view(np.uint32).astype(np.float32))
    # the fused forms of the uniform mapping (one fma with an exact product) equal the reference's mul-then-add forms
    r = np.concatenate([rng.integers(0, 1 << 32, n - 4096, dtype=np.uint64).astype(np.uint32),
                        np.arange(2048, dtype=np.uint32), np.uint32(0xffffffff) - np.arange(2048, dtype=np.uint32)])
    rf = r.astype(np.float32)
    u = rf * np.float32(2.3283064e-10) + np.float32(2.3283064e-10) / np.float32(2.0)
    assert _same(gpu.op_sweep(18, r.view(np.float32), b), u)
    assert _same(gpu.op_sweep(19, r.view(np.float32), b), u * np.float32(2.0) + np.float32(-1.0))
    # the FRINGE visit's inside test: NaN-propagating minimum (v_minimum3-style, with the sign-bit flip for counter-clockwise
    # triangles) == the three compares of is_interior_faster (primitives/tri.cu:121-128) on 2^22 operand triples
    # (a[k], b[k], a[k ^ 1]) incl. +-0, NaN, denormals, infinities -- and on a dense block of every special-value combination
    sp = np.array([0.0, -0.0, np.nan, -np.nan, 1e-45, -1e-45, 1e-38, -1e-38, np.inf, -np.inf, 1.0, -1.0, 3.4028235e38, -3.4028235e38], np.float32)
    a3, b3 = a.copy(), b.copy()
    combos = np.array([(x, y, z) for x in sp for y in sp for z in sp], np.float32)          # 2744 triples at even k: third operand = a[k + 1]
    a3[0:2 * combos.shape[0]:2] = combos[:, 0]; b3[0:2 * combos.shape[0]:2] = combos[:, 1]; a3[1:2 * combos.shape[0]:2] = combos[:, 2]
    c3 = a3.reshape(-1, 2)[:, ::-1].reshape(-1)                                          # a[k ^ 1]
    with np.errstate(all="ignore"):
        want_cw = ((a3 >= 0) & (b3 >= 0) & (c3 >= 0)).astype(np.float32)
        want_ccw = ((a3 <= 0) & (b3 <= 0) & (c3 <= 0)).astype(np.float32)
    assert np.array_equal(gpu.op_sweep(20, a3, b3), want_cw)
    assert np.array_equal(gpu.op_sweep(21, a3, b3), want_ccw)
    assert 0 < want_cw.sum() < n and 0 < want_ccw.sum() < n
    small = (rng.random(n).astype(np.float32) * 600.0 - 100.0).astype(np.float32)
    assert _same(gpu.op_sweep(7, small, b), np.trunc(small).astype(np.int32).astype(np.float32))


def test_rejection_loops_in_assembly_match_host_restatement(gpu):
    """rng_sphere_loop_asm / rng_disk_loop_asm (the v33 kernels' hand-scheduled random_in_unit_sphere / random_in_unit_disk): accepted point, |p|^2 and the
    stream position left behind, for 2^16 streams whose lanes need different numbers of tries, against XORWOW + the reference's loops in numpy
    (math/vec3.cuh:210-218,240-246; draws x, y, z in that order, D1)."""
    rng = np.random.default_rng(33)
    n = 1 << 16
    seeds = np.concatenate([np.arange(1984, 1984 + n // 2, dtype=np.uint32), rng.integers(0, 1 << 32, n // 2, dtype=np.uint64).astype(np.uint32)])
    a = seeds.view(np.float32); b = np.zeros(n, np.float32)
    f = np.float32
    def pm1(r):
        return (r.astype(f) * f(2.0 * 2.3283064e-10) + f(2.3283064e-10)) + f(-1.0)      # (exact product: one rounding at the first add, like the device's fma)
    fold = lambda st: st["d"] ^ (st["v"][0] * np.uint32(3)) ^ (st["v"][1] * np.uint32(5)) ^ (st["v"][2] * np.uint32(7)) ^ (st["v"][3] * np.uint32(11)) ^ (st["v"][4] * np.uint32(13))
    with np.errstate(over="ignore"):
        for draws, kinds in ((3, (23, 24, 25, 26, 27)), (2, (28, 29, None, None, 30))):
            st, nxt = _xorwow_host(seeds)
            todo = np.ones(n, bool)
            p = [np.zeros(n, f) for _ in range(3)]
            l2 = np.zeros(n, f)
            tries = 0
            while todo.any():
                c = [pm1(nxt(todo)) for _ in range(draws)] + [np.zeros(n, f)] * (3 - draws)
                q = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                for k in range(3): p[k] = np.where(todo, c[k], p[k])
                l2 = np.where(todo, q, l2)
                todo = todo & ~(q < f(1.0))
                tries += 1
            assert tries > 6      # (some lane needed many tries: the loops ran divergent)
            want = [p[0], p[1], p[2], l2, fold(st).view(np.float32)]
            for kind, w in zip(kinds, want):
                if kind is None: continue
                got = gpu.op_sweep(kind, a, b)
                assert np.array_equal(bits(got), bits(w)), "kind %d differs on %d streams" % (kind, int(np.sum(bits(got) != bits(w))))


def test_powf_matches_oracle_and_libm(gpu, orc):
    rng = np.random.default_rng(11)
    n = 1 << 18
    x = np.concatenate([rng.random(n).astype(np.float32), (rng.random(n) * 2).astype(np.float32),
                        np.float32(10.0) ** rng.uniform(-40, 0, n).astype(np.float32)]).astype(np.float32)
    for y in (5.0, 0.416666, 2.0):
        yy = np.full_like(x, np.float32(y))
        got = gpu.op_sweep(8, x, yy)
        want = np.array([orc.lib().orc_powf(float(v), float(np.float32(y))) for v in x[:20000]], np.float32)
        assert np.array_equal(bits(got[:20000]), bits(want)), y
        # independent check: correctly rounded pow via float64 libm agrees except at near-ties.  Squares (y = 2,
        # only used at scene-bake time) are special: x*x has 48 significant bits, so it lies within 2^-47 of a
        # rounding tie far more often than a generic real does.
        lib = np.power(x.astype(np.float64), np.float64(np.float32(y))).astype(np.float32)
        assert int(np.sum(bits(got) != bits(lib))) <= (16 if y == 2.0 else 2), y
    # the inlined Schlick power (srt_pow5f) is srt_powf(x, 5) bit for bit, special operands included
    xs = np.concatenate([x, _special_floats(rng, 4096)]).astype(np.float32)
    assert _same(gpu.op_sweep(17, xs, xs), gpu.op_sweep(8, xs, np.full_like(xs, np.float32(5.0))))


SCENES = [
    # (scene id, bvh mode, W, H, spp, depth)
    (1, 0, 64, 64, 16, 8),      # PRISM, reference topology (dispersion, NaN IOR quirk Q1/Q21)
    (1, 0, 96, 96, 32, 16),     # the SURVEY probe configuration
    (0, 0, 64, 48, 8, 8),       # CORNELL: metal, lambertian, glass pyramid
    (2, 0, 50, 70, 8, 12),      # TRIS: 9 materials, ragged image size
    (100, 1, 80, 45, 4, 16),    # random "spheres": SAH tree, defocus lens, sky background
    (101, 1, 48, 27, 2, 16),    # 100k-triangle mesh in the Cornell shell (cfg 5 scene): deep SAH tree, 8 waves / workgroup
    (1, 0, 33, 9, 3, 1),        # depth 1: every path ends at the bounce limit or on its first miss
    (0, 0, 8, 8, 1, 0),         # bounce limit 0: ray_bounce's loop never runs, RNG is still consumed per sample
    (1, 0, 1, 1, 5, 16),        # a single pixel: one lane of one wave
    (100, 1, 29, 17, 12, 16),   # one pixel past a 28x16 block in both directions; spp > 8: cost probe + ordered, split queue
    (1, 1, 57, 31, 9, 16),      # the reference scene on this build's SAH tree (the oracle imports it)
    (100, 0, 40, 24, 3, 16),    # the synthetic scene on the REFERENCE builder's tree (x/y-only median splits, Q14)
]


# Every adversarial input goes through BOTH builds of render_kernel: the instrumented one (MODE 1: C++ traversal steps, work
# counters) and the production one (MODE 0: the hand-scheduled assembly block for the INNER visits and the step choice when the
# tree is narrow and LDS resident -- which all of these small scenes are -- i.e. the kernel that ships and that bench.py times).
VARIANTS = [pytest.param(True, id="instrumented"), pytest.param(False, id="production")]


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("sid,mode,W,H,spp,depth", SCENES)
def test_image_bit_exact(srt, gpu, orc, sid, mode, W, H, spp, depth, count_traversal):
    scene = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
    cam = scene.default_camera(W, H)
    out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
    ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, spp, depth)
    assert_planes_equal(out["xyz"], ref["xyz"], "XYZ sums")
    assert_planes_equal(out["lin"], ref["lin"], "unquantised sRGB")
    assert_planes_equal(out["fb"], ref["fb"], "quantised framebuffer")
    linf = max(float(np.max(np.abs(a - b))) for a, b in zip(out["lin"], ref["lin"]))
    assert linf <= 1e-3                     # BASELINE tolerance (per-channel L-inf on sRGB in [0,1])
    st, rs = out["stats"], ref["stats"]
    assert st["rays"] == rs["rays"] and st["paths"] == rs["paths"]
    if not count_traversal:
        return                              # the production build keeps no work counters
    # work counters: identical to the reference's, except that NaN-direction queries are answered without
    # walking the tree -- the reference visits every internal node and tests every triangle for them and finds nothing
    n_nan, n_tris = st["util"][2], scene.n_tris
    assert st["node_visits"] + n_nan * (n_tris - 1) == rs["trav_iters"]
    assert st["tri_tests"] + n_nan * n_tris == rs["tri_tests"]
    assert st["box_tests"] + n_nan * (n_tris - 2) == rs["box_tests"]
    if sid in (0, 1, 2) and depth >= 8 and W * H * spp >= 2000:
        assert n_nan > 0                   # flint glass with C := B really produces NaN indices
    # row-major un-swizzle (render_manager::update_fb)
    g = out["geom"]
    for c in range(3):
        want = orc.unswizzle(ref["fb"][c], g["tx"], g["ty"], g["bx"], g["by"], W, H, 0, 0, W, H)
        assert np.array_equal(out["rowmajor"][c], want)


def test_reordered_tree_for_another_viewpoint_bit_exact(srt, gpu, orc):
    """srt_scene_order_children: the SAH tree re-ordered for a camera that is NOT the scene's default one (nearer child first at
    every node), rendered from that camera by both kernel builds == the oracle walking the same re-ordered tree; and fewer node
    visits than the default-camera order gives from there (the point of the call)."""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH)
    W, H, spp, depth = 96, 54, 6, 16
    eye = (-9.0, 2.5, -6.0)
    cam = srt.camera_init(W, H, 35.0, eye, (0.0, 0.5, 0.0))
    base = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=True)
    scene.order_children(eye)
    ref = oracle_scene_for(orc, scene, 1).render(cam, W, H, spp, depth)
    for counted in (True, False):
        out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=counted)
        assert_planes_equal(out["xyz"], ref["xyz"], "re-ordered tree XYZ, counted=%s" % counted)
        assert_planes_equal(out["fb"], ref["fb"], "re-ordered tree fb, counted=%s" % counted)
        assert out["stats"]["rays"] == ref["stats"]["rays"]
        if counted:
            assert out["stats"]["node_visits"] < base["stats"]["node_visits"]


def test_trace_rays_matches_oracle(srt, gpu, orc):
    """bvh::hit for explicit rays incl. degenerate ones (zero / NaN / axis-parallel directions, origins on surfaces)."""
    scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    gpu.upload_scene(scene)
    osc = oracle_scene_for(orc, scene, 0)
    rng = np.random.default_rng(3)
    n = 4000
    o = rng.uniform(-50, 600, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    o[:8] = [278, 278, -800]
    d[0] = [0.02, 0.15, 1]; d[1] = [0, 0, 1]; d[2] = [0, 0, 0]; d[3] = [np.nan, 0, 1]; d[4] = [1, 0, 0]; d[5] = [0, -1, 0]
    d[6] = [-0.0, 0.0, 1]; d[7] = [0, 1e-30, 1]
    o[8] = [278, 0, 278]; d[8] = [0, 1, 0]           # origin exactly on the floor plane (tmin = 0, Q9)
    o[9] = [0, 100, 100]; d[9] = [1, 0, 0]           # origin on the right wall
    got = gpu.trace_rays(np.concatenate([o, d], 1))
    for k in range(n):
        hit, out = osc.trace(o[k], d[k])
        if not hit:
            assert got[k, 1] == -1, k
        else:
            assert got[k, 1] >= 0 and bits(got[k, 0:1])[0] == bits(out[0:1])[0], k
            assert got[k, 2] == out[7] and got[k, 3] == out[8], k


def test_partition_invariance_and_chunks(srt, gpu, orc):
    """Any tile partition (world 1, 2, 5) produces the same framebuffer; tiles are rendered by separate launches and
    merged through the gathered-buffer layout exactly as the multi-GPU path does."""
    import ctypes as C
    import torch
    scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, spp, depth = 75, 41, 4, 8
    cam = scene.default_camera(W, H)
    ref = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu)
    for world, planes in ((2, 9), (5, 9), (3, 3)):      # planes = 3: the default exchange unit (quantised framebuffer only)
        parts = []
        gpu.set_gather_planes(planes)
        for rank in range(world):
            gpu.upload_scene(scene); gpu.set_camera(cam)
            gpu.init_device_params(W, H, spp, depth, 1984)
            gpu.set_partition(rank, world)
            gpu.render_chunk(W, H)
            gpu.synchronize()
            ptr, n_floats, tl, tp = gpu.tile_buffer()
            staging = torch.empty(n_floats, dtype=torch.float32, device="cuda")      # what bench.py hands to the RCCL gather
            gpu.copy_tile_buffer(staging.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            parts.append(staging.cpu().numpy().copy())
        gathered = torch.from_numpy(np.concatenate(parts)).cuda()
        gpu.scatter_tiles(gathered.data_ptr())
        gpu.synchronize()
        assert n_floats == gpu.tile_buffer()[3] * planes * 64
        assert_planes_equal(gpu.read_fb(), ref["fb"], "world %d" % world)
        if planes == 9:
            assert_planes_equal(gpu.read_fb_aux(2), ref["xyz"], "world %d xyz" % world)
    gpu.set_partition(0, 1)
    gpu.set_gather_planes(9)          # (the session's renderer keeps the parity planes on)


def test_default_context_writes_the_framebuffer_only(srt, orc):
    """A context as a caller of the boundary gets it (no srt_set_gather_planes): the render kernels write the quantised framebuffer
    planes only -- what the reference's renderer holds (rendering.cu:140-149) -- in both builds of the kernel; the framebuffer equals the
    oracle's, and asking for the parity planes is an error with a message, not stale or zero data."""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    W, H, spp, depth = 120, 70, 10, 16
    cam = scene.default_camera(W, H)
    ref = oracle_scene_for(orc, scene, 1).render(cam, W, H, spp, depth)
    r = srt.Renderer(0)
    try:
        for counted in (False, True):
            r.upload_scene(scene); r.set_camera(cam); r.set_partition(0, 1)
            r.set_count_traversal(counted)
            r.init_device_params(W, H, spp, depth, 1984)
            r.render_chunk(W, H)
            r.scatter_tiles()
            assert_planes_equal(r.read_fb(), ref["fb"], "default context, counted=%s" % counted)
            assert r.stats()["rays"] == ref["stats"]["rays"]
            with pytest.raises(srt.SrtError) as e:
                r.read_fb_aux(2)
            assert e.value.code == -5 and "not gathered" in str(e.value)
            _, n_floats, _, tp = r.tile_buffer()
            assert n_floats == tp * 3 * 64
    finally:
        r.close()


def test_ragged_chunks_multi_rank_match_oracle(srt, orc):
    """A chunked render (40x40 chunks of a 72x56 image: the edge chunks are narrower / shorter) split over 4 ranks.  Every rank
    is its own context with its own persistent RNG states (Q13), so the tile -> rank map must not depend on the size of the
    current chunk: a lane whose tile moved to another rank would continue from a stream that never advanced.  The image
    must equal the oracle's single-renderer chunk walk (render_manager.cu:3-66) bit for bit."""
    import ctypes as C
    import torch
    scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, spp, depth, cw, ch, world = 72, 56, 5, 8, 40, 40, 4
    cam = scene.default_camera(W, H)
    bx, by = cw // 28 + 1, ch // 16 + 1
    ranks = []
    for rank in range(world):
        r = srt.Renderer(0)
        r.upload_scene(scene); r.set_camera(cam)
        r.init_device_params(cw, ch, spp, depth, 1984)
        r.set_partition(rank, world)
        r.set_gather_planes(9)               # the XYZ sums are compared below
        ranks.append(r)
    osc = oracle_scene_for(orc, scene, 0)
    n = 28 * 16 * bx * by
    states = np.zeros(6 * n, np.uint32)
    for idx in range(n):
        s = orc.Rng()
        orc.lib().orc_rng_init(1984 + idx, C.byref(s))
        states[6 * idx: 6 * idx + 6] = [s.d] + list(s.v)
    image = tuple(np.full(W * H, -1.0, np.float32) for _ in range(3))      # row-major planes filled chunk by chunk (update_fb)
    want_image = [np.full(W * H, -1.0, np.float32) for _ in range(3)]
    for oy in range(0, H, ch):
        for ox in range(0, W, cw):
            w, h = min(cw, W - ox), min(ch, H - oy)
            parts = []
            for r in ranks:
                r.render_chunk(w, h, ox, oy)
                r.synchronize()
                _, n_floats, _, _ = r.tile_buffer()
                staging = torch.empty(n_floats, dtype=torch.float32, device="cuda")
                r.copy_tile_buffer(staging.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                parts.append(staging)
            gathered = torch.cat(parts)
            ranks[0].scatter_tiles(gathered.data_ptr())
            ranks[0].synchronize()
            want = osc.render(cam, w, h, spp, depth, bx=bx, by=by, offx=ox, offy=oy, states=states)
            got_fb, got_xyz = ranks[0].read_fb(), ranks[0].read_fb_aux(2)
            # lanes outside this chunk keep what an earlier chunk left in the framebuffer: compare the chunk's own lanes
            lane = np.arange(n)
            blk, t = lane // 448, lane % 448
            x, y = 28 * (blk % bx) + t % 28, 16 * (blk // bx) + t // 28
            inside = (x < w) & (y < h)
            for c in range(3):
                assert np.array_equal(bits(got_xyz[c][inside]), bits(want["xyz"][c][inside])), ("chunk", ox, oy, "xyz", c)
                assert np.array_equal(got_fb[c][inside], want["fb"][c][inside]), ("chunk", ox, oy, "fb", c)
            # srt_read_fb_rowmajor writes exactly the chunk's rectangle of the caller's planes (render_manager::update_fb)
            ranks[0].read_fb_rowmajor(W, H, into=image)
            for c in range(3):
                img = orc.unswizzle(want["fb"][c], 28, 16, bx, by, w, h, ox, oy, W, H)
                mask = np.zeros((H, W), bool)
                mask[oy:oy + h, ox:ox + w] = True
                want_image[c][mask.ravel()] = img[mask.ravel()]
                assert np.array_equal(image[c], want_image[c]), ("row-major after chunk", ox, oy, c)
    assert all(float(p.min()) >= 0.0 for p in image)            # every pixel of the image was written by some chunk
    for r in ranks:
        r.close()


def test_queue_scheduling_does_not_change_results(srt, gpu, orc, monkeypatch):
    """The pixel queue (cost order, expensive tiles split over several waves with parked lanes) is pure scheduling: the
    framebuffer is bit-identical with splitting off, with the default policy and with the most aggressive policy, and for
    different step-choice weights."""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
    W, H, spp, depth = 120, 72, 12, 16          # spp > 8: the cost probe and the ordered queue are active
    cam = scene.default_camera(W, H)
    ref = None
    for env in ({"SRT_SPLIT_LOAD": "0"}, {}, {"SRT_SPLIT_LOAD": "1"},
                {"SRT_SPLIT_LOAD": "1", "SRT_SCORE_SHADE": "9", "SRT_SCORE_FRINGE": "900"},
                {"SRT_SCORE_SHADE": "2000", "SRT_SCORE_FRINGE": "1"}, {"SRT_SCORE_SHADE": "1", "SRT_SCORE_FRINGE": "4000"},
                {"SRT_SCORE_FRINGE": "0"},      # clamped to 1: a zero weight would starve lanes at fringe records
                {"SRT_PROBE_SPP": "0"}):
        for k in ("SRT_SPLIT_LOAD", "SRT_PROBE_SPP", "SRT_SCORE_SHADE", "SRT_SCORE_FRINGE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = srt.Renderer(0)                       # the knobs are read when the context is created
        img = srt.render_image(scene, cam, W, H, spp, depth, renderer=r)
        if ref is None:
            ref = img
        else:
            assert_planes_equal(img["fb"], ref["fb"], "env %r" % (env,))
            assert_planes_equal(img["xyz"], ref["xyz"], "env %r xyz" % (env,))
        del r


def test_second_render_continues_rng_streams(srt, gpu, orc):
    """RNG states persist between launches (rendering.cu:209,232; Q13): two renders of spp each differ from each other and
    the second equals the oracle continued from the first one's states."""
    import ctypes as C
    scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, spp, depth = 40, 24, 3, 8
    cam = scene.default_camera(W, H)
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1)
    gpu.init_device_params(W, H, spp, depth, 1984)
    gpu.render_chunk(W, H); gpu.scatter_tiles(); first = gpu.read_fb_aux(2)
    gpu.render_chunk(W, H); gpu.scatter_tiles(); second = gpu.read_fb_aux(2)
    osc = oracle_scene_for(orc, scene, 0)
    n = gpu.geom["n_lanes"]
    states = np.zeros(6 * n, np.uint32)
    for idx in range(n):
        s = orc.Rng()
        orc.lib().orc_rng_init(1984 + idx, C.byref(s))
        states[6 * idx: 6 * idx + 6] = [s.d] + list(s.v)
    a = osc.render(cam, W, H, spp, depth, states=states)
    b = osc.render(cam, W, H, spp, depth, states=states)
    assert_planes_equal(first, a["xyz"], "first launch")
    assert_planes_equal(second, b["xyz"], "second launch")
    assert not np.array_equal(first[1], second[1])


@pytest.mark.parametrize("tuned", [True, False], ids=["throughput-tuned tree (what bench.py's headline renders)", "the SAH builder's tree"])
def test_full_size_blocks_bit_exact(srt, gpu, orc, tuned):
    """BASELINE's headline configuration at FULL size (random-spheres scene, 1920x1080, 1024 spp, depth 16) rendered on the
    GPU; a spread of the reference's 28x16-pixel blocks (top rows = sky, horizon, spheres, foreground) is re-rendered by
    the oracle at full spp and compared bit for bit.  Same seeds (1984 + block-linear index), same tree -- the tree bench.py's
    headline frame is measured on (srt.tune_tree_for_throughput: reinsertion + profiled child order) and the builder's."""
    import os
    W, H, spp, depth = 1920, 1080, 1024, 16
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH)
    if tuned:
        gpu.upload_scene(scene)
        assert srt.pixels_per_lane(gpu, W, H, 1) >= 6.0
        assert "nodes swapped" in srt.tune_tree_for_throughput(gpu, scene, W, H, depth)
    cam = scene.default_camera(W, H)
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1)
    gpu.init_device_params(W, H, spp, depth, 1984)
    gpu.set_count_traversal(False)
    gpu.render_chunk(W, H)
    gpu.scatter_tiles()
    fb, xyz = gpu.read_fb(), gpu.read_fb_aux(2)
    g = gpu.geom
    n_blocks = g["bx"] * g["by"]
    osc = oracle_scene_for(orc, scene, 1)
    threads = min(os.cpu_count() or 1, 16)
    stride = 587                                   # 69 x 68 = 4692 blocks -> 8 blocks spread over rows and columns
    ref = osc.render(cam, W, H, spp, depth, block_lo=301, block_stride=stride, threads=threads)
    checked = 0
    for b in range(301, n_blocks, stride):
        sl = slice(b * 448, (b + 1) * 448)
        for c in range(3):
            assert np.array_equal(bits(xyz[c][sl]), bits(ref["xyz"][c][sl])), ("block", b, "plane", c)
            assert np.array_equal(fb[c][sl], ref["fb"][c][sl]), ("block", b, "plane", c)
        checked += 1
    assert checked == 8
    # lanes the oracle did not render stay zero there; the GPU image is complete: no pixel of the image is left unwritten
    rm = gpu.read_fb_rowmajor(W, H)
    assert min(float(p.max()) for p in rm) > 0 and all(np.isfinite(p).all() for p in rm)


@pytest.mark.skipif(os.environ.get("SRT_LONG") != "1", reason="several minutes of oracle time on all host cores: SRT_LONG=1 to run")
def test_full_frame_full_spp_bit_exact(srt, gpu, orc):
    """The WHOLE headline frame (random-spheres scene, 1920x1080, 1024 spp, depth 16: every one of the 4 692 blocks, 5.2 G
    rays) against the oracle, bit for bit.  Opt-in (SRT_LONG=1): ~7 minutes of oracle time on 256 host threads.  Result of
    the last run: profiles/r02/full_frame_parity.txt."""
    import sys, time
    cfg = os.environ.get("SRT_LONG_CFG", "3")          # 3: the headline frame; 2: cfg 2's frame; 4: cfg 4's frame (PRISM); 5: cfg 5's scene at 3840x2160, 64 spp
    sid, W, H, spp = {"2": (srt.SCENE_RANDOM_SPHERES, 1280, 720, 256), "3": (srt.SCENE_RANDOM_SPHERES, 1920, 1080, 1024),
                      "4": (srt.SCENE_PRISM, 1920, 1080, 2048), "5": (srt.SCENE_MESH100K, 3840, 2160, 64)}[cfg]
    spp, depth = int(os.environ.get("SRT_LONG_SPP", str(spp))), 16
    bvh_mode = srt.BVH_REFERENCE if cfg == "4" else srt.BVH_SAH      # (the reference's scene on the reference builder's tree)
    scene = srt.Scene.builtin(sid, 0).build_bvh(bvh_mode, 1984)
    if bvh_mode == srt.BVH_SAH and os.environ.get("SRT_LONG_TUNED", "1") == "1":      # the tree bench.py measures this frame on
        gpu.upload_scene(scene)
        if srt.pixels_per_lane(gpu, W, H, 1) >= 6.0:
            print("tree: " + srt.tune_tree_for_throughput(gpu, scene, W, H, depth), file=sys.stderr, flush=True)
    cam = scene.default_camera(W, H)
    gpu.upload_scene(scene); gpu.set_camera(cam); gpu.set_partition(0, 1)
    gpu.init_device_params(W, H, spp, depth, 1984)
    gpu.set_count_traversal(False)
    gpu.render_chunk(W, H)
    gpu.scatter_tiles()
    fb, xyz = gpu.read_fb(), gpu.read_fb_aux(2)
    n_blocks = gpu.geom["bx"] * gpu.geom["by"]
    osc = oracle_scene_for(orc, scene, 0 if cfg == "4" else 1)
    threads = os.cpu_count() or 1
    slices, differing, checked, t0 = 16, 0, 0, time.time()
    threads = int(os.environ.get("SRT_LONG_THREADS", str(threads)))
    for k in range(slices):                           # the oracle in slices, so that a long run keeps printing
        ref = osc.render(cam, W, H, spp, depth, block_lo=k, block_stride=slices, threads=threads)
        for b in range(k, n_blocks, slices):
            sl = slice(b * 448, (b + 1) * 448)
            for c in range(3):
                differing += int(np.sum(bits(xyz[c][sl]) != bits(ref["xyz"][c][sl]))) + int(np.sum(fb[c][sl] != ref["fb"][c][sl]))
            checked += 1
        print("slice %d/%d: %d blocks checked, %d differing values, %.0f s" % (k + 1, slices, checked, differing, time.time() - t0), file=sys.stderr, flush=True)
    assert checked == n_blocks and differing == 0


def test_full_size_prism_blocks_bit_exact(srt, gpu, orc):
    """BASELINE cfg 4 at FULL size: the reference's PRISM scene (Sellmeier flint with quirk Q1, hero wavelengths, reference
    BVH builder), 1920x1080, 2048 spp, depth 16; four of the 28x16 blocks through the middle of the image against the
    oracle at full spp, bit for bit."""
    assert _blocks_bit_exact(srt, gpu, orc, srt.SCENE_PRISM, srt.BVH_REFERENCE, 1920, 1080, 2048, 16, 1200, 700, 6) >= 4


def test_full_resolution_mesh100k_blocks_bit_exact(srt, gpu, orc):
    """BASELINE cfg 5's scene and resolution (100k-triangle mesh in the Cornell shell, 3840x2160, depth 16; inner tree larger
    than LDS, 32-bit record references) at 64 spp instead of 4096 -- the full sample count is tens of GPU-seconds and minutes of
    oracle time per block; the code path does not depend on spp beyond the loop count (cfg 3's test runs 1024)."""
    assert _blocks_bit_exact(srt, gpu, orc, srt.SCENE_MESH100K, srt.BVH_SAH, 3840, 2160, 64, 16, 2000, 4100, 6) >= 4


def test_cfg5_full_workload_blocks_bit_exact(srt, gpu, orc):
    """BASELINE cfg 5 AS SPECIFIED, on one GPU: the 100k-triangle mesh, 3840x2160, **4096 spp**, depth 16 (34 G paths, ~100 G
    rays: ten-odd seconds of kernel time); four of the reference's 28x16 blocks spread over the frame re-rendered by the oracle at
    the full 4096 spp (about three minutes on 16 host threads -- its NaN-direction rays walk all 200 k nodes) and compared bit for bit.
    The 8-GPU partition of the same frame is covered by the partition / comm tests: pixels are independent."""
    assert _blocks_bit_exact(srt, gpu, orc, srt.SCENE_MESH100K, srt.BVH_SAH, 3840, 2160, 4096, 16, 2000, 4700, 5) >= 4
    st = gpu.stats()
    assert st["paths"] == 3840 * 2160 * 4096 and st["rays"] > 2 * st["paths"]


def test_cfg1_cornell_exact_size_full_image(srt, gpu, orc):
    """BASELINE cfg 1 at its exact size: the reference's CORNELL scene (own coloured-wall spectra, see DESIGN D-colours),
    256x256, 16 spp, depth 8, reference BVH builder; the WHOLE image against the oracle, bit for bit."""
    import os
    scene = srt.Scene.builtin(srt.SCENE_CORNELL, 0).build_bvh(srt.BVH_REFERENCE, 1984)
    W = H = 256
    cam = scene.default_camera(W, H)
    out = srt.render_image(scene, cam, W, H, 16, 8, renderer=gpu)
    ref = oracle_scene_for(orc, scene, 0).render(cam, W, H, 16, 8, threads=min(os.cpu_count() or 1, 16))
    assert_planes_equal(out["xyz"], ref["xyz"], "XYZ sums")
    assert_planes_equal(out["lin"], ref["lin"], "unquantised sRGB")
    assert_planes_equal(out["fb"], ref["fb"], "quantised framebuffer")
    assert out["stats"]["rays"] == ref["stats"]["rays"] and out["stats"]["paths"] == W * H * 16


def test_cfg2_exact_size_blocks_bit_exact(srt, gpu, orc):
    """BASELINE cfg 2 at its exact size: random-spheres scene, 1280x720, 256 spp, depth 16 (SAH tree); a handful of the
    reference's 28x16 blocks spread over the image against the oracle at full spp, bit for bit."""
    assert _blocks_bit_exact(srt, gpu, orc, srt.SCENE_RANDOM_SPHERES, srt.BVH_SAH, 1280, 720, 256, 16, 97, 263, 9) >= 6


def test_invalid_calls_fail_without_side_effects(srt, gpu):
    """Error behaviour of the boundary: bad arguments come back as negative codes with a message, nothing exits or faults
    (the reference calls exit(99) from checkCudaErrors, utils/cuda_utility.cu:8-18)."""
    import ctypes as C
    B = importlib.import_module("cuda-spectral-ray-tracer_amd.binding")
    lib = B.lib()
    ctx = gpu._h
    assert lib.srt_set_partition(ctx, 3, 2) < 0                         # rank >= world
    assert lib.srt_init_device_params(ctx, 0, 16, 1, 1, 8, 8, 1, 1, 1984) < 0     # zero dimension
    assert lib.srt_init_device_params(ctx, 65535, 65535, 65535, 65535, 8, 8, 1, 1, 1984) < 0   # grid too large
    assert lib.srt_trace_rays(ctx, None, 4, None) < 0
    assert lib.srt_read_fb_rowmajor(ctx, None, None, None, 8, 8) < 0
    assert lib.srt_upload_scene(ctx, None) < 0
    assert len(lib.srt_last_error(ctx)) > 0
    fresh = srt.Renderer(0)
    assert lib.srt_render_chunk(fresh._h, 8, 8, 0, 0, None) < 0         # "Device parameters were not initialized, render aborted"
    assert b"must be set first" in lib.srt_last_error(fresh._h)
    fresh.close()
    # the context is still usable afterwards
    scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    img = srt.render_image(scene, scene.default_camera(16, 16), 16, 16, 2, 4, renderer=gpu)
    assert all(np.isfinite(p).all() for p in img["fb"])


def _comm_image(srt, comm, scene, cam, W, H, spp, depth, planes=9):
    comm.set_gather_planes(planes)           # 9: the parity planes travel too (XYZ sums are compared); default of the library: 3
    comm.upload_scene(scene); comm.set_camera(cam)
    comm.init_device_params(W, H, spp, depth, 1984)
    comm.render_frame(W, H)
    comm.synchronize()
    root = comm.root
    return root.read_fb(), (root.read_fb_aux(2) if planes == 9 else None), comm.stats()


def test_comm_world1_matches_single_context(srt, gpu, orc):
    """The communicator path (srt_comm_*: RCCL loaded with dlopen, one stream per rank, gather + scatter) with ONE rank,
    formed both ways (ncclCommInitAll and ncclCommInitRank with a unique id), equals the plain single-context render."""
    scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, spp, depth = 61, 35, 10, 8
    cam = scene.default_camera(W, H)
    ref = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu)
    comm = srt.Comm.init_all([0])
    assert comm.world == 1 and len(comm.renderers) == 1
    fb, xyz, st = _comm_image(srt, comm, scene, cam, W, H, spp, depth)
    assert_planes_equal(fb, ref["fb"], "init_all fb"); assert_planes_equal(xyz, ref["xyz"], "init_all xyz")
    assert st["rays"] == ref["stats"]["rays"] and st["paths"] == ref["stats"]["paths"]
    comm.close()
    r = srt.Renderer(0)
    comm = srt.Comm.init_rank(r, srt.Comm.unique_id(), 0, 1)
    fb, xyz, st = _comm_image(srt, comm, scene, cam, W, H, spp, depth)
    assert_planes_equal(fb, ref["fb"], "init_rank fb"); assert_planes_equal(xyz, ref["xyz"], "init_rank xyz")
    comm.close(); r.close()


def test_comm_two_gpus_bit_identical(srt, gpu, orc):
    """Two ranks through the HIP path and the RCCL gather (single process, ncclCommInitAll): the framebuffer equals the
    one-GPU image bit for bit.  Needs two visible devices; the GPU box of the round-end suite has one."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (%d visible)" % torch.cuda.device_count())
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
    W, H, spp, depth = 160, 96, 12, 16
    cam = scene.default_camera(W, H)
    ref = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu)
    comm = srt.Comm.init_all([0, 1])
    fb, xyz, st = _comm_image(srt, comm, scene, cam, W, H, spp, depth)
    assert_planes_equal(fb, ref["fb"], "2 GPUs fb"); assert_planes_equal(xyz, ref["xyz"], "2 GPUs xyz")
    assert st["rays"] == ref["stats"]["rays"]
    fb3, _, _ = _comm_image(srt, comm, scene, cam, W, H, spp, depth, planes=3)      # the default exchange unit
    assert_planes_equal(fb3, ref["fb"], "2 GPUs fb, 3-plane gather")
    assert comm.last_gather_ms() >= 0.0
    comm.close()


def test_comm_two_and_three_ranks_one_gpu_mock_transport():
    """The W > 1 branch of srt_render_frame_multi -- gathered-buffer allocation, the grouped gather calls, the scatter from the
    rank-major buffer (3-plane exchange unit and 9-plane parity unit), exchange timing, per-comm statistics -- on ONE GPU: two / three
    ranks on device 0 (test hook SRT_COMM_TEST_SAME_DEVICE) over a test transport that implements the eight RCCL entry points with
    HIP copies (tests/cpp/mock_rccl.cpp, loaded through SRT_RCCL_LIB; the hook is honoured only for a transport that exports the
    mock's marker symbol).  Everything but RCCL itself.  The library caches its RCCL
    handle per process, so this runs in a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mock = os.path.join(root, "tests", "cpp", "_build", "libmock_rccl.so")
    if not os.path.exists(mock):
        pytest.skip("tests/cpp/_build/libmock_rccl.so not built (__graft_entry__.build())")
    run_mock_transport_child("""
import numpy as np
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES).build_bvh(srt.BVH_SAH, 1984)
W, H, spp, depth = 150, 90, 12, 16
cam = scene.default_camera(W, H)
ref = srt.render_image(scene, cam, W, H, spp, depth)
for world in (2, 3):
    comm = srt.Comm.init_all([0] * world)
    assert comm.world == world and len(comm.renderers) == world
    for planes in (3, 9):
        comm.set_gather_planes(planes)
        comm.upload_scene(scene); comm.set_camera(cam)
        comm.init_device_params(W, H, spp, depth, 1984)
        comm.render_frame(W, H); comm.synchronize()
        root = comm.root
        assert_planes_equal(root.read_fb(), ref['fb'], 'world %d planes %d fb' % (world, planes))
        if planes == 9:
            assert_planes_equal(root.read_fb_aux(2), ref['xyz'], 'world %d xyz' % world)
            assert_planes_equal(root.read_fb_aux(1), ref['lin'], 'world %d lin' % world)
        else:
            # the parity planes did not travel: asking for them is an error, not stale data (ADVICE r3)
            try:
                root.read_fb_aux(2)
                raise AssertionError('read_fb_aux after a 3-plane gather must fail')
            except srt.SrtError as e:
                assert e.code == -5 and 'not gathered' in str(e), e
        st = comm.stats()
        assert st['rays'] == ref['stats']['rays'] and st['paths'] == ref['stats']['paths'], (st, ref['stats'])
        assert comm.last_gather_ms() > 0.0
    comm.close()
print('mock transport ok')
""", "mock transport ok", timeout=300)


def test_comm_process_per_gpu_ranks_agree_or_fail_together_mock_transport():
    """the plane-count agreement of a process-per-GPU communicator (srt_comm_init_rank).  Two ranks of world 2,
    each driven by its own THREAD of one process on device 0 over the test transport (which now has a rendezvous all-gather / gather
    for such communicators): (1) both ranks at the default 3 planes and both at 9 -> the frame equals the single-context image;
    (2) rank 1 switches ITS CONTEXT to 9 planes behind the communicator's back (srt_set_gather_planes on the wrapped context --
    exactly what render_image() does) after a good frame, rank 0 does not -> BOTH ranks get SRT_ERR_INVALID with the same message
    from the same collective, nobody enters ncclGather alone, nothing hangs; (3) they agree again -> the next frame is good."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mock = os.path.join(root, "tests", "cpp", "_build", "libmock_rccl.so")
    if not os.path.exists(mock):
        pytest.skip("tests/cpp/_build/libmock_rccl.so not built (__graft_entry__.build())")
    code = """
import importlib, sys, threading
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
srt = importlib.import_module('cuda-spectral-ray-tracer_amd')
from helpers import assert_planes_equal
scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
W, H, spp, depth = 96, 64, 6, 8
cam = scene.default_camera(W, H)
ref = srt.render_image(scene, cam, W, H, spp, depth)
ident = srt.Comm.unique_id()
world = 2
rs = [srt.Renderer(0) for _ in range(world)]
comms = [None] * world
def make(rank):
    comms[rank] = srt.Comm.init_rank(rs[rank], ident, rank, world)
ts = [threading.Thread(target=make, args=(k,)) for k in range(world)]
[t.start() for t in ts]; [t.join(60) for t in ts]
assert all(c is not None and c.world == 2 for c in comms)
def frame(rank, result):
    try:
        c = comms[rank]
        c.upload_scene(scene); c.set_camera(cam)
        c.init_device_params(W, H, spp, depth, 1984)
        c.render_frame(W, H); c.synchronize()
        result[rank] = 'ok'
    except srt.SrtError as e:
        result[rank] = e
def run():
    result = [None] * world
    ts = [threading.Thread(target=frame, args=(k, result)) for k in range(world)]
    [t.start() for t in ts]
    [t.join(120) for t in ts]
    assert not any(t.is_alive() for t in ts), 'a rank hangs in the exchange'
    return result
# (1) agreement at 3 and at 9 planes
assert run() == ['ok', 'ok']
assert_planes_equal(rs[0].read_fb(), ref['fb'], '2 ranks, 3 planes')
for c in comms: c.set_gather_planes(9)
assert run() == ['ok', 'ok']
assert_planes_equal(rs[0].read_fb(), ref['fb'], '2 ranks, 9 planes'); assert_planes_equal(rs[0].read_fb_aux(2), ref['xyz'], '2 ranks xyz')
# (2) one rank changes the count on the wrapped context, not through the communicator
rs[1].set_gather_planes(3)
res = run()
assert all(isinstance(r, srt.SrtError) and r.code == -1 and 'disagree on the exchange unit' in str(r) for r in res), res
assert 'rank 0 gathers 9 planes, rank 1 3' in str(res[0]) and 'rank 0 gathers 9 planes, rank 1 3' in str(res[1]), res
# (3) agreement restored (through the context on the other rank, too)
rs[0].set_gather_planes(3)
assert run() == ['ok', 'ok']
assert_planes_equal(rs[0].read_fb(), ref['fb'], '2 ranks, 3 planes again')
for c in comms: c.close()
for r in rs: r.close()
print('agreement ok')
""" % (root, os.path.join(root, "tests"))
    env = dict(os.environ, SRT_RCCL_LIB=mock, SRT_TEST_KNOBS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "agreement ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def test_stray_knob_variables_do_not_change_the_plan():
    """SRT_WIDE_REFS / SRT_LDS_CACHE_MAX / SRT_DEBUG_LANE_LIMIT in a user's environment do nothing by themselves (the
    launch plan of a small scene stays NARROW + ALL_CACHED and the image is complete); with SRT_TEST_KNOBS=1 they are read once at
    srt_create, and srt_get_test_knobs / launch_plan() report them."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import importlib, json, sys
sys.path.insert(0, %r)
srt = importlib.import_module('cuda-spectral-ray-tracer_amd')
scene = srt.Scene.builtin(srt.SCENE_PRISM).build_bvh(srt.BVH_REFERENCE, 1984)
r = srt.Renderer(0)
out = srt.render_image(scene, scene.default_camera(40, 24), 40, 24, 2, 4, renderer=r)
plan = r.launch_plan()
print(json.dumps(dict(plan=plan, rays=out['stats']['rays'])))
""" % root
    base = {k: v for k, v in os.environ.items() if not k.startswith("SRT_")}

    def run(env):
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return [__import__("json").loads(l) for l in out.stdout.splitlines() if l.startswith("{")][0]
    plain = run(base)
    stray = run(dict(base, SRT_WIDE_REFS="1", SRT_LDS_CACHE_MAX="0", SRT_DEBUG_LANE_LIMIT="3"))
    assert stray == plain and plain["plan"]["narrow_refs"] and plain["plan"]["all_cached"]
    assert plain["plan"]["test_knobs"] == dict(wide_refs=False, lds_cache_max=-1, lane_limit=0, from_env=False)
    fenced = run(dict(base, SRT_TEST_KNOBS="1", SRT_WIDE_REFS="1", SRT_LDS_CACHE_MAX="0", SRT_DEBUG_LANE_LIMIT="3"))
    assert fenced["plan"]["test_knobs"] == dict(wide_refs=True, lds_cache_max=0, lane_limit=3, from_env=True)
    assert not fenced["plan"]["narrow_refs"] and not fenced["plan"]["all_cached"] and fenced["plan"]["n_cached"] == 0
    assert fenced["rays"] < plain["rays"]      # only 3 pixels of every tile were rendered


def test_bench_single_process_two_ranks_mock_transport():
    """`python bench.py --gpus 2` WITHOUT a launcher -- the shape of the driver's N = 1 command: one process drives the ranks through
    srt_comm_init_all / srt_render_frame_multi -- rehearsed at W = 2 on ONE GPU over the test transport: it must print a line
    (round 3 exited with "must be launched with torch.distributed.run"), the line must say which launch mode ran, carry per_rank
    rows, a passed gather_check, the cfg 5 sub-record, and the same framebuffer checksums as the one-GPU run of the same workload."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mock = os.path.join(root, "tests", "cpp", "_build", "libmock_rccl.so")
    if not os.path.exists(mock):
        pytest.skip("tests/cpp/_build/libmock_rccl.so not built (__graft_entry__.build())")
    common = ["--full", "--width", "200", "--height", "120", "--spp", "24", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-calibration",
              "--no-other-configs", "--cfg5-spp", "12", "--cfg5-size", "160x90"]

    def run(gpus, env):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus)] + common, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-1500:]
        return json.loads(lines[0])
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    one = run(1, env)
    two = run(2, dict(env, SRT_RCCL_LIB=mock, SRT_COMM_TEST_SAME_DEVICE="1", SRT_TEST_KNOBS="1"))
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert "one process drives all GPUs" in two["config"]["launch_mode"] and "srt_comm_init_all" in two["config"]["launch_mode"]
    assert "ncclGather inside libsrt_hip.so" in two["config"]["gather"], two["config"]["gather"]
    assert two["gather_check"].startswith("verified"), two["gather_check"]
    assert len(two["per_rank"]["kernel_ms"]) == 2 and all(x > 0 for x in two["per_rank"]["kernel_ms"])
    assert sum(two["per_rank"]["rays_per_frame"]) * two["steps"] == round(two["value"] * 1e6 * two["ms_per_step"] * 1e-3 * two["steps"])
    assert two["fb_checksum"] == one["fb_checksum"] and two["fb_checksum"] > 0
    assert sum(two["per_rank"]["rays_per_frame"]) == round(one["value"] * 1e6 * one["ms_per_step"] * 1e-3)          # the same rays, split
    for line in (one, two):
        assert line["cfg5"]["value"] > 0 and "100k-triangle mesh" in line["cfg5"]["workload"] and "160x90, 12 spp" in line["cfg5"]["workload"]
    assert two["cfg5"]["fb_checksum"] == one["cfg5"]["fb_checksum"] and two["cfg5"]["rays"] == one["cfg5"]["rays"]
    assert len(two["cfg5"]["per_rank_kernel_ms"]) == 2
    assert "nan_direction_rays" in two["config"]


from helpers import EDGE_CASES, custom_scene as _custom_scene, edge_case_scene, fuzz_case      # noqa: E402  (shared with tests/test_oracle_digests.py)


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("case", EDGE_CASES)
def test_custom_scenes_edge_cases(srt, gpu, orc, case, count_traversal):
    """the adversarial scenes of helpers.edge_case_scene, both kernel builds: GPU == oracle bit for bit"""
    scene, cam, W, H, spp, depth = edge_case_scene(srt, case)
    out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
    osc = oracle_scene_for(orc, scene, 0)
    ref = osc.render(cam, W, H, spp, depth)
    assert_planes_equal(out["xyz"], ref["xyz"], case + " XYZ")
    assert_planes_equal(out["fb"], ref["fb"], case + " fb")
    assert out["stats"]["rays"] == ref["stats"]["rays"]
    if case != "degenerate_and_odd_materials":
        assert max(float(p.max()) for p in out["xyz"]) > 0       # the camera sees something


@pytest.mark.parametrize("optimised", [False, True], ids=["top-down tree", "after srt_scene_optimise_bvh"])
@pytest.mark.parametrize("count_traversal", VARIANTS)
def test_profiled_child_order_bit_exact(srt, gpu, orc, count_traversal, optimised):
    """srt_order_children_by_profile: the children of the SAH tree re-ordered from one instrumented probe frame (which child held the
    closest hit while the other child's box lay beyond it).  Same nodes, same boxes, same depth, fewer node records + triangle tests
    on the probe frame -- and, the tree being an input of the traversal, GPU == CPU restatement on the re-ordered tree bit for bit
    (the restatement walks the tree it is given), both kernel builds."""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    if optimised:
        scene.optimise_bvh(3)      # (the two steps of srt.tune_tree_for_throughput, one after the other)
    l0, r0, p0, b0 = [np.array(a) for a in scene.bvh()]
    depth0 = scene.bvh_depth
    W, H, spp, depth = 120, 68, 6, 16
    cam = scene.default_camera(W, H)
    gpu.set_camera(cam)
    before = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=True)["stats"]
    n = gpu.order_children_by_profile(scene, W, H, spp, depth, min_samples=4)
    assert n > 0
    l1, r1, p1, b1 = [np.array(a) for a in scene.bvh()]
    assert scene.bvh_depth == depth0 and len(p1) == len(p0) and sorted(p1[p1 >= 0].tolist()) == sorted(p0[p0 >= 0].tolist())
    assert np.array_equal(np.sort(b0.reshape(-1, 6), axis=0), np.sort(b1.reshape(-1, 6), axis=0)) and not np.array_equal(b0, b1)
    out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
    ref = oracle_scene_for(orc, scene, 1).render(cam, W, H, spp, depth)
    _assert_render_matches(out, ref, "profiled child order", count_traversal, scene.n_tris)
    if count_traversal:
        st = out["stats"]
        assert st["node_visits"] + 2 * st["tri_tests"] < before["node_visits"] + 2 * before["tri_tests"]
    # a second call on the same frame finds nothing left to swap (the statistic does not depend on the order)
    assert gpu.order_children_by_profile(scene, W, H, spp, depth, min_samples=4) == 0


def test_profiled_child_order_fails_loudly_without_samples(srt, gpu):
    """a collecting probe launch that recorded nothing -- here a camera that looks away from the scene, so no query finds a triangle -- must
    not read as "the builder's order was already the cheapest" (0 swaps): srt_order_children_by_profile returns SRT_ERR_INVALID with a message.  (The
    profile header now sits at a fixed place in front of the per-wave debug words, so a launch cannot miss it either.)"""
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    gpu.upload_scene(scene)
    away = srt.camera_init(64, 48, 20.0, (13.0, 200.0, 3.0), (13.0, 400.0, 3.0), vup=(0, 0, 1))      # above the scene, looking up
    gpu.set_camera(away)
    with pytest.raises(srt.SrtError) as e:
        gpu.order_children_by_profile(scene, 64, 48, 2, 4, 1)
    assert e.value.code == -1 and "no samples" in str(e.value)
    gpu.upload_scene(scene)


def test_profiled_child_order_never_makes_the_probe_frame_worse(srt, gpu, orc):
    """The call checks its own result on the probe frame and undoes the swaps when the work counters did not fall: whatever it
    returns, the frame's node records + 2 x triangle tests are not above the builder's order's; 0 swaps = the tree is untouched."""
    for sid, mode in ((srt.SCENE_PRISM, srt.BVH_REFERENCE), (srt.SCENE_CORNELL, srt.BVH_REFERENCE), (srt.SCENE_TRIS, srt.BVH_SAH)):
        scene = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
        tree0 = [np.array(a).copy() for a in scene.bvh()]
        W, H, spp, depth = 64, 48, 4, 8
        cam = scene.default_camera(W, H)
        before = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=True)["stats"]
        gpu.set_camera(cam)
        n = gpu.order_children_by_profile(scene, W, H, spp, depth, min_samples=2)
        after = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=True)
        cost = lambda st: st["node_visits"] + 2 * st["tri_tests"]
        assert cost(after["stats"]) <= cost(before) and (n > 0) == (cost(after["stats"]) < cost(before))
        if n == 0:
            assert all(np.array_equal(a, np.array(b)) for a, b in zip(tree0, scene.bvh()))
        ref = oracle_scene_for(orc, scene, 1).render(cam, W, H, spp, depth)      # (1: the restatement imports the tree as it is now)
        _assert_render_matches(after, ref, "scene %d after the profile call" % sid, True, scene.n_tris)
    with pytest.raises(srt.SrtError):
        srt.Renderer(0).order_children_by_profile(scene, 32, 32, 1, 4)      # no camera set on that context


def _tree(scene):
    return [np.array(a).copy() for a in scene.bvh()] + [scene.bvh_depth]


def _same_tree(a, b):
    return a[-1] == b[-1] and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[:-1], b[:-1]))


@pytest.mark.gpu
def test_tree_tuning_is_its_steps(srt, gpu):
    """srt_tune_tree_for_throughput, ungated, on a 128 x 96 frame of the random spheres: the tree it leaves equals, array for array, a
    second copy of the scene taken through the recipe's steps by hand -- 3 reinsertion passes (none when the deeper tree would leave
    LDS), the scene's camera at the 32 x 32 probe size, the child order from an 8 spp probe frame with 16 deciding rays."""
    W, H, depth = 128, 96, 8
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    hand = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    built = _tree(hand)
    assert scene.n_tris <= 8192
    t = srt.tree_tuning(gpu, scene, W, H, depth)
    assert (t["probe_width"], t["probe_height"], t["probe_spp"]) == (32, 32, 8) and t["order_status"] == 0 and t["throughput_bound"] == 0
    # the reinsertion step, consistent with the launch plans of the tree before and after the passes
    gpu.upload_scene(hand)
    resident = gpu.launch_plan()["all_cached"]
    hand.optimise_bvh(3)
    gpu.upload_scene(hand)
    still = gpu.launch_plan()["all_cached"]
    assert t["reinsertion"] == (2 if resident and not still else 1)
    if t["reinsertion"] == 2:
        hand = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    else:
        assert not _same_tree(_tree(hand), built)
    gpu.set_camera(hand.default_camera(32, 32))
    n = gpu.order_children_by_profile(hand, 32, 32, 8, depth, 16)
    print("tree tuning: %r, by hand %d nodes swapped" % (t, n))
    assert t["nodes_swapped"] == n
    assert _same_tree(_tree(scene), _tree(hand))
    assert ("%d nodes swapped" % n if n else "builder's child order kept") in srt.tune_tree_for_throughput(gpu, hand, W, H, depth, gate=False)


@pytest.mark.gpu
def test_tree_tuning_gated_leaves_a_chain_bound_launch_alone(srt, gpu):
    """only_if_throughput_bound: the same frame has far fewer than 6 pixels per lane -- nothing is tried, no probe frame runs and the tree
    is byte-identical; pixels_per_lane is width * height over the lanes of the scene's launch."""
    W, H, depth = 128, 96, 8
    scene = srt.Scene.builtin(srt.SCENE_RANDOM_SPHERES, 0).build_bvh(srt.BVH_SAH, 1984)
    built = _tree(scene)
    t = srt.tree_tuning(gpu, scene, W, H, depth, gate=True)
    lanes = srt.binding.lib().srt_ctx_cu_count(gpu._h) * gpu.launch_plan()["waves_per_cu"] * 64
    print("gated tree tuning: %r, %d lanes" % (t, lanes))
    assert t["pixels_per_lane"] == W * H / lanes == srt.pixels_per_lane(gpu, W, H)
    assert t["throughput_bound"] == 0 and t["reinsertion"] == 0 and t["nodes_swapped"] == 0 and t["order_status"] == 0
    assert (t["probe_width"], t["probe_height"], t["probe_spp"]) == (0, 0, 0)
    assert _same_tree(_tree(scene), built)
    assert "chain-bound launch" in srt.tune_tree_for_throughput(gpu, scene, W, H, depth, gate=True) and _same_tree(_tree(scene), built)


@pytest.mark.gpu
def test_instrumented_launch_fits_its_debug_buffer(srt, gpu):
    """The per-wave debug words of an instrumented launch are sized from the launcher's own grid arithmetic and checked before anything
    is enqueued: the waves the kernel counts, the rows srt_get_wave_debug returns and the grid -- every CU filled, never more waves than
    queue rows, whole workgroups (16 waves for the Cornell box's shallow tree) -- agree, for an identity queue (4 spp: 88 tiles = 88
    rows) and for the cost probe's split queue (12 spp: up to 64 rows per tile), with and without a lane limit; the buffer holds the
    unclamped count, CUs x waves per CU, and no more."""
    import ctypes as C
    scene = srt.Scene.builtin(srt.SCENE_CORNELL, 0).build_bvh(srt.BVH_REFERENCE, 1984)
    W, H, depth = 64, 48, 8
    cam = scene.default_camera(W, H)
    cus = srt.binding.lib().srt_ctx_cu_count(gpu._h)
    try:
        for lane_limit in (0, 24):
            gpu.set_test_knobs(lane_limit=lane_limit)
            for spp, rows in ((4, 88), (12, 88 * 64)):
                out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=True)
                plan = gpu.launch_plan()
                assert plan["waves_per_cu"] == 16 and plan["test_knobs"]["lane_limit"] == lane_limit
                most = cus * plan["waves_per_cu"]
                grid_waves = -(-min(most, rows) // 16) * 16
                dbg = gpu.wave_debug()
                print("lane limit %d, %d spp: kernel counted %d waves, grid %d, buffer for %d" % (lane_limit, spp, out["stats"]["waves"][0], grid_waves, most))
                assert out["stats"]["waves"][0] == grid_waves == dbg.shape[0]
                words = np.zeros((most + 1, 4), np.uint32)
                ptr = words.ctypes.data_as(C.POINTER(C.c_uint32))
                assert srt.binding.lib().srt_get_wave_debug(gpu._h, ptr, most) == 0
                assert srt.binding.lib().srt_get_wave_debug(gpu._h, ptr, most + 1) == -1
    finally:
        gpu.set_test_knobs()
        gpu.set_count_traversal(False)
        gpu.upload_scene(scene)


def _soup(srt, seed, n, spread=6.0, size=0.25):
    """n small random triangles in a box, 6 materials (lambertian, metallic, dielectric, emissive), sky background"""
    rng = np.random.default_rng(4000 + seed)
    c = rng.uniform(-spread, spread, (n, 3))
    v = [c + rng.normal(0, size, (n, 3)) for _ in range(3)]
    v = [a.astype(np.float32).astype(np.float64) for a in v]
    mat = rng.integers(0, 6, n)
    tris = [(tuple(v[0][k]), tuple(v[1][k]), tuple(v[2][k]), int(mat[k]), 0) for k in range(n)]
    mats = [(0, (0.5, 0.5, 0.5), 0.0, 0.0), (0, (0.73, 0.73, 0.73), 0.0, 0.0), (1, (1.0, 1.0, 1.0), 0.2, 0.0), (2, (1.0, 1.0, 1.0), 0.0, 0.0),
            (4, (1.0, 1.0, 1.0), 0.0, 2.0), (1, (0.5, 0.5, 0.5), 0.0, 0.0)]
    return _custom_scene(srt, tris, mats, (0.5, 0.5, 0.5))


def _assert_render_matches(out, ref, what, count_traversal, n_tris):
    assert_planes_equal(out["xyz"], ref["xyz"], what + " XYZ")
    assert_planes_equal(out["lin"], ref["lin"], what + " unquantised sRGB")
    assert_planes_equal(out["fb"], ref["fb"], what + " fb")
    st, rs = out["stats"], ref["stats"]
    assert st["rays"] == rs["rays"] and st["paths"] == rs["paths"]
    if count_traversal:
        n_nan = st["util"][2]
        assert st["node_visits"] + n_nan * (n_tris - 1) == rs["trav_iters"] and st["tri_tests"] + n_nan * n_tris == rs["tri_tests"]


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("cap", [0, 3, 40])
@pytest.mark.parametrize("sid,mode,W,H,spp,depth", [SCENES[0], SCENES[2], SCENES[3], SCENES[4], SCENES[8], SCENES[9], SCENES[11]])
def test_wide_references_partly_cached_forced_on_small_scenes(srt, gpu, orc, sid, mode, W, H, spp, depth, cap, count_traversal):
    """render_kernel<MODE, NARROW = false, ALL_CACHED = false[, PAIRED]> -- the shape cfg 5's mesh launches -- forced on the small scenes with
    both test knobs (32-bit references, LDS cache capped at 0 / 3 / 40 records): the production build's INNER bursts are the hand-scheduled
    mixed-source block of round 5 (inner_burst4_mixed_asm: lanes inside the LDS prefix and lanes that read the pre-swizzled 80-byte records
    from memory in one visit; cap 0 = every lane from memory), the instrumented build's are the C++ visit: both == the oracle bit for bit."""
    gpu.set_test_knobs(wide_refs=True, lds_cache_max=cap)
    scene = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
    try:
        cam = scene.default_camera(W, H)
        out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
        plan = gpu.launch_plan()
        assert not plan["narrow_refs"] and plan["n_cached"] <= cap
        if scene.n_nodes > 2 * cap + 3:
            assert not plan["all_cached"]
        ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, spp, depth)
        _assert_render_matches(out, ref, "scene %d, wide references, cap %d" % (sid, cap), count_traversal, scene.n_tris)
    finally:
        gpu.set_test_knobs()
        gpu.upload_scene(scene)


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("n,expect_paired", [(600, True), (601, False), (2, True), (3, False), (40000, True), (40001, False)])
def test_paired_trees_launch_the_paired_variant_and_stay_exact(srt, gpu, orc, n, expect_paired, count_traversal):
    """Round 5: the SAH builder cuts every even span into two even halves, so a scene with an even triangle count gets a PAIRED tree (every
    internal node has two leaf children or none) and its launch uses render_kernel<.., PAIRED> -- FRINGE visits without the box test that only
    a leaf + subtree node needs: <.,1,1,paired> for LDS-resident trees, <.,0,0,paired> for the 40 000-triangle soup (32-bit references,
    inner tree partly in L2).  One more triangle: an unpaired tree, the general variant.  Both bit for bit == the oracle walking the same
    tree, work counters included; reinsertion (srt_scene_optimise_bvh) keeps a paired tree paired."""
    scene = _soup(srt, n, n).build_bvh(srt.BVH_SAH, 1984)
    assert scene.is_paired == expect_paired
    if 8 <= n <= 8192:
        scene.optimise_bvh(2)
        assert scene.is_paired == expect_paired
    W, H, spp, depth = 56, 40, 3, 8
    cam = srt.camera_init(W, H, 50.0, (0.5, 1.0, 16.0), (0.0, 0.0, 0.0), defocus_angle=0.6, focus_dist=14.0)
    out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
    plan = gpu.launch_plan()
    assert plan["paired"] == expect_paired, plan
    assert plan["narrow_refs"] == plan["all_cached"] == (n < 40000)
    ref = oracle_scene_for(orc, scene, 1).render(cam, W, H, spp, depth)
    _assert_render_matches(out, ref, "soup of %d (paired %s)" % (n, expect_paired), count_traversal, n)


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("sid,mode,W,H,spp,depth", [SCENES[0], SCENES[2], SCENES[3], SCENES[4], SCENES[8], SCENES[9], SCENES[11]])
def test_partly_cached_narrow_tree_forced_on_small_scenes(srt, gpu, orc, monkeypatch, sid, mode, W, H, spp, depth, cap, count_traversal):
    """render_kernel<MODE, NARROW = true, ALL_CACHED = false>: 16-bit child references, inner records beyond an LDS prefix served by
    L2 -- the variant mid-size scenes (about 5 k to 60 k triangles) launch, which neither the small test scenes (whole tree in LDS)
    nor cfg 5's mesh (32-bit references) reach.  Forced here on the small scenes by capping the LDS cache at `cap` records
    (srt_set_test_knobs; 0 = every inner record comes from L2), both kernel builds."""
    gpu.set_test_knobs(lds_cache_max=cap)
    scene = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
    try:
        cam = scene.default_camera(W, H)
        out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
        plan = gpu.launch_plan()
        assert plan["narrow_refs"] and not plan["all_cached"] and plan["n_cached"] <= cap and plan["test_knobs"]["lds_cache_max"] == cap
        ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, spp, depth)
        _assert_render_matches(out, ref, "scene %d cap %d" % (sid, cap), count_traversal, scene.n_tris)
    finally:
        gpu.set_test_knobs()
        gpu.upload_scene(scene)      # (leave the session's context with a plan that matches its upload)


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("sid,mode,W,H,spp,depth", [SCENES[0], SCENES[2], SCENES[4], SCENES[8], SCENES[9]])
def test_wide_references_forced_on_small_scenes(srt, gpu, orc, monkeypatch, sid, mode, W, H, spp, depth, count_traversal):
    """render_kernel<MODE, NARROW = false, ALL_CACHED = true>: 32-bit references with the whole inner tree in LDS.  No real tree
    gets there (more than 32 767 records of which fewer than ~2 400 are INNER would be deeper than the LDS stack allows), but the
    launcher instantiates it: the wide_refs test knob sends the small scenes through it so that every instantiated variant has run
    against the CPU restatement."""
    gpu.set_test_knobs(wide_refs=True)
    scene = srt.Scene.builtin(sid, 0).build_bvh(mode, 1984)
    try:
        cam = scene.default_camera(W, H)
        out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
        plan = gpu.launch_plan()
        assert not plan["narrow_refs"] and plan["test_knobs"]["wide_refs"] and not plan["test_knobs"]["from_env"]
        assert plan["all_cached"] == (sid != 100)      # (scene 100's 4 802-triangle tree no longer fits LDS with 56-byte records and 4-byte stack slots)
        ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, spp, depth)
        _assert_render_matches(out, ref, "scene %d, wide references" % sid, count_traversal, scene.n_tris)
    finally:
        gpu.set_test_knobs()
        gpu.upload_scene(scene)


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("n,mode", [(9000, 1), (14000, 0), (30000, 1)])
def test_mid_size_scenes_bit_exact(srt, gpu, orc, n, mode, count_traversal):
    """The same variant reached the natural way: soups of 9 000 / 14 000 / 30 000 triangles (SAH and the reference builder's tree):
    16-bit references, more inner records than the LDS cache holds.  GPU == the CPU restatement bit for bit, work counters included."""
    scene = _soup(srt, n, n).build_bvh(mode, 1984)
    W, H, spp, depth = 56, 40, 3, 8
    cam = srt.camera_init(W, H, 50.0, (0.5, 1.0, 16.0), (0.0, 0.0, 0.0), defocus_angle=0.6 if mode else 0.0, focus_dist=14.0)
    out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
    plan = gpu.launch_plan()
    assert plan["narrow_refs"] and not plan["all_cached"] and plan["n_cached"] > 0, plan
    ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, spp, depth)
    _assert_render_matches(out, ref, "soup of %d" % n, count_traversal, n)
    assert max(float(p.max()) for p in out["xyz"]) > 0


@pytest.mark.parametrize("count_traversal", VARIANTS)
@pytest.mark.parametrize("seed", range(12))
def test_random_scenes_fuzz(srt, gpu, orc, seed, count_traversal):
    """Random triangle soups with random materials, cameras and builders (both BVH builders, lens on / off, thin and
    axis-aligned triangles, shared edges and vertices so that exact t ties occur -- Q11): GPU == oracle bit for bit,
    work counters included."""
    scene, cam, W, H, spp, depth, mode, n = fuzz_case(srt, seed)
    out = srt.render_image(scene, cam, W, H, spp, depth, renderer=gpu, count_traversal=count_traversal)
    ref = oracle_scene_for(orc, scene, mode).render(cam, W, H, spp, depth)
    assert_planes_equal(out["xyz"], ref["xyz"], "seed %d XYZ" % seed)
    assert_planes_equal(out["fb"], ref["fb"], "seed %d fb" % seed)
    st, rs = out["stats"], ref["stats"]
    assert st["rays"] == rs["rays"]
    if not count_traversal:
        return
    n_nan = st["util"][2]
    assert st["node_visits"] + n_nan * (n - 1) == rs["trav_iters"] and st["tri_tests"] + n_nan * n == rs["tri_tests"]
