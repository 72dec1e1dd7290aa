"""Gathering an accumulation on the GPU (srt_pack_accum / srt_unpack_accum, csrc/srt_gather.hip): W contexts on device 0 under
srt_set_partition and one partition (0, 1) context with the same seed and the same passes.  The packed units are held to the numpy
restatement (tests/gather_reference.py) built from each rank's own read-backs; after the unpack rank 0 is held to the (0, 1) context,
bit for bit, in its read-backs and in every stage that used to refuse a partition."""
import os

import numpy as np
import pytest

import gather_reference as G
from accum_helpers import ERR_INVALID, ERR_UNSUPPORTED, SEED, converged_f32, expect_error, named_workload, read_sum_y
from features_reference import stack_features
from gather_reference import same
from stream_helpers import streams
from temporal_reference import move_camera

pytestmark = pytest.mark.gpu
REFUSAL = "needs the whole chunk on this context (partition (0, 1)): pixels of other ranks read +0 (or srt_comm_gather_accum first)"
REL_TOL, MIN_SPP = 0.05, 4


class Rig:
    """`world` partition contexts and one (0, 1) context on device 0, all set up alike"""

    def __init__(self, srt, scene, cam, w, h, depth, world, tx=28, ty=16, off=(0, 0), image=None, renderer=None):
        self.srt, self.w, self.h, self.off, self.world = srt, w, h, off, world
        self.seeding = (w, h, 4, depth, SEED, tx, ty)
        self.iw, self.ih = image or (w, h)
        self.ranks = [(renderer or srt.Renderer)(0) for _ in range(world)]
        self.whole = srt.Renderer(0)
        for k, r in enumerate(self.all):
            r.upload_scene(scene); r.set_camera(cam); r.set_count_traversal(False); r.set_gather_planes(9)
            r.init_device_params(*self.seeding)
            r.set_partition(*((k, world) if k < world else (0, 1)))
        g = self.whole.geom
        self.grid = (g["tx"], g["ty"], g["bx"], g["by"])
        self.pool, self.unpacked = {}, False

    @property
    def all(self):
        return self.ranks + [self.whole]

    @property
    def root(self):
        return self.ranks[0]

    def each(self, fn):
        return [fn(r) for r in self.all]

    def reseed(self):
        """every context back to its first RNG state (a reset does not re-seed)"""
        self.each(lambda r: r.init_device_params(*self.seeding))

    def passes(self, *spp):
        for s in spp:
            self.each(lambda r: r.render_chunk_accum(self.w, self.h, s, self.off[0], self.off[1]))

    def units(self, parts=None, stream=None):
        """every rank's unit packed into one rank-major device buffer (kept alive by the rig); (tensor, floats per unit)"""
        import torch
        n = self.root.accum_exchange_size(parts)
        assert all(r.accum_exchange_size(parts) == n for r in self.ranks)
        if n not in self.pool:      # (allocated once per size, so that a sequence on a stream repeats an earlier one without a wait)
            self.pool[n] = torch.empty(max(self.world * n, 1), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
        buf = self.pool[n]
        for k, r in enumerate(self.ranks):
            r.pack_accum(buf.data_ptr() + 4 * n * k, parts, stream)
        return buf, n

    def gather(self, parts=None, stream=None):
        buf, _ = self.units(parts, stream)
        self.root.unpack_accum(buf.data_ptr(), parts, stream)
        self.unpacked = True
        return buf

    def rect(self, a):
        """the chunk's rectangle of a row-major image read-back"""
        a = np.asarray(a)
        if a.ndim == 1:
            a = a.reshape(self.ih, self.iw)
        return a[self.off[1]:self.off[1] + self.h, self.off[0]:self.off[0] + self.w]

    def close(self):
        for r in self.all:
            r.synchronize()
        self.pool = {}
        for r in self.all:
            r.close()


KINDS = {
    "plain": (lambda r: r.accum_reset(), G.SUMS, False),
    "adaptive_features": (lambda r: r.accum_reset_adaptive_features(REL_TOL, 0.0, MIN_SPP), G.SUMS | G.COUNTS | G.FEATURES, False),
    "spectral_features": (lambda r: r.accum_reset_spectral_features(), G.SUMS | G.FEATURES, True),
    "adaptive_spectral_features": (lambda r: r.accum_reset_adaptive_spectral_features(REL_TOL, 0.0, MIN_SPP), G.SUMS | G.COUNTS | G.FEATURES, True),
    "streams": (lambda r: r.accum_reset_streams(2), G.SUMS, False),
    "features": (lambda r: r.accum_reset_features(), G.SUMS | G.FEATURES, False),
}


def _tile_xyz(rig, r):
    """a rank's XYZ sums as the accumulation tests read them: the third plane group of its tile buffer, [tile][plane][slot]"""
    import torch
    r.synchronize()
    _, n, _, padded = r.tile_buffer()
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    r.copy_tile_buffer(t.data_ptr())
    r.synchronize()
    return t.cpu().numpy().view(np.uint32).reshape(3, padded, 3, 64)[2]


def _restated_unit(rig, r, rank, parts):
    """rank's unit, restated from its own read-backs"""
    tx, ty, bx, by = rig.grid
    lanes = G.unit_lanes(rank, rig.world, rig.w, rig.h, tx, ty, bx, by)
    n_lanes = tx * ty * bx * by
    xyz = _tile_xyz(rig, r)                                   # (padded, 3, 64): already in unit order
    planes = [np.zeros(n_lanes, np.uint32) for _ in range(3)]
    ok = lanes >= 0
    for p in range(3):
        planes[p][lanes[ok]] = xyz[:, p, :][ok]
    y = G.to_lanes(rig.rect(read_sum_y(r, rig.iw, rig.ih)), rig.w, rig.h, tx, ty, bx, by)[:, 0]
    mine = np.zeros(n_lanes, bool)
    mine[lanes[ok]] = True
    assert np.array_equal(planes[1][mine], y[mine]), "the Y sums of the tile buffer and of srt_read_accum_stats"
    if not (rank == 0 and rig.unpacked):
        assert (y[~mine] == 0).all(), "a pixel of another rank reads +0 before any gather"
    if parts & G.COUNTS:
        st = r.accum_stats(rig.iw, rig.ih)
        n = G.to_lanes(rig.rect(st["samples"]), rig.w, rig.h, tx, ty, bx, by)[:, 0]
        s2 = G.to_lanes(rig.rect(st["sum_y2"]), rig.w, rig.h, tx, ty, bx, by)[:, 0]
        # the converged flag is not in the read-back: restated from the criterion (tests/accum_helpers.py), at the pixel's own count
        conv = converged_f32(y.view(np.float32), s2.view(np.float32), np.maximum(n.astype(np.int64), 2), MIN_SPP, REL_TOL, 0.0) & (n > 0)
        planes += [n | (conv.astype(np.uint32) << 31), s2]
    feat = film = None
    if parts & G.FEATURES:
        feat = G.to_lanes(rig.rect(stack_features(r.read_features(rig.iw, rig.ih))), rig.w, rig.h, tx, ty, bx, by)
    if parts & G.FILM:
        film = np.zeros((n_lanes, 96), np.uint32)
        film[:, :95] = G.to_lanes(rig.rect(r.read_spectral(rig.iw, rig.ih)), rig.w, rig.h, tx, ty, bx, by)
    return G.pack_unit(lanes, planes, feat, film)


def _check_pack(rig, parts):
    buf, n = rig.units(parts)
    tx, ty, bx, by = rig.grid
    assert n == G.unit_floats(parts, tx, ty, bx, by, rig.world)
    rig.each(lambda r: r.synchronize())
    got = buf.cpu().numpy().view(np.uint32)[:rig.world * n].reshape(rig.world, n)
    for rank, r in enumerate(rig.ranks):
        want = _restated_unit(rig, r, rank, parts)
        diff = np.nonzero(got[rank] != want)[0]
        assert diff.size == 0, "rank %d of %d: %d of %d words differ from the restatement, first at %d (record %d, word %d)" % (
            rank, rig.world, diff.size, n, diff[0], diff[0] // G.tile_floats(parts), diff[0] % G.tile_floats(parts))
    return got


def _readbacks(rig, r, parts):
    out = dict(sum_y=read_sum_y(r, rig.iw, rig.ih), expose=r.expose(rig.iw, rig.ih, gain=1.0, curve="linear"), meter=r.meter(with_hist=True))
    if parts & G.COUNTS:
        out["stats"] = r.accum_stats(rig.iw, rig.ih)
    if parts & G.FEATURES:
        out["features"] = r.read_features(rig.iw, rig.ih)
    if parts & G.FILM:
        out["film"] = r.read_spectral(rig.iw, rig.ih)
    return out


def _check_unpack(rig, parts, what):
    own_before = _own_unit(rig, parts)
    rig.gather(parts)
    assert rig.root.accum_gathered() == parts | G.SUMS
    same(_readbacks(rig, rig.root, parts), _readbacks(rig, rig.whole, parts), what + ": rank 0 after the unpack against the (0, 1) context")
    assert np.array_equal(own_before, _own_unit(rig, parts)), what + ": the unpack changed rank 0's own records"


def _own_unit(rig, parts):
    import torch
    n = rig.root.accum_exchange_size(parts)
    t = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rig.root.pack_accum(t.data_ptr(), parts)
    rig.root.synchronize()
    return t.cpu().numpy().view(np.uint32)[:n].copy()


def _run_kind(rig, kind, passes, film=False):
    reset, parts, spectral = KINDS[kind]
    if film:
        assert spectral
        parts |= G.FILM
    rig.each(reset)
    rig.passes(*passes)
    return parts


def _workload(srt, w, h):
    scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
    return scene, scene.default_camera(w, h)


# ---- shapes: pack and unpack at the smallest sizes at which the copy can go wrong --------------------------------------------------
SHAPE_CASES = {
    "45x27-W3": dict(w=45, h=27, world=3),
    "45x27-W3-offset": dict(w=45, h=27, world=3, off=(8, 16), image=(64, 48)),
    "45x27-W3-tx10-ty6": dict(w=45, h=27, world=3, tx=10, ty=6),
    "8x8-W5-tx8-ty8": dict(w=8, h=8, world=5, tx=8, ty=8),
    "64x48-W2": dict(w=64, h=48, world=2),
}


@pytest.mark.parametrize("case", list(SHAPE_CASES))
def test_shapes_pack_equals_the_restatement_and_unpack_the_whole_context(srt, case):
    cfg = dict(SHAPE_CASES[case])
    w, h, world = cfg.pop("w"), cfg.pop("h"), cfg.pop("world")
    scene, cam = _workload(srt, *(cfg.get("image") or (w, h)))
    rig = Rig(srt, scene, cam, w, h, 4, world, **cfg)
    try:
        parts = _run_kind(rig, "adaptive_spectral_features", (4, 2), film=True)      # every part there is: 109 words per pixel
        _check_pack(rig, parts)
        _check_unpack(rig, parts, case)
        # the next pass on every rank continues its own RNG streams and records; a second gather is equal again
        rig.passes(3)
        assert rig.root.accum_gathered() == 0
        _check_pack(rig, parts)
        _check_unpack(rig, parts, case + ", second gather")
    finally:
        rig.close()


def test_forced_scalar_path_packs_and_unpacks_the_same_bits(srt):
    """contexts whose kernel never takes the 16-byte paths (the fenced test knob) against the default ones, on the default block"""
    saved = {k: os.environ.get(k) for k in ("SRT_TEST_KNOBS", "SRT_GATHER_SCALAR")}
    scene, cam = _workload(srt, 45, 27)
    vec = Rig(srt, scene, cam, 45, 27, 4, 3)
    os.environ.update(SRT_TEST_KNOBS="1", SRT_GATHER_SCALAR="1")
    try:
        scalar = Rig(srt, scene, cam, 45, 27, 4, 3)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        units = []
        for rig in (vec, scalar):
            parts = _run_kind(rig, "adaptive_spectral_features", (4, 2), film=True)
            units.append(_check_pack(rig, parts))
            _check_unpack(rig, parts, "scalar" if rig is scalar else "vector")
        assert np.array_equal(units[0], units[1])
        same(_readbacks(vec, vec.root, parts), _readbacks(scalar, scalar.root, parts), "vector against scalar")
    finally:
        vec.close(); scalar.close()


# ---- kinds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,film", [("plain", False), ("adaptive_features", False), ("spectral_features", True), ("adaptive_spectral_features", False),
                                       ("streams", False)])
def test_kinds(srt, kind, film):
    scene, cam = _workload(srt, 45, 27)
    rig = Rig(srt, scene, cam, 45, 27, 4, 3)
    try:
        parts = _run_kind(rig, kind, (4, 4) if kind != "streams" else (4, 2), film)
        if parts & G.COUNTS:      # stopped after a second pass: converged and active pixels both exist
            n = rig.whole.accum_stats(45, 27)["samples"]
            assert (n == 4).any() and (n == 8).any(), np.unique(n)
        assert rig.root.accum_exchange_size(None) == G.unit_floats(parts & ~G.FILM, *rig.grid, 3), "parts = 0: everything the kind holds except the film"
        _check_pack(rig, parts)
        _check_unpack(rig, parts, kind)
        held = KINDS[kind][1] | (G.FILM if KINDS[kind][2] else 0)
        for bit in (G.COUNTS, G.FEATURES, G.FILM):      # a part the kind lacks is refused with nothing changed
            if not held & bit:
                before = rig.root.accum_gathered()
                expect_error(srt, lambda: rig.root.accum_exchange_size(bit), ERR_INVALID, "size")
                expect_error(srt, lambda: rig.root.pack_accum(next(iter(rig.pool.values())).data_ptr(), bit), ERR_INVALID, "pack")
                expect_error(srt, lambda: rig.root.unpack_accum(next(iter(rig.pool.values())).data_ptr(), G.SUMS | bit), ERR_INVALID, "unpack")
                assert rig.root.accum_gathered() == before
        same(_readbacks(rig, rig.root, parts), _readbacks(rig, rig.whole, parts), kind + " after the refusals")
    finally:
        rig.close()


# ---- stages ----------------------------------------------------------------------------------------------------------------------------
def _stage_calls(srt, W, H, kind):
    """name -> call(renderer): every stage that refuses a partition, for an accumulation of `kind`"""
    calls = {
        "despeckle": lambda r: r.despeckle(W, H),
        "denoise": lambda r: r.denoise(W, H),
        "denoise_vg": lambda r: r.denoise_vg(W, H),
        "denoise_despeckled": lambda r: r.denoise_despeckled(W, H, despeckle={}),
        "temporal": lambda r: r.temporal(W, H),
        "denoise_temporal": lambda r: r.denoise_temporal(W, H),
        "denoise_temporal_vg": lambda r: r.denoise_temporal_vg(W, H),
        "present denoise": lambda r: r.present(W, H, "denoise"),
        "present denoise_vg": lambda r: r.present(W, H, "denoise_vg"),
        "present_despeckled": lambda r: r.present_despeckled(W, H, "accum", despeckle={}),
        "present_temporal": lambda r: r.present_temporal(W, H, "denoise"),
        "present_temporal accum": lambda r: r.present_temporal(W, H, "accum"),
        "present_temporal_vg": lambda r: r.present_temporal_vg(W, H),
    }
    if kind == "adaptive_features":
        calls["denoise_mv"] = lambda r: r.denoise_mv(W, H)
        calls["present denoise_mv"] = lambda r: r.present(W, H, "denoise_mv")
    if kind == "spectral_features":
        calls["denoise_developed"] = lambda r: r.denoise_developed(W, H, srt.renderer.cie_response())
    return calls


@pytest.mark.parametrize("kind", ["features", "adaptive_features", "spectral_features"])
def test_every_stage_that_refused_equals_the_whole_context(srt, kind):
    W, H = 64, 48
    scene, cam = _workload(srt, W, H)
    cam2 = move_camera(cam, yaw_deg=1.2) if kind == "features" else None      # a turn of about two pixels
    rig = Rig(srt, scene, cam, W, H, 4, 3)
    try:
        film = kind == "spectral_features"
        parts = _run_kind(rig, kind, (4, 4), film)
        calls = _stage_calls(srt, W, H, kind)
        for name, call in calls.items():      # before any gather: the old refusal, with the hint appended
            with pytest.raises(srt.SrtError) as e:
                call(rig.root)
            assert e.value.code == ERR_UNSUPPORTED and REFUSAL in str(e.value), (name, e.value)
        if film:      # a gather without the film leaves srt_denoise_developed refusing, and it alone
            rig.gather(parts & ~G.FILM)
            with pytest.raises(srt.SrtError) as e:
                calls["denoise_developed"](rig.root)
            assert e.value.code == ERR_UNSUPPORTED and REFUSAL in str(e.value)
            same(rig.root.denoise(W, H), rig.whole.denoise(W, H), "denoise without the film")
        rig.gather(parts)
        rig.each(lambda r: r.temporal_reset())
        for name, call in calls.items():
            same(call(rig.root), call(rig.whole), "%s: %s" % (kind, name))
        # the sources that accept a partition count every pixel on a whole context
        for source in ("accum",) + (("develop",) if film else ()):
            same(rig.root.present(W, H, source), rig.whole.present(W, H, source), "present " + source)
        if cam2 is not None:      # the temporal stage over two cameras: the history belongs to the context and carries over
            rig.each(lambda r: r.temporal_reset())
            for k, c in enumerate((cam, cam2)):
                rig.each(lambda r: r.set_camera(c))
                rig.each(lambda r: r.accum_reset_features())
                rig.passes(4)
                rig.gather()
                a, b = rig.root.temporal(W, H), rig.whole.temporal(W, H)
                same(a, b, "temporal, camera %d" % k)
                assert a["stats"]["history_frames"] == k + 1
            assert a["stats"]["blended"] > 0
        # a pass clears the mark: the foreign records are stale, and the stages refuse again with the old text
        rig.passes(2)
        assert rig.root.accum_gathered() == 0
        for name, call in calls.items():
            with pytest.raises(srt.SrtError) as e:
                call(rig.root)
            assert e.value.code == ERR_UNSUPPORTED and REFUSAL in str(e.value), (name, e.value)
        rig.gather(parts)
        same(rig.root.denoise(W, H), rig.whole.denoise(W, H), "denoise after the next pass and gather")
        # a reset clears it too
        rig.root.accum_reset_features()
        assert rig.root.accum_gathered() == 0
    finally:
        rig.close()


def test_moving_chain_across_a_refit_of_every_context(srt):
    scene, cam, W, H, depth, _ = named_workload(srt, "cornell")
    v0 = scene.vertices()
    v1 = v0.copy()
    v1[12:24, :, 0] = (v1[12:24, :, 0] + np.float32(0.02 * np.linalg.norm(np.ptp(v0.reshape(-1, 3), axis=0)))).astype(np.float32)
    rig = Rig(srt, scene, cam, W, H, depth, 2)
    try:
        rig.each(lambda r: (r.track_motion(True), r.upload_scene(scene)))      # (tracking starts with an upload: the vertices are known)
        for k, verts in enumerate((None, v1)):
            if verts is not None:
                rig.each(lambda r: r.refit(verts))      # as Comm.refit: the same vertices on every context
            rig.each(lambda r: r.accum_reset_features())
            rig.passes(4)
            # not whole (no gather yet, or a pass since the last one): the moving variants refuse like the static ones, the history untouched
            assert rig.root.accum_gathered() == 0 and not rig.root.accum_whole("features")
            for name, call in (("temporal_moving", lambda r: r.temporal_moving(W, H)), ("denoise_temporal_moving", lambda r: r.denoise_temporal_moving(W, H)),
                               ("present_temporal_moving", lambda r: r.present_temporal_moving(W, H, "denoise"))):
                with pytest.raises(srt.SrtError) as e:
                    call(rig.root)
                assert e.value.code == ERR_UNSUPPORTED and REFUSAL in str(e.value), (name, k, e.value)
            rig.gather()
            assert rig.root.accum_whole("features") and not rig.root.accum_whole("film") and rig.whole.accum_whole("film")
            a, b = rig.root.denoise_temporal_moving(W, H), rig.whole.denoise_temporal_moving(W, H)
            same(a, b, "denoise_temporal_moving, frame %d" % k)
        assert a["stats"]["history_frames"] == 2 and a["surface"]["moved"] > 0
    finally:
        rig.close()


def test_refusals_change_nothing(srt):
    import torch
    scene, cam = _workload(srt, 45, 27)
    rig = Rig(srt, scene, cam, 45, 27, 4, 2)
    try:
        t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
        p = t.data_ptr()
        for what, call in (("size", lambda: rig.root.accum_exchange_size()), ("pack", lambda: rig.root.pack_accum(p)), ("unpack", lambda: rig.root.unpack_accum(p))):
            expect_error(srt, call, ERR_INVALID, what + " without an accumulation")
        rig.each(lambda r: r.accum_reset_features())
        expect_error(srt, lambda: rig.root.pack_accum(p), ERR_INVALID, "pack before the first pass")
        rig.passes(4)
        expect_error(srt, lambda: rig.root.pack_accum(0), ERR_INVALID, "null destination")
        expect_error(srt, lambda: rig.root.unpack_accum(0), ERR_INVALID, "null source")
        lib = srt.binding.lib()
        assert lib.srt_pack_accum(rig.root._h, 16, p, None) == ERR_INVALID and lib.srt_unpack_accum(rig.root._h, 32, p, None) == ERR_INVALID
        rig.root.set_count_traversal(True)
        expect_error(srt, lambda: rig.root.pack_accum(p), ERR_UNSUPPORTED, "instrumented context")
        expect_error(srt, lambda: rig.root.unpack_accum(p), ERR_UNSUPPORTED, "instrumented context")
        rig.root.set_count_traversal(False)
        rig.root.synchronize()
        assert rig.root.accum_gathered() == 0 and not t.cpu().numpy().any()
        # world 1: the unpack succeeds and enqueues nothing
        before = _readbacks(rig, rig.whole, G.SUMS | G.FEATURES)
        rig.whole.unpack_accum(p)
        same(_readbacks(rig, rig.whole, G.SUMS | G.FEATURES), before, "world 1")
        assert rig.whole.gather_last_ms()[1] == 0.0
        rig.gather()
        pack_ms, unpack_ms = rig.root.gather_last_ms()
        assert pack_ms > 0 and unpack_ms > 0
        # everything that invalidates the accumulation clears the mark
        assert rig.root.accum_gathered() == G.SUMS | G.FEATURES
        rig.root.set_camera(cam)
        assert rig.root.accum_gathered() == 0
    finally:
        rig.close()


# ---- stream order ------------------------------------------------------------------------------------------------------------------------
def test_pack_unpack_stage_on_a_non_blocking_stream_without_synchronisation(srt):
    W, H = 64, 48
    scene, cam = _workload(srt, W, H)
    rig = Rig(srt, scene, cam, W, H, 4, 2)
    try:
        parts = _run_kind(rig, "features", (4, 4))
        rig.gather(parts)
        want = rig.root.denoise(W, H)
        rig.passes(3)
        rig.gather(parts)
        want2 = rig.root.denoise(W, H)
        # the same sequence again from the reset, every pass, pack and unpack on one non-blocking stream, nothing waited for in between
        with streams("nonblocking") as (handle,):
            rig.reseed()
            rig.each(lambda r: r.accum_reset_features())
            for s in (4, 4):
                for r in rig.all:
                    r.render_chunk_accum(W, H, s, 0, 0, stream=handle)
            rig.gather(parts, stream=handle)
            same(rig.root.denoise(W, H), want, "pack -> unpack -> stage on one stream")
            for r in rig.all:
                r.render_chunk_accum(W, H, 3, 0, 0, stream=handle)
            rig.gather(parts, stream=handle)
            same(rig.root.denoise(W, H), want2, "second round on the stream")
            same(rig.whole.denoise(W, H), want2, "the (0, 1) context")
            rig.each(lambda r: r.synchronize())
    finally:
        rig.close()
