"""The order of a context's calls (srt_c_api.h, at srt_render_chunk): "A context's calls take effect in the order they were made, whichever
streams they name.  A stream handed to a call must stay valid until the next call on that context that synchronises."

Every kernel of this project is held bit for bit to an oracle or a restatement, always on the null stream with a synchronise in between.
Here the same sequences of calls run on streams of the caller's -- a blocking one, which the legacy null stream serialises with, and a
hipStreamNonBlocking one, which it does not -- with NO synchronisation between the calls, and must return what the synchronised null-stream
sequence returned from the same seed: every bit, every counter.  The synchronised sequence runs first, on the same context, so every
working buffer has its size when the sequence under test runs (a hipFree in a regrow waits for the whole device and would hide a race).

The premise of every case is asserted, not assumed: immediately before the first unsynchronised consumer, hipStreamQuery of the pass's
stream returns hipErrorNotReady.  It is carried by a sleep kernel of stream_helpers.DELAY_MS ms enqueued on the pass's stream in front of
the pass (torch.cuda._sleep through torch.cuda.ExternalStream): the host needs well under a millisecond for the calls behind it, so the
consumer is called before the pass has even started, and a library that does not order the two reads the state of BEFORE the pass -- a
failure by values, never by a fault: every buffer the consumer touches holds the valid data the synchronised run left.  N_PASS samples per
pass is therefore as small as the kinds allow (a multiple of the K = 4 streams, at least min_spp of the adaptive ones).  Measured on the
MI355X: a pass of 8 samples takes 0.17 ms of kernel time on the dielectric frame and 0.86 ms on the cornell frame, the host needs 0.05 -
0.10 ms to enqueue it and 0.03 - 0.04 ms for the call behind it, so hipStreamQuery finds even such a pass in flight without a sleep -- by
a margin no test should rest on, which is why the sleep (measured: the stream is busy for 4.2 ms) stands in front of it.  The
communicator's streams are its own, so that case makes its passes long by their sample count (COMM_PASS: 2048 samples, 41 - 43 ms of
kernel time per pass; both frames are enqueued and comm.meter is called 0.2 ms after the first was begun) and asserts the premise by the clock."""
import contextlib

import numpy as np
import pytest

import temporal_reference as T
from accum_helpers import SEED, fresh_context, named_workload, read_frame, read_sum_y, run_mock_transport_child
from stream_helpers import DELAY_MS, KINDS, Streamed, Synced, assert_same, create_stream, destroy_stream, streams

N_PASS = 8                    # samples per pass: a multiple of the K = 4 streams, and the adaptive kinds' min_spp
REL_TOL, MIN_SPP = 0.01, 8    # adaptive kinds: flat pixels stop at the first test, the others stay active through every pass of a case
COMM_PASS = 2048              # samples per pass of the communicator case, whose streams no sleep can be put on

RESETS = {
    "plain": lambda g: g.accum_reset(),
    "adaptive": lambda g: g.accum_reset_adaptive(REL_TOL, 0.0, MIN_SPP),
    "spectral": lambda g: g.accum_reset_spectral(),
    "features": lambda g: g.accum_reset_features(),
    "adaptive+features": lambda g: g.accum_reset_adaptive_features(REL_TOL, 0.0, MIN_SPP),
    "spectral+features": lambda g: g.accum_reset_spectral_features(),
    "adaptive+spectral": lambda g: g.accum_reset_adaptive_spectral(REL_TOL, 0.0, MIN_SPP),
    "adaptive+spectral+features": lambda g: g.accum_reset_adaptive_spectral_features(REL_TOL, 0.0, MIN_SPP),
    "streams4": lambda g: g.accum_reset_streams(4),
}
ACCUM_KINDS = list(RESETS)


@contextlib.contextmanager
def side_streams(gpu, *kinds):
    """streams of the caller's for one test; the context is synchronised before they go, as the contract asks of the caller"""
    with streams(*kinds) as made:
        try:
            yield made
        finally:
            gpu.synchronize()


def workload(srt, name="dielectric"):
    scene, cam, W, H, depth, _ = named_workload(srt, name)
    return scene, cam, W, H, depth


def response(srt):
    """three sensor curves that are not the colour-matching rows, and one that is negative in places"""
    rng = np.random.default_rng(77)
    return np.concatenate([srt.renderer.cie_response(), (rng.random((2, 95)) - 0.3).astype(np.float32)])


def run_pass(gpu, S, W, H, role, delayed=True, spp=N_PASS):
    """one accumulating pass on the stream of `role` (None: the null stream), behind a sleep when it is a stream of the caller's"""
    if delayed and role is not None:
        S.delay(role)
    gpu.render_chunk_accum(W, H, spp, stream=S.stream(role))
    S.done()


def counters(gpu):
    st = gpu.stats()
    return dict(rays=st["rays"], paths=st["paths"])


def state(gpu, kind, W, H):
    """everything the accumulation of `kind` can be read by: the scattered frame in all its planes, the sample total, the last pass's
    counters, and the maps, film and rows the kind has"""
    out = dict(frame=read_frame(gpu, W, H), samples=gpu.accum_samples, counters=counters(gpu), streams=gpu.accum_streams)
    if "adaptive" in kind:
        out["active"] = gpu.accum_active
        out["accum_stats"] = gpu.accum_stats(W, H)
    else:
        out["sum_y"] = read_sum_y(gpu, W, H)
    if "spectral" in kind:
        out["film"] = gpu.read_spectral(W, H)
    if "features" in kind:
        out["features"] = gpu.read_features(W, H)
    return out


def both_ways(gpu, sequence, roles, what):
    """`sequence(S)` synchronised on the null stream, then on fresh streams -- roles: role -> stream kind -- with no synchronisation; the
    second must return what the first returned.  Returns (expected, got, the Streamed policy)."""
    want = sequence(Synced(gpu))
    with side_streams(gpu, *roles.values()) as made:
        S = Streamed(gpu, dict(zip(roles, made)))
        got = sequence(S)
        gpu.synchronize()
        assert S.checked, what + ": no premise was checked"
        assert_same(got, want, what)
    return want, got, S


# ---- a. every accumulation kind, then its readers, no synchronisation in between ----------------------------------------------------------
def reader_rounds(kind):
    """(name, scatter on the pass's stream first, reader): each runs straight behind a further pass that is still in flight"""
    rounds = [("read_fb_rowmajor", True, lambda g, W, H: g.read_fb_rowmajor(W, H)),
              ("read_fb + read_fb_aux", True, lambda g, W, H: (g.read_fb(), g.read_fb_aux(1), g.read_fb_aux(2))),
              ("get_stats", False, lambda g, W, H: counters(g))]
    if "adaptive" in kind:
        rounds += [("accum_stats", False, lambda g, W, H: g.accum_stats(W, H)), ("accum_active", False, lambda g, W, H: g.accum_active)]
    else:
        rounds += [("read_accum_stats", False, lambda g, W, H: read_sum_y(g, W, H))]
    if "spectral" in kind:
        rounds += [("read_spectral", False, lambda g, W, H: g.read_spectral(W, H)),
                   ("read_spectral, part", False, lambda g, W, H: g.read_spectral(W, H, first=7, count=11))]
    if "features" in kind:
        rounds += [("read_features", False, lambda g, W, H: g.read_features(W, H))]
    return rounds


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
@pytest.mark.parametrize("kind", ACCUM_KINDS)
def test_readers_behind_a_pass_in_flight(srt, gpu, kind, stream_kind):
    scene, cam, W, H, depth = workload(srt)
    note = {}

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth)
        RESETS[kind](gpu); S.done()
        run_pass(gpu, S, W, H, "A")
        if not S.streamed:
            note["ms"] = gpu.last_kernel_ms()
        run_pass(gpu, S, W, H, "A", delayed=False)
        S.premise("A", "%s: scatter_tiles on the null stream behind two passes" % kind)
        gpu.scatter_tiles(); S.done()
        out = {"two passes": state(gpu, kind, W, H)}
        for name, scatter, reader in reader_rounds(kind):
            run_pass(gpu, S, W, H, "A")
            if scatter:
                gpu.scatter_tiles(stream=S.stream("A")); S.done()
            S.premise("A", "%s: %s behind a pass" % (kind, name))
            out[name] = reader(gpu, W, H); S.done()
        out["at the end"] = state(gpu, kind, W, H)
        if "adaptive" in kind and not S.streamed:
            note["active"] = [out["two passes"]["active"], out["at the end"]["active"]]
        return out

    want, got, S = both_ways(gpu, sequence, {"A": stream_kind}, "%s on a %s stream" % (kind, stream_kind))
    ms = gpu.last_kernel_ms()
    print("%s, %s stream: %d samples per pass, srt_last_kernel_ms %.3f (synchronised) / %.3f (on the stream) behind a %.0f ms sleep; the pass was in "
          "flight at all %d consumers; active %r" % (kind, stream_kind, N_PASS, note["ms"], ms, DELAY_MS, len(S.checked), note.get("active")))
    assert ms > 0 and note["ms"] > 0
    if "adaptive" in kind:      # pixels that stopped and pixels that did not: the compacted queue and the frozen slots both matter
        assert all(0 < a < W * H for a in note["active"]), note
    assert want["at the end"]["samples"] == N_PASS * (2 + len(reader_rounds(kind)))


# ---- b. every device stage behind an unsynchronised pass ------------------------------------------------------------------------------
def _all_positive(ms):
    vals = [ms] if isinstance(ms, float) else [v for x in ms.values() for v in (x if isinstance(x, list) else [x])]
    return bool(vals) and all(v > 0 for v in vals)


def _meter_ms(g):
    return g.expose_last_ms()["meter"]


def _tone_ms(g):
    return g.expose_last_ms()["tone"]


def _denoise_vg_ms(g):
    return dict(g.denoise_last_ms(), estimate=g.denoise_estimate_last_ms())


FLOOR = dict(floor=0.05)      # (a floor given: the firefly filter is itself the first consumer, not the meter that would find one)
# (id, accumulation kind, the stage, its timers -- all > 0 afterwards --, two frames under a moving camera)
STAGES = [
    ("meter", "plain", lambda srt, g, W, H: g.meter(with_hist=True), _meter_ms, False),
    ("meter-streams", "streams4", lambda srt, g, W, H: g.meter(with_hist=True, percentile_ppm=900000), _meter_ms, False),
    ("expose-metered", "plain", lambda srt, g, W, H: g.expose(W, H), lambda g: g.expose_last_ms(), False),
    ("expose-gain", "adaptive", lambda srt, g, W, H: g.expose(W, H, gain=1.5, curve="linear"), _tone_ms, False),
    ("develop_spectral", "spectral", lambda srt, g, W, H: g.develop_spectral(W, H, response(srt), 0.5), lambda g: g.develop_last_ms()["contract"], False),
    ("develop_spectral_srgb", "adaptive+spectral", lambda srt, g, W, H: g.develop_spectral_srgb(W, H), lambda g: g.develop_last_ms(), False),
    ("denoise", "features", lambda srt, g, W, H: g.denoise(W, H), lambda g: g.denoise_last_ms(), False),
    ("denoise_vg", "spectral+features", lambda srt, g, W, H: g.denoise_vg(W, H), _denoise_vg_ms, False),
    ("denoise_mv", "adaptive+features", lambda srt, g, W, H: g.denoise_mv(W, H), lambda g: g.denoise_last_ms(), False),
    ("denoise_developed", "spectral+features", lambda srt, g, W, H: g.denoise_developed(W, H, response(srt), 0.5), lambda g: g.denoise_last_ms(), False),
    ("denoise_developed-adaptive", "adaptive+spectral+features", lambda srt, g, W, H: g.denoise_developed(W, H, response(srt)[:3]),
     lambda g: g.denoise_last_ms(), False),
    ("despeckle-metered", "plain", lambda srt, g, W, H: g.despeckle(W, H), lambda g: g.despeckle_last_ms(), False),
    ("despeckle-floor", "spectral", lambda srt, g, W, H: g.despeckle(W, H, radius=1, **FLOOR), lambda g: g.despeckle_last_ms(), False),
    ("denoise_despeckled", "features", lambda srt, g, W, H: g.denoise_despeckled(W, H, despeckle=FLOOR), lambda g: g.denoise_last_ms(), False),
    ("temporal", "features", lambda srt, g, W, H: g.temporal(W, H), lambda g: g.temporal_last_ms(), True),
    ("temporal-adaptive", "adaptive+features", lambda srt, g, W, H: g.temporal(W, H, alpha_min=0.3), lambda g: g.temporal_last_ms(), True),
    ("denoise_temporal", "features", lambda srt, g, W, H: g.denoise_temporal(W, H, despeckle=FLOOR), lambda g: g.temporal_last_ms(), True),
    ("present-accum", "plain", lambda srt, g, W, H: g.present(W, H, "accum"), lambda g: g.present_last_ms(), False),
    ("present-accum-gain", "streams4", lambda srt, g, W, H: g.present(W, H, "accum", gain=2.0), lambda g: g.present_last_ms(), False),
    ("present-denoise", "features", lambda srt, g, W, H: g.present(W, H, "denoise"), lambda g: g.present_last_ms(), False),
    ("present-denoise_vg", "features", lambda srt, g, W, H: g.present(W, H, "denoise_vg", gain=1.0), lambda g: g.present_last_ms(), False),
    ("present-denoise_mv", "adaptive+features", lambda srt, g, W, H: g.present(W, H, "denoise_mv"), lambda g: g.present_last_ms(), False),
    ("present-develop", "spectral", lambda srt, g, W, H: g.present(W, H, "develop"), lambda g: g.present_last_ms(), False),
    ("present_despeckled", "plain", lambda srt, g, W, H: g.present_despeckled(W, H, "accum", despeckle=FLOOR), lambda g: g.present_last_ms(), False),
    ("present_temporal", "features", lambda srt, g, W, H: g.present_temporal(W, H, "accum"), lambda g: g.present_last_ms(), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
@pytest.mark.parametrize("stage", STAGES, ids=[s[0] for s in STAGES])
def test_stage_behind_a_pass_in_flight(srt, gpu, stage, stream_kind):
    name, kind, fn, timers, two_frames = stage
    scene, cam, W, H, depth = workload(srt, "cornell" if name.startswith("present") else "dielectric")
    note = {}

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth)
        out = {}
        if two_frames:      # the first frame, on the null stream: the history the second frame is blended into
            RESETS[kind](gpu); S.done()
            run_pass(gpu, S, W, H, None)
            out["first frame"] = fn(srt, gpu, W, H); S.done()
            gpu.set_camera(T.move_camera(cam, (0.02, 0.0, 0.0), yaw_deg=1.2))
        RESETS[kind](gpu); S.done()
        run_pass(gpu, S, W, H, "A")
        if not S.streamed:
            note["ms"] = gpu.last_kernel_ms()
        run_pass(gpu, S, W, H, "A", delayed=False)
        S.premise("A", "%s behind two passes" % name)
        out["stage"] = fn(srt, gpu, W, H); S.done()
        out["after"] = state(gpu, kind, W, H)      # (a stage only reads)
        return out

    both_ways(gpu, sequence, {"A": stream_kind}, "%s on a %s stream" % (name, stream_kind))
    ms = timers(gpu)
    print("%s (%s), %s stream: %d samples per pass, srt_last_kernel_ms %.3f; stage timers %r" % (name, kind, stream_kind, N_PASS, note["ms"], ms))
    assert _all_positive(ms), (name, ms)
    assert gpu.last_kernel_ms() > 0


# ---- c. one accumulation across streams ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "adaptive", "streams4"])
def test_one_accumulation_across_streams(srt, gpu, kind):
    """pass 1 on a non-blocking stream, pass 2 on another, pass 3 on the null stream: the sums, the RNG state, the probe's queue -- and
    the queue pass 1 compacted for pass 2 (adaptive), the combine kernel (streams) -- are shared, and only the context orders them"""
    scene, cam, W, H, depth = workload(srt)

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth)
        RESETS[kind](gpu); S.done()
        run_pass(gpu, S, W, H, "A")
        S.premise("A", "%s: pass 2 on stream B behind pass 1 on stream A" % kind)
        run_pass(gpu, S, W, H, "B")
        S.premise("B", "%s: pass 3 on the null stream behind pass 2 on stream B" % kind)
        run_pass(gpu, S, W, H, None)
        return state(gpu, kind, W, H)

    want, _, _ = both_ways(gpu, sequence, {"A": "nonblocking", "B": "nonblocking"}, "%s over two streams and the null stream" % kind)
    assert want["samples"] == 3 * N_PASS
    if kind == "adaptive":
        assert 0 < want["active"] < W * H, want["active"]


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
def test_scatter_on_another_stream_than_the_launch(srt, gpu, stream_kind):
    scene, cam, W, H, depth = workload(srt, "cornell")

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth, spp=N_PASS)
        gpu.render_chunk(W, H); S.done()      # (the frame a scatter that does not wait would find in the tile buffer)
        if S.streamed:
            S.delay("A")
        gpu.render_chunk(W, H, stream=S.stream("A")); S.done()      # (continues every pixel's RNG stream: another frame)
        S.premise("A", "scatter_tiles on stream B behind a launch on stream A")
        gpu.scatter_tiles(stream=S.stream("B")); S.done()
        return dict(fb=gpu.read_fb(), lin=gpu.read_fb_aux(1), xyz=gpu.read_fb_aux(2), rowmajor=gpu.read_fb_rowmajor(W, H), counters=counters(gpu))

    both_ways(gpu, sequence, {"A": stream_kind, "B": stream_kind}, "launch and scatter on two %s streams" % stream_kind)


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
def test_copy_tile_buffer_on_another_stream_than_the_pass(srt, gpu, stream_kind):
    import torch
    scene, cam, W, H, depth = workload(srt)

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset(); S.done()
        run_pass(gpu, S, W, H, "A")
        _, n_floats, _, _ = gpu.tile_buffer()
        staging = torch.full((n_floats,), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()      # (the fill, on torch's stream: the caller's own work, which the context does not order)
        run_pass(gpu, S, W, H, "A")   # (behind a sleep of its own: the synchronise above waited for the first)
        S.premise("A", "copy_tile_buffer on stream B behind a pass on stream A")
        gpu.copy_tile_buffer(staging.data_ptr(), stream=S.stream("B")); S.done()
        gpu.synchronize()
        tiles = staging.cpu().numpy().copy()
        assert (tiles != -1.0).all()
        return dict(tiles=tiles, after=state(gpu, "plain", W, H))

    both_ways(gpu, sequence, {"A": stream_kind, "B": stream_kind}, "pass and copy_tile_buffer on two %s streams" % stream_kind)


# ---- d. state changes behind a pass in flight ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
@pytest.mark.parametrize("kind", ACCUM_KINDS)
def test_reset_behind_a_pass_in_flight(srt, gpu, kind, stream_kind):
    """the reset zeroes on the null stream what the pass in flight is still adding to; the pass behind it runs on a second stream"""
    scene, cam, W, H, depth = workload(srt)

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth)
        RESETS[kind](gpu); S.done()
        run_pass(gpu, S, W, H, "A")
        S.premise("A", "accum_reset (%s) behind a pass" % kind)
        RESETS[kind](gpu); S.done()
        run_pass(gpu, S, W, H, "B")
        S.premise("B", "%s: the readers behind the pass on stream B" % kind)
        return state(gpu, kind, W, H)

    want, _, _ = both_ways(gpu, sequence, {"A": stream_kind, "B": stream_kind}, "reset of a %s accumulation behind a pass on a %s stream" % (kind, stream_kind))
    assert want["samples"] == N_PASS


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
@pytest.mark.parametrize("change", ["set_camera", "upload_scene + init_device_params"])
def test_new_view_behind_a_pass_in_flight(srt, gpu, change, stream_kind):
    """set_camera touches no device memory; upload_scene and init_device_params of an unchanged scene and grid release nothing (read in
    srt_capi.cpp: DeviceBuffer::reserve frees only when it grows, where hipFree waits for the device) and copy, zero and re-seed on the
    null stream what the pass in flight still reads and advances"""
    scene, cam, W, H, depth = workload(srt, "cornell")
    cam2 = T.move_camera(cam, (0.03, 0.01, 0.0), yaw_deg=2.0)

    def sequence(S):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset_features(); S.done()
        run_pass(gpu, S, W, H, "A")
        S.premise("A", "%s behind a pass" % change)
        if change == "set_camera":
            gpu.set_camera(cam2)
        else:
            fresh_context(gpu, scene, cam2, W, H, depth, seed=SEED + 1)
        S.done()
        gpu.accum_reset_features(); S.done()
        run_pass(gpu, S, W, H, None)
        return state(gpu, "features", W, H)

    both_ways(gpu, sequence, {"A": stream_kind}, "%s behind a pass on a %s stream" % (change, stream_kind))


# ---- e. stream lifetime -------------------------------------------------------------------------------------------------------------------
SYNCHRONISING = {
    "synchronize": lambda g, W, H: g.synchronize(),
    "read_fb": lambda g, W, H: g.read_fb(),
    "read_fb_rowmajor": lambda g, W, H: g.read_fb_rowmajor(W, H),
    "get_stats": lambda g, W, H: g.stats(),
    "meter": lambda g, W, H: g.meter(),
    "present": lambda g, W, H: g.present(W, H),
}


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", KINDS)
@pytest.mark.parametrize("call", list(SYNCHRONISING))
def test_a_stream_may_be_destroyed_after_a_synchronising_call(srt, gpu, call, stream_kind):
    """every call that synchronises drops the stream the context remembers: the consumer and the pass on the null stream behind it must
    not touch the destroyed handle (HIP refuses one: the call would fail)"""
    scene, cam, W, H, depth = workload(srt)

    def sequence(streamed):
        fresh_context(gpu, scene, cam, W, H, depth)
        gpu.accum_reset()
        handle = create_stream(stream_kind) if streamed else None
        try:
            gpu.render_chunk_accum(W, H, N_PASS, stream=handle)
            SYNCHRONISING[call](gpu, W, H)
        except BaseException:
            gpu.synchronize()
            raise
        finally:
            if handle:
                destroy_stream(handle)
        out = dict(meter=gpu.meter(with_hist=True))
        gpu.render_chunk_accum(W, H, N_PASS)
        out["after"] = state(gpu, "plain", W, H)
        return out

    want = sequence(False)
    assert_same(sequence(True), want, "a %s stream destroyed after %s" % (stream_kind, call))
    assert want["after"]["samples"] == 2 * N_PASS


# ---- f. the communicator: its streams are hipStreamNonBlocking and its own ----------------------------------------------------------------
@pytest.mark.gpu
def test_comm_stages_behind_frames_in_flight():
    printed = run_mock_transport_child("""
import time
import numpy as np
from accum_helpers import SEED, named_workload
from stream_helpers import assert_same
scene, cam, W, H, depth, _ = named_workload(srt, 'dielectric')
N = %d
resp = srt.renderer.cie_response()
comm = srt.Comm.init_all([0, 0])

def run(synced):
    comm.set_gather_planes(9)
    comm.upload_scene(scene); comm.set_camera(cam)
    comm.init_device_params(W, H, 12, depth, SEED)
    comm.accum_reset_spectral()
    note = {}
    t0 = time.perf_counter()
    for k in range(2):
        comm.render_frame_accum(W, H, N)
        if synced:
            comm.synchronize()
            for r in comm.renderers:
                r.synchronize()
            note.setdefault('kernel_ms', comm.stats()['max_kernel_ms'])
    note['enqueued_ms'] = (time.perf_counter() - t0) * 1e3
    out = dict(meter=comm.meter(with_hist=True))
    out['rank meters'] = [r.meter(with_hist=True) for r in comm.renderers]
    out['rank films developed'] = [r.develop_spectral(W, H, resp, 0.5) for r in comm.renderers]
    out['film'] = comm.read_spectral(W, H)
    out['developed'] = comm.develop_spectral(W, H, resp, 0.5)
    comm.synchronize()
    root = comm.root
    out['frame'] = dict(fb=root.read_fb(), lin=root.read_fb_aux(1), xyz=root.read_fb_aux(2), rowmajor=root.read_fb_rowmajor(W, H))
    out['stats'] = comm.stats()['paths']
    return out, note

want, ref = run(True)
got, note = run(False)
print('two ranks, %%d samples per pass: slowest render kernel of a pass %%.3f ms; both frames were enqueued, and comm.meter called, %%.3f ms after the first was begun'
      %% (N, ref['kernel_ms'], note['enqueued_ms']))
# THE PREMISE, by the clock (the communicator's streams are its own: there is no handle to query): the first consumer was called before
# even the first of the two passes can have finished
assert note['enqueued_ms'] < ref['kernel_ms'], ('the frames may have finished before comm.meter was called, so nothing was tested -- lengthen the passes', note, ref)
assert_same(got, want, 'two ranks, no comm.synchronize() before the stages')
assert want['meter']['metered'] > 0 and np.abs(want['developed']).max() > 0
comm.close()
print('comm stream order ok')
""" % COMM_PASS, "comm stream order ok", timeout=300)
    print("".join(line + "\n" for line in printed.splitlines() if line.startswith("two ranks")), end="")
