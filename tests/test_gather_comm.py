"""srt_comm_gather_accum over the test transport (tests/cpp/mock_rccl.cpp), all ranks on device 0: after the gather the root's stages
equal a single context's bit for bit, render_interactive_multi equals render_interactive frame for frame, and the ranks of a
process-per-GPU communicator agree on the accumulation or fail together."""
import pytest

from accum_helpers import run_mock_transport_child

pytestmark = pytest.mark.gpu

PRELUDE = """
import numpy as np
from accum_helpers import SEED, fresh_context
from gather_reference import same
from temporal_reference import move_camera
scene = srt.Scene.builtin(srt.SCENE_CORNELL).build_bvh(srt.BVH_REFERENCE, 1984)
W, H, depth = 64, 48, 4
cam = scene.default_camera(W, H)
cams = [cam, move_camera(cam, yaw_deg=1.2), move_camera(cam, yaw_deg=2.4, pitch_deg=0.5)]
single = srt.Renderer(0)
def single_passes(passes):
    fresh_context(single, scene, cam, W, H, depth)
    single.temporal_reset()
    single.accum_reset_features()
    for s in passes:
        single.render_chunk_accum(W, H, s)
"""


@pytest.mark.parametrize("world", [2, 3])
def test_init_all_gather_then_the_roots_stages_equal_a_single_context(world):
    run_mock_transport_child(PRELUDE + """
world = %d
comm = srt.Comm.init_all([0] * world)
comm.upload_scene(scene); comm.set_camera(cam)
comm.init_device_params(W, H, 4, depth, SEED)
comm.accum_reset_features()
for s in (4, 3):
    comm.render_frame_accum(W, H, s)
root = comm.gather_accum()
assert root is comm.root and root.accum_gathered() == 5
single_passes((4, 3))
root.temporal_reset()
same(root.denoise(W, H), single.denoise(W, H), 'denoise')
same(root.present_temporal(W, H, 'denoise'), single.present_temporal(W, H, 'denoise'), 'present_temporal')
pack_ms, exchange_ms, unpack_ms = comm.last_accum_gather_ms()
assert pack_ms > 0 and exchange_ms > 0 and unpack_ms > 0, (pack_ms, exchange_ms, unpack_ms)
# a further pass: the mark is gone and the root refuses until the next gather
comm.render_frame_accum(W, H, 2)
try:
    root.denoise(W, H)
    raise AssertionError('the root denoised stale records')
except srt.SrtError as e:
    assert e.code == -5 and '(or srt_comm_gather_accum first)' in str(e), e
single.render_chunk_accum(W, H, 2)
comm.gather_accum('features')
same(root.denoise(W, H), single.denoise(W, H), 'denoise after the next pass')
# a part the kind lacks: refused on every rank alike, nothing enqueued
try:
    comm.gather_accum('film')
    raise AssertionError('a featured accumulation gathered a film')
except srt.SrtError as e:
    assert e.code == -1 and 'does not hold that part' in str(e), e
same(root.denoise(W, H), single.denoise(W, H), 'denoise after the refusal')
# the moving camera: frame for frame what one GPU yields
want = list(srt.render_interactive(scene, cams, W, H, 4, depth, renderer=single))
got = list(srt.render_interactive_multi(scene, cams, W, H, 4, depth, comm=comm))
assert len(got) == len(want) == 3
for (k, res, feat, pic, st), (k2, res2, feat2, pic2, st2) in zip(got, want):
    assert k == k2
    for key in ('fb', 'lin', 'xyz', 'rowmajor', 'geom'):
        same(res[key], res2[key], 'frame %%d %%s' %% (k, key))
    assert (res['stats']['rays'], res['stats']['paths']) == (res2['stats']['rays'], res2['stats']['paths'])
    same(feat, feat2, 'frame %%d features' %% k); same(pic, pic2, 'frame %%d picture' %% k); same(st, st2, 'frame %%d stats' %% k)
assert got[2][4]['history_frames'] == 3 and got[2][4]['blended'] > 0
want = list(srt.render_interactive(scene, cams[:2], W, H, 4, depth, renderer=single, variance_guided=True))
got = list(srt.render_interactive_multi(scene, cams[:2], W, H, 4, depth, comm=comm, variance_guided=True))
for a, b in zip(got, want):
    same(a[3], b[3], 'variance-guided frame %%d' %% a[0])
comm.close(); single.close()
print('gather comm ok')
""" % world, "gather comm ok", 240)


def test_init_rank_ranks_agree_on_the_accumulation_or_fail_together():
    run_mock_transport_child(PRELUDE + """
import threading
ident = srt.Comm.unique_id()
world = 2
rs = [srt.Renderer(0) for _ in range(world)]
comms = [None] * world
def make(rank):
    comms[rank] = srt.Comm.init_rank(rs[rank], ident, rank, world)
ts = [threading.Thread(target=make, args=(k,)) for k in range(world)]
[t.start() for t in ts]; [t.join(60) for t in ts]
assert all(c is not None and c.world == 2 for c in comms)
def frame(rank, result, reset):
    try:
        c = comms[rank]
        c.upload_scene(scene); c.set_camera(cam)
        c.init_device_params(W, H, 4, depth, SEED)
        reset[rank](rs[rank])
        c.render_frame_accum(W, H, 4)
        c.gather_accum()
        c.synchronize()
        result[rank] = 'ok'
    except srt.SrtError as e:
        result[rank] = e
def run(reset):
    result = [None] * world
    ts = [threading.Thread(target=frame, args=(k, result, reset)) for k in range(world)]
    [t.start() for t in ts]
    [t.join(120) for t in ts]
    assert not any(t.is_alive() for t in ts), 'a rank hangs in the exchange'
    return result
featured = lambda r: r.accum_reset_features()
single_passes((4,))
want = single.denoise(W, H)
# (1) agreement
assert run([featured, featured]) == ['ok', 'ok']
assert comms[0].root is rs[0] and comms[1].root is None
same(rs[0].denoise(W, H), want, 'two ranks, denoise')
# (2) rank 1 resets to another kind behind the communicator's back: both fail, with one message, and nobody hangs
res = run([featured, lambda r: r.accum_reset()])
assert all(isinstance(r, srt.SrtError) and r.code == -1 and 'the ranks disagree on the accumulation to gather' in str(r) for r in res), res
assert str(res[0]) == str(res[1]) and "rank 1 differs from rank 0 in the accumulation's kind" in str(res[0]), res
assert rs[0].accum_gathered() == 0
# (3) agreement restored
assert run([featured, featured]) == ['ok', 'ok']
same(rs[0].denoise(W, H), want, 'two ranks again, denoise')
for c in comms: c.close()
for r in rs: r.close()
single.close()
print('gather agreement ok')
""", "gather agreement ok", 240)


def test_the_communicators_own_read_backs_stay_exact_across_gathers():
    """Comm.meter, Comm.read_spectral and Comm.develop_spectral put the frame together from the ranks: before a gather, while the root is
    whole, after a further pass (the root then holds stale copies of the other ranks' film), and after a gather that leaves the film
    behind -- always the single context's values, every pixel counted once"""
    run_mock_transport_child(PRELUDE + """
resp = srt.renderer.cie_response()
def single_now():
    return dict(meter=single.meter(with_hist=True), film=single.read_spectral(W, H), dev=single.develop_spectral(W, H, resp))
def comm_now(comm):
    return dict(meter=comm.meter(with_hist=True), film=comm.read_spectral(W, H), dev=comm.develop_spectral(W, H, resp))
for world in (2, 3):
    comm = srt.Comm.init_all([0] * world)
    comm.upload_scene(scene); comm.set_camera(cam)
    comm.init_device_params(W, H, 4, depth, SEED)
    comm.accum_reset_spectral_features()
    fresh_context(single, scene, cam, W, H, depth)
    single.accum_reset_spectral_features()
    comm.render_frame_accum(W, H, 4); single.render_chunk_accum(W, H, 4)
    want = single_now()
    assert want['meter']['metered'] > 0 and want['film'].any()
    same(comm_now(comm), want, 'W = %d, before any gather' % world)
    root = comm.gather_accum(('film', 'features'))
    assert root.accum_whole('film')
    same(comm_now(comm), want, 'W = %d, the root whole for the film' % world)
    comm.render_frame_accum(W, H, 3); single.render_chunk_accum(W, H, 3)
    assert not root.accum_whole()
    want = single_now()
    same(comm_now(comm), want, 'W = %d, a pass after the gather: stale copies on the root' % world)
    comm.gather_accum()      # sums and rows: the root is whole for the meter, not for the film
    assert root.accum_whole('features') and not root.accum_whole('film')
    same(comm_now(comm), want, 'W = %d, gathered without the film' % world)
    same(root.meter(with_hist=True), want['meter'], 'the whole root meters the frame')
    comm.close()
single.close()
print('comm read-backs ok')
""", "comm read-backs ok", 240)
