"""Shared by tests/test_stream_order.py: HIP streams of the caller's made with ctypes on the runtime the process already has mapped, the
premise every case asserts (the pass is still in flight when its consumer is called), the two ways a sequence of calls is run -- on the
null stream with a synchronise after every call, which the rest of the suite holds to the oracle and the restatements, and on streams
with no synchronisation at all -- and the comparison of everything such a sequence returns, bit for bit."""
import contextlib
import ctypes as C
import os

import numpy as np

from path_ends_reference import assert_same_floats

HIP_SUCCESS, HIP_ERROR_NOT_READY = 0, 600
STREAM_FLAGS = {"blocking": 0, "nonblocking": 1}      # hipStreamDefault, hipStreamNonBlocking
KINDS = tuple(STREAM_FLAGS)
DELAY_MS = 8.0      # the sleep kernel enqueued in front of a pass: the host needs well under a millisecond to make the calls behind it
_hip = None
_cycles_per_ms = None


def mapped_hip_runtimes():
    """the files named libamdhip64* this process has mapped"""
    found = set()
    with open("/proc/self/maps") as maps:
        for line in maps:
            fields = line.split(None, 5)
            if len(fields) == 6 and os.path.basename(fields[5].strip()).startswith("libamdhip64"):
                found.add(fields[5].strip())
    return sorted(found)


def hip():
    """The HIP runtime of this process, which must hold exactly one: a stream handle means something to libsrt_hip.so (and to torch) only
    when they speak to the same runtime instance.  torch bundles a copy of its own, so this is asserted, never assumed."""
    global _hip
    if _hip is None:
        import importlib
        import torch
        importlib.import_module("cuda-spectral-ray-tracer_amd").binding.lib()
        torch.cuda.init()
        found = mapped_hip_runtimes()
        assert len(found) == 1, ("exactly one libamdhip64 must be mapped for a stream handle to mean the same to libsrt_hip.so, torch and "
                                 "these tests; this process maps %d: %r" % (len(found), found))
        lib = C.CDLL(found[0])      # (already mapped: the same instance)
        lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        lib.hipStreamDestroy.argtypes = [C.c_void_p]
        lib.hipStreamQuery.argtypes = [C.c_void_p]
        for fn in (lib.hipStreamCreateWithFlags, lib.hipStreamDestroy, lib.hipStreamQuery):
            fn.restype = C.c_int
        _hip = lib
    return _hip


def create_stream(kind):
    h = C.c_void_p()
    rc = hip().hipStreamCreateWithFlags(C.byref(h), STREAM_FLAGS[kind])
    assert rc == HIP_SUCCESS and h.value, ("hipStreamCreateWithFlags", kind, rc)
    return h.value


def destroy_stream(handle):
    rc = hip().hipStreamDestroy(C.c_void_p(handle))
    assert rc == HIP_SUCCESS, ("hipStreamDestroy", rc)


@contextlib.contextmanager
def streams(*kinds):
    """one stream per entry of `kinds` ("blocking" / "nonblocking"), as integer handles; destroyed whatever the body did (after a
    device-wide wait: nothing may still run on them)"""
    import torch
    made = []
    try:
        for k in kinds:
            made.append(create_stream(k))
        yield list(made)
    finally:
        torch.cuda.synchronize()
        for h in made:
            destroy_stream(h)


def in_flight(handle):
    rc = hip().hipStreamQuery(C.c_void_p(handle))
    assert rc in (HIP_SUCCESS, HIP_ERROR_NOT_READY), ("hipStreamQuery", rc)
    return rc == HIP_ERROR_NOT_READY


def assert_in_flight(handle, what):
    """THE PREMISE of every case: the work on `handle` has not finished when the next call is made.  Not a skip: a test whose premise
    fails has tested nothing."""
    assert in_flight(handle), ("%s: the pass had already finished when its consumer was called, so nothing was tested -- lengthen the "
                               "pass (more samples) or the sleep in front of it (stream_helpers.DELAY_MS)" % what)


def sleep_cycles(ms):
    """the argument of torch.cuda._sleep that keeps a stream busy for about `ms` milliseconds, measured once on this device"""
    global _cycles_per_ms
    import torch
    if _cycles_per_ms is None:
        torch.cuda._sleep(1000)      # (loads the kernel)
        n = 200000
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); torch.cuda._sleep(n); e1.record(); e1.synchronize()
            took = e0.elapsed_time(e1)
            if took >= 1.0:
                break
            n *= 8
        assert took >= 1.0, "torch.cuda._sleep(%d) took %.3f ms: no way to keep a stream busy" % (n, took)
        _cycles_per_ms = n / took
        print("torch.cuda._sleep: %d cycles took %.3f ms" % (n, took))
    return int(_cycles_per_ms * ms)


def delay(handle, ms=DELAY_MS):
    """enqueue a sleep of about `ms` milliseconds on the caller's stream `handle`: what is enqueued behind it cannot have started, let alone
    finished, when the host makes its next calls"""
    import torch
    with torch.cuda.stream(torch.cuda.ExternalStream(handle)):
        torch.cuda._sleep(sleep_cycles(ms))


class Synced:
    """A sequence of calls run the way the rest of the suite runs them: every stream is the null stream, and the context is synchronised
    after every call.  What it returns is the expected value of the same sequence under `Streamed`."""
    streamed = False

    def __init__(self, gpu):
        self.gpu = gpu

    def stream(self, role):
        return None

    def delay(self, role, ms=DELAY_MS):
        pass

    def done(self):
        self.gpu.synchronize()

    def premise(self, role, what):
        pass


class Streamed:
    """The same sequence on the caller's streams -- `handles`: role -> handle; a role not named there, or None, is the null stream -- with no
    synchronisation between the calls."""
    streamed = True

    def __init__(self, gpu, handles):
        self.gpu, self.handles, self.checked = gpu, dict(handles), []

    def stream(self, role):
        return self.handles.get(role)

    def delay(self, role, ms=DELAY_MS):
        delay(self.handles[role], ms)

    def done(self):
        pass

    def premise(self, role, what):
        assert_in_flight(self.handles[role], what)
        self.checked.append(what)


def assert_same(got, want, what):
    """everything a sequence returned, against the synchronised run's: every bit of every float (NaN equals NaN of the same bits or any
    NaN, as assert_same_floats has it), every integer, every counter, every key"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (what, sorted(got), sorted(want))
        for k in want:
            assert_same(got[k], want[k], "%s[%r]" % (what, k))
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), (what, len(got), len(want))
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same(a, b, "%s[%d]" % (what, i))
    elif isinstance(want, np.ndarray) and want.dtype.kind == "f":
        assert_same_floats(got, want, what)
    elif isinstance(want, np.ndarray):
        got = np.asarray(got)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
        bad = np.argwhere(got != want)
        assert not len(bad), "%s: %d of %d entries differ, first at %r: got %r want %r" % (what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    elif isinstance(want, float):
        assert isinstance(got, float) and (got == want or (got != got and want != want)), (what, got, want)
    else:
        assert type(got) is type(want) and got == want, (what, got, want)
