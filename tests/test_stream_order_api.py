"""The order of a context's calls, without a GPU: include/srt_c_api.h states the contract where the first call that takes a stream is
declared and names the calls that synchronise, INTEGRATION.md repeats it, and every Python method that takes `stream=` hands it to the
library unchanged."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("A context's calls take effect in the order they were made, whichever streams they name.",
            "A stream handed to a call must stay valid until the next call on that context that synchronises.")
SYNCHRONISING = ("srt_synchronize", "srt_read_fb", "srt_read_fb_rowmajor", "srt_read_accum_stats", "srt_read_spectral", "srt_read_features", "srt_get_stats",
                 "srt_meter_", "srt_expose_", "srt_develop_", "srt_despeckle_", "srt_temporal_", "srt_denoise_", "srt_present")


def _flat(text):
    return re.sub(r"\s+", " ", re.sub(r"(?m)^\s*(/\*|\*/?|>)\s?", " ", text))


def test_header_states_the_contract_at_render_chunk():
    src = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    at = src.index("SRT_API int srt_render_chunk(")
    comment = src[src.rindex("/*", 0, at):at]
    assert comment.rstrip().endswith("*/") and comment.count("/*") == 1, "no comment directly in front of srt_render_chunk"
    flat = _flat(comment)
    for sentence in CONTRACT:
        assert sentence in flat, sentence
    for name in SYNCHRONISING:
        assert name in flat, "the calls that synchronise must be listed: " + name


def test_integration_guide_repeats_the_contract():
    flat = _flat(open(os.path.join(ROOT, "INTEGRATION.md")).read())
    for sentence in CONTRACT:
        assert sentence in flat, sentence
    assert "srt_synchronize" in flat and "hipStreamNonBlocking" in flat


class _Recorder:
    """stands in for the loaded library: every function returns SRT_OK and notes its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_every_stream_argument_reaches_the_library(srt, monkeypatch):
    header = open(os.path.join(ROOT, "include", "srt_c_api.h")).read()
    takes_stream = set(re.findall(r"SRT_API\s+int\s+(srt_\w+)\s*\([^;]*?void \*stream\)", header))
    assert takes_stream == {"srt_render_chunk", "srt_render_chunk_accum", "srt_copy_tile_buffer", "srt_scatter_tiles"}, takes_stream
    rec = _Recorder()
    monkeypatch.setattr(srt.binding, "lib", lambda: rec)
    r = srt.Renderer.__new__(srt.Renderer)
    r._h, r._owned = C.c_void_p(0x1000), False
    reached = set()
    methods = [(n, f) for n, f in inspect.getmembers(srt.Renderer, inspect.isfunction) if "stream" in inspect.signature(f).parameters]
    assert len(methods) == len(takes_stream), [n for n, _ in methods]
    for n, f in methods:
        params = inspect.signature(f).parameters
        assert params["stream"].default is None, n
        required = [p for p in list(params.values())[1:] if p.default is inspect.Parameter.empty]
        for handle, want in ((0x7f12345678, 0x7f12345678), (None, None)):      # (None: the null stream, a NULL pointer)
            del rec.calls[:]
            f(r, *[16] * len(required), stream=handle)
            assert len(rec.calls) == 1, (n, rec.calls)
            name, args = rec.calls[0]
            assert name in takes_stream and args[0] is r._h, (n, name)
            assert isinstance(args[-1], C.c_void_p) and args[-1].value == want, (n, name, args[-1])
            reached.add(name)
    r._h = None
    assert reached == takes_stream
