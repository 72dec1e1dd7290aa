"""The packing rule of the presented picture (srt_present / srt_present_kat; include/srt_c_api.h), stated once in numpy: the quantised sRGB
of the tone stage -- whole numbers in 0 .. 255 held in float32, what srt_expose_accum / srt_expose_kat return as out_q -- cast to bytes,
and A = 255 behind them.  tests/test_present_config.py holds the precondition (the quantised values ARE whole numbers in 0 .. 255 for every
input, NaN and infinities included: without it the cast would be undefined); tests/test_present.py holds the device to pack() of what the
existing calls return."""
import numpy as np


def pack(q):
    """rgba (..., 4) uint8 of quantised sRGB q (..., 3): rgba = stack(q.astype(uint8), 255)"""
    q = np.asarray(q, np.float32)
    assert q.shape[-1] == 3
    assert ((q >= 0) & (q <= 255) & (q == np.floor(q))).all(), "a quantised value that is no whole number in 0 .. 255"
    out = np.empty(q.shape[:-1] + (4,), np.uint8)
    out[..., :3] = q.astype(np.uint8)
    out[..., 3] = 255
    return out


def words(rgba):
    """the picture as one little-endian uint32 per pixel: R | G << 8 | B << 16 | A << 24"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    return rgba.view("<u4")[..., 0]
