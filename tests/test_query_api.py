"""CPU: the Python face of the ray queries -- ray_batch's layout, and every refusal of Renderer.intersect / occluded raised before any device
is touched (the library is replaced by a trap for the duration)."""
import numpy as np
import pytest


@pytest.fixture
def trapped(srt, monkeypatch):
    """a Renderer without a context whose library calls all fail the test: a check that ran after a call would not be a check"""
    def trap():
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(srt.binding, "lib", trap)
    r = object.__new__(srt.Renderer)
    r._h, r._owned, r.device = None, False, 0
    return r


def test_ray_batch_layout_numpy(srt):
    o = np.array([[1, 2, 3], [4, 5, 6]], np.float64)
    d = np.array([[0.5, 0, -1], [0, 1, 0]], np.float32)
    r = srt.ray_batch(o, d, tmin=[0.25, 1e-4], tmax=[7.0, np.inf])
    assert isinstance(r, np.ndarray) and r.dtype == np.float32 and r.shape == (2, 8) and r.flags.c_contiguous
    assert r.tolist() == [[1, 2, 3, 0.25, 0.5, 0, -1, 7.0], [4, 5, 6, np.float32(1e-4), 0, 1, 0, np.inf]]
    r = srt.ray_batch([0, 0, 1], d)        # one origin for all, tmin 0, tmax None -> FLT_MAX
    assert r[:, 0:3].tolist() == [[0, 0, 1]] * 2 and (r[:, 3] == 0).all() and (r[:, 7] == np.finfo(np.float32).max).all()
    assert r[:, 7].view(np.uint32).tolist() == [0x7F7FFFFF] * 2
    with pytest.raises(ValueError):
        srt.ray_batch(o, np.zeros((2, 4), np.float32))


def test_ray_batch_layout_torch(srt):
    torch = pytest.importorskip("torch")
    o = torch.tensor([[1.0, 2.0, 3.0]])
    d = torch.tensor([[0.0, 0.0, -2.0]])
    r = srt.ray_batch(o, d, tmin=0.5)
    assert isinstance(r, torch.Tensor) and r.dtype == torch.float32 and tuple(r.shape) == (1, 8) and r.is_contiguous()
    assert r.tolist() == [[1.0, 2.0, 3.0, 0.5, 0.0, 0.0, -2.0, float(np.finfo(np.float32).max)]]


@pytest.mark.parametrize("bad,exc", [
    (np.zeros((4, 8), np.float64), TypeError),            # dtype
    (np.zeros((4, 6), np.float32), ValueError),           # srt_trace_rays' rows are not query rows
    (np.zeros(8, np.float32), ValueError),                # one row must still be (1, 8)
    (np.zeros((2, 4, 8), np.float32), ValueError),
    ([[0.0] * 8], TypeError),                             # a list is neither numpy nor torch
], ids=["float64", "six-columns", "1-d", "3-d", "list"])
@pytest.mark.parametrize("entry", ["intersect", "occluded"])
def test_numpy_refusals(trapped, entry, bad, exc):
    with pytest.raises(exc):
        getattr(trapped, entry)(bad)


@pytest.mark.parametrize("entry", ["intersect", "occluded"])
def test_tensor_refusals(trapped, entry):
    """dtype, shape, contiguity, alignment and device, each checked on a CPU tensor that is right in every other respect"""
    torch = pytest.importorskip("torch")
    call = getattr(trapped, entry)
    with pytest.raises(TypeError, match="float32"):
        call(torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        call(torch.zeros((4, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros((8, 4), dtype=torch.float32).t())
    storage = torch.zeros(33 * 8 + 1, dtype=torch.float32)
    misaligned = storage[1:1 + 32 * 8].view(32, 8)
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="aligned"):
        call(misaligned)
    with pytest.raises(ValueError, match="lives on"):
        call(torch.zeros((4, 8), dtype=torch.float32))       # a CPU tensor
