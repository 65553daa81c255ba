"""Batch.to_tensor into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are those of the DeviceBuffer form, which
tests/test_tensor_gpu.py pins; what is checked here is the plumbing: torch's current stream, a non-default stream, the checks on `out`, and that the
result is a tensor a framework takes as it is."""
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from test_scale_gpu import VUI_FULL, VUI_LIMITED, _batch, _still

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES_IN = [(200, 136), (142, 94), (64, 64)]
ENTRIES = [(0, 37, 21, 101, 77, 1), (1, 0, 0, 0, 0, 0), (2, 1, 1, 63, 63, 0), (0, 0, 0, 0, 0, 0)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TORCH_BITS = {"uint8": torch.uint8, "float32": torch.int32, "float16": torch.int16, "bfloat16": torch.int16}


def _streams():
    return [_still(1, 8, VUI_FULL if k % 2 else VUI_LIMITED, s, seed=30 + k) for k, s in enumerate(SIZES_IN)]


def _bits(t, dtype):
    a = t.contiguous().view(TORCH_BITS[dtype]).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _want(b, size, dtype, layout, filt):
    n = len(ENTRIES)
    out = DeviceBuffer(n * 3 * size[0] * size[1] * 4)
    b.to_tensor(size, ENTRIES, dtype=dtype, layout=layout, mean=MEAN, std=STD, filter=filt, out=out)
    a = b.tensor_to_host()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32", "uint8"])
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
def test_to_tensor_into_a_torch_tensor_is_the_device_buffer_result(dtype, layout):
    assert torch.cuda.is_available()
    b = _batch(_streams())
    try:
        for filt in (SCALE_BOX, SCALE_NEAREST):
            want = _want(b, (56, 40), dtype, layout, filt)
            # out=None: allocated here, on torch's current stream
            t = b.to_tensor((56, 40), ENTRIES, dtype=dtype, layout=layout, mean=MEAN, std=STD, filter=filt)
            assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype) and t.is_contiguous()
            assert tuple(t.shape) == ((4, 3, 40, 56) if layout == "NCHW" else (4, 40, 56, 3))
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(_bits(t, dtype), want), (filt, "allocated")
            assert np.array_equal(b.tensor_to_host().view(want.dtype), want)
            # a tensor the caller brings, on a stream of its own
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                out = torch.zeros(t.shape, dtype=t.dtype, device="cuda")
                ptr = out.data_ptr()
                assert b.to_tensor((56, 40), ENTRIES, dtype=dtype, layout=layout, mean=MEAN, std=STD, filter=filt, out=out) is out
            side.synchronize()
            assert out.data_ptr() == ptr and np.array_equal(_bits(out, dtype), want), (filt, "side stream")
    finally:
        b.free()


def test_a_wrong_out_is_a_python_error_before_any_launch():
    b = _batch(_streams())
    try:
        n0 = decoder.tensor_stats()
        kw = dict(dtype="float16", layout="NCHW", filter=SCALE_BOX)
        with pytest.raises(ValueError):
            b.to_tensor((56, 40), ENTRIES, out=torch.empty((4, 3, 40, 57), dtype=torch.float16, device="cuda"), **kw)          # shape
        with pytest.raises(ValueError):
            b.to_tensor((56, 40), ENTRIES, out=torch.empty((4, 40, 56, 3), dtype=torch.float16, device="cuda"), **kw)          # the other layout's shape
        with pytest.raises(ValueError):
            b.to_tensor((56, 40), ENTRIES, out=torch.empty((4, 3, 40, 56), dtype=torch.float32, device="cuda"), **kw)          # dtype
        with pytest.raises(ValueError):
            b.to_tensor((56, 40), ENTRIES, out=torch.empty((4, 3, 40, 112), dtype=torch.float16, device="cuda")[..., ::2], **kw)   # not contiguous
        with pytest.raises(TypeError):
            b.to_tensor((56, 40), ENTRIES, out=torch.empty((4, 3, 40, 56), dtype=torch.float16), **kw)                         # a host tensor
        with pytest.raises(TypeError):
            b.to_tensor((56, 40), ENTRIES, out=np.empty((4, 3, 40, 56), np.float16), **kw)
        assert decoder.tensor_stats() == n0
    finally:
        b.free()


def test_the_tensor_feeds_a_convolution_without_a_copy():
    b = _batch(_streams())
    try:
        t = b.to_tensor((56, 40), ENTRIES, dtype="float16", layout="NCHW", mean=MEAN, std=STD)
        ptr = t.data_ptr()
        weight = torch.ones((8, 3, 3, 3), dtype=torch.float16, device="cuda")
        y = torch.nn.functional.conv2d(t, weight, padding=1)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (4, 8, 40, 56) and t.data_ptr() == ptr and t.is_contiguous()
        assert bool(torch.isfinite(y).all())
        # the same numbers as a convolution over the DeviceBuffer result brought to torch by hand
        want = torch.from_numpy(_want(b, (56, 40), "float16", "NCHW", SCALE_BOX).view(np.float16)).cuda()
        assert torch.equal(torch.nn.functional.conv2d(want, weight, padding=1), y)
    finally:
        b.free()
