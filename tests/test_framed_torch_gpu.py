"""Framed tensor output into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_framed_gpu.py; what is
checked here is the plumbing - `out=` and `mask=` as torch tensors on torch's current stream, equal to the slice of what the existing oriented to_tensor
writes at the full rectangle's size: the resize-then-crop a host does in two steps without the call."""
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC
from test_scale_gpu import _batch
from test_tensor_torch_gpu import ENTRIES, MEAN, STD, _bits, _streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANVAS = (24, 24)
CODES = (0, 2, 4, 6)                                       # every entry is resized to the same rectangle (the rule applied to item 0): one slice describes all four


@pytest.mark.parametrize("dtype,layout", [("float16", "NCHW"), ("uint8", "NHWC")])
def test_out_and_mask_as_torch_tensors_equal_the_slice_of_the_full_size_result(dtype, layout):
    assert torch.cuda.is_available()
    b = _batch(_streams())
    try:
        d = b.info(0)
        frame = decoder.resize_crop_place((d["width"], d["height"]), 28, CANVAS)      # Resize(28) -> CenterCrop(24)
        x, y, w, h = frame
        assert x < 0 and y < 0 and min(w, h) == 28
        for filt in (SCALE_BOX, SCALE_NEAREST, SCALE_BICUBIC):
            kw = dict(dtype=dtype, layout=layout, mean=MEAN, std=STD, filter=filt, orientations=CODES)
            full = b.to_tensor((w, h), ENTRIES, **kw)                                       # the existing call, at the rectangle's size
            torch.cuda.current_stream().synchronize()
            want = (full[:, :, -y:-y + CANVAS[1], -x:-x + CANVAS[0]] if layout == "NCHW" else full[:, -y:-y + CANVAS[1], -x:-x + CANVAS[0], :]).contiguous()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):                                                   # the current stream: one of the caller's own
                out = torch.full(want.shape, 3, dtype=want.dtype, device="cuda")
                mask = torch.full((4, CANVAS[1], CANVAS[0]), 9, dtype=torch.uint8, device="cuda")
                ptr = out.data_ptr()
                assert b.to_tensor(CANVAS, ENTRIES, frames=[frame] * 4, out=out, mask=mask, **kw) is out
            side.synchronize()
            assert out.data_ptr() == ptr and np.array_equal(_bits(out, dtype), _bits(want, dtype)), (filt, "side stream")
            assert not bool(mask.any())                                                     # the resized sample covers the canvas
            # out=None and mask=True: both allocated here, as torch tensors; a rectangle that leaves a margin on the right and below
            shifted = (x, y, CANVAS[0] - 5 - x, CANVAS[1] - 3 - y)
            full = b.to_tensor(shifted[2:], ENTRIES, **kw)
            got = b.to_tensor(CANVAS, ENTRIES, frames=[shifted] * 4, fill=0.5 if dtype != "uint8" else 7, fill_domain="element", mask=True, **kw)
            torch.cuda.current_stream().synchronize()
            assert isinstance(got, torch.Tensor)
            g = got if layout == "NCHW" else got.permute(0, 3, 1, 2)
            f = full if layout == "NCHW" else full.permute(0, 3, 1, 2)
            assert torch.equal(g[:, :, :CANVAS[1] - 3, :CANVAS[0] - 5], f[:, :, -y:, -x:])
            assert bool((g[:, :, CANVAS[1] - 3:, :] == (0.5 if dtype != "uint8" else 7)).all()) and bool((g[:, :, :, CANVAS[0] - 5:] == (0.5 if dtype != "uint8" else 7)).all())
            m = b.tensor_mask_to_host()
            assert not m[:, :CANVAS[1] - 3, :CANVAS[0] - 5].any() and m[:, CANVAS[1] - 3:, :].all() and m[:, :, CANVAS[0] - 5:].all()
        with pytest.raises(ValueError):
            b.to_tensor(CANVAS, ENTRIES, frames=[frame] * 4, places=[(0, 0) + CANVAS] * 4, dtype=dtype, layout=layout)
    finally:
        b.free()
