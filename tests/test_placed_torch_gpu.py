"""Placed tensor output into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_placed_gpu.py; what is
checked here is the plumbing - `out=` and `mask=` as torch tensors on torch's current stream, equal to torch.nn.functional.pad of what the existing
to_tensor writes at the rectangle's size - and the one path of the margin kernel a small canvas cannot reach: an entry of more than 2^31 elements, whose
blocks are indexed with 64 bits."""
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from test_scale_gpu import _batch
from test_tensor_torch_gpu import ENTRIES, MEAN, STD, _bits, _streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANVAS, RECT = (56, 40), (5, 3, 40, 28)
CODES = (0, 2, 4, 6)                                       # rows stay rows: every sample is 40 x 28, so one pad describes all four


@pytest.mark.parametrize("dtype,layout,fill", [("float16", "NCHW", 0.5), ("uint8", "NHWC", 7)])
def test_out_and_mask_as_torch_tensors_equal_a_padded_to_tensor(dtype, layout, fill):
    assert torch.cuda.is_available()
    F = torch.nn.functional
    x, y, w, h = RECT
    l, r, t, b_ = x, CANVAS[0] - x - w, y, CANVAS[1] - y - h
    b = _batch(_streams())
    try:
        for filt in (SCALE_BOX, SCALE_NEAREST):
            kw = dict(dtype=dtype, layout=layout, mean=MEAN, std=STD, filter=filt, orientations=CODES)
            sample = b.to_tensor((w, h), ENTRIES, **kw)                                     # the existing call, at the rectangle's size
            torch.cuda.current_stream().synchronize()
            want = F.pad(sample, (l, r, t, b_) if layout == "NCHW" else (0, 0, l, r, t, b_), value=fill)
            want_mask = F.pad(torch.zeros((4, h, w), dtype=torch.uint8, device="cuda"), (l, r, t, b_), value=1)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):                                                   # the current stream: one of the caller's own
                out = torch.full(want.shape, 3, dtype=want.dtype, device="cuda")
                mask = torch.full((4, CANVAS[1], CANVAS[0]), 9, dtype=torch.uint8, device="cuda")
                ptr = out.data_ptr()
                assert b.to_tensor(CANVAS, ENTRIES, places=[RECT] * 4, fill=fill, fill_domain="element", out=out, mask=mask, **kw) is out
            side.synchronize()
            assert out.data_ptr() == ptr and np.array_equal(_bits(out, dtype), _bits(want, dtype)), (filt, "side stream")
            assert torch.equal(mask, want_mask)
            assert np.array_equal(b.tensor_mask_to_host(), want_mask.cpu().numpy())
            # out=None and mask=True: both allocated here, as torch tensors
            got = b.to_tensor(CANVAS, ENTRIES, places=[RECT] * 4, fill=fill, fill_domain="element", mask=True, **kw)
            torch.cuda.current_stream().synchronize()
            assert isinstance(got, torch.Tensor) and np.array_equal(_bits(got, dtype), _bits(want, dtype))
            assert np.array_equal(b.tensor_mask_to_host(), want_mask.cpu().numpy())
        with pytest.raises(ValueError):
            b.to_tensor(CANVAS, ENTRIES, places=[RECT] * 4, dtype=dtype, layout=layout, mask=torch.empty((4, 40, 57), dtype=torch.uint8, device="cuda"))
        with pytest.raises(TypeError):
            b.to_tensor(CANVAS, ENTRIES, places=[RECT] * 4, dtype=dtype, layout=layout, mask=torch.empty((4, 40, 56), dtype=torch.int8, device="cuda"))
    finally:
        b.free()


def test_an_entry_of_more_than_2_to_the_31_elements():
    """3 * 26760 * 26760 = 2 148 292 800 elements: past 2^31, where the margin kernel indexes its blocks with 64 bits.  Everything is compared on the device."""
    W = H = 26760
    assert 3 * W * H > 2 ** 31
    x, y, w, h = W - 21, H - 13, 16, 9
    b = _batch(_streams()[:1])
    try:
        kw = dict(dtype="uint8", layout="NCHW", filter=SCALE_BOX, orientations=(1,))
        sample = b.to_tensor((w, h), [(0, 0, 0, 0, 0, 0)], **kw)
        out = torch.full((1, 3, H, W), 0xA5, dtype=torch.uint8, device="cuda")
        mask = torch.full((1, H, W), 0xA5, dtype=torch.uint8, device="cuda")
        b.to_tensor((W, H), [(0, 0, 0, 0, 0, 0)], places=[(x, y, w, h)], fill=(1, 2, 3), out=out, mask=mask, **kw)
        torch.cuda.current_stream().synchronize()
        assert torch.equal(out[:, :, y:y + h, x:x + w], sample)
        assert not bool(mask[:, y:y + h, x:x + w].any())
        mask[:, y:y + h, x:x + w] = 1
        assert bool((mask == 1).all())
        for c in range(3):
            out[0, c, y:y + h, x:x + w] = c + 1
            assert bool((out[0, c] == c + 1).all()), c
    finally:
        b.free()
