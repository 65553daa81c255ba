"""Augmented tensor output into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_augment_gpu.py; what
is checked here is the plumbing: `out=` as a torch tensor on a non-default stream - one of the caller's own - feeds a convolution queued on that stream
without a synchronise in between, decoder.tensor_augment takes a uint8 torch tensor as its source, and the stage chains with decoder.tensor_warp in either
order through a U8 / NHWC tensor: both orders against tests/warp_ref.py composed with tests/augment_ref.py."""
import numpy as np
import pytest

import augment_ref as ar
import warp_ref as wr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX
from libheif_amd.decoder import SCALE_BILINEAR
from test_scale_gpu import _batch
from test_tensor_torch_gpu import ENTRIES, MEAN, STD, _bits, _streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZE = (56, 40)
CODES = (0, 3, 4, 6)
CHAINS = [[("brightness", 1.2), ("contrast", 1.3), ("color", 0.7), ("hue", 25), ("color", 0.0), ("gaussian_blur", 1.3), ("solarize", 128)],
          [("gaussian_blur", 2.0)], [], [("hue", 231), ("equalize",), ("gaussian_blur", 0.4), ("sharpness", 1.7), ("hue", 1)]]
REF_CHAINS = [[(ar.NAMES[o[0]], o[1] if len(o) > 1 else 0.0) for o in ch] for ch in CHAINS]


def test_out_on_a_side_stream_feeds_a_convolution_without_a_synchronise():
    assert torch.cuda.is_available()
    b = _batch(_streams())
    try:
        kw = dict(orientations=CODES, filter=SCALE_BOX, dtype="float16", layout="NCHW", mean=MEAN, std=STD)
        want_buf = DeviceBuffer(4 * 3 * SIZE[0] * SIZE[1] * 2)
        b.to_tensor_augmented(SIZE, CHAINS, ENTRIES, out=want_buf, **kw)
        want = torch.from_numpy(b.tensor_to_host()).cuda()
        weight = torch.ones((8, 3, 3, 3), dtype=torch.float16, device="cuda")
        want_y = torch.nn.functional.conv2d(want, weight, padding=1)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                                                   # the current stream: one of the caller's own
            out = torch.full((4, 3, SIZE[1], SIZE[0]), 3, dtype=torch.float16, device="cuda")
            ptr = out.data_ptr()
            assert b.to_tensor_augmented(SIZE, CHAINS, ENTRIES, out=out, **kw) is out
            y = torch.nn.functional.conv2d(out, weight, padding=1)                      # queued behind the stage on the same stream, no synchronise
        side.synchronize()
        assert out.data_ptr() == ptr and np.array_equal(_bits(out, "float16"), _bits(want, "float16"))
        assert torch.equal(y, want_y)
        got = b.to_tensor_augmented(SIZE, CHAINS, ENTRIES, **kw)                        # out=None: a torch tensor allocated here
        torch.cuda.current_stream().synchronize()
        assert isinstance(got, torch.Tensor) and np.array_equal(_bits(got, "float16"), _bits(want, "float16"))
    finally:
        b.free()


def test_tensor_augment_takes_a_uint8_torch_tensor():
    src = np.random.default_rng(8).integers(0, 256, (4, SIZE[1], SIZE[0], 3), dtype=np.uint8)
    t = torch.from_numpy(src).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = decoder.tensor_augment(t, CHAINS, dtype="uint8", layout="NHWC")
    side.synchronize()
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (4, SIZE[1], SIZE[0], 3)
    assert np.array_equal(out.cpu().numpy(), np.stack([ar.apply_chain(src[e], REF_CHAINS[e]) for e in range(4)]))
    assert np.array_equal(t.cpu().numpy(), src)
    with pytest.raises(TypeError):
        decoder.tensor_augment(t.to(torch.int8), CHAINS, dtype="uint8")
    with pytest.raises(ValueError):
        decoder.tensor_augment(t[:2], CHAINS, dtype="uint8")


def test_the_stage_chains_with_the_warp_in_either_order():
    src_size = (64, 48)
    src = np.random.default_rng(9).integers(0, 256, (3, src_size[1], src_size[0], 3), dtype=np.uint8)
    t = torch.from_numpy(src).cuda()
    maps = [decoder.rotate_matrix(a, SIZE) for a in (30.0, -17.5, 0.0)]
    chains, ref = CHAINS[:2] + CHAINS[3:], REF_CHAINS[:2] + REF_CHAINS[3:]
    fill = (1, 2, 3)
    # warp (U8 / NHWC out), then the augment stage
    mid = decoder.tensor_warp(t, SIZE, maps, warp_filter=SCALE_BILINEAR, fill=fill, dtype="uint8", layout="NHWC")
    out = decoder.tensor_augment(mid, chains, dtype="uint8", layout="NCHW")
    torch.cuda.current_stream().synchronize()
    want = np.stack([ar.apply_chain(wr.warp(src[e], maps[e], SIZE, SCALE_BILINEAR, fill)[0], ref[e]) for e in range(3)])
    assert np.array_equal(out.cpu().numpy(), want.transpose(0, 3, 1, 2))
    # the augment stage (U8 / NHWC out), then the warp
    mid = decoder.tensor_augment(t, chains, dtype="uint8", layout="NHWC")
    out = decoder.tensor_warp(mid, SIZE, maps, warp_filter=SCALE_BILINEAR, fill=fill, dtype="uint8", layout="NHWC")
    torch.cuda.current_stream().synchronize()
    want = np.stack([wr.warp(ar.apply_chain(src[e], ref[e]), maps[e], SIZE, SCALE_BILINEAR, fill)[0] for e in range(3)])
    assert np.array_equal(out.cpu().numpy(), want)
