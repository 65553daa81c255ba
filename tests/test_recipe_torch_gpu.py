"""Recipe tensor output into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_recipe_gpu.py; what is
checked here is the plumbing: `out=` as a torch tensor on a non-default stream - one of the caller's own - feeds a convolution queued on that stream
without a synchronise in between, and decoder.tensor_recipe takes a uint8 torch tensor as its source, its result against tests/recipe_ref.py."""
import numpy as np
import pytest

import recipe_ref as rr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR
from test_scale_gpu import _batch
from test_tensor_torch_gpu import ENTRIES, MEAN, STD, _bits, _streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZE = (56, 40)
CODES = (0, 3, 4, 6)
MEAN_FILL = (124, 116, 104)                                                                # a dataset mean, as timm fills
CHAINS = [[("affine", decoder.rotate_matrix(30.0, SIZE), SCALE_BICUBIC, MEAN_FILL), ("color", 1.4)],
          [("posterize", 4), ("affine", decoder.shear_matrix(0.3, 0), SCALE_BILINEAR, MEAN_FILL)],
          [("affine", decoder.shear_matrix(0, -0.2), SCALE_BILINEAR, MEAN_FILL), ("affine", decoder.translate_matrix(-9, 0), SCALE_NEAREST, MEAN_FILL)],
          [("contrast", 1.5), ("affine", decoder.translate_matrix(0, 6.5), SCALE_BICUBIC, 0), ("gaussian_blur", 1.0), ("hue", 40)]]
REF_CHAINS = [[(rr.AFFINE,) + o[1:] if o[0] == "affine" else (decoder.RECIPE_OPS[o[0]], o[1]) for o in ch] for ch in CHAINS]


def test_out_on_a_side_stream_feeds_a_convolution_without_a_synchronise():
    assert torch.cuda.is_available()
    b = _batch(_streams())
    try:
        kw = dict(orientations=CODES, filter=SCALE_BOX, dtype="float16", layout="NCHW", mean=MEAN, std=STD)
        want_buf = DeviceBuffer(4 * 3 * SIZE[0] * SIZE[1] * 2)
        b.to_tensor_recipe(SIZE, CHAINS, ENTRIES, out=want_buf, **kw)
        want = torch.from_numpy(b.tensor_to_host()).cuda()
        weight = torch.ones((8, 3, 3, 3), dtype=torch.float16, device="cuda")
        want_y = torch.nn.functional.conv2d(want, weight, padding=1)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                                                   # the current stream: one of the caller's own
            out = torch.full((4, 3, SIZE[1], SIZE[0]), 3, dtype=torch.float16, device="cuda")
            ptr = out.data_ptr()
            assert b.to_tensor_recipe(SIZE, CHAINS, ENTRIES, out=out, **kw) is out
            y = torch.nn.functional.conv2d(out, weight, padding=1)                      # queued behind the stage on the same stream, no synchronise
        side.synchronize()
        assert out.data_ptr() == ptr and np.array_equal(_bits(out, "float16"), _bits(want, "float16"))
        assert torch.equal(y, want_y)
        got = b.to_tensor_recipe(SIZE, CHAINS, ENTRIES, **kw)                           # out=None: a torch tensor allocated here
        torch.cuda.current_stream().synchronize()
        assert isinstance(got, torch.Tensor) and np.array_equal(_bits(got, "float16"), _bits(want, "float16"))
    finally:
        b.free()


def test_tensor_recipe_takes_a_uint8_torch_tensor_and_writes_one_on_the_current_stream():
    src = np.random.default_rng(8).integers(0, 256, (4, SIZE[1], SIZE[0], 3), dtype=np.uint8)
    want = np.stack([rr.apply_chain(src[e], REF_CHAINS[e]) for e in range(4)])
    t = torch.from_numpy(src).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = decoder.tensor_recipe(t, CHAINS, dtype="uint8", layout="NHWC")
        given = torch.zeros((4, 3, SIZE[1], SIZE[0]), dtype=torch.uint8, device="cuda")
        assert decoder.tensor_recipe(t, CHAINS, dtype="uint8", layout="NCHW", out=given) is given
    side.synchronize()
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (4, SIZE[1], SIZE[0], 3)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(given.cpu().numpy(), want.transpose(0, 3, 1, 2))
    assert np.array_equal(t.cpu().numpy(), src)
    with pytest.raises(TypeError):
        decoder.tensor_recipe(t.to(torch.int8), CHAINS, dtype="uint8")
    with pytest.raises(ValueError):
        decoder.tensor_recipe(t[:2], CHAINS, dtype="uint8")
