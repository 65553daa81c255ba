"""Projective tensor output into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_project_gpu.py; what
is checked here is the plumbing: `out=` as a torch tensor on a stream of the caller's own feeds a convolution queued on that stream without a synchronise in
between and gives what the DeviceBuffer result gives, and decoder.tensor_project takes a uint8 torch tensor as its source."""
import numpy as np
import pytest

import project_ref as pr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR
from test_scale_gpu import _batch
from test_tensor_torch_gpu import ENTRIES, MEAN, STD, _bits, _streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZE, SRC = (56, 40), (64, 48)
CODES = (0, 3, 4, 6)


def _maps():
    """two PERSPECTIVE maps (one from four point pairs), two QUAD maps (one from four corners): both kinds in one call"""
    cls = dict((n, (k, m)) for n, k, m in pr.map_classes(SRC, SIZE))
    corners = [(0.0, 0.0), (SIZE[0] - 1.0, 0.0), (SIZE[0] - 1.0, SIZE[1] - 1.0), (0.0, SIZE[1] - 1.0)]
    start = [(3.0, 2.0), (60.0, 5.0), (57.0, 44.0), (1.0, 40.0)]
    return [cls["perspective_keystone_both"], decoder.perspective_map(start, corners), cls["quad_jittered"],
            decoder.quad_map([(2.0, 1.0), (5.0, 46.0), (61.0, 44.0), (63.0, 3.0)], SIZE)]


def test_out_on_a_side_stream_feeds_a_convolution_without_a_synchronise():
    assert torch.cuda.is_available()
    b = _batch(_streams())
    try:
        kw = dict(src_size=SRC, warp_filter=SCALE_BILINEAR, fill=114, orientations=CODES, filter=SCALE_BOX, dtype="float16", layout="NCHW", mean=MEAN, std=STD)
        want_buf = DeviceBuffer(4 * 3 * SIZE[0] * SIZE[1] * 2)
        b.to_tensor_projected(SIZE, _maps(), ENTRIES, out=want_buf, **kw)
        want = torch.from_numpy(b.tensor_to_host()).cuda()
        weight = torch.ones((8, 3, 3, 3), dtype=torch.float16, device="cuda")
        want_y = torch.nn.functional.conv2d(want, weight, padding=1)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                                                   # the current stream: one of the caller's own
            out = torch.full((4, 3, SIZE[1], SIZE[0]), 3, dtype=torch.float16, device="cuda")
            ptr = out.data_ptr()
            assert b.to_tensor_projected(SIZE, _maps(), ENTRIES, out=out, **kw) is out
            y = torch.nn.functional.conv2d(out, weight, padding=1)                      # queued behind the projection on the same stream, no synchronise
        side.synchronize()
        assert out.data_ptr() == ptr and np.array_equal(_bits(out, "float16"), _bits(want, "float16"))
        assert torch.equal(y, want_y)
        got = b.to_tensor_projected(SIZE, _maps(), ENTRIES, **kw)                       # out=None: a torch tensor allocated here
        torch.cuda.current_stream().synchronize()
        assert isinstance(got, torch.Tensor) and np.array_equal(_bits(got, "float16"), _bits(want, "float16"))
    finally:
        b.free()


@pytest.mark.parametrize("wf", [0, SCALE_BILINEAR, SCALE_BICUBIC])
def test_tensor_project_takes_a_uint8_torch_tensor(wf):
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (4, SRC[1], SRC[0], 3), dtype=np.uint8)
    maps = _maps()
    flat = [(m.kind, tuple(m.a)) if isinstance(m, decoder.TensorProjection) else m for m in maps]
    assert not any(pr.refused(m, k, SIZE) for k, m in flat)
    t = torch.from_numpy(src).cuda()
    out = decoder.tensor_project(t, SIZE, maps, warp_filter=wf, fill=(1, 2, 3), dtype="uint8", layout="NHWC")
    torch.cuda.current_stream().synchronize()
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (4, SIZE[1], SIZE[0], 3)
    want = np.stack([pr.project(src[e], flat[e][1], flat[e][0], SIZE, wf, (1, 2, 3))[0] for e in range(4)])
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(TypeError):
        decoder.tensor_project(t.to(torch.int8), SIZE, maps, dtype="uint8")
    with pytest.raises(ValueError):
        decoder.tensor_project(t[:2], SIZE, maps, dtype="uint8")
