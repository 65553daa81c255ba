"""Packed tensor output into a torch tensor (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_packed_gpu.py; what is
checked here is the plumbing: `out=` as a 1-D torch tensor on torch's current stream - one of the caller's own - and that the packed sequence is a
tensor a framework takes as it is: the view [tokens, 3 * P * P] of it, no copy, feeds torch.nn.functional.linear (a patch embedding) and equals the host
expectation - the existing to_tensor at each sample's size, put into token order by the header's index formulas."""
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX
from test_packed_gpu import place_sample
from test_scale_gpu import _batch
from test_tensor_torch_gpu import ENTRIES, MEAN, STD, _bits, _streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P, M = 4, 2
SIZES = [(40, 24), (24, 56), (8, 8), (64, 48)]            # displayed sizes, multiples of P * M
CODES = (0, 1, 6, 3)


def test_the_packed_sequence_in_a_torch_tensor_feeds_a_linear_layer_without_a_copy():
    assert torch.cuda.is_available()
    b = _batch(_streams())
    try:
        kw = dict(dtype="float16", layout="NCHW", mean=MEAN, std=STD, filter=SCALE_BOX)
        offsets, tokens, total = decoder.packed_layout(SIZES, P, M)
        want = np.zeros(total, np.uint16)
        for e, (size, off) in enumerate(zip(SIZES, offsets)):                              # the existing call, one sample at a time
            buf = DeviceBuffer(3 * size[0] * size[1] * 2)
            b.to_tensor(size, [ENTRIES[e]], out=buf, orientations=(CODES[e],), **kw)
            place_sample(want, off, b.tensor_to_host().view(np.uint16)[0], P, M, "NCHW")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                                                      # the current stream: one of the caller's own
            out = torch.full((total + 32,), 3.0, dtype=torch.float16, device="cuda")
            got, offs, grids = b.to_tensor_packed(SIZES, ENTRIES, patch=P, merge=M, orientations=CODES, out=out, **kw)
            assert got is out and offs == offsets and grids == [(h // P, w // P) for w, h in SIZES]
            seq = out[:total].view(sum(tokens), 3 * P * P)
            assert seq.data_ptr() == out.data_ptr() and seq.is_contiguous()               # a view, not a copy
            weight = torch.linspace(-1, 1, 8 * 3 * P * P, device="cuda").reshape(8, 3 * P * P).to(torch.float16)
            emb = torch.nn.functional.linear(seq, weight)
            ref = torch.nn.functional.linear(torch.from_numpy(want.view(np.float16)).to("cuda").view(sum(tokens), 3 * P * P), weight)
        side.synchronize()
        assert np.array_equal(_bits(seq, "float16").ravel(), want)
        assert bool((out[total:] == 3.0).all()), "elements behind the sequence were written"
        assert emb.shape == (sum(tokens), 8) and torch.equal(emb, ref)
        assert np.array_equal(b.tensor_packed_to_host().view(np.uint16).ravel(), want)
        # out=None: a 1-D torch tensor allocated here
        got, offs, _ = b.to_tensor_packed(SIZES, ENTRIES, patch=P, merge=M, orientations=CODES, **kw)
        torch.cuda.current_stream().synchronize()
        assert isinstance(got, torch.Tensor) and got.shape == (total,) and np.array_equal(_bits(got, "float16"), want)
        with pytest.raises(ValueError):
            b.to_tensor_packed(SIZES, ENTRIES, patch=P, merge=M, out=torch.empty((2, total), dtype=torch.float16, device="cuda"), **kw)       # not 1-D
        with pytest.raises(ValueError):
            b.to_tensor_packed(SIZES, ENTRIES, patch=P, merge=M, out=torch.empty((total,), dtype=torch.float32, device="cuda"), **kw)         # dtype
        with pytest.raises(TypeError):
            b.to_tensor_packed(SIZES, ENTRIES, patch=P, merge=M, out=torch.empty((total,), dtype=torch.float16), **kw)                        # a host tensor
    finally:
        b.free()
