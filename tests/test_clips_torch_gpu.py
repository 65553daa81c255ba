"""Clip tensors into torch tensors (GPU only: the emulator tier has no torch device).  The bytes are pinned by tests/test_clips_gpu.py; what is checked
here is the plumbing: `out=` as a torch tensor on torch's current stream - one of the caller's own - and that the results are tensors a framework takes as
they are: N x C x T x H x W float16 feeds torch.nn.functional.conv3d without a copy, the token sequence with a temporal patch, viewed
[tokens, 3 * 2 * P * P], feeds a linear layer, and both hold the bytes of the DeviceBuffer form of the same call."""
import numpy as np
import pytest

from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX
from libheif_amd.decoder import Clips, clip_packed_layout, uniform_frames
from test_clips_gpu import MAIN, N, track
from test_tensor_torch_gpu import MEAN, STD, _bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENTRIES = [(0, 0, 0, 0, 0, 0), (1, 3, 5, 101, 77, 1), (0, 37, 21, 64, 40, 0)]
T = 4
KW = dict(dtype="float16", mean=MEAN, std=STD, filter=SCALE_BOX)


def test_clips_in_torch_tensors_feed_conv3d_and_a_linear_layer_without_a_copy():
    assert torch.cuda.is_available()
    c = Clips([track(n)[0] for n in MAIN])
    try:
        c.run()
        c.status()
        frames = [uniform_frames(c.frame_count(e[0]), T, stride=2 + k, start=k) for k, e in enumerate(ENTRIES)]
        assert frames[2] == [2, 6, N - 1, N - 1]                                          # (repeat_last past the end of the track)
        W, H = 32, 24
        # the DeviceBuffer form of the same calls
        buf = DeviceBuffer(len(ENTRIES) * 3 * T * H * W * 2)
        c.to_tensor((W, H), T, ENTRIES, frames, order="CTHW", out=buf, **KW)
        want = c.tensor_to_host().view(np.uint16)
        assert want.shape == (len(ENTRIES), 3, T, H, W)
        P, M, TP = 4, 2, 2
        sizes = [(40, 24), (24, 56), (8, 8)]
        offsets, tokens, total = clip_packed_layout(sizes, T, P, M, TP)
        assert tokens == [(T // TP) * (w // P) * (h // P) for w, h in sizes] and total == sum(3 * T * w * h for w, h in sizes)
        tbuf = DeviceBuffer(total * 2)
        c.to_tokens(sizes, T, ENTRIES, frames, P, merge=M, temporal_patch=TP, out=tbuf, **KW)
        want_tokens = c.tensor_to_host().view(np.uint16)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):                                                      # the current stream: one of the caller's own
            out = torch.full((len(ENTRIES), 3, T, H, W), 3.0, dtype=torch.float16, device="cuda")
            got = c.to_tensor((W, H), T, ENTRIES, frames, order="CTHW", out=out, **KW)
            assert got is out and out.is_contiguous()
            weight = torch.linspace(-1, 1, 8 * 3 * 2 * 3 * 3, device="cuda").reshape(8, 3, 2, 3, 3).to(torch.float16)
            feat = torch.nn.functional.conv3d(out, weight, stride=(2, 1, 1))               # N C T H W as it is
            seq_buf = torch.full((total + 32,), 3.0, dtype=torch.float16, device="cuda")
            got, offs, grids = c.to_tokens(sizes, T, ENTRIES, frames, P, merge=M, temporal_patch=TP, out=seq_buf, **KW)
            assert got is seq_buf and offs == offsets and grids == [(T // TP, h // P, w // P) for w, h in sizes]
            seq = seq_buf[:total].view(sum(tokens), 3 * TP * P * P)
            assert seq.data_ptr() == seq_buf.data_ptr() and seq.is_contiguous()            # a view, not a copy
            lw = torch.linspace(-1, 1, 16 * 3 * TP * P * P, device="cuda").reshape(16, 3 * TP * P * P).to(torch.float16)
            emb = torch.nn.functional.linear(seq, lw)
            emb_ref = torch.nn.functional.linear(torch.from_numpy(want_tokens.view(np.float16)).to("cuda").view(sum(tokens), 3 * TP * P * P), lw)
        side.synchronize()
        assert np.array_equal(_bits(out, "float16"), want)
        assert feat.shape == (len(ENTRIES), 8, 2, H - 2, W - 2) and bool(torch.isfinite(feat).all())   # (its input is pinned byte for byte above)
        assert np.array_equal(_bits(seq, "float16").ravel(), want_tokens)
        assert bool((seq_buf[total:] == 3.0).all()), "elements behind the sequence were written"
        assert emb.shape == (sum(tokens), 16) and torch.equal(emb, emb_ref)
        # out=None: a torch tensor allocated here, of the order's shape
        got = c.to_tensor((W, H), T, ENTRIES, frames, order="THWC", **KW)
        torch.cuda.current_stream().synchronize()
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == (len(ENTRIES), T, H, W, 3)
        with pytest.raises(ValueError):
            c.to_tensor((W, H), T, ENTRIES, frames, order="CTHW", out=torch.empty((len(ENTRIES), T, 3, H, W), dtype=torch.float16, device="cuda"), **KW)   # shape
        with pytest.raises(TypeError):
            c.to_tensor((W, H), T, ENTRIES, frames, order="CTHW", out=torch.empty((len(ENTRIES), 3, T, H, W), dtype=torch.float16), **KW)                  # a host tensor
    finally:
        c.free()
