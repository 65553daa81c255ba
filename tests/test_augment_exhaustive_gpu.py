"""HUE on the device over every colour: the 4096 x 4096 sample that holds all 2^24 (R, G, B) triples goes through hipdec_tensor_augment with the shifts
0 and 85 as two entries, uint8 NHWC, and must equal tests/augment_ref.py - which tests/test_augment_ref.py pins to Pillow's convert("HSV") and
convert("RGB") over the same 2^24 inputs - bit for bit.  Shift 0 is the plain HSV round trip (not the identity: H, S are 8-bit); 85 moves every hue a
third of the circle, so every branch of hsv2rgb is taken from every branch of rgb2hsv.

Device only (`-m gpu`): it is not given to the emulator, where 16 M pixels under coroutine lanes would take minutes.  The expected side is about 12 s of
NumPy, in 16 slices of 2^20 pixels to bound its memory; the device side is milliseconds."""
import numpy as np
import pytest

import augment_ref as ar
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer

pytestmark = pytest.mark.gpu

SHIFTS = (0, 85)
SIDE = 4096
POISON = 0xA5


def test_hue_over_all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    sample = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(SIDE, SIDE, 3)
    del v
    src = np.stack([sample] * len(SHIFTS))
    nbytes = src.size
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    sbuf = DeviceBuffer.from_numpy(src)
    s0 = decoder.augment_stats()
    got = decoder.tensor_augment(sbuf, [[(ar.HUE, d)] for d in SHIFTS], src_size=(SIDE, SIDE), dtype="uint8", layout="NHWC", out=out, to_host=True)
    s1 = decoder.augment_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, len(SHIFTS), 1)
    assert got.shape == (len(SHIFTS), SIDE, SIDE, 3) and got.dtype == np.uint8
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    rows = SIDE // 16
    for k in range(16):
        part = sample[k * rows:(k + 1) * rows]
        hsv = ar.rgb2hsv(part)
        for e, d in enumerate(SHIFTS):
            shifted = hsv.copy()
            shifted[..., 0] = ((hsv[..., 0].astype(np.int32) + d) & 255).astype(np.uint8)
            exp = ar.hsv2rgb(shifted)
            bad = int((got[e, k * rows:(k + 1) * rows] != exp).sum())
            assert bad == 0, (d, k, bad)
    assert not np.array_equal(got[0], sample) and not np.array_equal(got[1], got[0])
