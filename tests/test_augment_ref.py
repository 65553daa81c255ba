"""tests/augment_ref.py - the NumPy restatement of the augment stage's two own operations (include/heif_hipdec.h, hipdec_tensor_augment) - against Pillow
itself, bit for bit: convert("HSV") and convert("RGB") from HSV over all 2^24 inputs each, the hue shift as torchvision's PIL adjust_hue performs it,
ImageFilter.GaussianBlur over sizes from 1 x 1 and radii either side of the steps of the box's whole radius, and chains of 1 .. 8 mixed operations as
successive Pillow calls.  Zero differing samples, no tolerance.

The pin holds on x86-64 builds of Pillow, which do not contract a * b + c (tests/test_photo_ref.py says the same of the photo stage)."""
import numpy as np
import pytest

import augment_ref as ar
import photo_ref as pr

Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: nothing to pin tests/augment_ref.py to")
from PIL import ImageFilter   # noqa: E402
from test_photo_ref import pil_op as pil_photo_op   # noqa: E402

SIZES = [(1, 1), (1, 7), (5, 1), (3, 3), (7, 9), (33, 20), (100, 37)]                                              # width x height
RADII = [0, 0.1, 0.3, 0.5, 0.75, 1.0, 1.37, 1.41, 1.42, 2.0, 2.44, 2.45, 3.3, 5.0, 8.0]
SHIFTS = [0, 1, 43, 128, 213, 255]


def pil_hue(S, d):
    h, s, v = Image.fromarray(S).convert("HSV").split()
    nh = np.array(h, np.uint8)
    with np.errstate(over="ignore"):
        nh = (nh + np.uint8(d)).astype(np.uint8)                     # the uint8 wrap-around add
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))


def pil_op(S, op, value):
    if op == ar.HUE:
        return pil_hue(S, int(value))
    if op == ar.GAUSSIAN_BLUR:
        return np.asarray(Image.fromarray(S).filter(ImageFilter.GaussianBlur(value)))
    return pil_photo_op(S, op, value)


def _all_colours(chunk):
    """chunk c of 16 of the 2^24 triples, as a 1024 x 1024 picture"""
    v = np.arange(chunk << 20, (chunk + 1) << 20, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(1024, 1024, 3)


def test_both_hsv_conversions_over_all_inputs():
    for chunk in range(16):
        T = _all_colours(chunk)
        exp = np.asarray(Image.fromarray(T, "RGB").convert("HSV"))
        assert int((ar.rgb2hsv(T) != exp).sum()) == 0, chunk
        exp = np.asarray(Image.fromarray(T, "HSV").convert("RGB"))
        assert int((ar.hsv2rgb(T) != exp).sum()) == 0, chunk


@pytest.mark.parametrize("d", SHIFTS)
def test_the_hue_shift_is_pillow_bit_for_bit(d):
    for k, size in enumerate(SIZES):
        S = np.random.default_rng(100 * d + k).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
        assert np.array_equal(ar.apply_op(S, ar.HUE, d), pil_hue(S, d)), (d, size)
    S = np.random.default_rng(d).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    if d == 0:
        grey = np.repeat(S[..., :1], 3, axis=2)
        assert np.array_equal(ar.apply_op(grey, ar.HUE, 77), grey)      # S = 0: the hue is not read


def _blur_pictures():
    out = []
    for k, size in enumerate(SIZES):
        out.append(np.random.default_rng(k).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8))
    step = np.zeros((16, 16, 3), np.uint8)
    step[:, 8:] = 255                                                    # half black, half white
    out.append(step)
    return out


@pytest.mark.parametrize("radius", RADII)
def test_the_blur_is_pillow_bit_for_bit(radius):
    for S in _blur_pictures():
        got, exp = ar.apply_op(S, ar.GAUSSIAN_BLUR, radius), pil_op(S, ar.GAUSSIAN_BLUR, radius)
        assert got.dtype == np.uint8 and got.shape == S.shape
        assert int((got != exp).sum()) == 0, (radius, S.shape, int((got != exp).sum()))


def test_the_box_parameters():
    assert ar.gaussian_box(0) == (0, 1 << 24, 0)
    S = np.random.default_rng(1).integers(0, 256, (9, 7, 3), dtype=np.uint8)
    assert np.array_equal(ar.gaussian_blur(S, 0), S)
    rs = [ar.gaussian_box(x)[0] for x in RADII]
    assert rs == sorted(rs) and rs[0] == 0 and rs[-1] == 7
    assert ar.gaussian_box(1.41)[0] == 0 and ar.gaussian_box(1.42)[0] == 1 and ar.gaussian_box(2.44)[0] == 1 and ar.gaussian_box(2.45)[0] == 2
    for x in RADII:
        r, ww, fw = ar.gaussian_box(x)
        assert (2 * r + 1) * ww + 2 * fw <= 1 << 24 and ww * (2 * r + 1) * 255 + fw * 510 + (1 << 23) < 1 << 32


def test_hue_shift_is_truncation_then_mod_256():
    assert [ar.hue_shift(f) for f in (0.0, 0.5, -0.5, 0.1, -0.1, 0.004, -0.004)] == [0, 127, 129, 25, 231, 1, 255]


def random_chain(rng, n):
    chain = []
    for _ in range(n):
        op = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, ar.HUE, ar.HUE, ar.GAUSSIAN_BLUR, ar.GAUSSIAN_BLUR]))
        if op == pr.POSTERIZE:
            v = int(rng.integers(0, 9))
        elif op == pr.SOLARIZE:
            v = float(rng.uniform(0, 256))
        elif op == ar.HUE:
            v = int(rng.integers(0, 256))
        elif op == ar.GAUSSIAN_BLUR:
            v = float(rng.uniform(0, 8))
        else:
            v = float(rng.uniform(-0.5, 2.5))
        chain.append((op, v))
    return chain


@pytest.mark.parametrize("size", [(1, 1), (5, 1), (7, 9), (33, 20)], ids=lambda s: "%dx%d" % s)
def test_chains_are_successive_pillow_calls(size):
    rng = np.random.default_rng(5 * size[0] + size[1])
    S = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    for k in range(16):
        chain = random_chain(rng, 1 + k % ar.MAX_OPS)
        exp = S
        for op, v in chain:
            exp = pil_op(exp, op, v)
        assert np.array_equal(ar.apply_chain(S, chain), exp), chain


def test_the_refusals_an_operation_decides():
    assert ar.refused(0, 1.0) and ar.refused(10, 1.0) and ar.refused(15, 0) and ar.refused(18, 0) and not ar.refused(pr.INVERT, 0)
    assert ar.refused(ar.HUE, 0.5) and ar.refused(ar.HUE, -1) and ar.refused(ar.HUE, 256) and ar.refused(ar.HUE, float("nan")) and not ar.refused(ar.HUE, 255)
    assert ar.refused(ar.GAUSSIAN_BLUR, -0.1) and ar.refused(ar.GAUSSIAN_BLUR, 8.01) and ar.refused(ar.GAUSSIAN_BLUR, float("inf"))
    assert not ar.refused(ar.GAUSSIAN_BLUR, 0) and not ar.refused(ar.GAUSSIAN_BLUR, 8.0)
