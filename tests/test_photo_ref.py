"""tests/photo_ref.py - the NumPy restatement of the photometric stage (include/heif_hipdec.h, hipdec_tensor_photo) - against Pillow itself, bit for bit:
ImageEnhance.Brightness / Color / Contrast / Sharpness, ImageOps.posterize / solarize / invert / autocontrast / equalize, and chains as successive Pillow
calls.  Zero differing samples, no tolerance.

Pictures: random, flat, a narrow value range, two-valued; sizes 1 x 1, 1 x 5, 5 x 1, 2 x 2, 3 x 3 and 33 x 17 (width x height).  Factors: 0, 1, values
between, above 1, negative, and one random double per case.

The pin holds on x86-64 builds of Pillow, which do not contract a * b + c (tests/test_warp_ref.py says the same of the warp)."""
import numpy as np
import pytest

import photo_ref as pr

Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: nothing to pin tests/photo_ref.py to")
from PIL import ImageEnhance, ImageOps   # noqa: E402

SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (33, 17)]
KINDS = ["random", "flat", "narrow", "two_valued"]
FACTORS = [0.0, 1.0, 0.3, 0.5, 0.999, 1.3, 1.9, 7.25, -0.5, -3.0]
ENHANCE = {pr.BRIGHTNESS: ImageEnhance.Brightness, pr.COLOR: ImageEnhance.Color, pr.CONTRAST: ImageEnhance.Contrast, pr.SHARPNESS: ImageEnhance.Sharpness}


def picture(kind, size, seed):
    rng = np.random.default_rng(seed)
    shape = (size[1], size[0], 3)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), shape).copy()
    if kind == "narrow":
        return rng.integers(100, 104, shape, dtype=np.uint8)
    return rng.choice(np.array([17, 230], np.uint8), shape)


def pil_op(S, op, value):
    im = Image.fromarray(S)
    if op in ENHANCE:
        im = ENHANCE[op](im).enhance(value)
    elif op == pr.POSTERIZE:
        im = ImageOps.posterize(im, int(value))
    elif op == pr.SOLARIZE:
        im = ImageOps.solarize(im, value)
    elif op == pr.INVERT:
        im = ImageOps.invert(im)
    elif op == pr.AUTOCONTRAST:
        im = ImageOps.autocontrast(im)
    else:
        im = ImageOps.equalize(im)
    return np.asarray(im)


def _same(S, op, value):
    got, exp = pr.apply_op(S, op, value), pil_op(S, op, value)
    assert got.dtype == np.uint8 and got.shape == S.shape
    assert int((got != exp).sum()) == 0, (op, value, S.shape, int((got != exp).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_enhancers_are_pillow_bit_for_bit(size, kind):
    S = picture(kind, size, 31 * size[0] + size[1])
    rng = np.random.default_rng(size[0] + 7 * size[1] + len(kind))
    for op in ENHANCE:
        for f in FACTORS + [float(rng.uniform(-2.0, 3.0))]:
            _same(S, op, f)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_image_ops_are_pillow_bit_for_bit(size, kind):
    S = picture(kind, size, 17 * size[0] + size[1])
    rng = np.random.default_rng(size[0] + 5 * size[1] + len(kind))
    for bits in range(0, 9):
        _same(S, pr.POSTERIZE, bits)
    for t in (0, 1, 17, 100.5, 102, 128, 230, 255, 256, -4, float(rng.uniform(0, 256))):
        _same(S, pr.SOLARIZE, t)
    for op in (pr.INVERT, pr.AUTOCONTRAST, pr.EQUALIZE):
        _same(S, op, 0.0)


def test_equalize_at_the_step_thresholds():
    """w * h - H[last] at 254 (step 0: identity), 255, 256 (step 1) and 509 .. 511 (step 1, 2, 2)"""
    for rest in (254, 255, 256, 509, 510, 511):
        rng = np.random.default_rng(rest)
        vals = np.concatenate([rng.integers(0, 200, rest), np.full(600 - rest, 200)]).astype(np.uint8)
        S = np.stack([rng.permutation(vals) for _ in range(3)], axis=-1).reshape(20, 30, 3)
        _same(S, pr.EQUALIZE, 0.0)
        assert (np.array_equal(pr.apply_op(S, pr.EQUALIZE), S)) == (rest < 255)


def test_contrast_rounds_a_mean_of_exactly_one_half_up():
    S = np.array([[[10, 10, 10], [11, 11, 11]]], np.uint8)
    assert pr.contrast_mean(21, 2) == 11
    _same(S, pr.CONTRAST, 0.0)
    assert (pr.apply_op(S, pr.CONTRAST, 0.0) == 11).all()


def test_color_zero_is_convert_l():
    S = picture("random", (33, 17), 4)
    L = np.asarray(Image.fromarray(S).convert("L"))
    assert np.array_equal(pr.apply_op(S, pr.COLOR, 0.0), np.repeat(L[..., None], 3, axis=2))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_chains_are_successive_pillow_calls(size):
    rng = np.random.default_rng(5 * size[0] + size[1])
    S = picture("random", size, 3)
    fixed = [[(pr.BRIGHTNESS, 0.6), (pr.CONTRAST, 1.4)], [(pr.POSTERIZE, 3), (pr.EQUALIZE, 0)], [(pr.SHARPNESS, 1.8), (pr.AUTOCONTRAST, 0)],
             [(pr.COLOR, 0.0), (pr.SOLARIZE, 128), (pr.INVERT, 0), (pr.SHARPNESS, 0.0)], []]
    for k in range(12):
        chain = fixed[k] if k < len(fixed) else []
        if k >= len(fixed):
            for _ in range(int(rng.integers(1, pr.MAX_OPS + 1))):
                op = int(rng.integers(1, 10))
                chain.append((op, int(rng.integers(0, 9)) if op == pr.POSTERIZE else float(rng.uniform(0, 256) if op == pr.SOLARIZE else rng.uniform(-0.5, 2.5))))
        exp = S
        for op, v in chain:
            exp = pil_op(exp, op, v)
        assert np.array_equal(pr.apply_chain(S, chain), exp), chain


def test_the_refusals_an_operation_decides():
    assert pr.refused(0, 1.0) and pr.refused(10, 1.0) and pr.refused(pr.BRIGHTNESS, float("nan")) and pr.refused(pr.COLOR, float("inf"))
    assert pr.refused(pr.CONTRAST, 65536.5) and not pr.refused(pr.CONTRAST, -65536.0)
    assert pr.refused(pr.POSTERIZE, 2.5) and pr.refused(pr.POSTERIZE, 9) and pr.refused(pr.POSTERIZE, -1) and not pr.refused(pr.POSTERIZE, 0)
