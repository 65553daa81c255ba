"""The definition of the framed tensor output (include/heif_hipdec.h hipdec_batch_to_tensor_framed) pinned to Pillow on the CPU tier, for code 0 and uint8:
(a) Image.new("RGB", canvas, fill) with full.crop(window).resize((w, h), F) pasted at (x, y) - x, y negative, positive or mixed; Pillow clips the paste -
against the NumPy statement the GPU tests use, "the oriented result at the rectangle's size, pasted with clipping", with tests/resample_ref.py (pinned to
PIL.Image.resize by tests/test_resample_ref.py) as the resize; and why the call exists: cropping BEFORE the resize gives other pixels at the border.
(b) the two rules of hipdec_resize_crop_place (host only) against plain Python arithmetic for a sweep of sizes, odd differences included."""
import os

import numpy as np
import pytest

import resample_ref as rr

# (picture w, h), window (left, top, w, h), canvas (w, h), rectangle (x, y, w, h)
CASES = [
    ((128, 96), (0, 0, 128, 96), (48, 40), (-8, -4, 64, 48)),          # resize, then crop: negative offsets, the rectangle covers the canvas
    ((128, 96), (16, 8, 96, 80), (33, 21), (-19, -11, 70, 44)),        # a window, all four sides overhang
    ((72, 40), (0, 0, 72, 40), (40, 40), (4, 6, 30, 17)),              # positive offsets: inside the canvas (the placed call)
    ((72, 40), (3, 1, 64, 37), (32, 32), (10, 20, 40, 30)),            # positive offsets, the rectangle leaves right and bottom
    ((41, 23), (0, 0, 41, 23), (24, 9), (-5, 2, 30, 13)),              # mixed: left overhang, margin above and below
    ((41, 23), (5, 3, 30, 19), (25, 9), (7, -6, 30, 13)),              # mixed: top overhang, margin on the left
    ((72, 40), (0, 0, 72, 40), (9, 7), (-29, -12, 30, 13)),            # one visible pixel
]
FILL = (114, 3, 250)


def framed(sample, canvas, place, fill):
    """the NumPy statement: the fill, and the sample (h, w, 3) pasted at place with clipping"""
    W, H = canvas
    x, y, w, h = place
    assert sample.shape == (h, w, 3)
    out = np.empty((H, W, 3), np.uint8)
    out[...] = np.asarray(fill, np.uint8)
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    out[y0:y1, x0:x1] = sample[y0 - y:y1 - y, x0 - x:x1 - x]
    return out


def test_the_definition_is_pillows_resize_then_paste():
    if os.path.isdir("/root/reference"):   # the development machine: skipping here would hide the pin
        import PIL   # noqa: F401
    Image = pytest.importorskip("PIL.Image")
    pil = {rr.BILINEAR: Image.BILINEAR, rr.BICUBIC: Image.BICUBIC}
    rng = np.random.default_rng(77)
    for size, win, canvas, place in CASES:
        a = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
        l, t, ww, wh = win
        x, y, w, h = place
        for f in (rr.BILINEAR, rr.BICUBIC):
            im = Image.new("RGB", canvas, FILL)
            im.paste(Image.fromarray(a).crop((l, t, l + ww, t + wh)).resize((w, h), pil[f]), (x, y))
            got = framed(rr.resample(a[t:t + wh, l:l + ww], w, h, f), canvas, place, FILL)
            assert np.array_equal(got, np.asarray(im)), (size, win, canvas, place, f)


def test_cropping_before_the_resize_is_another_operation():
    """resize((64, 48)).crop((8, 4, 56, 44)) against crop((16, 8, 112, 88)).resize((48, 40)) on a 128 x 96 picture: the pixels differ at the border only"""
    rng = np.random.default_rng(78)
    a = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    for f in (rr.BILINEAR, rr.BICUBIC):
        then_crop = framed(rr.resample(a, 64, 48, f), (48, 40), (-8, -4, 64, 48), FILL)
        crop_first = rr.resample(a[8:88, 16:112], 48, 40, f)
        differ = (then_crop != crop_first).any(axis=2)
        assert differ.any() and not differ[4:-4, 4:-4].any(), (f, int(differ.sum()))


def test_resize_crop_place_is_plain_arithmetic():
    from libheif_amd import decoder
    n = odd_down = odd_up = padded = 0
    for resize, crop in ((256, (224, 224)), (24, (16, 16)), (17, (20, 9)), (5, (8, 8))):
        for sw in range(1, 61, 1):
            for sh in range(1, 61, 3):
                short, long_ = min(sw, sh), max(sw, sh)
                w, h = (resize, resize * long_ // short) if sw <= sh else (resize * long_ // short, resize)
                exp = []
                for side, c in ((w, crop[0]), (h, crop[1])):
                    if side >= c:
                        exp.append(-round((side - c) / 2))          # Python's round(): half to even
                        odd_down += (side - c) % 4 == 1
                        odd_up += (side - c) % 4 == 3
                    else:
                        exp.append((c - side) // 2)
                        padded += 1
                assert decoder.resize_crop_place((sw, sh), resize, crop) == (exp[0], exp[1], w, h), (sw, sh, resize, crop)
                n += 1
    assert n == 4 * 60 * 20 and odd_down > 50 and odd_up > 50 and padded > 50
