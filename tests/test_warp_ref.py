"""tests/warp_ref.py - the NumPy restatement of the warp stage's integer arithmetic (include/heif_hipdec.h, hipdec_tensor_warp) - against
PIL.Image.transform(size, AFFINE, data, resample, fillcolor) and PIL.Image.rotate, bit for bit: zero differing samples, no tolerance.

Sources: random pictures of 1 x 1, 1 x 9, 13 x 9 and 40 x 33.  Maps: warp_ref.map_classes - identity (which must return the source itself), integer and
half-pixel translations, scale 0.5 and 2, a negative scale, rotations about the centre by 30, -17.5 and 123.4 degrees, shear 0.3, a map whose every pixel is
outside; NEAREST takes Pillow's scale path for the maps without a1 / a3 and its fixed-point path for the others.  The centred maps must have at least half
of their output pixels inside, so that the comparison cannot pass on fill alone.

The pin holds on x86-64 builds of Pillow.  An aarch64 build may contract a * b + c to a fused multiply-add and then differ in rare last-bit cases; this
test would report that as a difference, and the library - which never contracts - would then agree with warp_ref, not with that Pillow."""
import numpy as np
import pytest

import warp_ref as wr

Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: nothing to pin tests/warp_ref.py to")

SOURCES = [(1, 1), (1, 9), (13, 9), (40, 33)]            # (width, height)
FILTERS = [wr.NEAREST, wr.BILINEAR, wr.BICUBIC]
PIL_FILTER = {wr.NEAREST: Image.NEAREST, wr.BILINEAR: Image.BILINEAR, wr.BICUBIC: Image.BICUBIC}
FILL = (7, 201, 96)


def _source(size, seed):
    return np.random.default_rng(seed).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)


def _pil(src, m, size, filt, fill=FILL):
    return np.asarray(Image.fromarray(src).transform(size, Image.AFFINE, data=tuple(float(v) for v in m), resample=PIL_FILTER[filt], fillcolor=fill))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("src_size", SOURCES)
def test_every_map_class_is_pillow_bit_for_bit(src_size, filt):
    src = _source(src_size, 11 * src_size[0] + src_size[1])
    inside_total = 0
    for size in (src_size, (7, 5)):
        for name, m, centred in wr.map_classes(src_size, size):
            assert not wr.refused(m, size), name
            got, inside = wr.warp(src, m, size, filt, FILL)
            exp = _pil(src, m, size, filt)
            assert int((got != exp).sum()) == 0, (name, src_size, size, filt, int((got != exp).sum()))
            if name == "identity" and size == src_size:
                assert inside.all() and np.array_equal(got, src), (src_size, filt)
            if name == "all_outside":
                assert not inside.any() and (got == np.asarray(FILL, np.uint8)).all()
            if centred and size == src_size:
                assert 2 * int(inside.sum()) >= inside.size, (name, src_size, filt, int(inside.sum()), inside.size)
                inside_total += int(inside.sum())
    assert inside_total > 0


def test_nearest_takes_both_of_pillows_paths():
    """the scale path (tables of truncated running sums) and the fixed-point path give different pictures for the same scale once a1 is a hair off zero"""
    src = _source((40, 33), 5)
    size = (31, 29)
    scale = wr.centred(1.37, 0.0, 0.0, 0.81, (40, 33), size)
    general = scale[:1] + (1e-9,) + scale[2:]
    for m in (scale, general):
        got, inside = wr.warp(src, m, size, wr.NEAREST, FILL)
        assert int((got != _pil(src, m, size, wr.NEAREST)).sum()) == 0
        assert 2 * int(inside.sum()) >= inside.size


@pytest.mark.parametrize("filt", FILTERS)
def test_random_maps_are_pillow_bit_for_bit(filt):
    rng = np.random.default_rng(77)
    src = _source((40, 33), 9)
    for k in range(24):
        size = (int(rng.integers(1, 48)), int(rng.integers(1, 40)))
        lin = rng.uniform(-1.6, 1.6, 4)
        m = wr.centred(lin[0], lin[1], lin[2], lin[3], (40, 33), size)
        m = (m[0], m[1], m[2] + rng.uniform(-3, 3), m[3], m[4], m[5] + rng.uniform(-3, 3))
        got, _ = wr.warp(src, m, size, filt, FILL)
        exp = _pil(src, m, size, filt)
        assert int((got != exp).sum()) == 0, (k, m, size)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("angle", [30.0, -17.5, 123.4, 90.0, 405.0])
def test_rotate_matrix_is_image_rotate(angle, filt):
    for src_size in ((13, 9), (40, 33)):
        src = _source(src_size, 3)
        m = wr.rotate_matrix(angle, src_size)
        got, _ = wr.warp(src, m, src_size, filt, FILL)
        exp = np.asarray(Image.fromarray(src).rotate(angle, resample=PIL_FILTER[filt], fillcolor=FILL))
        assert int((got != exp).sum()) == 0, (angle, src_size, filt)


def test_the_matrix_helpers_of_the_package_are_the_restatement():
    from libheif_amd import decoder
    for angle in (0.0, 30.0, -17.5, 123.4, 90.0, 405.0, -720.25):
        for size in ((13, 9), (224, 224), (1, 1)):
            assert decoder.rotate_matrix(angle, size) == wr.rotate_matrix(angle, size), (angle, size)
    for args in (dict(center=(6.5, 4.5), angle=30.0), dict(center=(112.0, 112.0), angle=-12.0, translate=(3.0, -7.5), scale=1.2, shear=(8.0, -4.0)),
                 dict(center=(0.0, 0.0), scale=0.5), dict(center=(20.0, 16.5), shear=(0.0, 15.0), translate=(1.0, 1.0))):
        np.testing.assert_allclose(decoder.affine_matrix(**args), wr.affine_matrix(**args), rtol=1e-12, atol=1e-12)
    # a rotation about the centre without shear is Pillow's rotate map up to the rounding of cos / sin to 15 places
    np.testing.assert_allclose(decoder.affine_matrix((6.5, 4.5), 30.0), wr.rotate_matrix(30.0, (13, 9)), rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        decoder.affine_matrix((0.0, 0.0), scale=0.0)


def test_the_refusals_a_map_decides():
    assert wr.refused((float("nan"), 0, 0, 0, 1, 0), (4, 4)) and wr.refused((1, 0, float("inf"), 0, 1, 0), (4, 4))
    assert wr.refused((32000.0, 0, 0, 0, 1, 0), (4, 4)) and not wr.refused((15999.0, 0, -31998.0, 0, 1, 0), (4, 4))
    assert wr.refused((1, 0, 31996.0, 0, 1, 0), (4, 4)) and not wr.refused((1, 0, 31995.5, 0, 1, 0), (4, 4))
    assert wr.refused((1, 0, 0, 0, -1, -31999.0), (4, 4))
