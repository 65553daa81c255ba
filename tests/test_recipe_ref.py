"""tests/recipe_ref.py - the composition of tests/augment_ref.py and tests/warp_ref.py that states the recipe stage (include/heif_hipdec.h,
hipdec_tensor_recipe) - against Pillow itself, bit for bit: chains drawn with a fixed seed from all twelve kinds of operation (the nine photometric ones,
hue, Gaussian blur, the affine transform with its three filters and the maps of warp_ref.map_classes) as successive Pillow calls - Image.transform,
ImageEnhance.*, ImageOps.*, convert("HSV"), ImageFilter.GaussianBlur.  Zero differing samples, no tolerance.

Contrast and Equalize directly behind a rotation with a fill that is not black: their statistics include the fill pixels, which is why an interleaved
chain is not the warp stage followed by the colour stage.  The two map helpers the recipe adds to libheif_amd.decoder (shear_matrix, translate_matrix) are
the literal tuples timm and torchvision hand to Image.transform.

The pin holds on x86-64 builds of Pillow, which do not contract a * b + c (tests/test_warp_ref.py says the same of the warp stage)."""
import numpy as np
import pytest

import augment_ref as ar
import photo_ref as pr
import recipe_ref as rr
import warp_ref as wr

Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: nothing to pin tests/recipe_ref.py to")
from test_augment_ref import pil_op, random_chain   # noqa: E402
from test_warp_ref import PIL_FILTER                 # noqa: E402

SIZES = [(1, 1), (5, 1), (7, 9), (33, 20), (65, 17)]    # width x height
FILL = (3, 114, 250)


def pil_affine(S, m, filt, fill):
    size = (S.shape[1], S.shape[0])
    return np.asarray(Image.fromarray(S).transform(size, Image.AFFINE, data=tuple(float(v) for v in m), resample=PIL_FILTER[filt], fillcolor=tuple(fill)))


def pil_chain(S, chain, affines=None):
    for step in chain:
        if rr.is_affine(step):
            S = pil_affine(S, *rr.affine_of(step, affines))
        else:
            S = pil_op(S, step[0], step[1])
    return S


def random_recipe(rng, n, size):
    """n steps: an affine step with probability 5 / 14 - the share of the geometric operations in RandAugment's list -, else one of the eleven colour kinds"""
    maps = wr.map_classes(size, size)
    chain = []
    for _ in range(n):
        if rng.uniform() < 5.0 / 14.0:
            name, m, _centred = maps[int(rng.integers(0, len(maps)))]
            filt = int(rng.choice(rr.FILTERS))
            fill = tuple(int(v) for v in rng.integers(0, 256, 3))
            chain.append((rr.AFFINE, m, filt, fill))
        else:
            chain.extend(random_chain(rng, 1))
    return chain


def drawn(size):
    """the sample and the 24 chains of 1 .. 8 steps of a size, from a fixed seed"""
    rng = np.random.default_rng(31 * size[0] + size[1])
    S = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    return S, [random_recipe(rng, 1 + k % rr.MAX_OPS, size) for k in range(24)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_chains_of_all_twelve_kinds_are_successive_pillow_calls(size):
    S, chains = drawn(size)
    for chain in chains:
        assert np.array_equal(rr.apply_chain(S, chain), pil_chain(S, chain)), chain


def test_the_drawn_chains_hold_every_kind_and_every_filter():
    """(every map class with every filter: test_every_map_class_between_two_colour_steps)"""
    steps = [s for size in SIZES for chain in drawn(size)[1] for s in chain]
    kinds = {(s[0], s[2]) if rr.is_affine(s) else (s[0],) for s in steps}
    assert kinds == {(op,) for op in list(range(1, 10)) + [ar.HUE, ar.GAUSSIAN_BLUR]} | {(rr.AFFINE, f) for f in rr.FILTERS}, kinds


@pytest.mark.parametrize("filt", rr.FILTERS)
def test_every_map_class_between_two_colour_steps(filt):
    size = (33, 20)
    S = np.random.default_rng(filt).integers(0, 256, (20, 33, 3), dtype=np.uint8)
    for name, m, _centred in wr.map_classes(size, size):
        chain = [(pr.COLOR, 1.4), (rr.AFFINE, m, filt, FILL), (ar.GAUSSIAN_BLUR, 1.5)]
        assert np.array_equal(rr.apply_chain(S, chain), pil_chain(S, chain)), (name, filt)


@pytest.mark.parametrize("op", [pr.CONTRAST, pr.EQUALIZE, pr.AUTOCONTRAST])
def test_statistics_behind_a_rotation_include_the_fill(op):
    size = (33, 20)
    S = np.random.default_rng(9).integers(40, 200, (20, 33, 3), dtype=np.uint8)
    m = wr.rotate_matrix(30.0, size)
    value = 1.6 if op == pr.CONTRAST else 0.0
    results = []
    for fill in ((255, 255, 255), (0, 0, 0), FILL):
        chain = [(rr.AFFINE, m, rr.BILINEAR, fill), (op, value)]
        got = rr.apply_chain(S, chain)
        assert np.array_equal(got, pil_chain(S, chain)), (op, fill)
        results.append(got)
    inside = wr.warp(S, m, size, rr.BILINEAR)[1]
    assert 0 < int(inside.sum()) < inside.size
    assert not np.array_equal(results[0][inside], results[1][inside]), "the fill does not reach the statistics: the case shows nothing"
    # ... and the order matters: the colour step first is another picture
    swapped = rr.apply_chain(S, [(op, value), (rr.AFFINE, m, rr.BILINEAR, FILL)])
    assert np.array_equal(swapped, pil_chain(S, [(op, value), (rr.AFFINE, m, rr.BILINEAR, FILL)]))
    assert not np.array_equal(swapped, results[2])


def test_indexed_affine_steps_read_the_records():
    size = (7, 9)
    S = np.random.default_rng(2).integers(0, 256, (9, 7, 3), dtype=np.uint8)
    affines = [(wr.rotate_matrix(-17.5, size), rr.BICUBIC, 9), (rr.translate_matrix(2, -1), rr.NEAREST, FILL)]
    chain = [(rr.AFFINE, 1), (pr.INVERT, 0), (rr.AFFINE, 0), (rr.AFFINE, 1)]
    inline = [(rr.AFFINE,) + affines[1], (pr.INVERT, 0), (rr.AFFINE,) + affines[0], (rr.AFFINE,) + affines[1]]
    assert np.array_equal(rr.apply_chain(S, chain, affines), pil_chain(S, inline))
    assert rr.refused(affines[0][0], 3, 0, size) and rr.refused(affines[0][0], 1, 0, size) and rr.refused(affines[0][0], rr.NEAREST, (0, 256, 0), size)
    assert rr.refused((1, 0, 32000.0, 0, 1, 0), rr.NEAREST, 0, size) and not rr.refused(*affines[1], size)


def test_the_two_map_helpers_are_the_literal_tuples():
    from libheif_amd import decoder
    S = np.random.default_rng(4).integers(0, 256, (20, 33, 3), dtype=np.uint8)
    im = Image.fromarray(S)
    for v in (0.3, -0.3, 0.0, 0.123456789):
        assert decoder.shear_matrix(v, 0) == (1, v, 0, 0, 1, 0) == rr.shear_matrix(v, 0)
        assert decoder.shear_matrix(0, v) == (1, 0, 0, v, 1, 0) == rr.shear_matrix(0, v)
        for filt in rr.FILTERS:
            for m, literal in ((decoder.shear_matrix(v, 0), (1, v, 0, 0, 1, 0)), (decoder.shear_matrix(0, v), (1, 0, 0, v, 1, 0))):
                exp = np.asarray(im.transform(im.size, Image.AFFINE, literal, resample=PIL_FILTER[filt], fillcolor=FILL))
                assert np.array_equal(rr.apply_chain(S, [(rr.AFFINE, m, filt, FILL)]), exp), (v, filt)
    for px in (10, -10, 0, 3.5):
        assert decoder.translate_matrix(px, 0) == (1, 0, px, 0, 1, 0) == rr.translate_matrix(px, 0)
        assert decoder.translate_matrix(0, px) == (1, 0, 0, 0, 1, px) == rr.translate_matrix(0, px)
        for filt in rr.FILTERS:
            for m, literal in ((decoder.translate_matrix(px, 0), (1, 0, px, 0, 1, 0)), (decoder.translate_matrix(0, px), (1, 0, 0, 0, 1, px))):
                exp = np.asarray(im.transform(im.size, Image.AFFINE, literal, resample=PIL_FILTER[filt], fillcolor=FILL))
                assert np.array_equal(rr.apply_chain(S, [(rr.AFFINE, m, filt, FILL)]), exp), (px, filt)
    assert all(isinstance(v, float) for v in decoder.shear_matrix(1, 2) + decoder.translate_matrix(3, 4))
