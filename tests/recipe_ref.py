"""The recipe stage (include/heif_hipdec.h, hipdec_tensor_recipe) restated: a chain whose steps are the augment stage's operations or an affine
transform, each applied to the 8-bit result of the step before.  Pure composition of two restatements that are pinned to Pillow on their own:
tests/augment_ref.py (apply_op: opcodes 1 .. 9, 16, 17; tests/test_augment_ref.py, tests/test_photo_ref.py) and tests/warp_ref.py (warp:
PIL.Image.transform(size, AFFINE, data, resample, fillcolor); tests/test_warp_ref.py).  tests/test_recipe_ref.py pins the composition to Pillow.

A step is (op, value) as augment_ref takes it, or an affine step: (AFFINE, map, filter, fill) with the record in the step itself, or (AFFINE, index) into
`affines`, a sequence of (map, filter, fill) - the form the C interface has.  fill: three integers 0 .. 255, or one for all channels.

Nothing in this file comes from the library under test."""
import numpy as np

import augment_ref
import warp_ref

AFFINE = 32
MAX_OPS = augment_ref.MAX_OPS
NEAREST, BILINEAR, BICUBIC = warp_ref.NEAREST, warp_ref.BILINEAR, warp_ref.BICUBIC
FILTERS = (NEAREST, BILINEAR, BICUBIC)


def fill3(fill):
    return (int(fill),) * 3 if isinstance(fill, (int, np.integer)) else tuple(int(v) for v in fill)


def affine_of(step, affines=None):
    """(map, filter, fill) of an affine step"""
    if len(step) == 2:
        m, filt, fill = affines[int(step[1])]
    else:
        m, filt, fill = step[1], (step[2] if len(step) > 2 else BILINEAR), (step[3] if len(step) > 3 else 0)
    return tuple(float(v) for v in m), int(filt), fill3(fill)


def is_affine(step):
    return not isinstance(step, (str, int)) and step[0] == AFFINE


def refused(m, filt, fill, size):
    """what hipdec_tensor_recipe refuses of an affine record for samples of size = (w, h)"""
    return warp_ref.refused(m, size) or filt not in FILTERS or any(v < 0 or v > 255 for v in fill3(fill))


def apply_chain(S, chain, affines=None):
    assert len(chain) <= MAX_OPS
    S = np.ascontiguousarray(S, np.uint8)
    h, w = S.shape[:2]
    for step in chain:
        if is_affine(step):
            m, filt, fill = affine_of(step, affines)
            assert not refused(m, filt, fill, (w, h)), step
            S = warp_ref.warp(S, m, (w, h), filt, fill)[0]
        else:
            op, value = (step, 0.0) if isinstance(step, (str, int)) else (step[0], step[1] if len(step) > 1 else 0.0)
            S = augment_ref.apply_op(S, op, value)
    return np.ascontiguousarray(S, np.uint8)


def shear_matrix(sx, sy=0.0):
    return (1.0, float(sx), 0.0, float(sy), 1.0, 0.0)


def translate_matrix(tx, ty=0.0):
    return (1.0, 0.0, float(tx), 0.0, 1.0, float(ty))
