"""Resource budget of the kernels the recipe stage adds (k_recipe_affine_nearest / _bilinear / _bicubic; recipe_kernels.h through color.hip), read from
the gfx950 code objects in libheifhip.so the way tests/test_warp_kernel_resources.py does (no GPU needed).

The budget is k_warp_*'s, whose per-pixel arithmetic (warp_pixel) the kernels call: no scratch memory, no LDS - they gather from global memory; staging
source tiles in LDS is the unmeasured candidate profiles/warp_output.txt names -, at most 128 VGPRs.

Compiled values (gfx950), VGPRs per dtype U8 / F32 / F16 / BF16, scratch 0 and LDS 0 throughout:
  k_recipe_affine_nearest   24 / 35 / 31 / 31     (the float dtypes carry both stores: U8 / NHWC of a step that is not the last, the tensor of the last)
  k_recipe_affine_bilinear  42 / 42 / 42 / 42
  k_recipe_affine_bicubic   76 / 76 / 76 / 76
k_warp_*, k_photo_* and k_augment_* keep the figures their own tests record: the stage launches them as they are."""
import re

from test_kernel_resources import _kernels

NAME = re.compile(r"\d+k_recipe_affine_(nearest|bilinear|bicubic)ILi(\d)EE")   # the filter, and the template argument: the dtype (hipdec_tensor_dtype)


def _recipe_kernels():
    return {(m.group(1), int(m.group(2))): k for name, k in _kernels().items() for m in [NAME.search(name)] if m}


def test_the_twelve_instantiations_are_there_and_no_other_recipe_kernel():
    assert sorted(_recipe_kernels()) == [(f, d) for f in ("bicubic", "bilinear", "nearest") for d in (0, 1, 2, 3)]   # U8, F32, F16, BF16
    assert not [n for n in _kernels() if "k_recipe" in n and not NAME.search(n)], "a k_recipe* kernel this test does not know"


def test_the_new_kernels_use_no_scratch_no_lds_and_at_most_128_vgprs():
    ks = _recipe_kernels()
    assert len(ks) == 12
    for key, k in ks.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (key, k)
        assert k["vgpr"] <= 128, (key, k["vgpr"])


def test_the_names_stay_clear_of_the_sibling_stages_tests():
    """tests/test_warp_kernel_resources.py, test_photo_kernel_resources.py and test_augment_kernel_resources.py fail on unknown kernels with these substrings"""
    for name in _kernels():
        if NAME.search(name):
            assert "k_warp" not in name and "k_augment" not in name and "k_photo" not in name, name
