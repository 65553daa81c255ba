"""Resource budget of the kernels of the projective tensor output (k_project_nearest / k_project_bilinear / k_project_bicubic, project_kernels.h through
color.hip), read from the gfx950 code objects in libheifhip.so the way tests/test_warp_kernel_resources.py does (no GPU needed).

The budget is k_warp_*'s, whose sampling (warp_sample) the kernels call: no scratch memory, no LDS - they gather from global memory -, at most 128 VGPRs.
What the kernels add is the coordinate function: two fp64 divisions per pixel for PERSPECTIVE, which the compiler expands in registers.

Compiled values (gfx950), VGPRs per dtype U8 / F32 / F16 / BF16, scratch 0 and LDS 0 throughout:
  k_project_nearest   42 / 42 / 42 / 42
  k_project_bilinear  48 / 48 / 48 / 48
  k_project_bicubic   82 / 82 / 82 / 82     (k_warp_bicubic: 76; fp64 taps of one channel at a time)"""
import re

from test_kernel_resources import _kernels

NAME = re.compile(r"\d+k_project_(nearest|bilinear|bicubic)ILi(\d)EE")   # the filter, and the template argument: the dtype (hipdec_tensor_dtype)


def _project_kernels():
    return {(m.group(1), int(m.group(2))): k for name, k in _kernels().items() for m in [NAME.search(name)] if m}


def test_every_project_kernel_is_there_for_the_four_dtypes():
    assert sorted(_project_kernels()) == [(f, d) for f in ("bicubic", "bilinear", "nearest") for d in (0, 1, 2, 3)]   # U8, F32, F16, BF16
    assert not [n for n in _kernels() if "k_project" in n and not NAME.search(n)], "a k_project_* kernel this test does not know"


def test_the_project_kernels_use_no_scratch_no_lds_and_at_most_128_vgprs():
    ks = _project_kernels()
    assert ks
    for key, k in ks.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (key, k)
        assert k["vgpr"] <= 128, (key, k["vgpr"])
