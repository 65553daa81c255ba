"""Resource budget of the warp kernels of the warped tensor output (k_warp_nearest / k_warp_bilinear / k_warp_bicubic, warp_kernels.h through color.hip),
read from the gfx950 code objects in libheifhip.so the way tests/test_placed_kernel_resources.py does (no GPU needed).

The budget is the resampler siblings': no scratch memory - a spill or a dynamically indexed register array would be a design error in a kernel whose state
is four pixels of three elements - and at most 128 VGPRs.  The kernels gather from global memory and use no LDS.

Compiled values (gfx950), VGPRs per dtype U8 / F32 / F16 / BF16, scratch 0 and LDS 0 throughout:
  k_warp_nearest   24 / 26 / 25 / 25
  k_warp_bilinear  42 / 42 / 42 / 42
  k_warp_bicubic   76 / 76 / 76 / 76     (fp64 taps of one channel at a time: the kernel loops over the channels)"""
import re

from test_kernel_resources import _kernels

NAME = re.compile(r"\d+k_warp_(nearest|bilinear|bicubic)ILi(\d)EE")   # the filter, and the template argument: the dtype (hipdec_tensor_dtype)


def _warp_kernels():
    return {(m.group(1), int(m.group(2))): k for name, k in _kernels().items() for m in [NAME.search(name)] if m}


def test_every_warp_kernel_is_there_for_the_four_dtypes():
    assert sorted(_warp_kernels()) == [(f, d) for f in ("bicubic", "bilinear", "nearest") for d in (0, 1, 2, 3)]   # U8, F32, F16, BF16
    assert not [n for n in _kernels() if "k_warp" in n and not NAME.search(n)], "a k_warp_* kernel this test does not know"


def test_the_warp_kernels_use_no_scratch_no_lds_and_at_most_128_vgprs():
    ks = _warp_kernels()
    assert ks
    for key, k in ks.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (key, k)
        assert k["vgpr"] <= 128, (key, k["vgpr"])
