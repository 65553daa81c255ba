"""Resource budget of the kernels of the photometric tensor output (k_photo_hist, k_photo_apply; photo_kernels.h through color.hip), read from the gfx950
code objects in libheifhip.so the way tests/test_warp_kernel_resources.py does (no GPU needed).

The budget: no scratch memory - a spill or a dynamically indexed register array would be a design error in kernels whose state is four pixels of three
components -, at most 128 VGPRs, and the LDS the design states: k_photo_hist four wave copies of four 256-bin uint32 histograms, 16 KiB;
k_photo_apply 6 KiB for the two buffers of the three-channel prefix sums, 2 KiB for the 64-bit weighted sum, 768 B of tables, 18 x 66 x 3 = 3564 B for
the SHARPNESS tile with its halo and 36 B for the first / last non-zero bins: 12 560 B.

Compiled values (gfx950), scratch 0 throughout:
  k_photo_hist    31 VGPRs, 16 384 B LDS
  k_photo_apply   30 / 35 / 32 / 32 VGPRs for U8 / F32 / F16 / BF16, 12 560 B LDS"""
import re

from test_kernel_resources import _kernels

APPLY = re.compile(r"\d+k_photo_applyILi(\d)EE")   # the template argument: the dtype (hipdec_tensor_dtype)
HIST = re.compile(r"\d+k_photo_histE")
HIST_LDS = 4 * 4 * 256 * 4
APPLY_LDS = 2 * 3 * 256 * 4 + 256 * 8 + 3 * 256 + 18 * 66 * 3 + 9 * 4


def _apply_kernels():
    return {int(m.group(1)): k for name, k in _kernels().items() for m in [APPLY.search(name)] if m}


def _hist_kernels():
    return [k for name, k in _kernels().items() if HIST.search(name)]


def test_every_photo_kernel_is_there_for_its_dtypes():
    assert sorted(_apply_kernels()) == [0, 1, 2, 3]   # U8, F32, F16, BF16
    assert len(_hist_kernels()) == 1
    assert not [n for n in _kernels() if "k_photo" in n and not APPLY.search(n) and not HIST.search(n)], "a k_photo_* kernel this test does not know"


def test_the_photo_kernels_use_no_scratch_at_most_128_vgprs_and_the_lds_the_design_states():
    ks = _apply_kernels()
    assert ks
    for key, k in ks.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (key, k)
        assert 0 < k["lds"] <= APPLY_LDS, (key, k["lds"])
    for k in _hist_kernels():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, k
        assert 0 < k["lds"] <= HIST_LDS, k["lds"]
