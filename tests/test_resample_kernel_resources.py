"""Resource budgets of k_resample (color.hip: HIPDEC_SCALE_BILINEAR / _BICUBIC), read from the gfx950 code objects in libheifhip.so the way
tests/test_tensor_kernel_resources.py does (no GPU needed).

The kernel keeps 12 vertical and 3 horizontal int32 sums per thread and stages 4 x 1024 converted pixels, 4 x 64 horizontal results and the 16 x 65 output
tile in LDS: 21568 bytes.  It has to leave room for at least two workgroups in a CU's 160 KiB, stay at or below 128 VGPRs (four waves per SIMD), and use
no scratch memory - a spilled or dynamically indexed accumulator array would be a design error."""
import re

from test_kernel_resources import _kernels

# Itanium mangling: first template argument h = unsigned char (8-bit samples), t = unsigned short (16-bit); second the dtype (hipdec_tensor_dtype)
NAME = re.compile(r"\d+(k_resample)I([ht])Li(\d)EE")


def _resample_kernels():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(2), int(m.group(3)))] = k
    return out


def test_every_resample_kernel_is_there_and_uses_no_scratch_memory():
    ks = _resample_kernels()
    assert sorted(ks) == sorted((pix, dt) for pix in "ht" for dt in (0, 1, 2, 3))     # U8, F32, F16, BF16
    for key, k in ks.items():
        assert k["scratch"] == 0, key
    assert not [n for n in _kernels() if "k_resample" in n and not NAME.search(n)], "a k_resample kernel this test does not know"


def test_resample_kernels_stay_inside_their_occupancy_steps():
    ks = _resample_kernels()
    assert ks
    for key, k in ks.items():
        assert 0 < k["lds"] <= 160 * 1024 // 2, (key, k["lds"])
        assert k["vgpr"] <= 128, (key, k["vgpr"])
