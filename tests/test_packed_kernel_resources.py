"""Resource budgets of the patch-sequence kernels of the packed tensor output (color.hip: k_patch_box, k_patch_nearest, k_patch_resample), read from the
gfx950 code objects in libheifhip.so the way tests/test_tensor_kernel_resources.py does (no GPU needed).

They are the dense siblings' integer stages with the blocked store, and the budgets are the siblings': the box form at most 128 VGPRs for 8-bit samples
and 168 for 16-bit ones with LDS for three workgroups in a CU's 160 KiB; the resampler at most 128 VGPRs and 80 KiB of LDS; the nearest form no LDS and
at most 80 VGPRs (compiled: 62 - 75; the blocked addressing fits, the 96 the issue allowed is not needed).  No kernel uses scratch memory."""
import re

from test_kernel_resources import _kernels

# Itanium mangling: first template argument h = unsigned char (8-bit samples), t = unsigned short (16-bit); second the dtype (hipdec_tensor_dtype)
NAME = re.compile(r"\d+(k_patch_[a-z_]+)I([ht])Li(\d)EE")
FAMILIES = ("k_patch_box", "k_patch_nearest", "k_patch_resample")


def _patch_kernels():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(1), m.group(2), int(m.group(3)))] = k
    return out


def test_every_patch_kernel_is_there_and_uses_no_scratch_memory():
    ks = _patch_kernels()
    expected = [(k, pix, dt) for k in FAMILIES for pix in "ht" for dt in (0, 1, 2, 3)]     # U8, F32, F16, BF16
    assert sorted(ks) == sorted(expected)
    for key, k in ks.items():
        assert k["scratch"] == 0, key
    assert not [n for n in _kernels() if "k_patch" in n and not NAME.search(n)], "a k_patch_* kernel this test does not know"


def test_patch_kernels_stay_inside_the_budgets_of_their_dense_siblings():
    ks = _patch_kernels()
    assert ks
    for (name, pix, dt), k in ks.items():
        if name == "k_patch_box":
            assert 0 < k["lds"] <= 160 * 1024 // 3, (name, pix, dt, k["lds"])
            assert k["vgpr"] <= (168 if pix == "t" else 128), (name, pix, dt, k["vgpr"])
        elif name == "k_patch_resample":
            assert 0 < k["lds"] <= 80 * 1024, (name, pix, dt, k["lds"])
            assert k["vgpr"] <= 128, (name, pix, dt, k["vgpr"])
        else:
            assert k["lds"] == 0 and k["vgpr"] <= 80, (name, pix, dt, k["vgpr"])
