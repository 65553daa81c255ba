"""Resource budget of the margin kernel of the placed tensor output (k_canvas_margin, color.hip), read from the gfx950 code objects in libheifhip.so the
way tests/test_oriented_kernel_resources.py does (no GPU needed).

The kernel only stores: it has no use for LDS, scratch memory would be a dynamically indexed register array (a design error), and 64 VGPRs is the step at
which 8 waves per SIMD fit in the 512-register file - a store-only kernel has no reason to leave it."""
import re

from test_kernel_resources import _kernels

NAME = re.compile(r"\d+k_canvas_marginILi(\d)EE")          # the template argument: the dtype (hipdec_tensor_dtype)


def _margin_kernels():
    return {int(m.group(1)): k for name, k in _kernels().items() for m in [NAME.search(name)] if m}


def test_the_margin_kernel_is_there_for_the_four_dtypes():
    assert sorted(_margin_kernels()) == [0, 1, 2, 3]        # U8, F32, F16, BF16
    assert not [n for n in _kernels() if "k_canvas" in n and not NAME.search(n)], "a k_canvas_* kernel this test does not know"


def test_the_margin_kernel_uses_no_lds_no_scratch_and_at_most_64_vgprs():
    ks = _margin_kernels()
    assert ks
    for dt, k in ks.items():
        assert k["lds"] == 0 and k["scratch"] == 0, (dt, k)
        assert k["vgpr"] <= 64, (dt, k["vgpr"])
