"""Resource budget of the album paste kernel (transform.hip k_album_paste), read from the gfx950 code object in libheifhip.so the way
tests/test_kernel_resources.py does (no GPU needed).

A streaming copy has no business in LDS or scratch memory (scratch would be a dynamically indexed register array: a design error), and with <= 64
VGPRs a 256-thread workgroup never limits the occupancy: 8 waves per SIMD fit."""
from test_kernel_resources import _kernels


def _paste_kernels():
    return {n: k for n, k in _kernels().items() if "k_album_paste" in n}


def test_the_paste_kernel_is_there_exactly_once():
    assert len(_paste_kernels()) == 1, sorted(_paste_kernels())


def test_the_paste_kernel_uses_no_lds_no_scratch_and_few_registers():
    (name, k), = _paste_kernels().items()
    assert k["scratch"] == 0, (name, k)
    assert k["lds"] == 0, (name, k)
    assert k["vgpr"] <= 64, (name, k)
