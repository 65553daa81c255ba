"""Resource budgets of the oriented-output kernels (color.hip), read from the gfx950 code objects in libheifhip.so the way
tests/test_tensor_kernel_resources.py does (no GPU needed).

The box form is k_tensor_box's integer stage with another store: it has to stay on that kernel's VGPR steps (256 threads = one wave per SIMD; <= 128 VGPRs
for 8-bit samples, <= 168 for 16-bit ones with their 64-bit accumulators), and its LDS - the column sums plus the stage of the quarter-turn store - has to
leave room for three workgroups in a CU's 160 KiB.  The nearest form runs in output space: no LDS, <= 80 VGPRs.  Scratch memory would be a dynamically
indexed register array: a design error."""
import re

from test_kernel_resources import _kernels

# Itanium mangling: first template argument h = unsigned char (8-bit samples), t = unsigned short (16-bit); second the dtype (hipdec_tensor_dtype)
NAME = re.compile(r"\d+(k_oriented_[a-z_]+)I([ht])Li(\d)EE")
LDS_CAP = 160 * 1024 // 3


def _oriented_kernels():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(1), m.group(2), int(m.group(3)))] = k
    return out


def test_every_oriented_kernel_is_there_and_uses_no_scratch_memory():
    ks = _oriented_kernels()
    expected = [(k, pix, dt) for k in ("k_oriented_box", "k_oriented_nearest") for pix in "ht" for dt in (0, 1, 2, 3)]     # U8, F32, F16, BF16
    assert sorted(ks) == sorted(expected)
    for key, k in ks.items():
        assert k["scratch"] == 0, key
    assert not [n for n in _kernels() if "k_oriented" in n and not NAME.search(n)], "a k_oriented_* kernel this test does not know"


def test_oriented_kernels_stay_inside_their_occupancy_steps():
    ks = _oriented_kernels()
    assert ks
    for (name, pix, dt), k in ks.items():
        if name == "k_oriented_box":
            assert 0 < k["lds"] <= LDS_CAP, (name, pix, dt, k["lds"])
            assert k["vgpr"] <= (168 if pix == "t" else 128), (name, pix, dt, k["vgpr"])
        else:
            assert k["lds"] == 0 and k["vgpr"] <= 80, (name, pix, dt, k["vgpr"])
