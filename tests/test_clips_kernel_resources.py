"""Resource budgets of the strided box kernel of the clip output (k_clip_box, color.hip), read from the gfx950 code objects in libheifhip.so the way
tests/test_tensor_kernel_resources.py does (no GPU needed).

k_clip_box is k_tensor_box's integer stage with the oriented store's row pitch and plane stride, and it has to stay on that kernel's occupancy steps: a
workgroup is 256 threads = one wave per SIMD, <= 128 VGPRs give 4 workgroups per CU (8-bit samples), <= 168 give 3 (16-bit samples, 64-bit accumulators);
LDS is the same 15 KB / 27 KB - no second stage as k_oriented_box has one.  Scratch memory would be a dynamically indexed register array in a streaming
kernel: a design error."""
import re

from test_kernel_resources import _kernels

# Itanium mangling: first template argument h = unsigned char (8-bit samples), t = unsigned short (16-bit); second the dtype (hipdec_tensor_dtype)
NAME = re.compile(r"\d+(k_clip_box)I([ht])Li(\d)EE")


def _clip_kernels():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(2), int(m.group(3)))] = k
    return out


def test_all_eight_instantiations_are_there_and_use_no_scratch_memory():
    ks = _clip_kernels()
    assert sorted(ks) == sorted((pix, dt) for pix in "ht" for dt in (0, 1, 2, 3))     # U8, F32, F16, BF16
    for key, k in ks.items():
        assert k["scratch"] == 0, key
    assert not [n for n in _kernels() if "k_clip" in n and not NAME.search(n)], "a k_clip_* kernel this test does not know"


def test_the_kernel_stays_inside_the_occupancy_steps_of_the_unoriented_box_kernel():
    ks = _clip_kernels()
    assert ks
    for (pix, dt), k in ks.items():
        assert k["lds"] <= (27648 if pix == "t" else 15360), (pix, dt, k["lds"])
        assert k["vgpr"] <= (168 if pix == "t" else 128), (pix, dt, k["vgpr"])
