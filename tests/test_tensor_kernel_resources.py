"""Resource budgets of the tensor-output kernels (color.hip), read from the gfx950 code objects in libheifhip.so the way tests/test_kernel_resources.py
does (no GPU needed).

The box form is the fused box kernel of the scaled output with a window and another store path, and it has to stay on that kernel's occupancy steps
(tests/test_scale_kernel_resources.py derives them): a workgroup is 256 threads = one wave per SIMD, <= 128 VGPRs give 4 workgroups per CU (8-bit
samples), <= 168 give 3 (16-bit samples, 64-bit accumulators); LDS is the same 15 KB / 27 KB.  Scratch memory would be a dynamically indexed register
array in a streaming kernel: a design error.  The nearest form reads only the sampled pixels: no LDS; its registers allow 6 waves per SIMD (<= 80)."""
import re

from test_kernel_resources import _kernels

# Itanium mangling: first template argument h = unsigned char (8-bit samples), t = unsigned short (16-bit); second the dtype (hipdec_tensor_dtype)
NAME = re.compile(r"\d+(k_tensor_[a-z_]+)I([ht])Li(\d)EE")


def _tensor_kernels():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(1), m.group(2), int(m.group(3)))] = k
    return out


def test_every_tensor_kernel_is_there_and_uses_no_scratch_memory():
    ks = _tensor_kernels()
    expected = [(k, pix, dt) for k in ("k_tensor_box", "k_tensor_nearest") for pix in "ht" for dt in (0, 1, 2, 3)]     # U8, F32, F16, BF16
    assert sorted(ks) == sorted(expected)
    for key, k in ks.items():
        assert k["scratch"] == 0, key
    assert not [n for n in _kernels() if "k_tensor" in n and not NAME.search(n)], "a k_tensor_* kernel this test does not know"


def test_tensor_kernels_stay_inside_their_occupancy_steps():
    ks = _tensor_kernels()
    assert ks
    for (name, pix, dt), k in ks.items():
        if name == "k_tensor_box":
            assert k["lds"] <= (27648 if pix == "t" else 15360), (name, pix, dt, k["lds"])
            assert k["vgpr"] <= (168 if pix == "t" else 128), (name, pix, dt, k["vgpr"])
        else:
            assert k["lds"] == 0 and k["vgpr"] <= 80, (name, pix, dt, k["vgpr"])
