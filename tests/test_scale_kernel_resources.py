"""Resource budgets of the scaling kernels (color.hip), read from the gfx950 code objects in libheifhip.so the way tests/test_kernel_resources.py does
(no GPU needed).  The box kernels stream whole planes: scratch memory there would be a design error (a dynamically indexed register array), not a
number to raise.

Where the budgets come from.  A box workgroup is 256 threads = one wave on each of a CU's four SIMDs, so workgroups per CU = waves per SIMD.  A SIMD
has 512 VGPRs per lane, handed out in granules of 8: <= 128 VGPRs give 4 waves, <= 168 give 3 (512 / 168 = 3.05), anything above 168 only 2.  LDS
(160 KB per CU) holds the column sums of the workgroup's 1024-column span - 4 KB per plane as uint32 for 8-bit samples, 8 KB as uint64 for 16-bit
ones - plus 3 KB of averages in the fused kernel: 15 KB / 27 KB, i.e. 10 / 5 workgroups, so registers are the step that counts.  8-bit fused: 4
workgroups per CU; 16-bit fused (64-bit accumulators, three planes): 3."""
import re

from test_kernel_resources import _kernels

# Itanium mangling of the first template argument: h = unsigned char (8-bit samples), t = unsigned short (16-bit)
NAME = re.compile(r"\d+(k_scale_(?:rgb|plane)_(?:box|nearest)(?:_batch)?)I([ht])(?:Li(\d)E)?E")


def _scaling_kernels():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(1), m.group(2), m.group(3))] = k
    return out


def test_every_scaling_kernel_is_there_and_uses_no_scratch_memory():
    ks = _scaling_kernels()
    layouts8, layouts16 = ("1", "2"), ("1", "2", "3", "4")       # RGB24, RGBA32 | + RRGGBB BE / LE; the planar layout has no scaled form
    expected = [(k, pix, None) for k in ("k_scale_plane_box", "k_scale_plane_nearest") for pix in "ht"]
    for k in ("k_scale_rgb_box", "k_scale_rgb_nearest", "k_scale_rgb_box_batch", "k_scale_rgb_nearest_batch"):
        expected += [(k, "h", lo) for lo in layouts8] + [(k, "t", lo) for lo in layouts16]
    assert sorted(ks, key=str) == sorted(expected, key=str)
    for key, k in ks.items():
        assert k["scratch"] == 0, key


def test_scaling_kernels_stay_inside_their_occupancy_steps():
    ks = _scaling_kernels()
    assert ks
    for (name, pix, _), k in ks.items():
        if name.startswith("k_scale_rgb_box"):
            assert k["lds"] <= (27648 if pix == "t" else 15360), (name, pix)
            assert k["vgpr"] <= (168 if pix == "t" else 128), (name, pix, k["vgpr"])
        elif name == "k_scale_plane_box":
            assert k["lds"] <= (8192 if pix == "t" else 4096) and k["vgpr"] <= 64, (name, pix)
        else:   # nearest: no LDS, 8 waves per SIMD
            assert k["lds"] == 0 and k["vgpr"] <= 64, (name, pix)
