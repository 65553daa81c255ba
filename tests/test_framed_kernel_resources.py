"""Resource budgets of the framed tensor output's kernels (color.hip: k_frame_box, k_frame_nearest, k_frame_resample), read from the gfx950 code objects in
libheifhip.so the way tests/test_clips_kernel_resources.py does (no GPU needed).

They are the oriented / resampling kernels with a clipping store, and each has to stay on the occupancy step of the sibling it is derived from -
k_oriented_box, k_oriented_nearest, k_resample - whose figures are read from the SAME code object here, not from a constant.  A workgroup is 256 threads =
one wave per SIMD of a CU, a SIMD has 512 VGPRs per lane in granules of 8, so v VGPRs allow floor(512 / (8 * ceil(v / 8))) waves per SIMD (at most 8); LDS
allows floor(160 KiB / bytes) workgroups per CU.  Scratch memory would be a dynamically indexed register array in a streaming kernel: a design error."""
import re

from test_kernel_resources import _kernels

# Itanium mangling: first template argument h = unsigned char (8-bit samples), t = unsigned short (16-bit); second the dtype (hipdec_tensor_dtype)
NAME = re.compile(r"\d+(k_frame_[a-z_]+|k_oriented_box|k_oriented_nearest|k_resample)I([ht])Li(\d)EE")
SIBLING = {"k_frame_box": "k_oriented_box", "k_frame_nearest": "k_oriented_nearest", "k_frame_resample": "k_resample"}


def _family():
    out = {}
    for name, k in _kernels().items():
        m = NAME.search(name)
        if m:
            out[(m.group(1), m.group(2), int(m.group(3)))] = k
    return out


def vgpr_step(v):
    return min(8, 512 // (8 * ((v + 7) // 8)))


def lds_step(b):
    return 160 * 1024 // b if b else 1 << 30


def test_every_frame_kernel_is_there_and_uses_no_scratch_memory():
    ks = _family()
    frame = sorted(k for k in ks if k[0].startswith("k_frame"))
    assert frame == sorted((f, pix, dt) for f in SIBLING for pix in "ht" for dt in (0, 1, 2, 3))     # U8, F32, F16, BF16
    for key in frame:
        assert ks[key]["scratch"] == 0, key
    assert not [n for n in _kernels() if "k_frame" in n and not NAME.search(n)], "a k_frame_* kernel this test does not know"


def test_frame_kernels_stay_on_the_occupancy_steps_of_their_siblings():
    ks = _family()
    n = 0
    for (name, pix, dt), k in ks.items():
        if name not in SIBLING:
            continue
        s = ks[(SIBLING[name], pix, dt)]
        assert vgpr_step(k["vgpr"]) >= vgpr_step(s["vgpr"]), (name, pix, dt, k["vgpr"], s["vgpr"])
        assert lds_step(k["lds"]) >= lds_step(s["lds"]), (name, pix, dt, k["lds"], s["lds"])
        assert (k["lds"] == 0) == (s["lds"] == 0), (name, pix, dt)
        n += 1
    assert n == 24
