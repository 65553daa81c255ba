"""Resource budget of the two kernels the augment stage adds (k_augment_hue, k_augment_blur; augment_kernels.h through color.hip), read from the gfx950
code objects in libheifhip.so the way tests/test_photo_kernel_resources.py does (no GPU needed).

The budget: no scratch memory, at most 128 VGPRs, and the LDS the design states: k_augment_hue none - it is point-wise -;
k_augment_blur two buffers of the staged tile, rows x pitch bytes each, for boxes of whole radius up to RMAX = 1, 3, 7: the tile is 64 x 32, the halo
3 (RMAX + 1) pixels, the columns widened to a multiple of four on each side, the pitch the row's dwords made odd:
  RMAX 1: 2 x 44 x 244 = 21 472 B;  RMAX 3: 2 x 56 x 268 = 30 016 B;  RMAX 7: 2 x 80 x 340 = 54 400 B.
k_photo_hist and k_photo_apply keep the figures tests/test_photo_kernel_resources.py records: the stage launches them as they are."""
import re

from test_kernel_resources import _kernels

HUE = re.compile(r"\d+k_augment_hueILi(\d)EE")              # the template argument: the dtype (hipdec_tensor_dtype)
BLUR = re.compile(r"\d+k_augment_blurILi(\d)ELi(\d)EE")     # the dtype, RMAX
APPLY = re.compile(r"\d+k_photo_applyILi(\d)EE")
HIST = re.compile(r"\d+k_photo_histE")


def _blur_lds(rmax):
    halo = 3 * (rmax + 1)
    cols, rows = 64 + 2 * ((halo + 3) & ~3), 32 + 2 * halo
    pitch = 4 * (((cols * 3 + 3) // 4) | 1)
    return 2 * rows * pitch


def test_the_stated_lds_is_what_the_formula_gives():
    assert [_blur_lds(r) for r in (1, 3, 7)] == [21472, 30016, 54400]
    assert all(((_blur_lds(r) // 2 // (32 + 6 * (r + 1))) // 4) % 2 == 1 for r in (1, 3, 7))   # an odd number of dwords per row


def test_both_new_kernels_are_there_for_the_four_dtypes():
    names = _kernels()
    assert sorted(int(m.group(1)) for n in names for m in [HUE.search(n)] if m) == [0, 1, 2, 3]
    assert sorted((int(m.group(1)), int(m.group(2))) for n in names for m in [BLUR.search(n)] if m) == [(d, r) for d in range(4) for r in (1, 3, 7)]
    assert not [n for n in names if "k_augment" in n and not HUE.search(n) and not BLUR.search(n)], "a k_augment_* kernel this test does not know"


def test_the_new_kernels_use_no_scratch_at_most_128_vgprs_and_the_lds_the_design_states():
    for name, k in _kernels().items():
        if HUE.search(name):
            assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, (name, k)
        m = BLUR.search(name)
        if m:
            assert k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)
            assert k["lds"] == _blur_lds(int(m.group(2))), (name, k["lds"])


def test_the_photo_kernels_are_unchanged():
    """the figures of tests/test_photo_kernel_resources.py's docstring, exactly"""
    ks = _kernels()
    apply = {int(m.group(1)): k for n, k in ks.items() for m in [APPLY.search(n)] if m}
    hist = [k for n, k in ks.items() if HIST.search(n)]
    assert len(hist) == 1 and (hist[0]["vgpr"], hist[0]["lds"], hist[0]["scratch"]) == (31, 16384, 0)
    assert [apply[d]["vgpr"] for d in range(4)] == [30, 35, 32, 32]
    assert all(apply[d]["lds"] == 12560 and apply[d]["scratch"] == 0 for d in range(4))
