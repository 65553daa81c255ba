"""Resource budget of the cover kernel of the composed tensor output (k_compose_cover, color.hip), read from the gfx950 code objects in libheifhip.so the
way tests/test_placed_kernel_resources.py does (no GPU needed).

The kernel is k_canvas_margin with a cover table in place of the one rectangle: it only stores and reads a few table words, so it has no use for LDS (the
table is read from global memory; no staging was built), and scratch memory would be a dynamically indexed register array - a design error.  Its name does
not begin with k_canvas_: tests/test_placed_kernel_resources.py pins that family to the margin kernel alone.  The k_frame_* kernels that write the pieces
are not touched by the composed call - tests/test_framed_kernel_resources.py holds their figures as it stands.  The VGPR count and its occupancy step
against k_canvas_margin's are reported in profiles/composed_output.txt, not asserted."""
import re

from test_kernel_resources import _kernels

NAME = re.compile(r"\d+k_compose_coverILi(\d)EE")         # the template argument: the dtype (hipdec_tensor_dtype)
MARGIN = re.compile(r"\d+k_canvas_marginILi(\d)EE")


def _cover_kernels():
    return {int(m.group(1)): k for name, k in _kernels().items() for m in [NAME.search(name)] if m}


def vgpr_step(v):
    return min(8, 512 // (8 * ((v + 7) // 8)))


def test_the_cover_kernel_is_there_for_the_four_dtypes_and_for_nothing_else():
    assert sorted(_cover_kernels()) == [0, 1, 2, 3]         # U8, F32, F16, BF16
    assert not [n for n in _kernels() if "k_compose" in n and not NAME.search(n)], "a k_compose_* kernel this test does not know"


def test_the_cover_kernel_uses_no_lds_and_no_scratch():
    ks = _cover_kernels()
    assert ks
    for dt, k in ks.items():
        assert k["lds"] == 0 and k["scratch"] == 0, (dt, k)


def test_report_of_vgprs_against_the_margin_kernel(capsys):
    """not a bar: the figures of profiles/composed_output.txt (run with -s to see them)"""
    margin = {int(m.group(1)): k for name, k in _kernels().items() for m in [MARGIN.search(name)] if m}
    ks = _cover_kernels()
    assert sorted(margin) == sorted(ks) == [0, 1, 2, 3]
    for dt in sorted(ks):
        print("dtype %d: k_compose_cover %d VGPRs (%d waves / SIMD), k_canvas_margin %d VGPRs (%d waves / SIMD)"
              % (dt, ks[dt]["vgpr"], vgpr_step(ks[dt]["vgpr"]), margin[dt]["vgpr"], vgpr_step(margin[dt]["vgpr"])))
