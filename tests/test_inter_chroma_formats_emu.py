"""P and B pictures of 4:2:2 and 4:4:4 sequence tracks through the DEVICE code on the CPU (tests/emu: parse_core.h with the inter syntax and the
ChromaArrayType 2 / 3 paths, k_residual, k_motion, k_mc, reconstruction, deblocking, SAO compiled for the host) against the oracle: prediction
modes, reference indices, motion vectors and every plane of every picture.  The chroma vectors of 8.5.3.2.10 (mvLX * 2 / SubWidthC, / SubHeightC),
the chroma prediction blocks of nPbW / SubWidthC x nPbH / SubHeightC, the chroma transform trees of inter coded units in those formats."""
import ctypes as C
import numpy as np
import pytest

from oracle import pyoracle as orc
from test_inter_emu import _lib, _check_tracks, check_sequence, decode_sequence_emu, parameter_sets
from test_inter_oracle import make_frames, CHROMA_FORMAT_CONFIGS


@pytest.mark.parametrize("name", sorted(CHROMA_FORMAT_CONFIGS))
@pytest.mark.parametrize("cfi,bit_depth", [(3, 8), (2, 8), (3, 10), (2, 12)])
@pytest.mark.parametrize("chain", [0, 8])
def test_lossless_422_444_p_b_pictures(cfi, bit_depth, name, chain):
    frames = make_frames(104, 72, 5, bit_depth, chroma_format_idc=cfi)
    aus = orc.encode_sequence(frames, bit_depth=bit_depth, qp=30, global_mv_x=-6, global_mv_y=-3, inter_skip_pct=0, lossless_pct=100, seed=13,
                              **CHROMA_FORMAT_CONFIGS[name])
    check_sequence(aus, "%s cfi %d %d-bit" % (name, cfi, bit_depth), chain=chain)
    got = decode_sequence_emu(aus, chain=chain)
    # (lossless: the pictures are the source frames, in coding order here)
    pocs = [p["poc"] for p in orc.decode_sequence(aus)]
    for p, poc in zip(got, pocs):
        for c in range(3):
            np.testing.assert_array_equal(p["planes"][c], frames[poc][c], err_msg="%s: POC %d component %d" % (name, poc, c))


@pytest.mark.parametrize("name", sorted(CHROMA_FORMAT_CONFIGS))
@pytest.mark.parametrize("cfi", [2, 3])
@pytest.mark.parametrize("chain", [0, 8])
def test_lossy_422_444_p_b_pictures(cfi, name, chain):
    """QP 26, a quarter of the units skipped: residuals of every size in both chroma layouts, deblocking of inter edges (chroma at bS 2 only, QpC =
    Min(qPi, 51)), SAO"""
    frames = make_frames(136, 104, 6, chroma_format_idc=cfi)
    aus = orc.encode_sequence(frames, qp=26, global_mv_x=-8, global_mv_y=-4, inter_skip_pct=25, seed=21, **CHROMA_FORMAT_CONFIGS[name])
    check_sequence(aus, "%s cfi %d" % (name, cfi), chain=chain)


@pytest.mark.parametrize("cfi", [2, 3])
def test_422_444_tool_mix(cfi):
    """intra coded units inside P / B pictures (k_recon's inter build for the 4:2:2 pair and the 4:4:4 planes), PCM, lossless and transform-skip
    blocks, cu_qp_delta, deblocking offsets"""
    frames = make_frames(120, 88, 5, 10, chroma_format_idc=cfi)
    aus = orc.encode_sequence(frames, bit_depth=10, qp=24, global_mv_x=6, global_mv_y=-10, seed=5, b_frames=1, temporal_mvp=1, pcm_pct=10,
                              inter_intra_pct=40, cu_qp_delta=1, diff_cu_qp_delta_depth=2, deblock_disable=0, tc_offset_div2=2, beta_offset_div2=-2,
                              lossless_pct=20, transform_skip=1)
    check_sequence(aus, "tool mix cfi %d" % cfi)
    check_sequence(aus, "tool mix cfi %d" % cfi, chain=4)


def test_host_front_end_accepts_a_444_p_picture():
    L = _lib()
    aus = orc.encode_sequence(make_frames(72, 56, 2, chroma_format_idc=3), qp=26)
    q = C.c_void_p(L.emu_seq_new())
    try:
        err = C.create_string_buffer(512)
        pic = C.c_void_p(L.emu_seq_create_picture(q, aus[0], len(aus[0]), err, 512))
        assert pic and L.emu_run_parse(pic) == 0 and L.emu_run_pipeline(pic, 15) == 0 and L.emu_seq_commit(q, pic) == 0
        au = parameter_sets(aus[0]) + aus[1]
        pic = L.emu_seq_create_picture(q, au, len(au), err, 512)
        assert pic, err.value.decode()
        pic = C.c_void_p(pic)
        assert L.emu_run_parse(pic) == 0 and L.emu_run_pipeline(pic, 15) == 0 and L.emu_seq_commit(q, pic) == 0
    finally:
        L.emu_seq_free(q)


def test_reference_of_another_chroma_format_is_refused():
    """a 4:4:4 P picture whose reference was decoded as 4:2:0 (parameter sets changed without an IDR picture) still never reaches the kernels"""
    L = _lib()
    a = orc.encode_sequence(make_frames(72, 56, 2), qp=26)
    b = orc.encode_sequence(make_frames(72, 56, 2, chroma_format_idc=3), qp=26)
    q = C.c_void_p(L.emu_seq_new())
    try:
        err = C.create_string_buffer(512)
        pic = C.c_void_p(L.emu_seq_create_picture(q, a[0], len(a[0]), err, 512))
        assert pic and L.emu_run_parse(pic) == 0 and L.emu_run_pipeline(pic, 15) == 0 and L.emu_seq_commit(q, pic) == 0
        au = parameter_sets(b[0]) + b[1]
        assert not L.emu_seq_create_picture(q, au, len(au), err, 512)
        assert b"another format" in err.value
    finally:
        L.emu_seq_free(q)


def test_chain_across_a_420_and_a_444_sequence():
    """one launch set that holds 4:2:0 P pictures and 4:4:4 P pictures: a 4:2:0 sequence, then a 4:4:4 one starting at an IDR picture inside the chain
    (the set takes the parser build with both the inter syntax and the general chroma paths)"""
    a = orc.encode_sequence(make_frames(104, 72, 4), qp=26, global_mv_x=-6, global_mv_y=-3, inter_num_refs=2)
    b = orc.encode_sequence(make_frames(104, 72, 4, chroma_format_idc=3, seed=9), qp=26, global_mv_x=5, global_mv_y=2, inter_num_refs=2)
    both = a + [parameter_sets(b[0]) + x if i else x for i, x in enumerate(b)]
    ref = orc.decode_sequence(a) + orc.decode_sequence(b)
    got = decode_sequence_emu(both, chain=7)
    assert len(got) == len(ref)
    for i, (r, g) in enumerate(zip(ref, got)):
        for c in range(3):
            np.testing.assert_array_equal(g["planes"][c], r["planes"][c], err_msg="4:2:0 + 4:4:4 chain: picture %d plane %d" % (i, c))


def test_chains_of_420_422_444_tracks_share_one_launch_set():
    """the chains of a 4:2:0, a 4:2:2 and a 4:4:4 track in ONE launch set (the product's chain coalescer joins tracks whatever their formats): the
    reconstruction waves of a 4:4:4 picture use three row-progress slots and its motion wavefront a fourth"""
    specs = [("ippp_420", 1, dict(inter_num_refs=2, temporal_mvp=1), 3),
             ("ibbp_422", 2, dict(b_frames=2, b_ref=1, temporal_mvp=1, inter_num_refs=2, inter_intra_pct=30), 4),
             ("ippp_444", 3, dict(weighted_pred=1, log2_ctb=5, amp=1, inter_intra_pct=30), 2)]
    tracks = [orc.encode_sequence(make_frames(104, 72, 7, chroma_format_idc=cfi, seed=11 + k), qp=26, global_mv_x=-6, global_mv_y=3, seed=k, **kw)
              for k, (_, cfi, kw, _) in enumerate(specs)]
    _check_tracks(tracks, [s[3] for s in specs], [s[0] for s in specs])
