"""Extreme VALUES on the GPU: the stream sets of tests/test_value_extremes_emu.py (tests/value_extremes.py) through HipDecoder, Batch (planes,
maps, deblocked tap) and whole tracks with look-ahead chains, bit-exact against the oracle - whose own scaling / transformation the CPU tier pins
with an int64 restatement of 8.6.2 - 8.6.4.2.  Transform levels over the whole int16 range (rows that saturate the first transform stage and
drive the second beyond 16 bits, uniform noise, the code-length ladder of coeff_abs_level_remaining, levels one step outside the range), QpY
wrapping in (8-283), and planes of 0 and (1 << bitDepth) - 1 only."""
import numpy as np
import pytest

from oracle import pyoracle as orc
import value_extremes as vx

pytestmark = pytest.mark.gpu


def _decode(stream):
    from libheif_amd.decoder import HipDecoder
    d = HipDecoder()
    try:
        d.push_data(stream)
        img = d.decode_next_image()
        assert d.decode_next_image() is None
    finally:
        d.free()
    return img


def _check_still(stream, what=""):
    ref = orc.decode(stream)
    img = _decode(stream)
    assert len(img.planes) == len(ref["planes"])
    for c in range(len(ref["planes"])):
        np.testing.assert_array_equal(img.planes[c], ref["planes"][c], err_msg="%s component %d" % (what, c))


STILLS = [(bd, cf, qp) for bd in (8, 10, 12) for cf in (1, 2, 3) for qp in (0, 17, 36, 51)]


@pytest.mark.parametrize("bd,cf,qp", STILLS, ids=["%dbit_4%s_qp%d" % (bd, {1: "20", 2: "22", 3: "44"}[cf], qp) for bd, cf, qp in STILLS])
def test_tortured_stills_decode_bit_exact(bd, cf, qp):
    """aligned / uniform / ladder blocks of every size, DST, transform skip, transquant bypass, flat / default / explicit scaling lists; the flat
    source of the second stream gives 32x32 blocks (32x32 chroma in 4:4:4) whose residuals exceed 16 bits at 10 and 12 bits"""
    k = STILLS.index((bd, cf, qp))
    cfg = dict(qp=qp, stress=1, cu_qp_delta=k & 1, lossless_pct=10 if k % 3 == 0 else 0, transform_skip=(0, 1, 2)[k % 3], scaling_list=k % 4,
               cb_qp_offset=(k % 5) - 2, cr_qp_offset=2 - (k % 4), wpp=(k >> 1) & 1, qp_delta_wrap_pct=30 if k % 4 == 1 else 0)
    _check_still(vx.tortured_still(136, 72, bd, cf, kind=0, pct=40, seed=200 + k, **cfg), "mixed")
    _check_still(vx.tortured_still(128, 64, bd, cf, kind=vx.ALIGNED, pct=60, seed=300 + k, flat=True, qp=max(qp, 17), cu_qp_delta=0), "aligned 32x32")


@pytest.mark.parametrize("cfg", [dict(num_slices=3, wpp=0), dict(tile_cols=2, tile_rows=2, wpp=1), dict(log2_ctb=4, log2_max_tb=4, wpp=0), dict(dependent_segments=3)],
                         ids=["slices", "tiles_wpp", "ctb16", "dependent_segments"])
@pytest.mark.parametrize("kind", [vx.LADDER, vx.UNIFORM], ids=["ladder", "uniform"])
def test_levels_on_the_code_length_ladder_maps_and_tap(kind, cfg):
    """the parser's three coeff_abs_level_remaining paths at every window alignment the streams bring; the unit maps and the deblocked picture too"""
    from libheif_amd.decoder import Batch
    streams = [vx.tortured_still(264, 200, 8, 1, kind=kind, pct=40, seed=60, stress=1, **cfg), vx.tortured_still(72, 64, 8, 3, kind=kind, pct=50, seed=61, stress=1, **cfg)]
    b = Batch(streams)
    b.run(); b.status()
    for i, s in enumerate(streams):
        ref = orc.decode(s, taps=True)
        m = b.maps(i)
        np.testing.assert_array_equal(m["log2_tb"], ref["map_log2_tb"])
        np.testing.assert_array_equal(m["qp_y"], ref["map_qp_y"])
        np.testing.assert_array_equal(m["flags"] & 0x7f, ref["map_flags"] & 0x7f)
        for c in range(3):
            np.testing.assert_array_equal(b.tap(i, c), ref["post_deblock"][c], err_msg="item %d deblocked component %d" % (i, c))
            np.testing.assert_array_equal(b.planes(i)[c], ref["planes"][c], err_msg="item %d component %d" % (i, c))


def _ordinary(n, bd=8):
    return [orc.encode(orc.synth_image(200, 136, bd, 1, seed=80 + i), bit_depth=bd, stress=i & 1) for i in range(n)]


@pytest.mark.parametrize("tortured", ["main10_420", "444"])
def test_a_tortured_still_in_a_batch_of_ordinary_ones(tortured):
    """Main10 4:2:0 beside ordinary stills: the batch builds of the parser and of k_residual; a 4:4:4 item: the general builds"""
    from libheif_amd.decoder import Batch
    t = vx.tortured_still(192, 128, 10, 1, kind=vx.ALIGNED, pct=60, seed=9, flat=True, qp=35, cu_qp_delta=0) if tortured == "main10_420" else \
        vx.tortured_still(136, 72, 10, 3, kind=0, pct=50, seed=9, qp=30, stress=1)
    streams = _ordinary(3, 10) + [t] + _ordinary(2, 10)
    b = Batch(streams)
    b.run(); b.status()
    for i, s in enumerate(streams):
        ref = orc.decode(s)
        for c in range(3):
            np.testing.assert_array_equal(b.planes(i)[c], ref["planes"][c], err_msg="item %d component %d" % (i, c))


@pytest.mark.parametrize("kind", [vx.OVER_32768, vx.OVER_32769], ids=["plus32768", "magnitude32769"])
def test_a_level_outside_16_bits_is_refused_and_its_neighbours_stay_exact(kind):
    """a lone level of +32768 / of magnitude 32769: a syntax error from the device, alone and inside a batch (a batch reports one status: it fails as
    a whole, loudly); the same streams with the level one step inside decode, and so do the neighbours afterwards"""
    from libheif_amd.decoder import Batch, HipDecoder
    from libheif_amd import HipDecError
    cfg = dict(stress=1, pct=5, seed=51)
    bad = vx.tortured_still(136, 72, 8, 1, kind=kind, **cfg)
    with pytest.raises(orc.OracleError):
        orc.decode(bad)
    d = HipDecoder()
    d.push_data(bad)
    with pytest.raises(HipDecError):
        d.decode_next_image()
    d.free()
    good = _ordinary(3)
    b = Batch(good[:2] + [bad] + good[2:])
    b.run()
    with pytest.raises(HipDecError) as e:
        b.status()
    assert e.value.code == -8
    edge = vx.tortured_still(136, 72, 8, 1, kind=vx.EDGE, **cfg)
    streams = good[:2] + [edge] + good[2:]
    b = Batch(streams)
    b.run(); b.status()
    for i, s in enumerate(streams):
        ref = orc.decode(s)
        for c in range(3):
            np.testing.assert_array_equal(b.planes(i)[c], ref["planes"][c], err_msg="item %d component %d" % (i, c))


INTER_CASES = {
    "p_420": dict(cf=1, bit_depth=8, inter_num_refs=2, amp=1),
    "b_420_main10": dict(cf=1, bit_depth=10, b_frames=2, b_ref=1, weighted_pred=1, temporal_mvp=1),
    "b_444": dict(cf=3, bit_depth=8, b_frames=1, inter_bi_pct=70, transform_skip=1),
    "p_444_12bit": dict(cf=3, bit_depth=12, qp=35, max_transform_hierarchy_depth_inter=0, log2_min_cb=4),
    "p_422_lists": dict(cf=2, bit_depth=10, scaling_list=2, inter_intra_pct=30),
}


def _check_track(aus, what):
    from test_sequence_gpu import _play_track
    refs = orc.decode_sequence(aus)
    by_poc = {r["poc"]: r for r in refs}
    got = _play_track(aus, refs)
    assert len(got) == len(aus)
    for out_idx, (img, _) in enumerate(got):
        for c in range(3):
            np.testing.assert_array_equal(img.planes[c], by_poc[out_idx]["planes"][c], err_msg="%s POC %d plane %d" % (what, out_idx, c))


@pytest.fixture(params=[32, 0], ids=["lookahead32", "lookahead0"])
def lookahead(request):
    from test_sequence_gpu import _set_lookahead
    _set_lookahead(request.param)
    yield request.param
    _set_lookahead(32)


@pytest.mark.parametrize("name", sorted(INTER_CASES))
def test_tortured_residuals_in_p_and_b_tracks(name, lookahead):
    """k_mc adding the residual (the default) over whole tracks, sample by sample and as look-ahead chains"""
    cfg = dict(INTER_CASES[name])
    aus = vx.tortured_sequence(136, 104, 7, cfg.pop("bit_depth"), cfg.pop("cf"), kind=0, pct=35, seed=5, global_mv_x=-6, global_mv_y=3, inter_skip_pct=10, **cfg)
    _check_track(aus, name)


def test_tortured_residuals_per_block_reconstruction():
    """HIPDEC_INTER_RECON_PER_BLOCK=1 (k_recon adds the residual of inter blocks instead of k_mc; read once per process, so in a child): tracks like
    those of the test above, with the library's default look-ahead and pipelined chains"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import value_extremes as vx, test_value_extremes_gpu as t\n"
            "for name in ('p_420', 'b_444', 'p_444_12bit'):\n"
            "    cfg = dict(t.INTER_CASES[name])\n"
            "    aus = vx.tortured_sequence(136, 104, 9, cfg.pop('bit_depth'), cfg.pop('cf'), kind=0, pct=35, seed=6, global_mv_x=5, global_mv_y=-7, inter_skip_pct=10, **cfg)\n"
            "    t._check_track(aus, name)\n") % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HIPDEC_INTER_RECON_PER_BLOCK="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("pattern", vx.EXTREME_PATTERNS)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_extreme_sample_planes_intra(bd, pattern):
    """planes of 0 and max with lossless / PCM units as exact prediction neighbours, QP 0 and 51, tc / beta offsets at +-6: the decoded planes, and the
    deblocked picture so that a wrong clip is attributed to its stage"""
    from libheif_amd.decoder import Batch
    streams = []
    for k, cfg in enumerate(vx.EXTREME_INTRA_CONFIGS):
        cf = (1, 3, 1, 2)[k]
        streams.append(orc.encode(vx.extreme_planes(pattern, 136, 72, bd, cf), bit_depth=bd, seed=k, **cfg))
    b = Batch(streams)
    b.run(); b.status()
    for i, s in enumerate(streams):
        ref = orc.decode(s, taps=True)
        for c in range(3):
            np.testing.assert_array_equal(b.tap(i, c), ref["post_deblock"][c], err_msg="config %d deblocked component %d" % (i, c))
            np.testing.assert_array_equal(b.planes(i)[c], ref["planes"][c], err_msg="config %d component %d" % (i, c))
    _check_still(streams[0], "single")


@pytest.mark.parametrize("k", range(len(vx.EXTREME_INTER_CONFIGS)))
@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 1), (8, 3), (12, 3)])
def test_extreme_sample_planes_inter(bd, cf, k, lookahead):
    """a max-valued box moving over zero: 8-tap / 4-tap overshoot at fractional phases, bi-predictive and weighted sums"""
    _check_track(vx.extreme_sequence(6, 136, 104, bd, cf, vx.EXTREME_INTER_CONFIGS[k], seed=k), "extreme inter %d" % k)
