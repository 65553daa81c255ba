"""P and B pictures of 4:2:2 and 4:4:4 sequence tracks on the GPU (k_parse_inter_gen, k_mc with per-axis chroma subsampling, the reconstruction and
filter kernels of those formats): every frame bit-exact against the oracle, through the decoder object, with and without look-ahead chains and
chains in flight, tracks of different chroma formats side by side in shared launch sets, the real libheif's track loop, a damaged sample."""
import os
import sys
import threading
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import pyoracle as orc
import libheif_host as lh
from test_sequence_gpu import _set_lookahead, _play_track, _nals, SRGB_VUI

pytestmark = pytest.mark.gpu

GOPS = {"ippp": dict(inter_num_refs=2, amp=1, inter_intra_pct=20),
        "ibbp": dict(b_frames=2, b_ref=1, temporal_mvp=1, weighted_pred=1, inter_num_refs=2, inter_intra_pct=20)}


def _sequence(n, cfi, w=200, h=136, bit_depth=8, seed=5, **cfg):
    from test_inter_oracle import make_frames
    frames = make_frames(w, h, n, bit_depth, seed=seed, chroma_format_idc=cfi)
    cfg = dict(cfg)
    aus = orc.encode_sequence(frames, bit_depth=bit_depth, qp=cfg.pop("qp", 26), global_mv_x=cfg.pop("global_mv_x", -8),
                              global_mv_y=cfg.pop("global_mv_y", -4), seed=seed, **cfg)
    refs = orc.decode_sequence(aus)
    assert all(r["chroma_format_idc"] == cfi for r in refs)
    return aus, refs


def _check(got, aus, refs, what=""):
    by_poc = {r["poc"]: r for r in refs}
    coding = [r["poc"] for r in refs]
    assert len(got) == len(aus), what
    for out_idx, (img, ud) in enumerate(got):
        assert ud == 900 + coding.index(out_idx), (what, out_idx, ud)
        for c in range(3):
            np.testing.assert_array_equal(img.planes[c], by_poc[out_idx]["planes"][c], err_msg="%s POC %d plane %d" % (what, out_idx, c))


@pytest.fixture(params=[(32, 3), (32, 1), (0, 3), (0, 1)], ids=["lookahead32_pipeline3", "lookahead32_plain", "lookahead0_pipeline3", "lookahead0_plain"])
def chains(request):
    from libheif_amd.decoder import set_sequence_pipeline
    k, d = request.param
    _set_lookahead(k)
    set_sequence_pipeline(d)
    yield request.param
    _set_lookahead(32)
    set_sequence_pipeline(3)


@pytest.mark.parametrize("gop", sorted(GOPS))
@pytest.mark.parametrize("cfi,bit_depth", [(2, 8), (3, 8), (2, 10), (3, 10)], ids=["422_8", "444_8", "422_10", "444_10"])
def test_422_444_tracks_decode_bit_exact_in_output_order(gop, cfi, bit_depth, chains):
    aus, refs = _sequence(11, cfi, bit_depth=bit_depth, seed=20 + cfi, **GOPS[gop])
    _check(_play_track(aus, refs), aus, refs, "%s cfi %d" % (gop, cfi))


@pytest.mark.parametrize("cfi", [2, 3])
def test_422_444_p_pictures_one_by_one_through_the_decoder_object(cfi):
    """every sample pushed on its own and decoded at once (decoding order = output order for IPPP), lossless and lossy, a cropped picture size"""
    from libheif_amd.decoder import HipDecoder
    for kw in (dict(lossless_pct=100, inter_skip_pct=0), dict(w=70, h=42, global_mv_y=17, amp=1, inter_num_refs=2)):
        kw = dict(kw)
        aus, refs = _sequence(5, cfi, w=kw.pop("w", 200), h=kw.pop("h", 136), seed=7, **kw)
        d = HipDecoder()
        try:
            for k, (au, ref) in enumerate(zip(aus, refs)):
                d.push_data(au)
                img = d.decode_next_image()
                assert img is not None and d.decode_next_image() is None
                for c in range(3):
                    np.testing.assert_array_equal(img.planes[c], ref["planes"][c], err_msg="cfi %d %r: picture %d plane %d" % (cfi, kw, k, c))
        finally:
            d.free()


def test_420_and_444_tracks_side_by_side_share_launch_sets():
    """a 4:2:0 and a 4:4:4 track from two host threads: their look-ahead chains meet in one launch set (the parser build with the inter syntax and the
    general chroma paths, a 4:4:4 motion wavefront beside three reconstruction waves per row), every picture exact"""
    from libheif_amd.decoder import chain_stats
    tracks = [_sequence(13, 1, seed=61, temporal_mvp=1, inter_num_refs=2), _sequence(13, 3, seed=62, b_frames=1, temporal_mvp=1, inter_intra_pct=20),
              _sequence(9, 2, w=136, h=104, seed=63, amp=1, inter_num_refs=2)]
    _set_lookahead(4)
    before = chain_stats()
    try:
        for attempt in range(3):      # (whether the threads' chains meet is a matter of timing: the pictures are checked every time, the sharing once)
            results, errors = [None] * len(tracks), []

            def run(t):
                try:
                    results[t] = _play_track(*tracks[t])
                except Exception as e:      # noqa: BLE001 - reported below with the track's number
                    errors.append((t, repr(e)))

            threads = [threading.Thread(target=run, args=(t,)) for t in range(len(tracks))]
            for th in threads: th.start()
            for th in threads: th.join()
            assert not errors, errors
            for t, (aus, refs) in enumerate(tracks):
                _check(results[t], aus, refs, "track %d" % t)
            after = chain_stats()
            if after[2] > before[2]:
                break
        else:
            raise AssertionError("no launch set held more than one track's chain in three runs: %r -> %r" % (before, after))
    finally:
        _set_lookahead(32)


@pytest.mark.skipif(not lh.available(), reason="oracle/_ref/libheif.so not built")
@pytest.mark.parametrize("cfi", [2, 3])
def test_422_444_track_through_libheif(cfi):
    """heif_track_decode_next_image over an image-sequence file whose track is 4:2:2 / 4:4:4 (what x265 --chroma 444 writes into one): every image, in
    the order libheif delivers them"""
    from heic_util import build_sequence
    lh.load_hip_plugin()
    aus, refs = _sequence(9, cfi, seed=40, **dict(GOPS["ibbp"], **SRGB_VUI))
    expect = [r for _, r in sorted((r["poc"], r) for r in refs)]
    got = lh.decode_track(build_sequence(aus, 200, 136, chroma_format_idc=cfi))
    assert len(got) == len(expect)
    for k, (g, r) in enumerate(zip(got, expect)):
        for c in range(3):
            np.testing.assert_array_equal(g["planes"][c], r["planes"][c], err_msg="cfi %d: image %d plane %d" % (cfi, k, c))


def test_a_damaged_444_sample_fails_its_own_track_only():
    """bytes inside the slice data of a 4:4:4 P sample are damaged: that track reports the error after the pictures in front of it, the 4:2:0 track
    decoded beside it stays exact"""
    from libheif_amd import HipDecError
    from libheif_amd.decoder import HipDecoder
    good_aus, good_refs = _sequence(12, 1, seed=90, temporal_mvp=1, inter_num_refs=2)
    bad_aus, bad_refs = _sequence(12, 3, seed=95)
    where = 5
    bad_aus = list(bad_aus)
    nals = _nals(bad_aus[where])
    last = bytearray(nals[-1])
    m = 4 + (len(last) - 4) * 2 // 3
    for i in range(m, min(m + 6, len(last) - 2)):
        last[i] ^= 0x5a
    bad_aus[where] = b"".join(nals[:-1]) + bytes(last)
    _set_lookahead(3)
    outcomes = {}

    def run_bad():
        d = HipDecoder()
        got, err = [], None
        try:
            for k, au in enumerate(bad_aus):
                d.push_data(au)
                r = d.next_picture(user_data=900 + k)
                while r is not None:
                    got.append(r)
                    r = d.next_picture()
            r = d.next_picture(flush=True)
            while r is not None:
                got.append(r)
                r = d.next_picture(flush=True)
        except HipDecError as e:
            err = e
        finally:
            d.free()
        outcomes["bad"] = (got, err)

    def run_good():
        try:
            outcomes["good"] = _play_track(good_aus, good_refs)
        except Exception as e:      # noqa: BLE001
            outcomes["good"] = e

    try:
        threads = [threading.Thread(target=run_good), threading.Thread(target=run_bad)]
        for th in threads: th.start()
        for th in threads: th.join()
    finally:
        _set_lookahead(32)
    got, err = outcomes["bad"]
    assert isinstance(err, HipDecError), outcomes["bad"]
    by_poc = {r["poc"]: r for r in bad_refs}
    for out_idx, (img, ud) in enumerate(got):       # IPPP: output order = coding order
        assert out_idx < where and ud == 900 + out_idx
        for c in range(3):
            np.testing.assert_array_equal(img.planes[c], by_poc[out_idx]["planes"][c])
    assert not isinstance(outcomes["good"], Exception), outcomes["good"]
    _check(outcomes["good"], good_aus, good_refs, "4:2:0 track")
