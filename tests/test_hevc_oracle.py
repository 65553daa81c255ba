"""CPU tests of the HEVC oracle (oracle/hevc_oracle.c) and of the test-stream generator.

Pinning available in this environment: no decoded-pixel golden exists for HEVC in the
reference tree, so the oracle is pinned structurally against the reference's REAL x265-produced
fixtures — every CABAC substream must terminate exactly on the entry point the encoder signalled,
with the stop bit and zero alignment in place, and the decoded size must equal what the reference's
own tests assert (tests/component_descriptions.cc:286-323)."""
import glob
import os
import numpy as np
import pytest

from heic_util import HeicFile
from oracle import pyoracle as orc


def _psnr(a, b, hi):
    m = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if m == 0 else 10 * np.log10(hi * hi / m)


# ---- real fixtures of the reference (stored under tests/golden/reference/) ----------------------
def test_example_heic_decodes_with_exact_substream_termination(reference_dir):
    f = HeicFile(os.path.join(reference_dir, "examples", "example.heic"))
    items = f.hevc_items()
    assert len(items) == 4
    for iid in items:
        r = orc.decode(f.plugin_stream(iid))
        assert (r["width"], r["height"]) == f.ispe(iid)
        assert r["nclx"] == (2, 2, 2, 0)            # VUI without video_signal_type
        assert r["chroma_format_idc"] == 1 and r["bit_depth_luma"] == 8
    r = orc.decode(f.plugin_stream(f.primary))
    assert (r["width"], r["height"]) == (1280, 854)
    assert r["n_substreams"] == 14                   # WPP: one substream per 64-row
    # natural image sanity: a decode error in intra pictures is catastrophic, never subtle
    y = r["planes"][0].astype(np.int32)
    assert 40 < y.mean() < 220
    assert np.abs(np.diff(y, axis=1)).mean() < 20


def test_thumbnail_agrees_with_downscaled_main_image(reference_dir):
    """two independently coded items of the same photo must agree (cross-item plausibility pin)."""
    f = HeicFile(os.path.join(reference_dir, "examples", "example.heic"))
    main = orc.decode(f.plugin_stream(20004))["planes"][0].astype(np.float64)
    thumb = orc.decode(f.plugin_stream(20005))["planes"][0].astype(np.float64)
    h, w = thumb.shape
    ys = (np.arange(h) * main.shape[0] / h).astype(int)
    xs = (np.arange(w) * main.shape[1] / w).astype(int)
    k = main.shape[1] // w
    box = np.add.reduceat(np.add.reduceat(main[:h * k, :w * k], np.arange(0, h * k, k), 0), np.arange(0, w * k, k), 1) / (k * k)
    assert _psnr(box, thumb, 255) > 20


def test_reference_test_fixtures_dimensions(reference_dir):
    """tests/component_descriptions.cc:286-323: rainbow is 452x462 coded/ispe, 3 comps 8 bit;
    :362-366 with-alpha carries a second (alpha) HEVC item."""
    f = HeicFile(os.path.join(reference_dir, "tests", "data", "rainbow-451x461.heic"))
    r = orc.decode(f.plugin_stream(f.hevc_items()[0]))
    assert (r["width"], r["height"]) == (452, 462) == f.ispe(f.hevc_items()[0])
    assert r["nclx"] == (1, 13, 6, 1) and r["bit_depth_luma"] == 8 and len(r["planes"]) == 3
    f = HeicFile(os.path.join(reference_dir, "tests", "data", "with-alpha-512x512.heic"))
    a, b = f.hevc_items()
    assert orc.decode(f.plugin_stream(a))["chroma_format_idc"] == 1
    alpha = orc.decode(f.plugin_stream(b))
    assert alpha["chroma_format_idc"] == 0 and (alpha["width"], alpha["height"]) == (512, 512)


def test_fuzz_corpus_never_crashes(reference_dir):
    ok = 0
    for path in sorted(glob.glob(os.path.join(reference_dir, "fuzzing", "data", "corpus", "*.heic"))):
        try:
            f = HeicFile(path)
        except Exception:
            continue
        for iid in f.hevc_items():
            try:
                orc.decode(f.plugin_stream(iid))
                ok += 1
            except (orc.OracleError, ValueError, IndexError):
                pass
    assert ok >= 9  # the well-formed colors-*.heic items


# ---- generator <-> oracle round trips over the coding-tool matrix --------------------------------
CONFIGS = [
    dict(),
    dict(wpp=0),
    dict(stress=1),
    dict(stress=1, wpp=0, log2_ctb=4, log2_max_tb=4),
    dict(tile_cols=2, tile_rows=2, wpp=0),
    dict(tile_cols=3, tile_rows=2, wpp=1, loop_filter_across_tiles=0),
    dict(num_slices=3, loop_filter_across_slices=0),
    dict(num_slices=4, wpp=0, stress=1),
    dict(transform_skip=1, stress=1),
    dict(lossless_pct=30),
    dict(pcm_pct=20, stress=1, pcm_loop_filter_disabled=1),
    dict(bit_depth=10, vui_matrix=9, vui_primaries=9, vui_transfer=16),
    dict(scaling_list=1),
    dict(log2_ctb=5, log2_min_cb=4, log2_max_tb=5, max_transform_hierarchy_depth_intra=2, stress=1),
    dict(sao=0, deblock_disable=1),
    dict(cb_qp_offset=3, cr_qp_offset=-4, beta_offset_div2=2, tc_offset_div2=-2, qp=34),
    dict(qp=12, stress=1, zero_residual_pct=30),
    dict(sign_data_hiding=0, cu_qp_delta=0, strong_intra_smoothing=0),
    dict(dependent_segments=3, wpp=0, stress=1),
    dict(dependent_segments=2, num_slices=2, wpp=1),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()) or "default")
def test_generator_oracle_round_trip(cfg):
    bd = cfg.get("bit_depth", 8)
    planes = orc.synth_image(200, 136, bd, 1, seed=3)
    stream = orc.encode(planes, **cfg)
    r = orc.decode(stream)
    assert (r["width"], r["height"]) == (200, 136)
    floor = 22 if cfg.get("qp", 27) >= 34 or cfg.get("scaling_list") or cfg.get("zero_residual_pct") else 29
    assert _psnr(r["planes"][0], planes[0], (1 << bd) - 1) > floor
    if "vui_matrix" in cfg:
        assert r["nclx"] == (9, 16, 9, 0)


def test_lossless_round_trip_is_exact_before_loop_filters():
    """cu_transquant_bypass on every CU: reconstruction must equal the source exactly, and the
    in-loop filters must leave bypass samples untouched (8.7.2 / 8.7.3 pcm/bypass rules)."""
    planes = orc.synth_image(136, 72, 8, 1, seed=9)
    r = orc.decode(orc.encode(planes, lossless_pct=100, sao=1))
    for c in range(3):
        np.testing.assert_array_equal(r["planes"][c], planes[c])


@pytest.mark.parametrize("cfg", [dict(dependent_segments=3, wpp=0), dict(dependent_segments=5, wpp=0, log2_ctb=4, log2_max_tb=4, stress=1),
                                 dict(dependent_segments=3, wpp=1), dict(dependent_segments=4, num_slices=2, wpp=0, stress=1)],
                         ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_dependent_slice_segments_round_trip_exactly_when_lossless(cfg):
    """the generator's dependent slice segments (contexts, qPY_PREV and availability continue across segment boundaries, 9.3.1 / 8.6.1 /
    6.4.1) against the oracle's reading of the same clauses: with every CU lossless the decoded picture IS the source"""
    planes = orc.synth_image(200, 136, 8, 1, seed=13)
    stream = orc.encode(planes, lossless_pct=100, **cfg)
    nals = []
    p = 0
    while p < len(stream):
        n = int.from_bytes(stream[p:p + 4], "big"); nals.append(stream[p + 4:p + 4 + n]); p += 4 + n
    assert sum(1 for x in nals if (x[0] >> 1) & 63 < 32) >= 3          # really several slice segment NAL units
    r = orc.decode(stream)
    for c in range(3):
        np.testing.assert_array_equal(r["planes"][c], planes[c])


def test_monochrome_and_odd_sizes():
    planes = orc.synth_image(75, 41, 8, 0, seed=5)
    r = orc.decode(orc.encode(planes))
    assert (r["width"], r["height"]) == (75, 41) and r["chroma_format_idc"] == 0
    planes = orc.synth_image(70, 42, 8, 1, seed=5)
    r = orc.decode(orc.encode(planes))
    assert (r["width"], r["height"]) == (70, 42)


def test_truncated_and_garbage_streams_error_out():
    planes = orc.synth_image(64, 64, 8, 1, seed=2)
    stream = orc.encode(planes)
    with pytest.raises(orc.OracleError):
        orc.decode(stream[:len(stream) - 40])
    with pytest.raises(orc.OracleError):
        orc.decode(stream[:7])
    bad = bytearray(stream)
    bad[len(bad) // 2] ^= 0x55
    try:
        orc.decode(bytes(bad))  # may decode to garbage but must not crash; usually desynchronises
    except orc.OracleError:
        pass
    with pytest.raises(orc.OracleError):
        orc.decode(b"")
