"""Extreme VALUES through the device code on the CPU (tests/emu: the kernel sources compiled for the host) and through the oracle: transform
levels over the whole int16 range (the generator's level_torture knobs: rows that saturate the first transform stage, uniform int16 noise,
levels on the code-length boundaries of coeff_abs_level_remaining, levels one step outside the range), QpY wrapping in (8-283), and sample
planes made of 0 and (1 << bitDepth) - 1 only.  The residual arithmetic is checked against an int64 NumPy restatement of 8.6.2 - 8.6.4.2
(tests/value_extremes.py) which is also run against the oracle's own scaling / transformation.

Largest |residual| the restatement finds for a block whose levels are +-32767 * sign(E[j][0]) at qP 35 + QpBdOffset with flat lists
(test_restated_maxima; the scaled levels saturate at 32767 / -32768, so a first-stage row sits at 32767 and another may reach -32768):

    N        8 bit   10 bit   12 bit      r[0][0] = (32767 * sum_j E[j][0] + round) >> (20 - bitDepth), sum = 247 / 479 / 940 / 1862
    4 DCT    1 976    7 904   31 615      1 976    7 904   31 615
    4 DST    1 936    7 744   30 975
    8        3 832   15 328   61 312      3 832   15 328   61 310
    16       7 520   30 080  120 320      7 520   30 079  120 316
    32      14 896   59 584  238 336     14 896   59 582  238 329

(the hand-derived table of the issue that asked for these tests left the rounding term out: 1 975 / 7 903 / 7 519 / 14 895 / 238 328 are one low)
i.e. a conforming stream carries residuals beyond int16 from 10 bit (N = 32) and 12 bit (N >= 8) on: k_residual, which hands its residual on as
int16, has to SATURATE it (the sample behind Clip1(pred + res) is the same); before this file existed it kept the low 16 bits."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as orc
import test_parse_emu as tp
import test_pipeline_emu as tpe
import value_extremes as vx

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------
# the knobs are off by default: the generator's streams are the ones it wrote before it had them
# ------------------------------------------------------------------------------------------------
def test_default_streams_are_byte_identical_to_the_generator_without_torture_knobs():
    """SHA-256 over the streams of every tests/test_decode_gpu.py:CONFIGS entry (both sizes) and over the tracks of the _p_sequence configurations of
    tests/test_sequence_gpu.py (five pictures each), taken from the generator as it was before the level_torture / qp_delta_wrap knobs"""
    import test_decode_gpu
    import test_sequence_gpu
    from test_inter_oracle import make_frames
    h = hashlib.sha256()
    for cfg in test_decode_gpu.CONFIGS:
        for w, hh in ((200, 136), (64, 64)):
            h.update(orc.encode(orc.synth_image(w, hh, cfg.get("bit_depth", 8), 1, seed=3 + w), **cfg))
    assert h.hexdigest() == "66ca781b7f751e555927100ef20dffd7c110a5b39ad73de80296b12132cb785b"
    seqs = [dict(), dict(amp=1, inter_num_refs=3, max_merge_cand=3, parallel_merge_level=4, log2_ctb=4, log2_max_tb=4),
            dict(stress=1, amp=1, inter_num_refs=2, lists_modification=1, cabac_init_present=1, num_slices=2, wpp=0),
            dict(bit_depth=10, tile_cols=2, tile_rows=2, inter_num_refs=2), dict(w=70, h=42, amp=1, inter_num_refs=2, global_mv_y=17)]
    seqs += [test_sequence_gpu.B_CASES[k] for k in sorted(test_sequence_gpu.B_CASES)]
    h = hashlib.sha256()
    for cfg in seqs:
        cfg = dict(cfg)
        w, hh, bd = cfg.pop("w", 200), cfg.pop("h", 136), cfg.pop("bit_depth", 8)
        for au in orc.encode_sequence(make_frames(w, hh, 5, bd), bit_depth=bd, qp=26, global_mv_x=cfg.pop("global_mv_x", -8),
                                      global_mv_y=cfg.pop("global_mv_y", -4), **cfg):
            h.update(au)
    assert h.hexdigest() == "f7cf1903f0dea5a5e034e5df1cdfb63ac913ae971aebb54e908ee2c80ce235fc"


# ------------------------------------------------------------------------------------------------
# the restatement itself, and the oracle's arithmetic against it
# ------------------------------------------------------------------------------------------------
def _oracle_residual(levels, bit_depth, qP, m, ts, dst):
    L = orc.lib()
    n = levels.shape[0]
    lev = np.ascontiguousarray(levels, np.int32)
    res = np.zeros((n, n), np.int32)
    mm = np.ascontiguousarray(m, np.uint8) if m is not None else None
    L.hevc_scale_and_transform.restype = None
    L.hevc_scale_and_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.hevc_scale_and_transform(res.ctypes.data, lev.ctypes.data, n, qP, bit_depth, mm.ctypes.data if mm is not None else None, int(ts), int(dst))
    return res.astype(np.int64)


def _aligned(n, y0, dst=False, mirror=False, deep=False):
    E = vx._DST if dst else vx.trans_matrix(n)
    neg = (E[:, y0] < 0) ^ mirror
    col = np.where(neg, -32768 if deep else -32767, 32767).astype(np.int64)
    return np.repeat(col[:, None], n, axis=1)


def test_restated_maxima():
    """the table of the module docstring (and of the issue that asked for these tests), from the restatement"""
    assert [int(vx.trans_matrix(n)[:, 0].sum()) for n in (4, 8, 16, 32)] == [247, 479, 940, 1862]
    sums = {4: 247, 8: 479, 16: 940, 32: 1862}
    want = {4: (1976, 7904, 31615), 8: (3832, 15328, 61312), 16: (7520, 30080, 120320), 32: (14896, 59584, 238336)}
    for n in (4, 8, 16, 32):
        for k, bd in enumerate((8, 10, 12)):
            r = vx.residual_int64(_aligned(n, 0), bd, 35 + 6 * (bd - 8))
            assert int(np.abs(r).max()) == want[n][k], (n, bd, int(np.abs(r).max()))
            assert int(r[0, 0]) == (32767 * sums[n] + (1 << (19 - bd))) >> (20 - bd)
    assert [int(np.abs(vx.residual_int64(_aligned(4, 0, dst=True), bd, 35 + 6 * (bd - 8), dst=True)).max()) for bd in (8, 10, 12)] == [1936, 7744, 30975]


@pytest.mark.parametrize("bit_depth", [8, 10, 12])
@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_oracle_scaling_and_transformation_against_the_int64_restatement(n, bit_depth):
    """hevc_scale_and_transform() of oracle/hevc_oracle.c, the reference of every GPU parity test, on hand-made blocks at the edges: aligned rows at
    +-32767 / -32768, uniform int16 noise, single coefficients; flat lists, the default lists and a list of 1 and 255"""
    rng = np.random.default_rng(1000 * n + bit_depth)
    blocks = [_aligned(n, y0, mirror=bool(k & 1), deep=bool(k & 2)) for k, y0 in enumerate(sorted({0, 1, n // 2, n - 1}))]
    blocks += [rng.integers(-32768, 32768, (n, n)).astype(np.int64) for _ in range(3)]
    for v in (32767, -32768):
        for pos in ((0, 0), (n - 1, n - 1)):
            b = np.zeros((n, n), np.int64); b[pos] = v; blocks.append(b)
    lists = [None, vx.default_scaling_factor(n, False), np.where((np.add.outer(np.arange(n), np.arange(n)) & 1) == 1, 255, 1)]
    off = 6 * (bit_depth - 8)
    for lev in blocks:
        for qp in (0, 1, 17, 35, 36, 51):
            for m in lists:
                for ts, dst in ((False, False), (n == 4, False), (False, n == 4)):
                    want = vx.residual_int64(lev, bit_depth, qp + off, m, transform_skip=ts, dst=dst)
                    got = _oracle_residual(lev, bit_depth, qp + off, m, ts, dst)
                    np.testing.assert_array_equal(got, want, err_msg="n %d, %d bit, qp %d, ts %d dst %d" % (n, bit_depth, qp, ts, dst))


# ------------------------------------------------------------------------------------------------
# the parser: levels on the code-length ladder and over the whole range
# ------------------------------------------------------------------------------------------------
def _path_counts():
    L = tp.emu()
    out = (C.c_uint64 * 8)()
    L.emu_path_counts(out)
    return list(out)


PARSE_CONFIGS = [
    dict(stress=1),                                                              # 4x4 .. 32x32, the three scan orders of 4x4 / 8x8 luma blocks
    dict(stress=1, wpp=0, log2_ctb=4, log2_max_tb=4),
    dict(stress=1, num_slices=3, wpp=0),
    dict(stress=1, tile_cols=2, tile_rows=2, wpp=1),
    dict(stress=1, transform_skip=1, lossless_pct=20, sign_data_hiding=0),
    dict(log2_ctb=5, log2_max_tb=5, qp=38, scaling_list=2, bit_depth=10),
    dict(stress=1, qp_delta_wrap_pct=60, diff_cu_qp_delta_depth=2),
]


@pytest.mark.parametrize("kind", [vx.LADDER, vx.UNIFORM], ids=["ladder", "uniform"])
def test_parser_levels_equal_the_oracles_on_tortured_blocks(kind):
    """`coef` of the device parser == the oracle's `coeff` tap, and the three ways the parser decodes coeff_abs_level_remaining (one division: codes of up
    to 8 bins; two: up to 16; bin by bin) plus the bin-by-bin form inside a window with emulation-prevention candidates are each TAKEN (counted
    by the emulator build)"""
    _path_counts()
    sizes, scans = set(), set()
    for k, cfg in enumerate(PARSE_CONFIGS):
        for cf, (w, h) in ((1, (136, 72)), (3, (72, 40)), (2, (72, 40))):
            if cf != 1 and k not in (0, 4):
                continue
            stream = vx.tortured_still(w, h, cfg.get("bit_depth", 8), cf, kind=kind, pct=40, seed=10 + k, **{a: b for a, b in cfg.items() if a != "bit_depth"})
            status, got = tp.run_emu([stream])
            assert status == 0, "device status 0x%x (config %d, chroma format %d)" % (status & 0xffffffff, k, cf)
            tp.check_against_oracle(stream, got[0])
            big = np.abs(got[0]["coef"][0]) > 1000
            ys, xs = np.nonzero(big)
            for y, x in zip(ys[::7], xs[::7]):
                t = int(got[0]["log2_tb"][y // 4, x // 4]); sizes.add(t)
                m = int(got[0]["intra_luma"][y // 4, x // 4])
                if t <= 3:
                    scans.add(2 if 6 <= m <= 14 else (1 if 22 <= m <= 30 else 0))
            assert max(int(np.abs(c).max()) for c in got[0]["coef"]) >= 32767
    counts = _path_counts()
    print("coeff_abs_level_remaining paths (8-bin, 16-bin, bin by bin, ... in a slow window, refusals):", counts[:5])
    assert sizes == {2, 3, 4, 5} and scans == {0, 1, 2}
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and counts[3] > 0 and counts[4] == 0


@pytest.mark.parametrize("pool", [0, 1])
def test_parser_levels_in_a_batch_and_under_the_pool_scheduler(pool, monkeypatch):
    if pool:
        monkeypatch.setenv("HIPDEC_PARSE_POOL", "1")
        monkeypatch.setenv("HIPDEC_POOL_YIELD", "1")
    streams = [vx.tortured_still(136, 72, 8, 1, kind=k, seed=30 + k, stress=1, wpp=k & 1) for k in (1, 2, 3)] + \
              [orc.encode(orc.synth_image(136, 72, 8, 1, seed=4))]
    status, got = tp.run_emu(streams)
    assert status == 0
    for s, g in zip(streams, got):
        tp.check_against_oracle(s, g)


@pytest.mark.parametrize("cf", [1, 3])
@pytest.mark.parametrize("kind", [vx.OVER_32768, vx.OVER_32769], ids=["plus32768", "magnitude32769"])
def test_levels_outside_16_bits_are_a_device_error_and_their_neighbours_decode(kind, cf):
    _path_counts()
    for seed in range(3):
        cfg = dict(stress=1, pct=3 if seed else 100, seed=50 + seed, sign_data_hiding=seed & 1)
        bad = vx.tortured_still(72, 40, 8, cf, kind=kind, **cfg)
        with pytest.raises(orc.OracleError):
            orc.decode(bad)
        status, _ = tp.run_emu([bad])
        assert status != 0
        ok = vx.tortured_still(72, 40, 8, cf, kind=vx.EDGE, **cfg)      # the same blocks one step inside: +32767 / -32768
        tpe._check(ok, tpe.decode_emu([ok])[0])
    assert _path_counts()[4] >= 3


# ------------------------------------------------------------------------------------------------
# k_residual against the restatement, the whole pipeline against the oracle
# ------------------------------------------------------------------------------------------------
def _residual_tap(stream):
    """post-k_residual residual planes (int32, coded size) of the one picture of `stream`, and its decoded planes"""
    L = tpe._lib()
    arr = (C.c_char_p * 1)(stream)
    sizes = (C.c_size_t * 1)(len(stream))
    err = C.create_string_buffer(512)
    h = L.emu_create(1, arr, sizes, err, 512)
    assert h, err.value.decode()
    try:
        assert L.emu_run_parse(h) == 0
        assert L.emu_run_pipeline(h, 1) == 0
        info = (C.c_int * 7)()
        L.emu_info(h, 0, info)
        w, hgt, _, _, _, cf, _ = list(info)
        chh, cw = (hgt if cf in (2, 3) else hgt // 2), (w if cf == 3 else w // 2)
        res = [np.zeros((hgt, w), np.int32), np.zeros((chh, cw), np.int32), np.zeros((chh, cw), np.int32)]
        assert L.emu_coeffs(h, 0, *[r.ctypes.data for r in res]) == 0
        return res
    finally:
        L.emu_free(h)


def check_residuals(stream, cfg, stats=None):
    """every coded block: restatement == oracle arithmetic; device residual word == restatement where the true residual fits int16 (where it does not,
    the sample is decided by Clip1 alone: the planes are compared by the caller).  Returns (coded blocks, blocks with a residual beyond int16)"""
    ref = orc.decode(stream, taps=True)
    res = _residual_tap(stream)
    n_blocks = n_wide = 0
    for b in vx.transform_blocks(ref, cfg):
        want = vx.residual_int64(b["levels"], b["bit_depth"], b["qP"], b["m"], b["ts"], b["bypass"], b["dst"])
        if not b["bypass"]:
            np.testing.assert_array_equal(_oracle_residual(b["levels"], b["bit_depth"], b["qP"], b["m"], b["ts"], b["dst"]), want, err_msg="oracle: %r" % (b,))
        got = res[b["c"]][b["y"]:b["y"] + b["n"], b["x"]:b["x"] + b["n"]].astype(np.int64)
        fits = np.abs(want) <= 32767
        np.testing.assert_array_equal(got[fits], want[fits], err_msg="component %d block %d at (%d, %d), qP %d" % (b["c"], b["n"], b["x"], b["y"], b["qP"]))
        n_blocks += 1
        n_wide += int((~fits).any())
        if stats is not None:
            key = (b["n"], b["bit_depth"])
            stats[key] = max(stats.get(key, 0), int(np.abs(want).max()))
    return n_blocks, n_wide


RESIDUAL_MATRIX = [(bd, cf, qp) for bd in (8, 10, 12) for cf in (1, 2, 3) for qp in (0, 1, 17, 35, 36, 51)]


@pytest.mark.parametrize("bd,cf,qp", RESIDUAL_MATRIX, ids=["%dbit_4%s_qp%d" % (bd, {1: "20", 2: "22", 3: "44"}[cf], qp) for bd, cf, qp in RESIDUAL_MATRIX])
def test_residuals_of_tortured_blocks(bd, cf, qp):
    """N = 4 (DST, DCT of chroma, transform skip) .. 32 incl. 32x32 chroma (4:4:4) and the stacked pairs of 4:2:2; both shift directions of the scaling
    (qP / 6 against bdShift); flat and default lists; transquant bypass beside them"""
    k = RESIDUAL_MATRIX.index((bd, cf, qp))
    cfg = dict(qp=qp, stress=1, cu_qp_delta=k & 1, lossless_pct=10 if k % 3 == 0 else 0, transform_skip=2 if k % 2 else 0, scaling_list=(k // 2) & 1,
               cb_qp_offset=(k % 5) - 2, cr_qp_offset=2 - (k % 4), log2_ctb=5 if k % 4 == 3 else 6)
    stream = vx.tortured_still(72 if cf != 1 else 136, 72, bd, cf, kind=(vx.ALIGNED, vx.ALIGNED, vx.UNIFORM, 0)[k % 4], pct=45, seed=100 + k, **cfg)
    n_blocks, _ = check_residuals(stream, cfg)
    assert n_blocks > 20
    tpe._check(stream, tpe.decode_emu([stream])[0])


def test_residuals_beyond_int16_occur_and_decode():
    """32x32 / 16x16 / 8x8 blocks whose second-stage residual does not fit 16 bits (Main10 and 12 bit): counted, and the samples equal the oracle's"""
    wide_total = 0
    stats = {}
    for bd, cf, qp in ((10, 1, 35), (10, 3, 30), (12, 1, 36), (12, 2, 40), (12, 3, 35)):
        cfg = dict(qp=qp, cu_qp_delta=0)
        stream = vx.tortured_still(192, 128, bd, cf, kind=vx.ALIGNED, pct=60, seed=7 + bd + cf, flat=True, **cfg)
        _, n_wide = check_residuals(stream, cfg, stats)
        wide_total += n_wide
        assert n_wide > 0, (bd, cf)
        tpe._check(stream, tpe.decode_emu([stream])[0])
    print("largest |residual| by (N, bit depth):", sorted(stats.items()))
    assert stats[(32, 10)] > 32767 and stats[(32, 12)] > 32767 and stats[(16, 12)] > 32767


@pytest.mark.parametrize("cfg", [dict(scaling_list=2, stress=1), dict(scaling_list=3, transform_skip=1, bit_depth=10, stress=1), dict(transform_skip=1, lossless_pct=30, stress=1),
                                 dict(qp_delta_wrap_pct=70, stress=1, diff_cu_qp_delta_depth=2), dict(qp_delta_wrap_pct=70, bit_depth=10, qp=48, cb_qp_offset=9, cr_qp_offset=-9),
                                 dict(num_slices=3, wpp=0, pcm_pct=15, stress=1), dict(tile_cols=2, tile_rows=2, bit_depth=12, stress=1)],
                         ids=["sps_lists", "pps_lists_tskip_main10", "tskip_lossless", "qp_wrap", "qp_wrap_main10", "slices_pcm", "tiles_12bit"])
@pytest.mark.parametrize("cf", [1, 2, 3], ids=["420", "422", "444"])
def test_tortured_stills_through_the_whole_pipeline(cf, cfg):
    """sign data hiding, random transform skip, transquant bypass, explicit scaling lists, PCM beside tortured blocks; QpY wrapping below -QpBdOffsetY and
    above 51 ((8-283))"""
    cfg = dict(cfg)
    bd = cfg.pop("bit_depth", 8)
    stream = vx.tortured_still(136, 72, bd, cf, kind=0, pct=30, seed=3, **cfg)
    if "qp_delta_wrap_pct" in cfg:
        qp = orc.decode(stream, taps=True)["map_qp_y"]
        assert int(qp.max()) - int(qp.min()) >= 30                 # group QPs far apart beside each other: the one legal CuQpDeltaVal (+-26) between them wraps
    tpe._check(stream, tpe.decode_emu([stream])[0])


def test_untortured_qp_never_wraps_without_the_knob():
    """(what the issue asked to find out) without qp_delta_wrap_pct the generator keeps qPY_PRED + CuQpDeltaVal inside 1 .. 50"""
    for qp in (2, 26, 49):
        m = orc.decode(orc.encode(orc.synth_image(200, 136, 8, 1, seed=qp), qp=qp, stress=1, diff_cu_qp_delta_depth=2), taps=True)["map_qp_y"]
        assert 1 <= m.min() and m.max() <= 50


# ------------------------------------------------------------------------------------------------
# inter pictures: the same residuals through k_mc (residual added there) and through the per-block reconstruction
# ------------------------------------------------------------------------------------------------
INTER_CASES = {
    "p_420": dict(cf=1, bit_depth=8, inter_num_refs=2, amp=1),
    "b_420_main10": dict(cf=1, bit_depth=10, b_frames=2, b_ref=1, weighted_pred=1, temporal_mvp=1),
    "b_444": dict(cf=3, bit_depth=8, b_frames=1, inter_bi_pct=70, transform_skip=1),
    "p_444_12bit": dict(cf=3, bit_depth=12, qp=35, max_transform_hierarchy_depth_inter=0, log2_min_cb=4),
    "p_422_lists": dict(cf=2, bit_depth=10, scaling_list=2, inter_intra_pct=30),
}


def _inter_stream(name):
    cfg = dict(INTER_CASES[name])
    return vx.tortured_sequence(104, 72, 4, cfg.pop("bit_depth"), cfg.pop("cf"), kind=0, pct=35, seed=5, global_mv_x=-6, global_mv_y=3, inter_skip_pct=10, **cfg)


@pytest.mark.parametrize("name", sorted(INTER_CASES))
@pytest.mark.parametrize("chain", [0, 3])
def test_tortured_residuals_in_p_and_b_pictures(name, chain):
    from test_inter_emu import check_sequence
    check_sequence(_inter_stream(name), name, chain=chain)


@pytest.mark.parametrize("name", ["p_420", "b_444", "p_444_12bit"])
def test_tortured_residuals_in_p_and_b_pictures_per_block_reconstruction(name):
    """HIPDEC_INTER_RECON_PER_BLOCK=1 (k_recon adds the residual of inter blocks instead of k_mc): read once per process, so in a child"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_value_extremes_emu as t\nfrom test_inter_emu import check_sequence\n"
            "check_sequence(t._inter_stream(%r), %r)\ncheck_sequence(t._inter_stream(%r), %r, chain=3)\n") % (os.path.dirname(HERE), HERE, name, name, name, name)
    env = dict(os.environ, HIPDEC_INTER_RECON_PER_BLOCK="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------
# samples at 0 and (1 << bitDepth) - 1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", vx.EXTREME_PATTERNS)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_extreme_sample_planes_intra(bd, pattern):
    """0 / max planes with lossless and PCM units as exact neighbours: Clip1 behind intra smoothing, angular prediction, the edge filters of DC /
    horizontal / vertical modes, deblocking's tc clip at both table ends, SAO.  Each configuration also runs with SAO off and with both loop
    filters off, so that a wrong clip shows in the earliest stage that has it"""
    for k, cfg in enumerate(vx.EXTREME_INTRA_CONFIGS):
        for cf in ((1, 3) if k < 2 else (1, 2)):
            planes = vx.extreme_planes(pattern, 136, 72, bd, cf)
            for stage in (dict(sao=0, deblock_disable=1), dict(sao=0), dict()):
                stream = orc.encode(planes, bit_depth=bd, seed=k, **dict(cfg, **stage))
                try:
                    tpe._check(stream, tpe.decode_emu([stream])[0])
                except AssertionError as e:
                    raise AssertionError("config %d chroma format %d, stages %r: %s" % (k, cf, stage or "all", e))


@pytest.mark.parametrize("k", range(len(vx.EXTREME_INTER_CONFIGS)))
@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 1), (8, 3), (12, 3)])
def test_extreme_sample_planes_inter(bd, cf, k):
    """a max-valued box moving over zero, checkerboards: the 8-tap / 4-tap filters overshoot at every fractional phase, bi-predictive and weighted
    sums leave the sample range before their clip"""
    from test_inter_emu import check_sequence
    aus = vx.extreme_sequence(5, 104, 72, bd, cf, vx.EXTREME_INTER_CONFIGS[k], seed=k)
    check_sequence(aus, "extreme inter %d" % k)
    check_sequence(aus, "extreme inter %d" % k, chain=4)
