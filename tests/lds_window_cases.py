"""Inputs shared by tests/test_parse_lds_window_emu.py (CPU tier) and tests/test_parse_lds_window_gpu.py: the small stills whose coefficient blocks
the parser writes straight into the arena, and the byte strings for the LDS-resident bitstream window of the throughput parser
(HIPDEC_PARSE_LDS_WIN: the prefetched next byte, the 512-byte ring of the current and the next window).  The byte-reader scripts are written with
tests/cabac_cases.py: every operation of the arithmetic decoder, at all eight bit alignments, against the plain 9.3.4.3 of tests/cabac_ref.py."""
import numpy as np

import cabac_cases as cc
from oracle import pyoracle as orc

# (name, chroma format, encoder settings, indices of parse_core.h's glue counters the case must reach - see the PC_GLUE() sites in residual_coding:
#  1 .. 4 luma 4x4 .. 32x32, 5 / 6 chroma 4x4 / 8x8, 7 .. 9 / 10 .. 12 the diagonal, horizontal, vertical scan of 4x4 / 8x8 blocks, 16
#  coded_sub_block_flag decoded as 0, 0 transform_skip_flag set, 23 a block of a cu_transquant_bypass unit, 27 / 28 4:2:2 / 4:4:4)
STILLS = [
    ("stress", 1, dict(stress=1), (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16)),
    ("qp40", 1, dict(qp=40), (16,)),
    ("qp12-zero-residual", 1, dict(qp=12, stress=1, zero_residual_pct=30), (1, 2, 3)),
    ("transform-skip", 1, dict(transform_skip=1, stress=1), (0,)),
    ("lossless", 1, dict(lossless_pct=30), (23,)),
    ("pcm", 1, dict(pcm_pct=30), ()),
    ("pcm-lossless-ctb32", 1, dict(pcm_pct=40, wpp=0, log2_ctb=5, log2_max_tb=5, lossless_pct=20), (23,)),
    ("422", 2, dict(stress=1), (27,)),
    ("422-pcm", 2, dict(pcm_pct=30, lossless_pct=20), (27, 23)),
    ("444", 3, dict(stress=1), (28,)),
    ("444-pcm", 3, dict(pcm_pct=30), (28,)),
    ("main10", 1, dict(bit_depth=10, vui_primaries=9, vui_transfer=16, vui_matrix=9, vui_full_range=0, stress=1), (1, 2, 3)),
    ("mono", 0, dict(stress=1), (1, 2)),
]
SIZES = [(64, 64), (136, 72)]     # one CTB; CTBs clipped on both edges
_streams = {}


def still(k, size):
    """the coded still of case k at one of SIZES (coded once per process)"""
    if (k, size) not in _streams:
        name, cf, cfg, _ = STILLS[k]
        planes = orc.synth_image(size[0], size[1], cfg.get("bit_depth", 8), cf, seed=300 + k)
        _streams[(k, size)] = orc.encode(planes, **cfg)
    return _streams[(k, size)]


# ---- the byte reader -------------------------------------------------------------------------------------------------------------------
# (offset of the substream's start in its 256-byte window, payload bytes, [(at, bytes spliced in)]), as cabac_cases.PLACEMENTS.  Every substream
# here starts in the middle of a window; the ones from offset 236 cross into the next window, so a refill consumes byte 255 and the next one
# byte 256 - at every bit alignment and for every operation kind (cabac_cases._supply_on).
EP = cc.EP
CLEAN = [(236, 40, []), (255, 24, []), (254, 3, []), (120, 30, [])]
# no emulation prevention (a buffer of its own, without a candidate in any window): the short path over the seam - the prefetch of byte 256 comes from
# the other half of the ring -, the end inside the next window.  Then 00 00 03 with its first byte at every window offset 250 .. 262, and as the last
# three bytes of the substream, inside a window and across the seam
WITH_EP = [(236, 44, [(off - 236, EP)]) for off in range(250, 263)] + [(100, 30, [(27, EP)]), (236, 22, [(19, EP)]), (236, 21, [(18, EP)]), (236, 20, [(17, EP)])]
_groups = None


def window_scripts():
    """[(Buf, scripts)], built once: the substreams without emulation prevention, and the others in two buffers"""
    global _groups
    if _groups is None:
        rng = np.random.default_rng(20240)
        _groups = []
        for part in (CLEAN, WITH_EP[0::2], WITH_EP[1::2]):
            buf = cc.Buf()
            buf.place(b"\x80" * 7)
            scripts = []
            for mod, n, splice in part:
                d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                for at, seq in splice:
                    d[at:at + len(seq)] = seq
                st, en = buf.place(bytes(d), mod=mod)
                cc._supply_on(rng, buf, st, en, "at %d (+%d)%s" % (mod, n, " ep at %d" % (mod + splice[0][0]) if splice else ""), scripts)
            if part is CLEAN:
                assert not any(cc.window_has_candidate(buf.data, base) for base in range(0, len(buf.data), 256))
            _groups.append((buf, scripts))
    return _groups


def run_window_scripts(build):
    """every script through the probe of one build, compared record by record; returns the number of scripts"""
    n = 0
    for buf, scripts in window_scripts():
        cc.run_and_check(build, buf, scripts)
        n += len(scripts)
    return n
