"""CPU checks of the reconstruction plan (recon_kernel.hip: k_recon_plan in front of the wavefront, which reads the plan's records instead of staging
the unit words, walking them and keeping an availability bitmap) on the host emulation:
(a) for every block of every CTB the lane masks the block functions build from a record's counts equal the masks of the bitmap walk, and the two
    fronts ends agree on the blocks themselves (order, position, size, mode, flags, residual index, smoothing) - tests/emu/recon_plan_probe.cc runs
    the kernel's own k_recon_plan / plan_mask() and restates the sequential front end;
(b) the planes decoded through the plan are bit-exact against the oracle (8 / 10 bit, 4:2:0 / 4:0:0, PCM and transquant-bypass units);
(c) P pictures and 4:4:4 stills do not launch the plan kernel (their decode is pinned by the existing suites);
(d) a unit map with an impossible transform size gives DEV_ERR_SYNTAX and no record outside its CTB."""
import ctypes as C
import fcntl
import os
import subprocess
import numpy as np
import pytest

import test_parse_emu as T
import test_pipeline_emu as PE
from oracle import pyoracle as orc

DEV_ERR_SYNTAX = 3
_probe_lib = []


def _probe():
    """librecon_plan_probe.so beside the emulation libraries, compiled with the flags of tests/emu/Makefile (same layout of the batch object)"""
    if _probe_lib: return _probe_lib[0]
    emu = os.path.join(T.HERE, "emu")
    root = os.path.dirname(T.HERE)
    csrc = os.path.join(root, "libheif_amd", "csrc")
    src, out = os.path.join(emu, "recon_plan_probe.cc"), os.path.join(emu, "librecon_plan_probe.so")
    deps = [src, os.path.join(emu, "emu_batch.h"), os.path.join(emu, "shim", "hip", "hip_runtime.h")] + \
           [os.path.join(csrc, f) for f in ("recon_kernel.hip", "hevc_device.h", "kernels.h", "batch_layout.h")]
    with open(os.path.join(emu, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
            tmp = "%s.tmp.%d" % (out, os.getpid())
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                                   "-DHIPDEC_HOST_EMU=1", "-DHIPDEC_PARSE_INTER=1", "-I" + os.path.join(emu, "shim"), "-I" + emu, "-I" + os.path.join(root, "include"),
                                   "-I" + csrc, "-shared", "-o", tmp, src, "-lpthread"])
            os.replace(tmp, out)
    P = C.CDLL(out)
    for f in (P.emu_plan_blocks, P.emu_bitmap_blocks):
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    P.emu_plan_run.argtypes = [C.c_void_p]
    P.emu_plan_clear_status.argtypes = [C.c_void_p]
    P.emu_plan_poke_size.argtypes = [C.c_void_p] + [C.c_int] * 4
    P.emu_plan_fill.argtypes = [C.c_void_p, C.c_int, C.c_int]
    _probe_lib.append(P)
    return P


def _parsed(stream):
    L = T.emu()
    arr = (C.c_char_p * 1)(stream); sizes = (C.c_size_t * 1)(len(stream)); err = C.create_string_buffer(512)
    h = L.emu_create(1, arr, sizes, err, 512)
    assert h, err.value.decode()
    assert L.emu_run_parse(h) == 0
    return L, h


def _blocks(fn, h):
    cap = 1 << 16
    buf = np.zeros((cap, 8), np.uint64)
    n = fn(h, 0, buf.ctypes.data, cap)
    assert n >= 0, "probe error %d" % n
    return buf[:n]


# (width, height, encoder settings).  One and two CTB rows / columns of CTB 16, 32 and 64; 72x40 and 136x72: right and bottom CTBs cut at a 4- and an 8-sample
# boundary of the chroma / luma planes; stress = 1 mixes all transform sizes and NxN 4x4 luma quads; two / three slices and 2x2 tiles take the left, up,
# up-right and up-left neighbour CTBs away in turn (a slice that starts inside a CTB row: up-right without up)
GEOMETRY = []
for lc in (4, 5, 6):
    c = 1 << lc
    kw = dict(log2_ctb=lc, log2_max_tb=min(lc, 5), stress=1)
    GEOMETRY += [(c, c, kw), (2 * c, c, kw), (c, 2 * c, kw), (2 * c, 2 * c, kw)]
GEOMETRY += [(72, 40, dict(stress=1)), (136, 72, dict(stress=1)), (136, 72, dict(qp=38)), (72, 40, dict(log2_ctb=4, log2_max_tb=4, stress=1)),
             (136, 72, dict(log2_ctb=5, stress=1, qp=20)),
             (136, 72, dict(log2_ctb=4, log2_max_tb=4, num_slices=2, wpp=0, stress=1)), (136, 72, dict(log2_ctb=4, log2_max_tb=4, num_slices=3, stress=1)),
             (136, 72, dict(log2_ctb=5, num_slices=2, stress=1)),
             (136, 72, dict(log2_ctb=4, log2_max_tb=4, tile_cols=2, tile_rows=2, wpp=0, stress=1)), (200, 136, dict(log2_ctb=5, tile_cols=2, tile_rows=2, wpp=0, stress=1)),
             (72, 40, dict(chroma=0, stress=1))]
GEOMETRY_IDS = ["%dx%d,%s" % (w, h, ",".join("%s=%s" % kv for kv in kw.items())) for w, h, kw in GEOMETRY]
_cases = {}


def _case(k):
    """(blocks from the plan, blocks from the bitmap walk) of geometry case k, computed once"""
    if k not in _cases:
        w, h, kw = GEOMETRY[k]
        kw = dict(kw)
        cf = kw.pop("chroma", 1)
        stream = orc.encode(orc.synth_image(w, h, 8, cf, seed=900 + k), **kw)
        L, b = _parsed(stream)
        try:
            P = _probe()
            P.emu_plan_fill(b, 0, 0xee)
            assert P.emu_plan_run(b) == 0
            _cases[k] = (_blocks(P.emu_plan_blocks, b), _blocks(P.emu_bitmap_blocks, b))
        finally:
            L.emu_free(b)
    return _cases[k]


@pytest.mark.parametrize("k", range(len(GEOMETRY)), ids=GEOMETRY_IDS)
def test_masks_from_the_plan_equal_the_bitmap_walk(k):
    plan, walk = _case(k)
    assert len(walk) > 0
    assert plan.shape == walk.shape, "number of blocks: plan %d, walk %d" % (len(plan), len(walk))
    bad = np.nonzero((plan != walk).any(axis=1))[0]
    assert bad.size == 0, "first differing block %d: plan %s, walk %s" % (bad[0], [hex(int(v)) for v in plan[bad[0]]], [hex(int(v)) for v in walk[bad[0]]])


def test_the_geometry_cases_cover_all_sizes():
    """every transform size 4 .. 32, the chroma sizes 4 .. 16, 4x4 luma quads, and every neighbour region missing at some block while others are there"""
    luma, chroma, quads, partial = set(), set(), 0, 0
    for k in range(len(GEOMETRY)):
        walk = _case(k)[1]
        lists, lg = walk[:, 0] >> np.uint64(32), (walk[:, 1] >> np.uint64(16)) & np.uint64(255)
        luma.update(int(v) for v in lg[lists == 0]); chroma.update(int(v) for v in lg[lists == 1])
        quads += int(((lists == 1) & (lg == 2) & ((walk[:, 2] & np.uint64(3)) == 0)).sum())
        for r in walk:   # a neighbourhood that is neither complete nor empty: the substitution process has something to do
            n = 1 << ((int(r[1]) >> 16) & 255)
            passes = min(4 * n + 1, 64) if int(r[0]) >> 32 == 0 or n == 4 else (64 if n == 16 else 32)
            partial += int(r[4]) not in (0, (1 << passes) - 1)
    assert luma == {2, 3, 4, 5} and chroma == {2, 3, 4}
    assert quads > 0 and partial > 0


def _plan_flag():
    L = T.emu()
    L.hipdec_debug_recon_plan_launched.restype = C.c_int
    return L.hipdec_debug_recon_plan_launched()


PLANES = [(72, 40, 8, 1, dict(stress=1)), (136, 72, 8, 1, dict(stress=1)), (136, 72, 10, 1, dict(bit_depth=10, stress=1)), (72, 40, 10, 0, dict(bit_depth=10)),
          (136, 72, 8, 0, dict(stress=1)), (136, 72, 8, 1, dict(pcm_pct=30, lossless_pct=20)), (72, 40, 10, 1, dict(bit_depth=10, pcm_pct=25, lossless_pct=20, log2_ctb=4, log2_max_tb=4)),
          (136, 72, 8, 1, dict(log2_ctb=4, log2_max_tb=4, num_slices=3, tile_cols=1, stress=1)), (136, 72, 8, 1, dict(log2_ctb=4, log2_max_tb=4, tile_cols=2, tile_rows=2, wpp=0))]


@pytest.mark.parametrize("w,h,bd,cf,kw", PLANES, ids=["%dx%d,%dbit,cf%d,%s" % (w, h, bd, cf, ",".join("%s=%s" % kv for kv in kw.items())) for w, h, bd, cf, kw in PLANES])
def test_planes_through_the_plan_match_the_oracle(w, h, bd, cf, kw):
    stream = orc.encode(orc.synth_image(w, h, bd, cf, seed=33), **kw)
    PE._check(stream, PE.decode_emu([stream])[0])
    assert _plan_flag() == 1, "the plan kernel did not run for an intra 4:0:0 / 4:2:0 batch"


def test_p_pictures_and_444_stills_do_not_launch_the_plan_kernel():
    import test_inter_emu as IE
    from test_inter_oracle import make_frames
    still = orc.encode(orc.synth_image(72, 40, 8, 1, seed=4))
    PE.decode_emu([still])
    assert _plan_flag() == 1
    s444 = orc.encode(orc.synth_image(72, 40, 8, 3, seed=4))
    PE._check(s444, PE.decode_emu([s444])[0])
    assert _plan_flag() == 0
    PE.decode_emu([still])
    assert _plan_flag() == 1
    aus = orc.encode_sequence(make_frames(72, 40, 2), qp=26, seed=21)
    IE.check_sequence(aus, "p")       # (the last launch is the P picture's)
    assert _plan_flag() == 0


@pytest.mark.parametrize("value", [1, 9, 0x36])
def test_broken_unit_map_is_a_syntax_error_without_stray_records(value):
    """an impossible transform size (1, 9; 6 in the low nibble of 0x36) in the middle of a CTB: DEV_ERR_SYNTAX, the lists stay inside their slots and their CTBs"""
    stream = orc.encode(orc.synth_image(136, 72, 8, 1, seed=12), stress=1)
    L, b = _parsed(stream)
    try:
        P = _probe()
        P.emu_plan_fill(b, 0, 0xee)
        assert P.emu_plan_run(b) == 0
        good = _blocks(P.emu_plan_blocks, b)
        P.emu_plan_poke_size(b, 0, 1, 37, value)
        P.emu_plan_fill(b, 0, 0)      # (workgroups that start behind the error leave their CTBs alone: whatever WAS written is looked at)
        st = P.emu_plan_run(b)
        assert st & 0xff == DEV_ERR_SYNTAX and st & 0x40000000
        broken = _blocks(P.emu_plan_blocks, b)        # (asserts: counts within the slots, every record inside its CTB with a size 4 .. 32)
        assert len(broken) <= len(good)
        # ... and the whole pipeline reports the same instead of decoding the picture
        P.emu_plan_clear_status(b)
        L.emu_run_pipeline.argtypes = [C.c_void_p, C.c_int]
        assert L.emu_run_pipeline(b, 2) & 0xff == DEV_ERR_SYNTAX
    finally:
        L.emu_free(b)
