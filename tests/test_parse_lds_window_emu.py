"""CPU checks of two properties of the CABAC parser (libheif_amd/csrc/parse_core.h):

* levels go straight to HBM.  residual_coding stores the 16 levels of every sub-block it parses at their raster places in the coefficient arena and
  zero-fills the block's other sub-blocks once; there is no staging block any more.  The coefficient regions are poisoned BEFORE the parse
  (tests/emu/coef_arena_probe.cc): afterwards every coded block equals the oracle's coefficient tap - the zeros of its uncoded sub-blocks included -
  and every word outside the coded blocks (and the PCM units' sample blocks) still holds the poison.  Both host emulations run the cases: the
  register-file build (the source of the general and inter kernels) and the build of the throughput kernel.
* the bitstream window lives in LDS and the next byte is prefetched (HIPDEC_PARSE_LDS_WIN, the throughput build): the byte reader bin by bin
  against the plain 9.3.4.3 of tests/cabac_ref.py over the byte strings of tests/lds_window_cases.py, and a row parked and resumed in the middle of
  a window under the work pool."""
import ctypes as C
import fcntl
import os
import subprocess
import numpy as np
import pytest

import cabac_cases as cc
import lds_window_cases as W
import test_parse_emu as T
import test_parse_unit_maps_lds as U
from oracle import pyoracle as orc

POISON = 0x5a17
LIBS = ["libparse_emu.so", "libparse_emu_lds.so"]
_probe_lib = []


def _probe():
    """libcoef_arena_probe.so beside the emulation libraries, compiled with the flags of tests/emu/Makefile (same layout of the batch object)"""
    if _probe_lib: return _probe_lib[0]
    emu = os.path.join(T.HERE, "emu")
    root = os.path.dirname(T.HERE)
    src, out = os.path.join(emu, "coef_arena_probe.cc"), os.path.join(emu, "libcoef_arena_probe.so")
    with open(os.path.join(emu, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in (src, os.path.join(emu, "emu_batch.h"))):
            tmp = "%s.tmp.%d" % (out, os.getpid())
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                                   "-DHIPDEC_HOST_EMU=1", "-DHIPDEC_PARSE_INTER=1", "-I" + os.path.join(emu, "shim"), "-I" + emu, "-I" + os.path.join(root, "include"),
                                   "-I" + os.path.join(root, "libheif_amd", "csrc"), "-shared", "-o", tmp, src])
            os.replace(tmp, out)
    P = C.CDLL(out)
    P.emu_poison_coeffs.restype = C.c_long
    P.emu_poison_coeffs.argtypes = [C.c_void_p, C.c_int, C.c_int]
    P.emu_coeffs_outside.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_long)]
    _probe_lib.append(P)
    return P


class _PoisonedParse:
    """emu_run_parse with the coefficient regions of every item poisoned in front of it and looked at behind it"""
    def __init__(self, lib, log):
        self.lib, self.log = lib, log

    def __call__(self, h):
        P = _probe()
        self.lib.emu_num_items.argtypes = [C.c_void_p]
        n = self.lib.emu_num_items(h)
        for i in range(n):
            assert P.emu_poison_coeffs(h, i, POISON) > 0
        status = self.lib.emu_run_parse(h)
        if status == 0:
            for i in range(n):
                out = (C.c_long * 3)()
                assert P.emu_coeffs_outside(h, i, POISON, out) == 0
                self.log.append(tuple(out))
        return status


class _Poisoning:
    """a library handle for test_parse_emu / test_inter_emu whose every parse runs on poisoned coefficient regions"""
    def __init__(self, lib):
        self._lib = lib
        self.outside = []      # per parsed item: (words in coded blocks, words outside still poisoned, words outside overwritten)
        self.emu_run_parse = _PoisonedParse(lib, self.outside)

    def __getattr__(self, name):
        return getattr(self._lib, name)


def _glue(lib):
    return np.array((C.c_uint64 * 32).in_dll(lib, "hipdec_emu_glue_counts"), np.int64)


@pytest.mark.parametrize("size", W.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("k", range(len(W.STILLS)), ids=[s[0] for s in W.STILLS])
@pytest.mark.parametrize("libname", LIBS, ids=["rf", "lds"])
def test_levels_go_straight_to_the_arena(libname, k, size, monkeypatch):
    name, cf, cfg, reach = W.STILLS[k]
    lib = U._load(libname)
    stream = W.still(k, size)
    proxy = _Poisoning(lib)
    monkeypatch.setattr(T, "_LIB", proxy)
    before = _glue(lib)
    status, got = T.run_emu([stream])
    assert status == 0, "device status 0x%x" % status
    T.check_against_oracle(stream, got[0])            # coded blocks: the oracle's tap, zeros where a sub-block was not coded
    inside, kept, lost = proxy.outside[0]
    assert lost == 0, "%d words outside the coded blocks were overwritten" % lost
    assert inside > 0
    if size == (136, 72):                              # (one 64x64 CTB does not hold every block size and scan, and may be coded everywhere)
        assert kept > 0                                # the units outside the picture are never parsed
        hit = _glue(lib) - before
        assert all(hit[i] > 0 for i in reach), "the case does not reach what it is here for: counters %s" % [i for i in reach if hit[i] == 0]


@pytest.mark.parametrize("libname", LIBS, ids=["rf", "lds"])
def test_levels_of_a_p_picture_go_straight_to_the_arena(libname, monkeypatch):
    """an I and a P picture through the inter syntax (transform trees of inter units, rqt_root_cbf, units without a tree): planes and motion against
    the oracle from parses over poisoned coefficient regions, nothing outside the coded blocks overwritten"""
    import test_inter_emu as IE
    from test_inter_oracle import make_frames
    lib = U._load(libname)
    proxy = _Poisoning(lib)
    monkeypatch.setattr(T, "_LIB", proxy)
    aus = orc.encode_sequence(make_frames(136, 72, 2), qp=26, global_mv_x=-8, global_mv_y=-4, inter_skip_pct=20, inter_intra_pct=20, seed=5)
    IE.check_sequence(aus, "I P")
    assert len(proxy.outside) == 2
    for inside, kept, lost in proxy.outside:
        assert lost == 0 and inside > 0 and kept > 0


def test_byte_reader_with_the_window_in_lds_bin_by_bin():
    """00 00 03 at every offset 250 .. 262 of a window and as the last bytes, refills that consume byte 255 and then byte 256, substreams that start
    in the middle of a window: bypass and context-coded bins, the runs, coeff_abs_level_remaining, terminate + PCM bytes + restart, at all eight
    bit alignments, through the C++ twins of the throughput build's statements"""
    assert W.run_window_scripts("emu_lds") >= 80 * (len(W.CLEAN) + len(W.WITH_EP))


def test_row_parked_and_resumed_in_the_middle_of_a_window(monkeypatch):
    """pool mode with a yield behind every CTB on a batch of two small stills: every CTB but a row's first starts from a parked record, wherever in
    its window the row stood - the window is loaded again and the prefetched byte primed again"""
    monkeypatch.setenv("HIPDEC_PARSE_POOL", "1")
    monkeypatch.setenv("HIPDEC_POOL_YIELD", "1")
    lib = U._load("libparse_emu_lds.so")
    proxy = _Poisoning(lib)
    monkeypatch.setattr(T, "_LIB", proxy)
    streams = [orc.encode(orc.synth_image(w, h, 8, 1, seed=410 + i), qp=12, stress=1) for i, (w, h) in enumerate([(136, 72), (200, 136)])]
    assert all(len(s) > 4 * 256 for s in streams)      # several windows per row
    status, got = T.run_emu(streams)
    assert status == 0, "device status 0x%x" % status
    for s, g in zip(streams, got):
        T.check_against_oracle(s, g)
    assert all(lost == 0 for _, _, lost in proxy.outside)
