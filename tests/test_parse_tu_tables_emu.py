"""CPU checks of the TU tables of the throughput CABAC parser (HIPDEC_PARSE_TU_TABLES, libheif_amd/csrc/parse_tables.h + parse_core.h): what
residual_coding used to derive per transform block and per sub-block by select chains now comes from tables - the sig_coeff_flag context rows and
the sub-block scans in LDS, the per-block descriptor in constant memory.

* every entry of the tables against a plain restatement here of 9.3.4.2.5 (sig_coeff_flag ctxInc), 6.5.3 - 6.5.5 (scans), 9.3.4.2.3 (last-position
  contexts) and 7.4.9.11 (scanIdx), through the parser's own row arithmetic (tests/emu/tu_tables_probe.cc);
* the 8-bit and 10-bit 4:0:0 / 4:2:0 stills of tests/lds_window_cases.py through the host emulation of the throughput build against the oracle, once
  more under the work pool with a yield behind every CTB (a resumed row must find the LDS tables intact), with the glue counters showing that the
  cases reach what the tables decide."""
import ctypes as C
import fcntl
import os
import subprocess
import numpy as np
import pytest

import lds_window_cases as W
import test_parse_emu as T
import test_parse_unit_maps_lds as U
from oracle import pyoracle as orc

_probe_lib = []


def _probe():
    """libtu_tables_probe.so beside the emulation libraries, compiled with the flags of tests/emu/Makefile and the layout of the throughput build"""
    if _probe_lib: return _probe_lib[0]
    emu = os.path.join(T.HERE, "emu")
    root = os.path.dirname(T.HERE)
    csrc = os.path.join(root, "libheif_amd", "csrc")
    src, out = os.path.join(emu, "tu_tables_probe.cc"), os.path.join(emu, "libtu_tables_probe.so")
    deps = [src] + [os.path.join(csrc, f) for f in ("parse_core.h", "parse_tables.h")]
    with open(os.path.join(emu, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
            tmp = "%s.tmp.%d" % (out, os.getpid())
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                                   "-DHIPDEC_HOST_EMU=1", "-DHIPDEC_PARSE_INTER=1", "-DHIPDEC_PARSE_LDS_CTX=1", "-I" + os.path.join(emu, "shim"), "-I" + emu,
                                   "-I" + os.path.join(root, "include"), "-I" + csrc, "-shared", "-o", tmp, src])
            os.replace(tmp, out)
    P = C.CDLL(out)
    P.tu_row_of.restype = C.c_uint32
    P.tu_row_of.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int]
    _probe_lib.append(P)
    return P


# ---- the standard, restated plainly -------------------------------------------------------------------------------------------------------
def diag_scan(n):
    """6.5.3 up-right diagonal scan of an n x n array: [(x, y)]"""
    out, x, y = [], 0, 0
    while True:
        while y >= 0:
            if x < n and y < n: out.append((x, y))
            y -= 1; x += 1
        y, x = x, 0
        if len(out) >= n * n: return out


def horizontal_scan(n):   # 6.5.4
    return [(x, y) for y in range(n) for x in range(n)]


def vertical_scan(n):     # 6.5.5
    return [(x, y) for x in range(n) for y in range(n)]


def scan_order(n, scan_idx):
    return (diag_scan, horizontal_scan, vertical_scan)[scan_idx](n)


CTX_IDX_MAP = [0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8]   # 9.3.4.2.5, i = 0 .. 14


def sig_ctx_inc(log2n, c_idx, scan_idx, xc, yc, right, below):
    """9.3.4.2.5: ctxInc of sig_coeff_flag at (xc, yc) of a block; right / below: coded_sub_block_flag of the sub-block's neighbours"""
    if log2n == 2: sig = CTX_IDX_MAP[(yc << 2) + xc]
    elif xc + yc == 0: sig = 0
    else:
        xs, ys, xp, yp = xc >> 2, yc >> 2, xc & 3, yc & 3
        prev = right | (below << 1)
        if prev == 0: sig = 2 if xp + yp == 0 else (1 if xp + yp < 3 else 0)
        elif prev == 1: sig = 2 if yp == 0 else (1 if yp == 1 else 0)
        elif prev == 2: sig = 2 if xp == 0 else (1 if xp == 1 else 0)
        else: sig = 2
        if c_idx == 0:
            if xs + ys > 0: sig += 3
            sig += (9 if scan_idx == 0 else 15) if log2n == 3 else 21
        else:
            sig += 9 if log2n == 3 else 12
    return sig if c_idx == 0 else 27 + sig


def scan_indices(log2n, c_idx, cf):
    """7.4.9.11: the scan indices that occur for a block kind in a picture of chroma format cf"""
    if log2n == 2 or (log2n == 3 and (c_idx == 0 or cf == 3)): return (0, 1, 2)
    return (0,)


def scan_idx_of(log2n, c_idx, cf, pred_mode):
    if log2n == 2 or (log2n == 3 and (c_idx == 0 or cf == 3)):
        if 6 <= pred_mode <= 14: return 2
        if 22 <= pred_mode <= 30: return 1
    return 0


def _kinds(cf=3):
    for c_idx in (0, 1):
        for log2n in (2, 3, 4, 5):
            for scan_idx in scan_indices(log2n, c_idx, cf):
                yield log2n, c_idx, scan_idx


def _tables():
    P = _probe()
    lay = (C.c_int32 * 8)(); P.tu_layout(lay)
    n_rows, row0, ctx_b, sbscan, lds_bytes, rows_420, kinds, sb_bytes = list(lay)
    lds = np.zeros(lds_bytes, np.uint8)
    P.tu_loaded_lds(lds.ctypes.data_as(C.POINTER(C.c_uint8)))
    return P, lds, dict(n_rows=n_rows, row0=row0, ctx_b=ctx_b, sbscan=sbscan, lds_bytes=lds_bytes, rows_420=rows_420, kinds=kinds, sb_bytes=sb_bytes)


def _desc(P, log2n, c_idx, scan_idx):
    d = (C.c_uint32 * 4)()
    P.tu_desc(P.tu_kind(log2n, c_idx, scan_idx), d)
    return list(d)


def test_sig_context_rows_against_9_3_4_2_5():
    """sizes 4 - 32, luma / chroma, every scan index 7.4.9.11 allows (4:4:4 included), the four neighbour patterns, DC / other sub-block, positions 0 -
    15: the address the run reads at row + 2 k - position 0 of a DC sub-block at entry 0 of the descriptor's DC row - is that of the context variable
    9.3.4.2.5 names.  (The last position of a 4x4 block has no ctxIdxMap entry: its flag is never parsed.)"""
    P, lds, L = _tables()
    assert L["rows_420"] == 46 and L["n_rows"] == 54 and L["row0"] % 4 == 0
    u16 = lambda addr: int(lds[addr]) | (int(lds[addr + 1]) << 8)
    n, rows_seen = 0, set()
    for log2n, c_idx, scan_idx in _kinds():
        d = _desc(P, log2n, c_idx, scan_idx)
        dc0_row = d[1] >> 18
        inside = scan_order(4, scan_idx)
        grid = 1 << (log2n - 2)
        for right in (0, 1):
            for below in (0, 1):
                if log2n == 2 and (right or below): continue          # a 4x4 block's sub-block has no neighbours
                for xs, ys in ((0, 0), (grid - 1, 0), (0, grid - 1), (grid - 1, grid - 1)):
                    row = P.tu_row_of(d[0], right, below, ys * 8 + xs)
                    assert L["row0"] <= row and row + 32 <= L["row0"] + 32 * L["n_rows"] and (row - L["row0"]) % 32 == 0
                    if scan_idx == 0 or not (c_idx and log2n == 3): assert row + 32 <= L["row0"] + 32 * L["rows_420"]   # what a 4:2:0 build keeps
                    rows_seen.add(row)
                    for k, (xp, yp) in enumerate(inside):
                        if log2n == 2 and k == 15: continue
                        want = L["ctx_b"] + 4 * sig_ctx_inc(log2n, c_idx, scan_idx, xs * 4 + xp, ys * 4 + yp, right, below)
                        got = u16(dc0_row) if (k == 0 and xs + ys == 0) else u16(row + 2 * k)
                        assert got == want, (log2n, c_idx, scan_idx, right, below, xs, ys, k)
                        n += 1
    assert n == 6 * 4 * 15 + 10 * 16 * 16 and len(rows_seen) == 54      # 4x4 kinds (one pattern), the ten others (4 patterns x 4 sub-blocks)
    # nothing but the tables is written by the load
    untouched = np.ones(L["lds_bytes"], bool)
    untouched[L["row0"]:L["row0"] + 32 * L["n_rows"]] = False
    untouched[L["sbscan"]:L["sbscan"] + L["sb_bytes"]] = False
    assert np.all(lds[untouched] == 0xa5)


def test_descriptors_against_the_scans_and_the_last_position_rule():
    P, lds, L = _tables()
    assert L["kinds"] == 24
    for log2n, c_idx, scan_idx in _kinds():
        d = _desc(P, log2n, c_idx, scan_idx)
        # 9.3.4.2.3: ctxOffset, ctxShift of last_sig_coeff_x / y_prefix, and their cMax (9.3.3.? : (log2TrafoSize << 1) - 1)
        if c_idx == 0: off, shift = 3 * (log2n - 2) + ((log2n - 1) >> 2), (log2n + 1) >> 2
        else: off, shift = 15, log2n - 2
        assert (d[1] & 31, (d[1] >> 5) & 3, (d[1] >> 7) & 15) == (off, shift, (log2n << 1) - 1)
        # the scan inside a sub-block: nibble k = x | y << 2
        scan4 = d[2] | (d[3] << 32)
        assert [(scan4 >> (4 * k)) & 15 for k in range(16)] == [x | (y << 2) for x, y in scan_order(4, scan_idx)]
        # the sub-block scan of the block's grid, in LDS: byte i = ys << 3 | xs
        grid = 1 << (log2n - 2)
        at = L["sbscan"] + ((d[1] >> 11) & 127)
        assert at + grid * grid <= L["sbscan"] + L["sb_bytes"]
        assert list(lds[at:at + grid * grid]) == [xs | (ys << 3) for xs, ys in scan_order(grid, scan_idx)]


def test_scan_index_rule_of_7_4_9_11():
    P = _probe()
    for cf in (0, 1, 2, 3):
        for c_idx in ((0,) if cf == 0 else (0, 1)):
            for log2n in (2, 3, 4, 5):
                for mode in range(35):
                    assert P.tu_scan_idx_of(cf, log2n, c_idx, mode) == scan_idx_of(log2n, c_idx, cf, mode), (cf, c_idx, log2n, mode)


# ---- streams ------------------------------------------------------------------------------------------------------------------------------
CASES = [k for k, c in enumerate(W.STILLS) if c[1] in (0, 1)]    # 4:0:0 / 4:2:0, 8 and 10 bit: what k_parse_occ8 is launched for
# all block sizes, chroma 4x4 / 8x8 / 16x16 (15), the three scans of 4x4 and 8x8 blocks, the last position in the first / last sub-block,
# coded_sub_block_flag 0 / 1 with every neighbour pattern, hidden signs
STRESS_REACH = tuple(range(1, 15)) + (15,) + tuple(range(16, 22))


def _glue(lib):
    return np.array((C.c_uint64 * 32).in_dll(lib, "hipdec_emu_glue_counts"), np.int64)


def _run(monkeypatch, streams):
    lib = U._load("libparse_emu_lds.so")
    monkeypatch.setattr(T, "_LIB", lib)
    before = _glue(lib)
    status, got = T.run_emu(streams)
    assert status == 0, "device status 0x%x" % status
    for s, g in zip(streams, got):
        T.check_against_oracle(s, g)
    return _glue(lib) - before


@pytest.mark.parametrize("size", W.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("k", CASES, ids=[W.STILLS[k][0] for k in CASES])
def test_stills_through_the_throughput_emulation(k, size, monkeypatch):
    hit = _run(monkeypatch, [W.still(k, size)])
    if W.STILLS[k][0] == "stress":
        assert all(hit[i] > 0 for i in STRESS_REACH), "the case does not reach what the tables decide: counters %s" % [i for i in STRESS_REACH if hit[i] == 0]


def test_stills_under_the_pool_with_a_yield_behind_every_ctb(monkeypatch):
    """every CTB but a row's first starts from a parked record, on a wave that ran other rows in between: the tables are loaded once per wave"""
    monkeypatch.setenv("HIPDEC_PARSE_POOL", "1")
    monkeypatch.setenv("HIPDEC_POOL_YIELD", "1")
    hit = 0
    for bd in (8, 10):   # (a batch holds one bit depth)
        hit = hit + _run(monkeypatch, [W.still(k, size) for k in CASES if W.STILLS[k][2].get("bit_depth", 8) == bd for size in W.SIZES])
    assert all(hit[i] > 0 for i in STRESS_REACH)
