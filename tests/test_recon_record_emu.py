"""CPU checks of the 16-byte reconstruction-plan records (recon_kernel.hip: k_recon_plan fills the availability mask of a block's first 64 reference
samples, its offset in the LDS tile, the class of its sample loop and "a reference sample is missing"; the wavefront dispatches on them) on the host
emulation:
(a) stills of 72x40, 136x72 and 200x136 - none a CTB multiple, so the picture edge clips the availability runs on both axes - in 4:2:0 and 4:0:0 at
    QP 22 and 37 with the encoder's `stress` mix of all transform sizes, one still with two slices (above-right without above) and one with PCM units:
    planes decoded through the records bit for bit against the oracle;
(b) for every record of those stills, the pre-digested words equal what the block functions used to derive per block from w0 / w1 - restated here in
    plain Python from the record layout and 8.4.4.2.2 / 8.4.4.2.6, without calling the code under test;
(c) over the set every dispatch class is reached: the register-resident 4x4 and 8x8 forms and the general form of luma, the 4x4 and the general form
    of the chroma pair, each with planar, DC, pure angular with edge filter (luma below 32x32), angular with non-negative and with negative angle, with
    and without substitution and smoothing - and all 35 luma modes, mode 34 and the other chroma modes."""
import ctypes as C
import fcntl
import os
import subprocess
import numpy as np
import pytest

import test_parse_emu as T
import test_pipeline_emu as PE
import test_recon_plan_emu as RP
import recon_record_cases as cases
from oracle import pyoracle as orc

PK_PLANAR, PK_DC, PK_PURE_EDGE, PK_POS, PK_NEG = range(5)
# intraPredAngle of modes 2 .. 34 (table 8-4)
ANGLE = dict(zip(range(2, 35), [32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32]))

STILLS, IDS, _stream = cases.STILLS, cases.IDS, cases.stream
_probe_lib = []
_cases = {}


def _probe():
    """librecon_record_probe.so beside the emulation libraries (flags of tests/emu/Makefile, as the plan probe is built)"""
    if _probe_lib: return _probe_lib[0]
    emu = os.path.join(T.HERE, "emu")
    root = os.path.dirname(T.HERE)
    csrc = os.path.join(root, "libheif_amd", "csrc")
    src, out = os.path.join(emu, "recon_record_probe.cc"), os.path.join(emu, "librecon_record_probe.so")
    deps = [src, os.path.join(emu, "emu_batch.h")] + [os.path.join(csrc, f) for f in ("hevc_device.h", "batch_layout.h")]
    with open(os.path.join(emu, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
            tmp = "%s.tmp.%d" % (out, os.getpid())
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                                   "-DHIPDEC_HOST_EMU=1", "-DHIPDEC_PARSE_INTER=1", "-I" + os.path.join(emu, "shim"), "-I" + emu, "-I" + os.path.join(root, "include"),
                                   "-I" + csrc, "-shared", "-o", tmp, src, "-lpthread"])
            os.replace(tmp, out)
    P = C.CDLL(out)
    P.emu_plan_records.restype = C.c_long
    P.emu_plan_records.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    P.emu_plan_log2_ctb.argtypes = [C.c_void_p, C.c_int]
    _probe_lib.append(P)
    return P


def _case(k):
    """(records of still k as rows of ctb, list, w0, w1, w2, w3; log2 of its CTB size), computed once"""
    if k not in _cases:
        L, b = RP._parsed(_stream(k))
        try:
            plan, P = RP._probe(), _probe()
            plan.emu_plan_fill(b, 0, 0xee)
            assert plan.emu_plan_run(b) == 0
            cap = 1 << 16
            buf = np.zeros((cap, 6), np.uint32)
            n = P.emu_plan_records(b, 0, buf.ctypes.data, cap)
            assert n > 0, "probe error %d" % n
            _cases[k] = (buf[:n].copy(), P.emu_plan_log2_ctb(b, 0))
        finally:
            L.emu_free(b)
    return _cases[k]


def _fields(w0, w1):
    return dict(gx=w0 & 15, gy=(w0 >> 4) & 15, lg=(w0 >> 8) & 7, smooth=(w0 >> 11) & 1, nl=(w0 >> 12) & 31, nt=(w0 >> 17) & 31, above=(w0 >> 22) & 1,
                corner=(w0 >> 23) & 1, mode=w1 & 255)


def _available(f, e):
    """reference sample e of the block in scan order (left column bottom-up, corner, top row left to right), from the record's counts (units of 4 samples)"""
    n = 1 << f["lg"]
    if e < 2 * n: return (2 * n - 1 - e) < 4 * f["nl"]          # e = 2n - 1 is the left neighbour of the block's first row; the run goes downward
    if e == 2 * n: return bool(f["corner"])
    c = e - 2 * n - 1                                           # column of the top row, from the block's left edge
    return c < 4 * f["nt"] if f["above"] else n <= c < n + 4 * f["nt"]


def _expected(list_, w0, w1, log2_ctb):
    """(w1's upper half, w2, w3) as the per-block derivation of the 8-byte records gave them"""
    f = _fields(w0, w1)
    n = 1 << f["lg"]
    total = 4 * n + 1
    covered = min(total, 64)                    # the lanes of the first pass(es)
    if list_ == 1 and n < 16: covered = 32      # the chroma pair: 32 lanes per component; one pass below 16x16
    mask = sum(1 << e for e in range(min(covered, total)) if _available(f, e))
    subst = int(any(not _available(f, e) for e in range(total)))
    toff = ((f["gy"] * 4) << (log2_ctb - list_)) + f["gx"] * 4
    mode = f["mode"]
    if mode == 0: kind = PK_PLANAR
    elif mode == 1: kind = PK_DC
    else:
        angle = ANGLE[mode]
        edge = list_ == 0 and n < 32            # boundary filters: luma below 32x32
        kind = PK_NEG if angle < 0 else (PK_PURE_EDGE if angle == 0 and edge else PK_POS)
    return toff | (kind << 12) | (subst << 15), mask & 0xffffffff, mask >> 32


@pytest.mark.parametrize("k", range(len(STILLS)), ids=IDS)
def test_planes_through_the_records_match_the_oracle(k):
    stream = _stream(k)
    PE._check(stream, PE.decode_emu([stream])[0])
    assert RP._plan_flag() == 1, "the plan kernel did not run"


@pytest.mark.parametrize("k", range(len(STILLS)), ids=IDS)
def test_predigested_words_equal_the_per_block_derivation(k):
    recs, log2_ctb = _case(k)
    for ctb, list_, w0, w1, w2, w3 in recs.tolist():
        hi, m_lo, m_hi = _expected(list_, w0, w1, log2_ctb)
        got = (w1 >> 16, w2, w3)
        assert got == (hi, m_lo, m_hi), "CTB %d list %d w0 %#x w1 %#x: got %s, expected %s" % (ctb, list_, w0, w1, [hex(v) for v in got], [hex(v) for v in (hi, m_lo, m_hi)])


def test_every_dispatch_class_is_reached():
    seen, luma_modes, chroma_modes = set(), set(), set()
    above_right_alone = 0
    for k in range(len(STILLS)):
        recs, _ = _case(k)
        for ctb, list_, w0, w1, w2, w3 in recs.tolist():
            f = _fields(w0, w1)
            form = ("4x4", "8x8", "general", "general")[f["lg"] - 2] if list_ == 0 else ("4x4" if f["lg"] == 2 else "general")
            kind, subst = (w1 >> 28) & 7, w1 >> 31
            seen.add((list_, form, kind)); seen.add((list_, kind, "subst", subst)); seen.add((list_, kind, "smooth", f["smooth"]))
            (chroma_modes if list_ else luma_modes).add(f["mode"])
            above_right_alone += int(not f["above"] and f["nt"] > 0)
    for form in ("4x4", "8x8", "general"):
        for kind in (PK_PLANAR, PK_DC, PK_PURE_EDGE, PK_POS, PK_NEG):
            assert (0, form, kind) in seen, "luma %s class %d" % (form, kind)
    for form in ("4x4", "general"):
        for kind in (PK_PLANAR, PK_DC, PK_POS, PK_NEG):
            assert (1, form, kind) in seen, "chroma %s class %d" % (form, kind)
    assert not any(s[0] == 1 and s[1] == PK_PURE_EDGE for s in seen if len(s) == 4), "the chroma pair has no boundary filters"
    for kind in (PK_PLANAR, PK_DC, PK_PURE_EDGE, PK_POS, PK_NEG):
        for subst in (0, 1):
            assert (0, kind, "subst", subst) in seen, "luma class %d, substitution %d" % (kind, subst)
        assert (0, kind, "smooth", 0) in seen
    for kind in (PK_PLANAR, PK_POS, PK_NEG):      # (DC and the pure modes are never smoothed)
        assert (0, kind, "smooth", 1) in seen, "luma class %d with smoothing" % kind
    assert luma_modes == set(range(35)), sorted(set(range(35)) - luma_modes)
    assert 34 in chroma_modes and len(chroma_modes) >= 5, sorted(chroma_modes)     # mode 34 (the substitute of a derived mode equal to a listed one) and derived modes
    assert above_right_alone > 0
