"""Scripts for the arithmetic-decoder probe (tests/probe/cabac_probe.hip) and what the plain reference (tests/cabac_ref.py) says they must give.
Shared by tests/test_cabac_engine_emu.py (CPU tier: the C++ forms) and tests/test_cabac_engine_gpu.py (the four device builds).

A Script is written operation by operation; every operation is run through the reference at once, so a script carries its expected records.
The mapping between the standard's terms and the probe's scaled-window state lives here, not in the probe:
    ivlCurrRange = range >> 7           ivlOffset = value >> 7
    bits consumed = 8 * (payload bytes read) + bits_needed + 1     (bits_needed in -8 .. -1; an emulation prevention byte is no payload byte)
    pStateIdx = 62 - p', p' the low half of the context variable (divided by 4 where the contexts live in LDS), valMps = bit 16
so a state that has consumed B bits has read m = ceil(B / 8) payload bytes, stands with bits_needed = B - 1 - 8 m, and its raw byte position is
one behind the raw index of payload byte m - 1 (an emulation prevention byte behind it is skipped only when the next byte is read).
The comparison is exact.  Bytes past the end of the substream read as 0 and the (m - n)-th of them sets DEV_ERR_BITSTREAM_END when m - n > 8."""
import ctypes as C
import fcntl
import os
import subprocess
from collections import Counter

import numpy as np

from cabac_ref import Engine, ERR_SYNTAX

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_DIR = os.path.join(HERE, "probe")

(OP_END, OP_START, OP_SET_CTX, OP_SET_STATE, OP_BIN, OP_BYPASS, OP_BYPASS_MULTI, OP_BYPASS_BITS, OP_TERMINATE, OP_UNARY, OP_G1_RUN, OP_SIG_RUN,
 OP_REMAINING_V, OP_REMAINING, OP_DUMP_CTX, OP_RESTART, OP_READ_BYTES) = range(17)
OP_NAMES = ["END", "START", "SET_CTX", "SET_STATE", "BIN", "BYPASS", "BYPASS_MULTI", "BYPASS_BITS", "TERMINATE", "UNARY", "G1_RUN", "SIG_RUN",
            "REMAINING_V", "REMAINING", "DUMP_CTX", "RESTART", "READ_BYTES"]
QUIET = 1 << 31
NOT_COMPARED = 99
REC_WORDS = 12
DEV_ERR_BITSTREAM_END, DEV_ERR_SYNTAX = 2, 3
DECODE_OPS = ["BIN", "BYPASS", "BYPASS_MULTI", "BYPASS_BITS", "TERMINATE", "UNARY", "G1_RUN", "SIG_RUN", "REMAINING_V", "REMAINING"]
# where a byte an operation had to fetch can lie (section C of the test plan)
BOUNDARY_KINDS = ["flim_last", "flim_first", "win_last", "win_first", "cand_window", "cand_first", "ep_skipped", "past_end"]

EMU_BUILDS = ["emu_rf", "emu_lds"]
GPU_BUILDS = ["rf", "lds", "rf_cxx", "lds_cxx"]


# ---- the probe libraries ---------------------------------------------------------------------------------------------------------------
_LIBS = {}


def probe(build):
    """the probe library of one build, made on demand (make under a file lock: pytest-xdist workers ask at the same time).  A compiler or an object
    that is missing fails the test."""
    if build not in _LIBS:
        name = "libcabac_probe_%s.so" % build
        with open(os.path.join(HERE, "emu", ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", PROBE_DIR, name])
        L = C.CDLL(os.path.join(PROBE_DIR, name))
        L.cabac_probe_run.restype = C.c_int
        L.cabac_probe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIBS[build] = L
    return _LIBS[build]


def is_lds(build):
    return "lds" in build


# ---- the raw buffer --------------------------------------------------------------------------------------------------------------------
class Buf:
    """one bitstream buffer per launch; substreams are placed at chosen offsets inside a 256-byte window.  The filler between substreams is 0x80
    (non-zero, as the last byte of every substream and of the slice segment header is: they end in an alignment bit)."""
    def __init__(self):
        self.data = bytearray()

    def place(self, payload, mod=None, lead=b""):
        """appends `lead` + payload so that the payload starts at an offset = mod (mod 256); returns (start, end)"""
        if self.data or lead or mod:          # (only the first substream may start at buffer offset 0)
            self.data.append(0x80)
        while mod is not None and (len(self.data) + len(lead)) % 256 != mod % 256:
            self.data.append(0x80)
        self.data += lead
        start = len(self.data)
        self.data += payload
        return start, len(self.data)

    def place_at(self, payload, offset):
        """the payload at exactly this buffer offset (filler in front)"""
        assert len(self.data) <= offset
        self.data += b"\x80" * (offset - len(self.data))
        self.data += payload
        return offset, len(self.data)

    def padded(self):
        """the padding the product gives its own bitstreams (batch_layout.hip: off = align_up(off + size + 512, 256), zeroed): the parser's window
        loads run up to 512 bytes past a substream's end"""
        n = len(self.data)
        alloc = (n + 512 + 255) & ~255
        a = np.zeros(alloc, np.uint8)
        a[:n] = np.frombuffer(bytes(self.data), np.uint8)
        return a, n, alloc


def window_has_candidate(raw, base):
    """a 03 behind a zero byte inside the window, or a 03 as its first byte (what is in front is not looked at: load_window's rule)"""
    w = raw[base:base + 256]
    if len(w) and w[0] == 3:
        return True
    return any(w[i] == 3 and w[i - 1] == 0 for i in range(1, len(w)))


# ---- a script and its expectation ------------------------------------------------------------------------------------------------------
class Script:
    def __init__(self, raw, start, end, name=""):
        self.raw, self.start, self.end, self.name = raw, start, end, name
        self.words = []
        self.rows = []       # (record offset, [op, result, range, offset, bits_needed, pos, err, pStateIdx, valMps, aux]); -1 = not compared
        self.dumps = []      # (record offset, group, {lane: (pStateIdx, valMps)}, is_baseline)
        self.rec_words = 0
        self.eng = None
        self.err = 0
        self.ctx_model = {}  # (group, lane) -> known by the reference
        self.bounds = Counter()   # (operation kind, boundary kind)
        self.ops = Counter()
        self.patch = []      # word indices of (group, lane) pairs, for retarget()
        self._cand = {}
        self._flim_prev = None

    # -- the mapping
    def _pos_of(self, m):
        n = len(self.eng.payload)
        if m == 0:
            return self.eng.start
        return self.eng.raw_idx[m - 1] + 1 if m <= n else self.end + (m - n)

    def _raw_of(self, i):
        n = len(self.eng.payload)
        return self.eng.raw_idx[i] if i < n else self.end + (i - n)

    def _classify(self, kind, fetched):
        n = len(self.eng.payload)
        for i in fetched:
            p = self._raw_of(i)
            k = []
            base = p & ~255
            if base not in self._cand:
                self._cand[base] = window_has_candidate(self.raw, base)
            if i >= n:
                k.append("past_end")
                if i - n + 1 > 8:
                    self.err = DEV_ERR_BITSTREAM_END
            if p == self.end:
                k.append("flim_first")
            elif p < self.end:
                if self._cand[base]:
                    k.append("cand_window")
                    if i > 0 and (self._raw_of(i - 1) & ~255) != base:
                        k.append("cand_first")      # the window is entered at its first payload byte, coming from the one in front
                elif p + 1 == min(base + 256, self.end):
                    k.append("flim_last")
                if p % 256 == 255:
                    k.append("win_last")
                if p % 256 == 0:
                    k.append("win_first")
                    if p > self.eng.start:
                        k.append("flim_first")
                if i > 0 and i < n and self.eng.raw_idx[i] - self.eng.raw_idx[i - 1] == 2:
                    k.append("ep_skipped")
            for x in k:
                self.bounds[(kind, x)] += 1

    def _zeros_at(self, pos):
        """the zero run the byte reader stands with at raw position pos, where it keeps one (windows with a candidate; it is recovered from the two
        bytes in front when such a window is entered at its first byte, so 2 stands for 2 or more); -1: not kept there"""
        if pos <= self.eng.start or pos > self.end or not window_has_candidate(self.raw, (pos - 1) & ~255):
            return -1
        z = 0
        while z < 2 and pos - 1 - z >= 0 and self.raw[pos - 1 - z] == 0:
            z += 1
        return z

    def _row(self, op, rec, quiet, ctx=None, aux=-1, zeros=False):
        kind = OP_NAMES[op]
        self.ops[kind] += 1
        self._classify(kind, rec.fetched)
        if rec.err == ERR_SYNTAX:
            self.err = DEV_ERR_SYNTAX
        if quiet:
            return
        m = (rec.bits + 7) >> 3
        p, mps = (-1, -1) if ctx is None else tuple(self.eng.ctx[ctx])
        # (the probe records 32 bits of a result: a coeff_abs_level_remaining beyond them is no conforming value)
        self.rows.append((self.rec_words, [op, rec.result & 0xffffffff, rec.rng << 7, rec.offset, rec.bits - 1 - 8 * m, self._pos_of(m), self.err, p, mps, aux,
                                           self._zeros_at(self._pos_of(m)) if zeros else -1]))
        self.rec_words += REC_WORDS

    def _emit(self, op, args, quiet):
        self.words.append(op | (QUIET if quiet else 0))
        self.words.extend(int(a) & 0xffffffff for a in args)

    # -- operations
    def START(self, quiet=False):
        self._emit(OP_START, [self.start, self.end], quiet)
        ctx = self.eng.ctx if self.eng else {}
        self.eng = Engine(self.raw, self.start, self.end)
        self.eng.ctx = ctx
        self._row(OP_START, self.eng.init(0), quiet)
        return self

    def SET_CTX(self, group, lane, p_state, mps):
        self.patch.append(len(self.words) + 1)
        self._emit(OP_SET_CTX, [group, lane, p_state, mps], True)
        self.eng.set_ctx((group, lane), p_state, mps)

    def SET_STATE(self, rng, offset, bits_needed, pos):
        """resume at raw position `pos` with the given engine state: the byte in front of pos holds the look-ahead bits (it must be a payload byte)"""
        assert self.start < pos <= self.end and -8 <= bits_needed <= -1
        z = 0
        while pos - 2 - z >= 0 and self.raw[pos - 2 - z] == 0 and z < 2:
            z += 1
        assert not (z >= 2 and self.raw[pos - 1] == 3)
        ctx, cells, shifts = self.eng.ctx, self.eng.cells, self.eng.shifts
        self.eng = Engine(self.raw, pos - 1, self.end, zeros=z)
        self.eng.ctx, self.eng.cells, self.eng.shifts = ctx, cells, shifts
        self.eng.bitpos = 9 + bits_needed
        self.eng.set_state(rng, offset)
        nla = -bits_needed - 1
        value = (offset << 7) | (self.eng.peek_bits(nla) << (7 - nla))
        zeros_at_pos = 0 if self.raw[pos - 1] != 0 else min(z + 1, 3)
        self._emit(OP_SET_STATE, [rng << 7, value, bits_needed, pos, zeros_at_pos], True)

    def BIN(self, group, lane, quiet=False):
        self.patch.append(len(self.words) + 1)
        self._emit(OP_BIN, [group, lane], quiet)
        r = self.eng.decision((group, lane))
        self._row(OP_BIN, r, quiet, ctx=(group, lane))
        return r

    def BYPASS(self, quiet=False):
        self._emit(OP_BYPASS, [], quiet)
        r = self.eng.bypass()
        self._row(OP_BYPASS, r, quiet)
        return r

    def BYPASS_MULTI(self, n, quiet=False):
        self._emit(OP_BYPASS_MULTI, [n], quiet)
        r = self.eng.bypass_bits(n)
        self._row(OP_BYPASS_MULTI, r, quiet)
        return r

    def BYPASS_BITS(self, n, quiet=False):
        self._emit(OP_BYPASS_BITS, [n], quiet)
        r = self.eng.bypass_bits(n)
        self._row(OP_BYPASS_BITS, r, quiet)
        return r

    def TERMINATE(self, quiet=False):
        self._emit(OP_TERMINATE, [], quiet)
        r = self.eng.terminate()
        self._row(OP_TERMINATE, r, quiet)
        return r

    def UNARY(self, group, base, shift, cmax, quiet=False):
        self._emit(OP_UNARY, [group, base, shift, cmax], quiet)
        r = self.eng.unary(lambda c: (group, c), base, shift, cmax)
        self._row(OP_UNARY, r, quiet)
        return r

    def G1_RUN(self, base, n, g, quiet=False):
        self._emit(OP_G1_RUN, [base, n, g], quiet)
        r = self.eng.g1_run(lambda c: (2, c), base, n, g)
        self._row(OP_G1_RUN, r, quiet, aux=r.aux)
        return r

    def SIG_RUN(self, n_start, idx, quiet=False):
        assert len(idx) == 16
        self._emit(OP_SIG_RUN, [n_start] + list(idx), quiet)
        r = self.eng.sig_run(lambda c: (1, c), idx, n_start)
        self._row(OP_SIG_RUN, r, quiet)
        return r

    def REMAINING_V(self, rice, quiet=False):
        self._emit(OP_REMAINING_V, [rice], quiet)
        r = self.eng.remaining(rice)
        self._row(OP_REMAINING_V, r, quiet)
        return r

    def REMAINING(self, rice, quiet=False):
        self._emit(OP_REMAINING, [rice], quiet)
        r = self.eng.remaining(rice)
        self._row(OP_REMAINING, r, quiet)
        return r

    def RESTART(self, quiet=False):
        """9.3.2.5 behind a terminating bin of 1 (pcm_flag, end_of_subset_one_bit): the engine has read 9 + (all shifts) bits, the last of them is the
        final 1 that the encoder's flush writes (9.3.4.3.5 / EncodeFlush: write_bits(((ivlLow >> 7) & 3) | 1, 2)), the bits up to the byte boundary
        are alignment zeros (7.3.8.7 pcm_alignment_zero_bit, 7.3.8.1 byte_alignment()), and what follows starts at the next byte boundary of the payload"""
        self._emit(OP_RESTART, [], quiet)
        self._row(OP_RESTART, self.eng.init(None), quiet, zeros=True)

    def READ_BYTES(self, n, quiet=False):
        """n PCM sample bytes behind pcm_flag (n <= 4: the record holds 32 bits)"""
        assert 1 <= n <= 4
        self._emit(OP_READ_BYTES, [n], quiet)
        r = self.eng.read_bytes(n)
        self._row(OP_READ_BYTES, r, quiet, zeros=True)
        if not quiet:       # the engine's own state means nothing between the terminating bin and 9.3.2.5: result, position, zero run and err only
            self.rows[-1][1][2:5] = [-1, -1, NOT_COMPARED]
        return r

    def DUMP(self, group, baseline=False):
        self._emit(OP_DUMP_CTX, [group], False)
        known = {l: tuple(v) for (g, l), v in self.eng.ctx.items() if g == group}
        self.dumps.append((self.rec_words, group, known, baseline))
        self.rec_words += 64

    def END(self):
        self.words.append(OP_END)
        return self


def run_scripts(build, buf, scripts):
    """one launch: every script over the one buffer; returns the record words of each script"""
    L = probe(build)
    bs, n, alloc = buf.padded()
    soff = np.zeros(len(scripts) + 1, np.uint32)
    roff = np.zeros(len(scripts) + 1, np.uint32)
    for i, s in enumerate(scripts):
        soff[i + 1] = soff[i] + len(s.words)
        roff[i + 1] = roff[i] + s.rec_words
    words = np.concatenate([np.asarray(s.words, np.uint32) for s in scripts]) if scripts else np.zeros(0, np.uint32)
    rec = np.full(int(roff[-1]) + 1, 0xdddddddd, np.uint32)
    rc = L.cabac_probe_run(words.ctypes.data, soff.ctypes.data, roff.ctypes.data, len(scripts), rec.ctypes.data, bs.ctypes.data, n, alloc)
    assert rc == 0, "probe %s: error %d" % (build, rc)
    return [rec[int(roff[i]):int(roff[i + 1])] for i in range(len(scripts))]


COLS = ["op", "result", "range", "ivlOffset", "bits_needed", "pos", "err", "pStateIdx", "valMps", "aux", "zeros"]


def _ctx_split(v, lds):
    lo = v & 0xffff
    if lds:
        assert np.all(lo % 4 == 0), "LDS context variable: low half not a multiple of 4"
        lo = lo >> 2
    return 62 - lo.astype(np.int64), (v >> 16).astype(np.int64)


def check(build, script, rec):
    """exact comparison of one script's records with the reference's"""
    lds = is_lds(build)
    if isinstance(script, BulkScript):
        off, exp = script.rows_off, script.rows_exp
    elif script.rows:
        off = np.array([o for o, _ in script.rows], np.int64)
        exp = np.array([r for _, r in script.rows], np.int64)
    else:
        off = None
    if off is not None and len(off):
        raw = rec[off[:, None] + np.arange(REC_WORDS)[None, :]].astype(np.int64)
        p, mps = _ctx_split(np.where(exp[:, 7] >= 0, raw[:, 9], 0).astype(np.uint32), lds)
        got = np.stack([raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3] >> 7, raw[:, 4].astype(np.uint32).astype(np.int32).astype(np.int64), raw[:, 5],
                        raw[:, 7], p, mps, raw[:, 10], np.minimum(raw[:, 8], 2)], axis=1)
        bad = (got != exp) & (exp >= 0)
        bad[:, 4] = (got[:, 4] != exp[:, 4]) & (exp[:, 4] != NOT_COMPARED)     # bits_needed is negative: compared unless marked
        if bad.any():
            i = int(np.argmax(bad.any(axis=1)))
            lines = ["%s %s: record %d (%s) differs in %s" % (build, script.name, i, OP_NAMES[int(exp[i, 0])], [COLS[c] for c in np.nonzero(bad[i])[0]])]
            for j in range(max(0, i - 2), i + 1):
                lines.append("  rec %d expected %s" % (j, dict(zip(COLS, exp[j].tolist()))))
                lines.append("  rec %d got      %s (fast_limit %d zeros %d win_base %#x)" % (j, dict(zip(COLS, got[j].tolist())), raw[j, 6], raw[j, 8], raw[j, 11]))
            raise AssertionError("\n".join(lines))
    base = {}
    for off, group, known, is_base in script.dumps:
        v = rec[off:off + 64]
        if is_base:
            base[group] = v.copy()
        p, mps = _ctx_split(v, lds)
        for lane in range(64):
            if lane in known:
                assert (int(p[lane]), int(mps[lane])) == known[lane], "%s %s: context (%d, %d) is %s, expected %s" % (
                    build, script.name, group, lane, (int(p[lane]), int(mps[lane])), known[lane])
            elif group in base:
                assert v[lane] == base[group][lane], "%s %s: untouched context (%d, %d) changed" % (build, script.name, group, lane)


def run_and_check(build, buf, scripts):
    recs = run_scripts(build, buf, scripts)
    for s, r in zip(scripts, recs):
        check(build, s, r)
    return recs


def retarget(script, group, lane_of):
    """the same script with every BIN / SET_CTX moved to another context home (the expectation does not change: it speaks of pStateIdx / valMps)"""
    import copy
    t = copy.copy(script)
    w = list(script.words)
    for i in script.patch:
        w[i], w[i + 1] = group, lane_of(w[i + 1])
    t.words = w
    return t


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def biased_bytes(rng, n):
    """uniform runs, runs of bytes below 16 and zero runs (so that context states climb); no byte string that would need emulation prevention
    is avoided: the reference removes what 7.4.2 removes"""
    out = bytearray()
    while len(out) < n:
        kind = rng.integers(0, 4)
        ln = int(rng.integers(4, 48))
        if kind <= 1:
            out += rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        elif kind == 2:
            out += rng.integers(0, 16, ln, dtype=np.uint8).tobytes()
        else:
            out += bytes(ln)
    return bytes(out[:n])


def make_cells_script(seed, n_bytes=4096, every=6):
    """section A: bins on one context through a biased byte string; the context is re-seeded every few bins at a random (pStateIdx, valMps), half
    of the time at a high pStateIdx, where an LPS is rare.  Built once, retargeted to every context home"""
    rng = np.random.default_rng(seed)
    buf = Buf()
    data = biased_bytes(rng, n_bytes)
    start, end = buf.place(data, mod=int(rng.integers(0, 256)))
    s = Script(buf.data, start, end, "cells seed %d" % seed)
    s.START()
    n = 0
    while s.eng.bitpos < n_bytes * 8 - 16:
        if n % every == 0:
            s.SET_CTX(0, 0, int(rng.integers(0, 63)) if rng.integers(0, 2) else int(rng.integers(44, 63)), int(rng.integers(0, 2)))
        s.BIN(0, 0)
        n += 1
    s.END()
    return buf, s


def edge_scripts():
    """section A, the named edges: pStateIdx 0 with an LPS (valMps flips), pStateIdx 62 with an MPS (saturates), a long all-MPS run, MPS / LPS in turn"""
    buf = Buf()
    out = []
    # a zero payload keeps ivlOffset at 0: every bin is an MPS, whatever the state; the state climbs to 62 and stays
    st, en = buf.place(bytes(64), mod=5)
    s = Script(buf.data, st, en, "all MPS")
    s.START()
    for lane, p0 in ((0, 0), (1, 61), (62, 62), (63, 30)):
        s.SET_CTX(1, lane, p0, lane & 1)
        for _ in range(90):
            r = s.BIN(1, lane)
            assert r.result == (lane & 1)
        assert s.eng.ctx[(1, lane)][0] == 62
    s.DUMP(1)
    out.append(s.END())
    # 0xff bytes drive ivlOffset to the top of the range: LPS after LPS walks the state down to 0, then every LPS flips valMps
    st, en = buf.place(b"\xfe" + b"\xff" * 95, mod=250)
    s = Script(buf.data, st, en, "LPS down to 0 and flips")
    s.START()
    s.SET_CTX(2, 63, 40, 1)
    flips = 0
    for _ in range(120):
        before = tuple(s.eng.ctx[(2, 63)])
        s.BIN(2, 63)
        flips += before[0] == 0 and s.eng.ctx[(2, 63)][1] != before[1]
    assert flips >= 3
    out.append(s.END())
    # alternating on one context: random bytes, state pinned low by re-seeding at pStateIdx 1
    rng = np.random.default_rng(77)
    st, en = buf.place(rng.integers(0, 256, 200, dtype=np.uint8).tobytes(), mod=100)
    s = Script(buf.data, st, en, "alternating")
    s.START()
    s.SET_CTX(0, 62, 1, 0)
    seq = ""
    for _ in range(400):
        before = s.eng.ctx[(0, 62)][1]
        r = s.BIN(0, 62)
        seq += "M" if r.result == before else "L"
    assert "MLML" in seq or "LMLM" in seq
    out.append(s.END())
    return buf, out


# (shift, max) of every call of decode_unary_ctx_run in parse_core.h: last_sig_coeff_x / y_prefix with log2TrafoSize 2 .. 5, luma
# (ctx_shift = (log2 + 1) >> 2, max = 2 * log2 - 1) and chroma (ctx_shift = log2 - 2; 4:4:4 has 32x32 chroma), plus max 0 and 1
UNARY_PAIRS = sorted({((l + 1) >> 2, 2 * l - 1) for l in (2, 3, 4, 5)} | {(l - 2, 2 * l - 1) for l in (2, 3, 4, 5)} | {(0, 0), (0, 1), (1, 1)})


def _lead_in(s, rng, k):
    for _ in range(k):
        s.BYPASS(quiet=True)


def run_case_scripts(seed, placements):
    """section B: every run case through random bytes, once per placement (offset of the substream in its window, bytes of payload, emulation
    prevention sequences spliced in): the runs are long enough to cross whatever boundary the placement puts in their way"""
    rng = np.random.default_rng(seed)
    buf = Buf()
    out = []

    def payload(n, splice):
        d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        for at, seq in splice:
            d[at:at + len(seq)] = seq
        return bytes(d)

    for mod, n, splice in placements:
        cases = []
        for n_start in range(1, 16):
            for pat in range(5):
                if pat == 0:
                    idx = [int(x) for x in rng.permutation(44)[:16]]          # all distinct
                elif pat == 1:
                    idx = [int(rng.integers(0, 44))] * 16                      # the same context at consecutive positions
                elif pat == 2:
                    a, b = (int(x) for x in rng.permutation(44)[:2])
                    idx = [a if k % 2 == 0 else b for k in range(16)]          # the same context at distance 2
                elif pat == 3:
                    idx = [int(x) for x in rng.permutation(62)[:16] + 1]
                    idx[1] = 0                                                 # the list ends in lane 0
                else:
                    idx = [int(x) for x in rng.permutation(62)[:16] + 1]
                    idx[1] = 63                                                # ... in lane 63
                    idx[n_start] = 0
                cases.append(("sig", n_start, idx))
        for ng in range(1, 9):
            for g in range(4):
                cases.append(("g1", int(rng.integers(0, 6)) * 4, ng, g))
        for shift, cmax in UNARY_PAIRS:
            for grp, base in ((0, 22), (0, 40), (1, 3), (2, 46)):
                cases.append(("unary", grp, base, shift, cmax))
        order = rng.permutation(len(cases))
        st, en = buf.place(payload(n, splice), mod=mod)
        s = Script(buf.data, st, en, "runs at %d (+%d bytes)" % (mod, n))
        s.START()
        for g in range(3):
            s.DUMP(g, baseline=True)
            for lane in range(64):
                s.SET_CTX(g, lane, int(rng.integers(0, 63)), int(rng.integers(0, 2)))
        for ci in order:
            c = cases[ci]
            if c[0] == "sig":
                s.SIG_RUN(c[1], c[2])
            elif c[0] == "g1":
                s.G1_RUN(c[1], c[2], c[3])
            else:
                s.UNARY(c[1], c[2], c[3], c[4])
        for g in range(3):
            s.DUMP(g)
        out.append(s.END())
    return buf, out


def forced_run_scripts():
    """section B: a 1 at every position / no 1 at all for G1_RUN, all ones up to max / a zero at every position for UNARY - forced through the
    context: with ivlOffset 0 (zero payload) every bin is the MPS, so valMps of each context chooses the bin"""
    buf = Buf()
    st, en = buf.place(bytes(48), mod=17)
    s = Script(buf.data, st, en, "forced runs")
    s.START()
    for n in range(1, 9):
        for g in range(4):
            for ones in (0, 1):
                for lane in range(4):
                    s.SET_CTX(2, 8 + lane, 20 + lane, ones)
                r = s.G1_RUN(8, n, g)
                assert r.result == ((1 << n) - 1 if ones else 0)
            # a single 1 at position k
            for k in range(n):
                for lane in range(4):
                    s.SET_CTX(2, 8 + lane, 10, 0)
                # position k is decoded with ctxInc min(g_k, 3); give exactly that context valMps 1 when no other position shares it
                gk, inc = g, []
                for _ in range(n):
                    inc.append(min(gk, 3))
                    gk = gk + 1 if gk > 0 else 0
                if inc.count(inc[k]) == 1:
                    s.SET_CTX(2, 8 + inc[k], 10, 1)
                    r = s.G1_RUN(8, n, g)
                    assert r.result == 1 << (n - 1 - k)
    for shift, cmax in UNARY_PAIRS:
        nctx = ((cmax - 1) >> shift) + 1 if cmax else 1
        for zero_at in range(cmax + 1):     # zero_at == cmax: all ones
            for c in range(nctx):
                s.SET_CTX(0, 22 + c, 5, 1)
            if zero_at < cmax:
                zc = zero_at >> shift
                if zero_at != zc << shift:   # the context of the 0 also served earlier 1s: not forceable through valMps
                    continue
                for c in range(zc, nctx):
                    s.SET_CTX(0, 22 + c, 5, 0)
            r = s.UNARY(0, 22, shift, cmax)
            assert r.result == zero_at, (shift, cmax, zero_at, r.result)
    s.DUMP(0)
    s.DUMP(2)
    out = [s.END()]
    return buf, out


# the placements of section C: (offset of the substream start in its window, payload bytes, [(at, bytes spliced in)])
EP = b"\x00\x00\x03"
PLACEMENTS = [
    # (substream starts at buffer offsets 0, 1, 2, 3, 255, 256 and 257 have buffers of their own: supply_scripts)
    # the first and the last byte of a window as the substream's start
    (0, 24, []), (255, 24, []),
    # across the window boundary; the substream's end (fast_limit = end) in the middle of a window, and right behind the start
    (236, 40, []), (100, 20, []), (100, 21, []), (250, 3, []), (250, 6, []), (254, 2, []),
    # 00 00 03 at each alignment across the window boundary (254 255 | 256, 255 | 256 257, 253 254 255 |, | 256 257 258)
    (230, 44, [(24, EP)]), (230, 44, [(25, EP)]), (230, 44, [(23, EP)]), (230, 44, [(26, EP)]),
    # in the middle of a window entered in the middle / at its first byte / from the window in front; back to back; as the last three bytes
    (10, 40, [(20, EP)]), (0, 40, [(20, EP)]), (236, 60, [(40, EP)]), (10, 40, [(20, EP + EP)]), (30, 30, [(27, EP)]),
    # false candidates
    (7, 60, [(10, b"\x01\x00\x03"), (20, b"\x00\x00\x00\x03"), (30, b"\x00\x00\x04"), (40, b"\x07\x00\x03")]),
    (250, 30, [(5, b"\x09\x03")]), (250, 30, [(4, b"\x09\x00\x03")]),
]


def supply_scripts(seed):
    """section C: every operation kind on every placement, at all eight bit alignments.  Returns [(Buf, scripts)]: the substreams that start at
    buffer offsets 0, 1, 2, 3, 255, 256 and 257 have a buffer of their own each"""
    rng = np.random.default_rng(seed)
    out = []
    shared = Buf()
    shared.place(b"\x80" * 7)
    groups = [(shared, [])]
    for off in (0, 1, 2, 3, 255, 256, 257):
        b = Buf()
        groups.append((b, []))
        st, en = b.place_at(rng.integers(0, 256, 24, dtype=np.uint8).tobytes(), off)
        _supply_on(rng, b, st, en, "offset %d" % off, groups[-1][1])
    for mod, n, splice in PLACEMENTS:
        d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        for at, seq in splice:
            d[at:at + len(seq)] = seq
        lead = b"\x00\x07" if mod >= 3 and not splice else b""   # a zero two bytes in front of a substream is not its business
        st, en = shared.place(bytes(d), mod=mod, lead=lead)
        _supply_on(rng, shared, st, en, "at %d (+%d)" % (mod, n), groups[0][1])
    return groups


def _supply_on(rng, buf, st, en, where, out):
    for kind in DECODE_OPS:
        for k in range(8):
            s = Script(buf.data, st, en, "%s %s lead-in %d" % (kind, where, k))
            s.START()
            for g in range(3):
                for lane in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 62, 63):
                    s.SET_CTX(g, lane, int(rng.integers(0, 12)), int(rng.integers(0, 2)))
            for _ in range(k):
                s.BYPASS(quiet=True)
            guard = 0
            if kind == "TERMINATE":
                # in front of every byte of the substream (and of the first one behind it), at bits_needed -1 - k (k: the script's number):
                #  - ivlCurrRange 257 / 256 at the last bit of the byte in front: 0 with the one renormalisation shift DecodeTerminate can have, which
                #    reads the byte (only there: at another bits_needed the shift reads none);
                #  - ivlCurrRange >= 258, ivlOffset below ivlCurrRange - 2: 0, no shift, nothing read;
                #  - ivlOffset = ivlCurrRange - 2 or - 1: 1, nothing read; then 9.3.2.5 at the next byte boundary (end of a substream), or PCM sample
                #    bytes first and then 9.3.2.5 (pcm_flag), and the engine goes on
                for t in range(st + 1, en + 1):
                    if buf.data[t - 1] == 3 and t >= 3 and buf.data[t - 2] == 0 and buf.data[t - 3] == 0:
                        continue        # (the byte in front is an emulation prevention byte: no state stands there)
                    bn = -1 - k
                    s.SET_STATE(257 - (t + k) % 2, int(rng.integers(0, 200)), -1, t)
                    assert s.TERMINATE().result == 0
                    s.BYPASS_MULTI(2 + k % 7)
                    r0 = int(rng.integers(258, 511))
                    s.SET_STATE(r0, int(rng.integers(0, r0 - 2)), bn, t)
                    before = s.eng.bitpos
                    assert s.TERMINATE().result == 0 and s.eng.bitpos == before
                    s.BYPASS_MULTI(2 + (k + 3) % 7)
                    r1 = int(rng.integers(256, 511))
                    s.SET_STATE(r1, r1 - 2 + (t + k) % 2, bn, t)
                    assert s.TERMINATE().result == 1
                    if (t + k) % 3:
                        s.READ_BYTES(1 + (t + k) % 4)
                    s.RESTART()
                    s.BYPASS_MULTI(2 + (k + 5) % 7)
                    s.BIN(0, 0)
            while kind != "TERMINATE" and s.eng.bitpos < 8 * (len(s.eng.payload) + 12) and guard < 4000:
                guard += 1
                if kind == "BIN":
                    s.BIN(guard % 3, (0, 1, 62, 63)[guard % 4])
                elif kind == "BYPASS":
                    s.BYPASS()
                elif kind == "BYPASS_MULTI":
                    s.BYPASS_MULTI(2 + guard % 7)
                elif kind == "BYPASS_BITS":
                    s.BYPASS_BITS((9, 16, 17, 24, 32, 1, 5)[guard % 7])
                elif kind == "UNARY":
                    s.UNARY(guard % 3, 0, guard % 2, 9)
                elif kind == "G1_RUN":
                    s.G1_RUN(0, 1 + guard % 8, guard % 4)
                elif kind == "SIG_RUN":
                    s.SIG_RUN(1 + guard % 15, [(0, 1, 2, 3, 20, 62, 63)[(guard + j) % 7] for j in range(16)])
                elif kind == "REMAINING_V":
                    s.REMAINING_V(guard % 5)
                else:
                    s.REMAINING(guard % 5)
                if s.err == DEV_ERR_SYNTAX:
                    break
            out.append(s.END())


# ---- section D: the divisions ---------------------------------------------------------------------------------------------------------
class BulkScript:
    """a script built with NumPy (hundreds of thousands of injected states): the same fields check() reads from a Script"""
    def __init__(self, name, words, rows_off, rows_exp):
        self.name, self.words, self.rec_words, self.dumps = name, words, int(len(rows_off)) * REC_WORDS, []
        self.rows_off, self.rows_exp = rows_off, rows_exp


def bypass_bins_np(rng_, offset, bits, n):
    """n steps of 9.3.4.3.4 DecodeBypass over arrays: bits[:, k] is the k-th bit read"""
    q = np.zeros_like(offset)
    for k in range(n):
        offset = (offset << 1) | bits[:, k]
        ge = offset >= rng_
        offset = offset - np.where(ge, rng_, 0)
        q = (q << 1) | ge
    return q, offset


def division_states(seed, full_n=(8,), full_bn=(-8, -3)):
    """the states of D for BYPASS_MULTI: arrays (n, bits_needed, R, q, r).  n = 8: every R x every q x r in {0, 1, R - 2, R - 1} at two values of
    bits_needed; n = 2 .. 7 (and n = 8 at the other six values of bits_needed): every R, q in {0, 1, 2^n - 2, 2^n - 1} and eight seeded q"""
    rng = np.random.default_rng(seed)
    R = np.arange(256, 511, dtype=np.int64)
    parts = []
    for n in range(2, 9):
        for bn in range(-8, 0):
            if n in full_n and bn in full_bn:
                qs = np.arange(1 << n, dtype=np.int64)
            else:
                qs = np.unique(np.concatenate([np.array([0, 1, (1 << n) - 2, (1 << n) - 1]), rng.integers(0, 1 << n, 8)])).astype(np.int64)
            RR, QQ, KK = np.meshgrid(R, qs, np.arange(4), indexing="ij")
            rr = np.where(KK == 0, 0, np.where(KK == 1, 1, np.where(KK == 2, RR - 2, RR - 1)))
            parts.append(np.stack([np.full(RR.size, n), np.full(RR.size, bn), RR.ravel(), QQ.ravel(), rr.ravel()], axis=1))
    return np.concatenate(parts)


def division_scripts(seed, n_scripts=256):
    """D for BYPASS_MULTI.  X = q R + r < R 2^n, ivlOffset = X >> n, the next n stream bits = X mod 2^n, the 7 bits behind them all 0 for r = 0 and
    all 1 for r = R - 1 (the scaled remainder is then 0 and range - 1 exactly), random otherwise.  A state is injected with SET_STATE (the way a
    parked row resumes) at the given bits_needed: the -bits_needed - 1 look-ahead bits of the scaled window are the first of those stream bits.
    Four bytes of the buffer per state: the byte in front of pos (unused high bits 1: never zero), two bytes, a filler."""
    st = division_states(seed)
    rng = np.random.default_rng(seed + 1)
    N = len(st)
    n, bn, R, q, r = (st[:, i] for i in range(5))
    X = q * R + r
    off0 = X >> n
    fill = np.where(r == 0, 0, np.where(r == R - 1, 127, rng.integers(0, 128, N)))
    # the stream behind the consumed bits: n bits of X, 7 filler bits, then ones (24 bits in all, left-aligned)
    S = (((X & ((1 << n) - 1)) << 7 | fill) << (24 - n - 7)) | ((1 << (24 - n - 7)) - 1)
    nla = -bn - 1
    look = S >> (24 - nla)
    rest = (S << nla) & 0xffffff
    b_prev = ((0xff << nla) & 0xff) | look
    b0, b1 = rest >> 16, (rest >> 8) & 255
    buf = Buf()
    base = 4
    raw = np.full(base + 4 * N + 4, 0x55, np.uint8)
    raw[base + 0:base + 4 * N:4] = b_prev
    raw[base + 1:base + 4 * N:4] = b0
    raw[base + 2:base + 4 * N:4] = b1
    buf.data = bytearray(raw.tobytes())
    end = len(buf.data)
    pos = base + 4 * np.arange(N) + 1
    value = (off0 << 7) | (look << (7 - nla))
    # the reference: n DecodeBypass steps over the stream bits
    bits = np.stack([(S >> (23 - k)) & 1 for k in range(8)], axis=1)
    q_ref, r_ref = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for nn in range(2, 9):
        m = n == nn
        q_ref[m], r_ref[m] = bypass_bins_np(R[m], off0[m], bits[m], nn)
    assert np.array_equal(q_ref, q) and np.array_equal(r_ref, r), "the construction does not give the quotient / remainder it names"
    took = (bn + n) >= 0
    exp = np.stack([np.full(N, OP_BYPASS_MULTI), q_ref, R << 7, r_ref, np.where(took, bn + n - 8, bn + n), pos + took, np.zeros(N, np.int64),
                    np.full(N, -1), np.full(N, -1), np.full(N, -1), np.full(N, -1)], axis=1)
    w = np.stack([np.full(N, OP_SET_STATE | QUIET), R << 7, value, bn & 0xffffffff, pos, np.zeros(N, np.int64), np.full(N, OP_BYPASS_MULTI), n], axis=1)
    scripts = []
    per = (N + n_scripts - 1) // n_scripts
    head = np.array([OP_START | QUIET, 0, end], np.int64)
    for k in range(n_scripts):
        sl = slice(k * per, min(N, (k + 1) * per))
        if sl.start >= N:
            break
        words = np.concatenate([head, w[sl].ravel(), [OP_END]]).astype(np.uint32)
        cnt = sl.stop - sl.start
        scripts.append(BulkScript("divisions %d" % k, words, np.arange(cnt, dtype=np.int64) * REC_WORDS, exp[sl]))
    return buf, scripts, st


def bypass_bits_scripts(seed, n_states=1500):
    """D for BYPASS_BITS: n = 9, 16, 17, 24 and 32 (two to four divisions, single bins for a rest of one or two) over random injected states: any
    ivlCurrRange, any ivlOffset below it, every bits_needed, random bytes behind (emulation prevention sequences among them as chance has it)"""
    rng = np.random.default_rng(seed)
    buf = Buf()
    st, en = buf.place(rng.integers(0, 256, 8 * n_states + 16, dtype=np.uint8).tobytes(), mod=3)
    scripts = []
    per = 100
    for k0 in range(0, n_states, per):
        s = Script(buf.data, st, en, "bypass_bits %d" % k0)
        s.START(quiet=True)
        for k in range(k0, min(n_states, k0 + per)):
            pos = st + 2 + 8 * k
            if buf.data[pos - 1] == 3 and buf.data[pos - 2] == 0 and buf.data[pos - 3] == 0:
                pos += 1
            R = int(rng.integers(256, 511))
            s.SET_STATE(R, int(rng.integers(0, R)), -1 - k % 8, pos)
            s.BYPASS_BITS((9, 16, 17, 24, 32)[(k // 8) % 5])
        scripts.append(s.END())
    return buf, scripts


def rem_code(rice, prefix, suffix=None):
    """the bins of coeff_abs_level_remaining with this prefix and suffix (default 0101...; 9.3.3.11): returns (bins as a string, value)"""
    slen = rice if prefix <= 3 else prefix - 3 + rice
    suffix = ((1 << slen) - 1) & (0x55555555 if suffix is None else suffix)
    bins = "1" * prefix + "0" + (format(suffix, "0%db" % slen) if slen else "")
    val = (prefix << rice) + suffix if prefix <= 3 else (((1 << (prefix - 3)) + 2) << rice) + suffix
    return bins, val


def remaining_scripts(seed):
    """D for REMAINING_V: rice 0 .. 4, every prefix 0 .. 32 (codes of 1 .. 32 bins and longer: one division, two divisions, the bin-by-bin form,
    prefix 32 refused), at every bits_needed, with the remainder of the first / the second division on its edges, on three placements: inside a
    window without candidates, with the first looked-at byte the last one before fast_limit, and inside a window with a candidate.
    Returns (buf, scripts, expected path counts [one division, two, bin by bin, ... of those because of the window])"""
    rng = np.random.default_rng(seed)
    buf = Buf()
    scripts = []
    paths = [0, 0, 0, 0]
    pending = []
    for place in ("free", "limit", "cand"):
        s = None
        for rice in range(5):
            for prefix in range(33):
                code, val = rem_code(rice, prefix) if prefix < 32 else ("1" * 32, 0)
                L = len(code)
                for k in range(8):
                    edge = (prefix + k + rice) % 5          # 0 .. 3: r in {0, 1, R - 2, R - 1}, 4: random
                    R = int(rng.integers(256, 511))
                    lead = 1 + k                           # quiet bypass bins (all 0) in front: the first loads the window, the others move bits_needed
                    div_bins = 8 if L <= 8 else (16 if L <= 16 else L)
                    tail = "".join("01"[int(x)] for x in rng.integers(0, 2, max(0, div_bins - L)))
                    if L <= 16 and L + len(tail) == div_bins and "0" not in (code + tail)[:div_bins]:
                        tail = "0" + tail[1:]
                    B = int("0" * lead + code + tail, 2)
                    nb = lead + L + len(tail)
                    r = (0, 1, R - 2, R - 1)[edge] if edge < 4 else int(rng.integers(0, R))
                    X = B * R + r
                    fill = 0 if r == 0 else (127 if r == R - 1 else int(rng.integers(0, 128)))
                    stream = ((X & ((1 << nb) - 1)) << 7) | fill
                    nbits = nb + 7
                    pad = (-nbits) % 8
                    data = ((stream << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big") + b"\xaa\xab"
                    if place == "free":
                        st, en = buf.place(b"\x91" + data + b"\x80" * 4, mod=int(rng.integers(0, 200)))
                    elif place == "limit":
                        st, en = buf.place(b"\x91" + data[:1], mod=int(rng.integers(0, 200)))   # the substream ends behind the first looked-at ... byte
                        # (the bytes behind the end read as 0: the reference decodes what is there)
                    else:
                        st, en = buf.place(b"\x91" + data + b"\x80\x00\x03\x80", mod=int(rng.integers(0, 150)))
                    s = Script(buf.data, st, en, "remaining %s rice %d prefix %d lead %d" % (place, rice, prefix, lead))
                    s.START(quiet=True)
                    s.SET_STATE(R, X >> nb, -1, st + 1)
                    for _ in range(lead):
                        assert s.BYPASS(quiet=True).result == 0
                    pos_before = s._pos_of((s.eng.bitpos + 7) >> 3)
                    rec = s.REMAINING_V(rice)
                    if place == "free" and len(s.eng.payload) == en - st:   # (unless the bytes happen to hold an emulation prevention sequence)
                        assert (rec.result, rec.aux) == (val, prefix), (rec, val, prefix, bytes(buf.data[st:en]).hex())
                    p_ = rec.aux
                    pending.append((pos_before, en, 32 if p_ >= 32 else p_ + 1 + (rice if p_ <= 3 else p_ - 3 + rice)))
                    s.BYPASS_MULTI(5)
                    scripts.append(s.END())
    # the two-division path with BOTH remainders on an edge.  The first eight bins b1 leave r1 = X1 - b1 R; the second division divides
    # 256 r1 + (the next 8 stream bits) = b2 R + r2.  With R >= 256 and 8 free bits that has a solution for (r1, r2) in {0, 1} x {0, 1} (b2 = r1,
    # bits = r1 (R - 256) + r2) and for r1 = R - 1, r2 in {R - 1, R - 2} (b2 = 255, bits = r2 - R + 256): the others do not exist.  b2 is then
    # given, so the codes are those whose bins 8 .. 15 are free: prefix <= 7 with 9 .. 16 bins, the suffix and the bins behind the code chosen to fit
    for rice in range(5):
        for prefix in range(8):
            slen = rice if prefix <= 3 else prefix - 3 + rice
            L = prefix + 1 + slen
            if not 9 <= L <= 16:
                continue
            for k in range(8):
                for r1k, r2k in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (2, 3)):
                    R = int(rng.integers(256, 511))
                    r1 = (0, 1, R - 1)[r1k]
                    r2 = (0, 1, R - 1, R - 2)[r2k]
                    b2 = r1 if r1k < 2 else 255
                    bits2 = r1 * (R - 256) + r2 if r1k < 2 else r2 - R + 256
                    assert 0 <= bits2 <= 255 and 256 * r1 + bits2 == b2 * R + r2
                    free1 = int(rng.integers(0, 1 << (7 - prefix))) if prefix < 7 else 0
                    b1 = (((1 << prefix) - 1) << (8 - prefix)) | free1              # prefix ones, the 0, the first suffix bits
                    bins16 = (b1 << 8) | b2
                    suffix = (bins16 >> (16 - L)) & ((1 << slen) - 1)
                    code, val = rem_code(rice, prefix, suffix)
                    assert format(bins16, "016b").startswith(code)
                    lead = 1 + k
                    nb = lead + 8
                    X = b1 * R + r1
                    fill = 0 if r2 == 0 else (127 if r2 == R - 1 else int(rng.integers(0, 128)))
                    stream = ((((X & ((1 << nb) - 1)) << 8) | bits2) << 7) | fill
                    nbits = nb + 15
                    pad = (-nbits) % 8
                    data = ((stream << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big") + b"\xaa\xab"
                    st, en = buf.place(b"\x91" + data + b"\x80" * 4, mod=int(rng.integers(0, 200)))
                    s = Script(buf.data, st, en, "remaining two edges rice %d prefix %d lead %d r1 %d r2 %d" % (rice, prefix, lead, r1, r2))
                    s.START(quiet=True)
                    s.SET_STATE(R, X >> nb, -1, st + 1)
                    for _ in range(lead):
                        assert s.BYPASS(quiet=True).result == 0
                    pos_before = s._pos_of((s.eng.bitpos + 7) >> 3)
                    rec = s.REMAINING_V(rice)
                    clean = len(s.eng.payload) == en - st
                    if clean:
                        assert (rec.result, rec.aux) == (val, prefix), (rec, val, prefix)
                    pending.append((pos_before, en, rec.aux + 1 + (rice if rec.aux <= 3 else rec.aux - 3 + rice)))
                    s.BYPASS_MULTI(5)
                    scripts.append(s.END())
    # which path decode_remaining_v has to take for each code (once the buffer is complete: a later substream may put a candidate into the window)
    for pos_before, en, length in pending:
        base = pos_before & ~255
        flim = 0 if window_has_candidate(buf.data, base) else min(base + 256, en)
        if not pos_before < flim:
            paths[2] += 1
            paths[3] += 1
        elif length <= 8:       # (behind the end of a substream the bytes read as 0: the code is what the reference decoded)
            paths[0] += 1
        elif length <= 16 and pos_before + 1 < flim:
            paths[1] += 1
        else:
            paths[2] += 1
    return buf, scripts, paths


# ---- the checks, shared by both tiers --------------------------------------------------------------------------------------------------
import functools

CELL_SEEDS = (11, 12, 13)
HOMES = [(g, l) for g in range(3) for l in (0, 1, 62, 63)]


@functools.lru_cache(maxsize=None)
def cells_case(seed):
    buf, s = make_cells_script(seed)
    # condition A, on the reference's own counters: all 63 x 4 x 2 cells, MPS shifts 0 and 1, LPS shifts 1 .. 6
    cells = {(p, q, k) for p in range(63) for q in range(4) for k in "ML"}
    missing = cells - set(s.eng.cells)
    assert not missing, "seed %d: the reference does not reach %d cells, e.g. %s" % (seed, len(missing), sorted(missing)[:5])
    need = {("M", 0), ("M", 1)} | {("L", n) for n in range(1, 7)}
    assert need <= set(s.eng.shifts), "seed %d: renormalisation shifts %s not reached" % (seed, sorted(need - set(s.eng.shifts)))
    assert not [k for k in s.eng.shifts if k not in need], "a shift count the standard does not allow"
    return buf, s


def suite_cells(build, seed):
    buf, s = cells_case(seed)
    scripts = [retarget(s, g, lambda _l, l=l: l) for g, l in HOMES]
    for t, (g, l) in zip(scripts, HOMES):
        t.name = "%s home (%d, %d)" % (s.name, g, l)
    run_and_check(build, buf, scripts)


@functools.lru_cache(maxsize=None)
def _edges():
    return edge_scripts()


def suite_edges(build):
    run_and_check(build, *_edges())


@functools.lru_cache(maxsize=None)
def _runs(seed):
    return run_case_scripts(seed, [(13, 420, []), (200, 420, [(30, EP), (100, EP), (200, EP), (300, EP + EP)]), (251, 420, [(2, EP)]), (100, 90, [])])


def suite_runs(build, seed):
    run_and_check(build, *_runs(seed))


@functools.lru_cache(maxsize=None)
def _forced():
    return forced_run_scripts()


def suite_forced_runs(build):
    run_and_check(build, *_forced())


@functools.lru_cache(maxsize=None)
def _supply():
    groups = supply_scripts(5)
    total = Counter()
    for _, scripts in groups:
        for s in scripts:
            total.update(s.bounds)
    # condition C, on the reference's own counters: every boundary kind for every operation kind
    missing = [(k, b) for k in DECODE_OPS for b in BOUNDARY_KINDS if not total[(k, b)]]
    assert not missing, "no refill of these operation kinds falls on these boundaries: %s" % missing
    return groups, total


def suite_supply(build):
    groups, _ = _supply()
    for buf, scripts in groups:
        run_and_check(build, buf, scripts)


@functools.lru_cache(maxsize=None)
def _divisions():
    return division_scripts(3)


def suite_divisions(build):
    """returns how often the quotient estimate needed each repair: {-1, 0, +1: count} (the estimate is the probe's, see OP_BYPASS_MULTI there)"""
    buf, scripts, _ = _divisions()
    recs = run_and_check(build, buf, scripts)
    rep = Counter()
    for r in recs:
        a = r.reshape(-1, REC_WORDS).astype(np.int64)
        d, c = np.unique(a[:, 1] - a[:, 10], return_counts=True)
        rep.update(dict(zip(d.tolist(), c.tolist())))
    return rep


@functools.lru_cache(maxsize=None)
def _bypass_bits():
    return bypass_bits_scripts(21)


def suite_bypass_bits(build):
    run_and_check(build, *_bypass_bits())


@functools.lru_cache(maxsize=None)
def _remaining():
    return remaining_scripts(9)


def suite_remaining(build):
    buf, scripts, paths = _remaining()
    L = probe(build)
    counts = (C.c_uint64 * 8)()
    if build.startswith("emu"):
        L.cabac_probe_path_counts(counts)
    run_and_check(build, buf, scripts)
    if build.startswith("emu"):     # which path decode_remaining_v took: the counters of the host build (PC_COUNT)
        L.cabac_probe_path_counts(counts)
        assert list(counts)[:4] == paths and min(paths) > 0, "paths taken %s, expected %s" % (list(counts)[:4], paths)
