"""A plain, bit-serial restatement of the arithmetic decoding engine of ITU-T H.265 9.3.4.3, in the standard's own terms: a 9-bit ivlCurrRange,
ivlOffset, read_bits(1), pStateIdx / valMps per context, tables 9-46 and 9-47 typed in from the standard.  It shares nothing with
libheif_amd/csrc/parse_core.h, parse_tables.h or oracle/: tests/test_cabac_engine_emu.py::test_tables_equal_the_parsers is the only place where the
two meet.  Emulation prevention bytes are removed up front (7.4.2, 7.3.1.1) before any bit is read; bytes past the end of the substream read as 0.

Every operation returns a Rec: result, ivlCurrRange, ivlOffset, bits consumed so far, the (context id, pStateIdx, valMps) of every context it
touched, and the unescaped byte indices the engine had to fetch for it (the tests classify those by where they lie in the raw buffer)."""
from collections import Counter, namedtuple

# Table 9-46 - rangeTabLps[pStateIdx][qRangeIdx]
RANGE_TAB_LPS = [
    [128, 176, 208, 240], [128, 167, 197, 227], [128, 158, 187, 216], [123, 150, 178, 205], [116, 142, 169, 195], [111, 135, 160, 185],
    [105, 128, 152, 175], [100, 122, 144, 166], [95, 116, 137, 158], [90, 110, 130, 150], [85, 104, 123, 142], [81, 99, 117, 135],
    [77, 94, 111, 128], [73, 89, 105, 122], [69, 85, 100, 116], [66, 80, 95, 110], [62, 76, 90, 104], [59, 72, 86, 99],
    [56, 69, 81, 94], [53, 65, 77, 89], [51, 62, 73, 85], [48, 59, 69, 80], [46, 56, 66, 76], [43, 53, 63, 72],
    [41, 50, 59, 69], [39, 48, 56, 65], [37, 45, 54, 62], [35, 43, 51, 59], [33, 41, 48, 56], [32, 39, 46, 53],
    [30, 37, 43, 50], [29, 35, 41, 48], [27, 33, 39, 45], [26, 31, 37, 43], [24, 30, 35, 41], [23, 28, 33, 39],
    [22, 27, 32, 37], [21, 26, 30, 35], [20, 24, 29, 33], [19, 23, 27, 31], [18, 22, 26, 30], [17, 21, 25, 28],
    [16, 20, 23, 27], [15, 19, 22, 25], [14, 18, 21, 24], [14, 17, 20, 23], [13, 16, 19, 22], [12, 15, 18, 21],
    [12, 14, 17, 20], [11, 14, 16, 19], [11, 13, 15, 18], [10, 12, 15, 17], [10, 12, 14, 16], [9, 11, 13, 15],
    [9, 11, 12, 14], [8, 10, 12, 14], [8, 9, 11, 13], [7, 9, 11, 12], [7, 9, 10, 12], [7, 8, 10, 11],
    [6, 8, 9, 11], [6, 7, 9, 10], [6, 7, 8, 9], [2, 2, 2, 2]]
# Table 9-47 - state transitions
TRANS_IDX_LPS = [0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
                 24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63]
TRANS_IDX_MPS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
                 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 62, 63]

ERR_SYNTAX = "syntax"   # coeff_abs_level_remaining: a prefix of 32 ones (9.3.3.11 bounds it)

Rec = namedtuple("Rec", "result rng offset bits ctxs fetched err aux")


def unescape(raw, start, end, zeros=0):
    """7.3.1.1 / 7.4.2 over raw[start:end]: returns (payload bytes, raw index of each payload byte).  A 0x03 behind two zero bytes is an
    emulation_prevention_three_byte and carries no payload - also as the last byte (7.3.1.1 tests i + 2 < NumBytesInNalUnit: the byte at
    i + 2 may be the last one; it is there behind cabac_zero_words).  `zeros`: the zero run in front of `start`."""
    out, idx = bytearray(), []
    z = zeros
    for i in range(start, end):
        b = raw[i]
        if z >= 2 and b == 3:
            z = 0
            continue
        z = z + 1 if b == 0 else 0
        out.append(b)
        idx.append(i)
    return bytes(out), idx


class Engine:
    def __init__(self, raw, start, end, zeros=0):
        self.raw, self.start, self.end = raw, start, end
        self.payload, self.raw_idx = unescape(raw, start, end, zeros)
        self.bitpos = 0            # bits consumed, in the payload
        self.rng, self.offset = 510, 0
        self.ctx = {}              # context id -> [pStateIdx, valMps]
        self.err = None
        self._fetched = []
        # counters of its own
        self.cells = Counter()     # (pStateIdx, qRangeIdx, 'M' / 'L')
        self.shifts = Counter()    # ('M' / 'L', renormalisation shifts)

    # ---- bits
    def read_bit(self):
        i = self.bitpos >> 3
        if (self.bitpos & 7) == 0:
            self._fetched.append(i)
        b = self.payload[i] if i < len(self.payload) else 0
        v = (b >> (7 - (self.bitpos & 7))) & 1
        self.bitpos += 1
        return v

    def peek_bits(self, n):
        """the next n bits, not consumed (the tests build the look-ahead bits of the probe's scaled window from them)"""
        v = 0
        for k in range(self.bitpos, self.bitpos + n):
            b = self.payload[k >> 3] if (k >> 3) < len(self.payload) else 0
            v = (v << 1) | ((b >> (7 - (k & 7))) & 1)
        return v

    def _rec(self, result, ctxs=(), aux=None):
        f, self._fetched = self._fetched, []
        return Rec(result, self.rng, self.offset, self.bitpos, tuple((c, self.ctx[c][0], self.ctx[c][1]) for c in ctxs), tuple(f), self.err, aux)

    # ---- 9.3.2.5 initialisation, at a payload byte boundary (None: where the engine stands, aligned up)
    def init(self, at_byte=None):
        if at_byte is None:
            at_byte = (self.bitpos + 7) >> 3
        self.bitpos = at_byte * 8
        self.rng, self.offset = 510, 0
        for _ in range(9):
            self.offset = (self.offset << 1) | self.read_bit()
        return self._rec(0)

    def read_bytes(self, n):
        """n byte-aligned payload bytes behind a terminating bin of 1 (7.3.8.7: pcm_alignment_zero_bit up to the byte boundary, then pcm_sample data);
        result: the bytes, first one in the highest place"""
        self.bitpos = ((self.bitpos + 7) >> 3) * 8
        v = 0
        for _ in range(n * 8):
            v = (v << 1) | self.read_bit()
        return self._rec(v)

    def set_state(self, rng, offset):
        self.rng, self.offset = rng, offset

    def set_ctx(self, cid, p_state, mps):
        self.ctx[cid] = [p_state, mps]

    # ---- 9.3.4.3.2 DecodeDecision (with 9.3.4.3.3 RenormD)
    def _decision(self, cid):
        st = self.ctx[cid]
        p, mps = st
        q = (self.rng >> 6) & 3
        lps = RANGE_TAB_LPS[p][q]
        self.rng -= lps
        if self.offset >= self.rng:
            kind, binval = 'L', 1 - mps
            self.offset -= self.rng
            self.rng = lps
            if p == 0:
                st[1] = 1 - mps
            st[0] = TRANS_IDX_LPS[p]
        else:
            kind, binval = 'M', mps
            st[0] = TRANS_IDX_MPS[p]
        self.cells[(p, q, kind)] += 1
        n = 0
        while self.rng < 256:
            self.rng <<= 1
            self.offset = (self.offset << 1) | self.read_bit()
            n += 1
        self.shifts[(kind, n)] += 1
        return binval

    def decision(self, cid):
        return self._rec(self._decision(cid), (cid,))

    # ---- 9.3.4.3.4 DecodeBypass
    def _bypass(self):
        self.offset = (self.offset << 1) | self.read_bit()
        if self.offset >= self.rng:
            self.offset -= self.rng
            return 1
        return 0

    def bypass(self):
        return self._rec(self._bypass())

    def _bypass_bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self._bypass()
        return v

    def bypass_bits(self, n):
        return self._rec(self._bypass_bits(n))

    # ---- 9.3.4.3.5 DecodeTerminate
    def terminate(self):
        self.rng -= 2
        if self.offset >= self.rng:
            return self._rec(1)    # no renormalisation; the engine has finished
        n = 0
        while self.rng < 256:
            self.rng <<= 1
            self.offset = (self.offset << 1) | self.read_bit()
            n += 1
        self.shifts[('T', n)] += 1
        return self._rec(0)

    # ---- runs of context-coded bins
    def unary(self, ctx_of, base, shift, cmax):
        """truncated unary prefix: bin i uses context base + (i >> shift); stops at a 0 or after cmax ones (9.3.3.2 with the ctxInc of
        last_sig_coeff_prefix, 9.3.4.2.3).  ctx_of maps a context index to a context id."""
        i, touched = 0, []
        while i < cmax:
            cid = ctx_of(base + (i >> shift))
            if cid not in touched:
                touched.append(cid)
            if not self._decision(cid):
                break
            i += 1
        return self._rec(i, touched)

    def g1_run(self, ctx_of, base, n, g):
        """n coeff_abs_level_greater1_flag bins, ctxInc = min(greater1Ctx, 3); greater1Ctx becomes 0 behind a 1 and counts up behind a 0
        while it is > 0 (9.3.4.2.6).  Result: the flags, first one in bit n - 1; aux: greater1Ctx behind the run."""
        bits, touched = 0, []
        for _ in range(n):
            cid = ctx_of(base + min(g, 3))
            if cid not in touched:
                touched.append(cid)
            b = self._decision(cid)
            bits = (bits << 1) | b
            if b:
                g = 0
            elif g > 0:
                g += 1
        return self._rec(bits, touched, aux=g)

    def sig_run(self, ctx_of, idx, n_start):
        """sig_coeff_flag of the scan positions n_start .. 1, context index idx[k] at position k; bit k of the result = position k"""
        sig, touched = 0, []
        for k in range(n_start, 0, -1):
            cid = ctx_of(idx[k])
            if cid not in touched:
                touched.append(cid)
            sig |= self._decision(cid) << k
        return self._rec(sig, touched)

    # ---- 9.3.3.11 coeff_abs_level_remaining: prefix of ones (at most 4 of them TR, then EGk), all bypass
    def remaining(self, rice):
        prefix = 0
        while prefix < 32 and self._bypass():
            prefix += 1
        if prefix >= 32:          # no conforming value has it (9.3.3.11: the prefix is bounded at 32)
            self.err = ERR_SYNTAX
            return self._rec(0, aux=32)
        if prefix <= 3:
            v = (prefix << rice) + self._bypass_bits(rice)
        else:
            v = (((1 << (prefix - 3)) + 3 - 1) << rice) + self._bypass_bits(prefix - 3 + rice)
        return self._rec(v, aux=prefix)

    # ---- 9.3.3.5 k-th order Exp-Golomb
    def egk(self, k):
        v = 0
        while self._bypass():
            v += 1 << k
            k += 1
            if k > 32:
                self.err = ERR_SYNTAX
                return self._rec(0)
        v += self._bypass_bits(k)
        return self._rec(v)
