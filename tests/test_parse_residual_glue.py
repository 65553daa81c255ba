"""CPU check of the lean residual_coding glue of the throughput parser (HIPDEC_PARSE_LEAN_GLUE, implied by HIPDEC_PARSE_LDS_CTX): small stills that
reach every branch the shorter form touches - 4x4 blocks with transform_skip, 8x8 .. 32x32 luma and 4x4 / 8x8 chroma blocks, the three scan orders at
4x4 and 8x8, a last position in the first and in the last sub-block, coded_sub_block_flag inferred and decoded with the right / lower neighbour on and
off, sign data hiding on and off, cu_transquant_bypass, cu_qp_delta, 4:2:2 and 4:4:4 (the emulation compiles the switch into the general-chroma
form too; on the GPU only the 4:2:0 throughput kernel has it), and level-torture streams on both sides of the 16-bit range check.  That each branch
was TAKEN is asserted on the emulator's counters (PC_GLUE in parse_core.h).  Parsed by the host emulation of the throughput build under the work
pool; coefficients, the five maps, SAO parameters and planes against the oracle, and raw maps, coefficients and hand-off records byte for byte
against the build without the switch (libparse_emu.so: register-file contexts, plain glue)."""
import ctypes as C
import numpy as np
import pytest

import test_parse_emu as T
import test_pipeline_emu as PE
import test_parse_unit_maps_lds as U
import value_extremes as vx
from oracle import pyoracle as orc

# (width, height, chroma_format_idc, encoder settings); the first eight are the stills of tests/test_parse_unit_maps_lds.py
CASES = [(w, h, 1, cfg) for w, h, cfg in U.CASES] + [
    (72, 40, 1, dict(transform_skip=1, stress=1)),
    (72, 40, 1, dict(lossless_pct=30, stress=1)),
    (72, 40, 1, dict(sign_data_hiding=0, stress=1)),
    (64, 64, 1, dict(stress=1, qp=4)),                       # busy blocks: last positions in the last sub-block, both neighbours coded
    (64, 64, 1, dict(qp=40)),                                # quiet blocks: only the DC sub-block coded
    (72, 40, 2, dict(stress=1)),
    (72, 40, 3, dict(stress=1, transform_skip=1)),
]
IDS = ["%dx%d,cf%d,%s" % (w, h, cf, ",".join("%s=%s" % kv for kv in c.items())) for w, h, cf, c in CASES]
GPU_CASES = [k for k, c in enumerate(CASES) if c[2] == 1]    # what k_parse_occ8 is launched for
_streams = {}
_state = {}


def stream(k):
    if k not in _streams:
        w, h, cf, cfg = CASES[k]
        _streams[k] = orc.encode(orc.synth_image(w, h, 8, cf, seed=700 + k), **cfg)
    return _streams[k]


def torture(kind, seed=50, **kw):
    return vx.tortured_still(72, 40, 8, 1, kind=kind, stress=1, pct=100, seed=seed, **kw)


def _glue_counts(libs, reset=False):
    """the branch counters of parse_core.h; the array is one object per library, or ONE per process where the loader unifies it: the maximum serves both"""
    arrs = [(C.c_uint64 * 32).in_dll(L, "hipdec_emu_glue_counts") for L in libs]
    out = [max(a[k] for a in arrs) for k in range(32)]
    if reset:
        for a in arrs:
            for k in range(32): a[k] = 0
    return out


def _path_counts(L):
    out = (C.c_uint64 * 8)()
    L.emu_path_counts(out)
    return list(out)


@pytest.fixture(scope="module")
def parsed():
    """every still parsed ONCE by each build (lean glue first, its counters read before the other build runs)"""
    if _state: return _state
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("HIPDEC_PARSE_POOL", "1")
        mp.setenv("HIPDEC_POOL_YIELD", "1")
        lds, rf = U._load("libparse_emu_lds.so"), U._load("libparse_emu.so")
        lds.emu_path_counts.argtypes = [C.POINTER(C.c_uint64)]
        _glue_counts([lds, rf], reset=True); _path_counts(lds)
        mp.setattr(T, "_LIB", lds)
        lean = []
        for k in range(len(CASES)):
            s = stream(k)
            status, got = T.run_emu([s])
            assert status == 0, "case %s: device status 0x%x" % (IDS[k], status & 0xffffffff)
            lean.append((got[0], PE.decode_emu([s])[0], U.raw_maps(lds, s)))
        ok, bad = torture(vx.EDGE), torture(vx.OVER_32768)
        st_ok, got_ok = T.run_emu([ok])
        st_bad, _ = T.run_emu([bad])
        _state.update(glue=_glue_counts([lds, rf]), path=_path_counts(lds), lean=lean, ok=(ok, st_ok, got_ok), bad=(bad, st_bad))
        mp.setattr(T, "_LIB", rf)
        plain = []
        for k in range(len(CASES)):
            status, got = T.run_emu([stream(k)])
            assert status == 0
            plain.append((got[0], U.raw_maps(rf, stream(k))))
        _state.update(plain=plain, ok_plain=T.run_emu([ok]))
    finally:
        mp.undo()
    return _state


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_lean_glue_matches_oracle_and_the_plain_build(k, parsed):
    s = stream(k)
    got, planes, (info, maps, rec) = parsed["lean"][k]
    T.check_against_oracle(s, got)
    PE._check(s, planes)
    got_p, (info_p, maps_p, rec_p) = parsed["plain"][k]
    assert info == info_p
    for c in range(3):
        np.testing.assert_array_equal(got["coef"][c], got_p["coef"][c], err_msg="coefficients of component %d, lean against plain glue" % c)
    for name, a, b in zip(("size", "flags", "ipm", "ipmc", "qp"), maps, maps_p):
        np.testing.assert_array_equal(a, b, err_msg="published map %s, lean against plain glue" % name)
    np.testing.assert_array_equal(rec, rec_p, err_msg="hand-off records")


def test_the_range_check_passes_at_the_edge_and_fires_one_step_outside(parsed):
    ok, st_ok, got_ok = parsed["ok"]
    assert st_ok == 0
    T.check_against_oracle(ok, got_ok[0])
    assert max(int(np.abs(c).max()) for c in got_ok[0]["coef"]) >= 32767
    st_p, got_p = parsed["ok_plain"]
    assert st_p == 0
    for c in range(3):
        np.testing.assert_array_equal(got_ok[0]["coef"][c], got_p[0]["coef"][c])
    bad, st_bad = parsed["bad"]
    with pytest.raises(orc.OracleError):
        orc.decode(bad)
    assert st_bad != 0
    assert parsed["path"][4] >= 1 and parsed["glue"][26] >= 1   # fired / passed with a level at the edge


BRANCHES = {0: "transform_skip_flag set", 1: "luma 4x4", 2: "luma 8x8", 3: "luma 16x16", 4: "luma 32x32", 5: "chroma 4x4", 6: "chroma 8x8",
            7: "4x4 diagonal", 8: "4x4 horizontal", 9: "4x4 vertical", 10: "8x8 diagonal", 11: "8x8 horizontal", 12: "8x8 vertical",
            13: "last position in the first sub-block (only the DC sub-block coded)", 14: "last position in the last sub-block",
            16: "coded_sub_block_flag decoded 0", 17: "coded_sub_block_flag decoded 1", 18: "right neighbour coded", 19: "lower neighbour coded",
            20: "neither neighbour coded", 21: "sign hidden", 22: "sign not hidden at a hiding distance", 23: "cu_transquant_bypass block",
            24: "cu_qp_delta parsed", 27: "4:2:2 block", 28: "4:4:4 block"}


def test_every_branch_of_the_glue_was_taken(parsed):
    counts = parsed["glue"]
    print("glue branch counters:", {BRANCHES[k]: counts[k] for k in sorted(BRANCHES)})
    missing = [BRANCHES[k] for k in sorted(BRANCHES) if counts[k] == 0]
    assert not missing, missing
