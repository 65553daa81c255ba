"""The arithmetic decoder of libheif_amd/csrc/parse_core.h (9.3.4.3) bin by bin against the plain restatement of the standard in tests/cabac_ref.py,
on the CPU tier: the probe (tests/probe/cabac_probe.hip) compiled for the host runs the C++ forms of the statements, with the contexts in registers
(emu_rf) and in LDS (emu_lds).  tests/test_cabac_engine_gpu.py runs the same scripts through the gfx950 assembly.  Cases: tests/cabac_cases.py."""
import os
import re

import pytest

import cabac_cases as cc
import cabac_ref

HERE = os.path.dirname(os.path.abspath(__file__))
BUILDS = cc.EMU_BUILDS


def _c_array(text, name):
    m = re.search(name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", text)
    return [int(x) for x in re.findall(r"\d+", m.group(1))]


def test_tables_equal_the_parsers():
    """tables 9-46 / 9-47 as typed in from the standard against c_range_lps / c_next_lps of parse_tables.h: the only place where the two meet"""
    text = open(os.path.join(HERE, "..", "libheif_amd", "csrc", "parse_tables.h")).read()
    lps = _c_array(text, "c_range_lps")
    assert lps == [v for row in cabac_ref.RANGE_TAB_LPS for v in row]
    assert _c_array(text, "c_next_lps") == cabac_ref.TRANS_IDX_LPS
    assert cabac_ref.TRANS_IDX_MPS == [min(p + 1, 62) for p in range(63)] + [63]


@pytest.mark.parametrize("seed", cc.CELL_SEEDS)
@pytest.mark.parametrize("build", BUILDS)
def test_every_table_cell_in_every_context_home(build, seed):
    cc.suite_cells(build, seed)


@pytest.mark.parametrize("build", BUILDS)
def test_state_edges(build):
    cc.suite_edges(build)


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("build", BUILDS)
def test_runs(build, seed):
    cc.suite_runs(build, seed)


@pytest.mark.parametrize("build", BUILDS)
def test_forced_runs(build):
    cc.suite_forced_runs(build)


@pytest.mark.parametrize("build", BUILDS)
def test_byte_supply(build):
    """Every operation kind with its refill on every boundary of the byte supply.  A 00 00 03 as the last three bytes of a substream: by 7.3.1.1 /
    7.4.2 the 03 is an emulation_prevention_three_byte (the syntax tests i + 2 < NumBytesInNalUnit, so the last byte qualifies; it is there behind
    cabac_zero_words) and carries no payload: the reference drops it and reads zeros behind it."""
    cc.suite_supply(build)


@pytest.mark.parametrize("build", BUILDS)
def test_divisions(build):
    rep = cc.suite_divisions(build)
    assert set(rep) <= {-1, 0, 1}


@pytest.mark.parametrize("build", BUILDS)
def test_bypass_bits(build):
    cc.suite_bypass_bits(build)


@pytest.mark.parametrize("build", BUILDS)
def test_remaining(build):
    cc.suite_remaining(build)
