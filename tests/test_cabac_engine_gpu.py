"""The arithmetic decoder of libheif_amd/csrc/parse_core.h (9.3.4.3) bin by bin against the plain restatement of the standard in tests/cabac_ref.py,
on the device: the hand-scheduled gfx950 statements with the contexts in registers (rf: parse_bins_gfx950.h) and in LDS (lds:
parse_bins_lds_gfx950.h), and the compiler's form of their C++ twins (rf_cxx, lds_cxx: a case that fails in an assembly build only is the
assembly's, one that fails in both is arithmetic).  Same scripts as tests/test_cabac_engine_emu.py; cases: tests/cabac_cases.py."""
import time

import pytest

import cabac_cases as cc

pytestmark = pytest.mark.gpu
BUILDS = cc.GPU_BUILDS


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
    """see tests/test_cabac_engine_emu.py::test_byte_supply"""
    cc.suite_supply(build)


@pytest.mark.parametrize("build", BUILDS)
def test_divisions(build):
    """v_rcp_f32 (1 ulp) in place of the host's exact 1.0f / x: every range, every quotient, the remainder on both edges.  Prints how often the
    quotient estimate needed each repair."""
    t0 = time.time()
    rep = cc.suite_divisions(build)
    print("divisions %s: repairs of the quotient estimate %s, %.2f s" % (build, dict(sorted(rep.items())), time.time() - t0))
    assert set(rep) <= {-1, 0, 1}


@pytest.mark.parametrize("build", BUILDS)
def test_bypass_bits(build):
    cc.suite_bypass_bits(build)


@pytest.mark.parametrize("build", BUILDS)
def test_remaining(build):
    cc.suite_remaining(build)
