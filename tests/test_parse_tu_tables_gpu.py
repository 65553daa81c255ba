"""The TU tables of k_parse_occ8 on the GPU (HIPDEC_PARSE_TU_TABLES: sig_coeff_flag context rows and sub-block scans in LDS, the per-block descriptor
in constant memory): the 8-bit and 10-bit 4:0:0 / 4:2:0 stills of tests/lds_window_cases.py at 64x64 and 136x72 through the C ABI under the work pool
with a yield behind every CTB and six pool waves - every CTB but a row's first resumes from a parked record, on a wave whose tables were loaded once,
in front of its first task -: planes and RGB byte for byte against the oracle.  One child process under a time limit of its own (the pool switch
is read when a batch is laid out)."""
import os
import subprocess
import sys
import numpy as np
import pytest

import lds_window_cases as W
import test_parse_lds_window_gpu as G
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_stills():
    """(in the child process) two batches, 8-bit and 10-bit: what k_parse_occ8 is launched for"""
    from libheif_amd.decoder import Batch
    for bd in (8, 10):
        items = [(k, size) for k in range(len(W.STILLS)) if W.STILLS[k][1] in (0, 1) and W.STILLS[k][2].get("bit_depth", 8) == bd for size in W.SIZES]
        streams = [W.still(k, size) for k, size in items]
        b = Batch(streams)
        b.run(); b.status()
        for i, (k, size) in enumerate(items):
            name, cf, cfg, _ = W.STILLS[k]
            ref = orc.decode(streams[i])
            got = b.planes(i)
            for c in range(3 if cf else 1):
                np.testing.assert_array_equal(got[c], ref["planes"][c], err_msg="%s %dx%d component %d" % (name, size[0], size[1], c))
            if cf:
                np.testing.assert_array_equal(b.to_rgb(i, 10), G._expected_rgb(ref, cf, bd), err_msg="%s %dx%d RGB" % (name, size[0], size[1]))
        b.free()


def test_small_stills_under_the_pool_through_the_c_abi():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_parse_tu_tables_gpu as t\n"
            "t.run_stills()\n") % (os.path.dirname(HERE), HERE)
    env = dict(os.environ, HIPDEC_PARSE_POOL="1", HIPDEC_POOL_YIELD="1", HIPDEC_POOL_WAVES="6")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
