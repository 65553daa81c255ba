"""The lean residual_coding glue of k_parse_occ8 on the GPU: the 4:2:0 stills of tests/test_parse_residual_glue.py as one batch of 64 items of mixed
sizes under the work pool (HIPDEC_PARSE_POOL=1: the throughput kernel; HIPDEC_POOL_WAVES=12, far fewer waves than rows), then a second batch with
other contents on the same arena.  Unit maps through Batch.maps() and the planes, byte for byte against the oracle.  Each run is a child process
under a time limit of its own: the first batch alone, and only when that ended well the two batches one after the other."""
import os
import subprocess
import sys
import pytest

from oracle import pyoracle as orc
import test_parse_residual_glue as G
from test_parse_unit_maps_lds_gpu import _check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_batches(second_too):
    """(in the child process) the first batch; then, on its arena, the same shapes item by item with other contents"""
    from libheif_amd.decoder import Batch
    ks = G.GPU_CASES
    first = [G.stream(ks[(i * 3) % len(ks)]) for i in range(64)]
    b = Batch(first)
    b.run(); b.status()
    _check(b, first)
    if second_too:
        other = {k: orc.encode(orc.synth_image(G.CASES[k][0], G.CASES[k][1], 8, 1, seed=900 + k), **G.CASES[k][3]) for k in ks}
        second = [other[ks[(i * 3) % len(ks)]] for i in range(64)]
        b2 = Batch(second, recycle=b)
        b2.run(); b2.status()
        _check(b2, second)


def _child(second_too):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_parse_residual_glue_gpu as t\n"
            "t.run_batches(%d)\n") % (os.path.dirname(HERE), HERE, second_too)
    env = dict(os.environ, HIPDEC_PARSE_POOL="1", HIPDEC_POOL_WAVES="12")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)


def test_mixed_batch_of_64_and_a_second_batch_on_the_same_arena():
    r = _child(0)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = _child(1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
