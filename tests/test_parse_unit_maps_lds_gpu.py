"""The LDS-resident unit maps of k_parse_occ8 on the GPU: the stills of tests/test_parse_unit_maps_lds.py as one batch of 64 items of mixed sizes
under the work pool (HIPDEC_PARSE_POOL=1: the throughput kernel; HIPDEC_POOL_WAVES=12, far fewer waves than rows, so that every wave runs rows of
different pictures one after the other and a wave's LDS maps outlive a task), then a second batch with other contents on the same arena.  Unit maps
through Batch.maps() and the planes, byte for byte against the oracle.  Each run is a child process under a time limit of its own: the first batch
alone, and only when that ended well the two batches one after the other (the second takes over the first's arena, so they share a process)."""
import os
import subprocess
import sys
import numpy as np
import pytest

from oracle import pyoracle as orc
import test_parse_unit_maps_lds as U

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _check(b, streams):
    refs = {}
    for i, s in enumerate(streams):
        if s not in refs: refs[s] = orc.decode(s, taps=True)
        ref = refs[s]
        m = b.maps(i)
        for name in ("log2_cb", "log2_tb", "intra_luma", "intra_chroma", "qp_y"):
            np.testing.assert_array_equal(m[name], ref["map_" + name], err_msg="item %d map %s" % (i, name))
        np.testing.assert_array_equal(m["flags"] & 0x7f, ref["map_flags"] & 0x7f, err_msg="item %d flags" % i)
        planes = b.planes(i)
        for c in range(3):
            np.testing.assert_array_equal(planes[c], ref["planes"][c], err_msg="item %d component %d" % (i, c))


def run_batches(second_too):
    """(in the child process) the first batch; then, on its arena, the same shapes item by item with other contents"""
    from libheif_amd.decoder import Batch
    n = len(U.CASES)
    first = [U.stream((i * 3) % n) for i in range(64)]
    b = Batch(first)
    b.run(); b.status()
    _check(b, first)
    if second_too:
        other = [orc.encode(orc.synth_image(U.CASES[k][0], U.CASES[k][1], 8, 1, seed=900 + k), **U.CASES[k][2]) for k in range(n)]
        second = [other[(i * 3) % n] for i in range(64)]
        b2 = Batch(second, recycle=b)
        b2.run(); b2.status()
        _check(b2, second)


def _child(second_too):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_parse_unit_maps_lds_gpu as t\n"
            "t.run_batches(%d)\n") % (os.path.dirname(HERE), HERE, second_too)
    env = dict(os.environ, HIPDEC_PARSE_POOL="1", HIPDEC_POOL_WAVES="12")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)


def test_mixed_batch_of_64_and_a_second_batch_on_the_same_arena():
    r = _child(0)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = _child(1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
