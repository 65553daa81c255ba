"""The 16-byte reconstruction-plan records on the GPU (k_recon_plan fills masks, tile offsets and loop classes; k_recon8 fetches a record with one scalar
load and dispatches on its class): the stills of tests/test_recon_record_emu.py - 72x40, 136x72 and 200x136, 4:2:0 and 4:0:0, QP 22 and 37, all
transform sizes and modes, two slices, PCM units - as one batch, and a batch of 8 copies of each of the 200x136 stills, so that several chains run the
wavefront together; planes byte for byte against the oracle.  Each run is a child process under a time limit of its own."""
import os
import subprocess
import sys
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _check(streams):
    from libheif_amd.decoder import Batch
    b = Batch(streams)
    b.run(); b.status()
    refs = {}
    for i, s in enumerate(streams):
        if s not in refs: refs[s] = orc.decode(s)
        ref = refs[s]
        planes = b.planes(i)
        assert len(planes) >= len(ref["planes"])
        for c in range(len(ref["planes"])):
            np.testing.assert_array_equal(planes[c], ref["planes"][c], err_msg="item %d component %d" % (i, c))


def _streams():
    import recon_record_cases as cases
    return [cases.stream(k) for k in range(len(cases.STILLS))], cases.STILLS


def run_stills():
    """(in the child process)"""
    _check(_streams()[0])


def run_copies():
    """(in the child process) 8 copies of every 200x136 still, interleaved"""
    streams, stills = _streams()
    big = [s for s, (w, h, cf, kw) in zip(streams, stills) if (w, h) == (200, 136)]
    _check([big[i % len(big)] for i in range(8 * len(big))])


def _child(call):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_recon_record_gpu as t\n"
            "t.%s\n") % (os.path.dirname(HERE), HERE, call)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


def test_stills_through_the_records_match_the_oracle():
    r = _child("run_stills()")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_batches_of_8_copies_match_the_oracle():
    r = _child("run_copies()")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
