"""The reconstruction plan on the GPU (k_recon_plan in front of k_recon8 / k_recon16, which read its records): the stills of tests/test_recon_plan_emu.py at
72x40 and 136x72 - 8 and 10 bit, 4:2:0 and 4:0:0, PCM and transquant-bypass units, slices and tiles - as one batch per bit depth, and one batch of 64
items of 200x136, so that the plans of many pictures sit side by side in one arena; planes byte for byte against the oracle.  Each run is a child
process under a time limit of its own."""
import os
import subprocess
import sys
import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SMALL8 = [(72, 40, 1, dict(stress=1)), (136, 72, 1, dict(stress=1)), (136, 72, 0, dict(stress=1)), (136, 72, 1, dict(pcm_pct=30, lossless_pct=20)),
          (72, 40, 1, dict(log2_ctb=4, log2_max_tb=4, stress=1)), (136, 72, 1, dict(log2_ctb=4, log2_max_tb=4, num_slices=3, stress=1)),
          (136, 72, 1, dict(log2_ctb=4, log2_max_tb=4, tile_cols=2, tile_rows=2, wpp=0)), (136, 72, 1, dict(log2_ctb=5, num_slices=2, qp=38))]
SMALL10 = [(72, 40, 0, dict(bit_depth=10)), (136, 72, 1, dict(bit_depth=10, stress=1)), (72, 40, 1, dict(bit_depth=10, pcm_pct=25, lossless_pct=20, log2_ctb=4, log2_max_tb=4))]


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


def run_small(bit_depth):
    """(in the child process)"""
    cases = SMALL8 if bit_depth == 8 else SMALL10
    _check([orc.encode(orc.synth_image(w, h, bit_depth, cf, seed=60 + k), **kw) for k, (w, h, cf, kw) in enumerate(cases)])


def run_batch_of_64():
    """(in the child process) eight contents, 64 items"""
    distinct = [orc.encode(orc.synth_image(200, 136, 8, 1, seed=80 + k), stress=k & 1, qp=22 + 3 * k) for k in range(8)]
    _check([distinct[(i * 3) % 8] for i in range(64)])


def _child(call):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_recon_plan_gpu as t\n"
            "t.%s\n") % (os.path.dirname(HERE), HERE, call)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_small_stills_through_the_plan_match_the_oracle(bit_depth):
    r = _child("run_small(%d)" % bit_depth)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_batch_of_64_items_matches_the_oracle():
    r = _child("run_batch_of_64()")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
