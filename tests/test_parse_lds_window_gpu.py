"""On the GPU: levels stored straight to the coefficient arena and the LDS-resident bitstream window of the throughput parser.

* the small stills of tests/lds_window_cases.py through the C ABI, in static mode (one wave per substream chain: k_parse, the general kernels for
  4:2:2 / 4:4:4) and under the work pool with a yield behind every CTB (k_parse_occ8 / k_parse_gen_occ8: every CTB but a row's first starts from a
  parked record, in the middle of its window): planes and RGB byte for byte against the oracle.  Each mode is one child process under a time limit
  of its own (the pool switch is read when a batch is laid out);
* the byte reader bin by bin through the hand-scheduled statements of the throughput build and their C++ twins on the device (the probe of
  tests/test_cabac_engine_gpu.py), over the byte strings of tests/lds_window_cases.py."""
import os
import subprocess
import sys
import numpy as np
import pytest

import lds_window_cases as W
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _expected_rgb(ref, cf, bit_depth):
    """interleaved 8-bit RGB of the oracle's planes by the oracle's colour chain (tests/test_chroma_formats_gpu.py, tests/test_decode_gpu.py)"""
    y, cb, cr = ref["planes"]
    h = y.shape[0]
    r, g, b = orc.color_ycbcr_to_rgb_planar(y, cb, cr, bit_depth, cf, ref["nclx"])
    if bit_depth == 8:
        return orc.color_rgb_planar_to_interleaved8(r, g, b).reshape(h, -1)
    return np.stack([r >> 2, g >> 2, b >> 2], axis=-1).astype(np.uint8).reshape(h, -1)


def run_stills():
    """(in the child process) the stills as three batches - 8-bit 4:0:0 / 4:2:0, 10-bit, 4:2:2 / 4:4:4 (the general kernels) -: planes and RGB
    against the oracle"""
    from libheif_amd.decoder import Batch
    for cfs, bd in (((0, 1), 8), ((0, 1), 10), ((2, 3), 8)):
        items = [(k, size) for k in range(len(W.STILLS)) if W.STILLS[k][1] in cfs and W.STILLS[k][2].get("bit_depth", 8) == bd for size in W.SIZES]
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
                np.testing.assert_array_equal(b.to_rgb(i, 10), _expected_rgb(ref, cf, cfg.get("bit_depth", 8)), err_msg="%s %dx%d RGB" % (name, size[0], size[1]))
        b.free()


def _child(env):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_parse_lds_window_gpu as t\n"
            "t.run_stills()\n") % (os.path.dirname(HERE), HERE)
    return subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=150)


@pytest.mark.parametrize("mode", ["static", "pool"])
def test_small_stills_through_the_c_abi(mode):
    env = dict(HIPDEC_PARSE_POOL="0") if mode == "static" else dict(HIPDEC_PARSE_POOL="1", HIPDEC_POOL_YIELD="1", HIPDEC_POOL_WAVES="6")
    r = _child(env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("build", ["lds", "lds_cxx"])
def test_byte_reader_with_the_window_in_lds_bin_by_bin(build):
    assert W.run_window_scripts(build) >= 80 * (len(W.CLEAN) + len(W.WITH_EP))
