"""HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC on the CPU tier: tests/test_resample_gpu.py - unchanged, the 1024 x 768 case included - against
tests/emu/libheifhip_emu.so, the whole library compiled for the host with k_resample under the SIMT emulator (barriers and LDS as on the device; the
coefficient tables come from the same host code), the way tests/test_tensor_emu.py runs its module."""
import os

from test_product_on_emulator import _build, _run

MODULES = ["test_resample_gpu.py"]


def test_resampled_output_on_the_emulated_library():
    _build()
    r = _run([os.path.join("tests", m) for m in MODULES], timeout=3000)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
