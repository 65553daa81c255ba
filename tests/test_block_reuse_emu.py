"""Block-array reuse and the second z-chunk on the CPU tier: tests/test_block_reuse_gpu.py - unchanged, the 65537-entry calls included (the emulator has no
grid limit of its own) - against tests/emu/libheifhip_emu.so, the whole library compiled for the host with the kernels under the SIMT emulator, the way
tests/test_packed_emu.py runs its module."""
import os

from test_product_on_emulator import _build, _run

MODULES = ["test_block_reuse_gpu.py"]


def test_block_reuse_and_second_chunk_on_the_emulated_library():
    _build()
    r = _run([os.path.join("tests", m) for m in MODULES], timeout=3000)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
