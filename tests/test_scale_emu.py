"""Scaled output on the CPU tier: tests/test_scale_gpu.py - unchanged, the full-shape case included (seconds under the emulator) - against
tests/emu/libheifhip_emu.so, the whole library compiled for the host with the kernels under the SIMT emulator, the way
tests/test_product_on_emulator.py runs its modules; and a host-only check that the new symbols exist in both builds' sources and refuse bad
arguments before they touch a device."""
import ctypes as C
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_scale_gpu.py"]
SYMBOLS = ["hipdec_image_scale", "hipdec_plane_scale", "hipdec_batch_to_rgb_scaled", "hipdec_batch_to_rgb_scaled_all", "hipdec_batch_read_plane_scaled"]


def test_scaled_output_on_the_emulated_library():
    _build()
    r = _run([os.path.join("tests", m) for m in MODULES], timeout=3000)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


HOST_ONLY = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
L.hipdec_last_error.restype = C.c_char_p
for n in sys.argv[2:]:
    assert hasattr(L, n), n
class Img(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("chroma", C.c_int), ("bit_depth", C.c_int), ("plane", C.c_void_p * 4), ("stride", C.c_size_t * 4), ("on_device", C.c_int)]
buf = C.create_string_buffer(64 * 64)
a, b = Img(), Img()
a.width, a.height, a.chroma, a.bit_depth = 64, 64, 0, 8
a.plane[0], a.stride[0] = C.addressof(buf), 64
b.plane[0], b.stride[0] = C.addressof(buf), 64
L.hipdec_image_scale.argtypes = [C.POINTER(Img), C.c_int, C.c_int, C.c_int, C.POINTER(Img)]
def refused(rc):
    assert rc == -1, rc
    assert L.hipdec_last_error()
refused(L.hipdec_image_scale(None, 8, 8, 0, C.byref(b)))
refused(L.hipdec_image_scale(C.byref(a), 0, 8, 0, C.byref(b)))
refused(L.hipdec_image_scale(C.byref(a), 8, -1, 1, C.byref(b)))
refused(L.hipdec_image_scale(C.byref(a), 8, 8, 2, C.byref(b)))
a.bit_depth = 7
refused(L.hipdec_image_scale(C.byref(a), 8, 8, 0, C.byref(b)))
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
L.hipdec_batch_to_rgb_scaled.argtypes = [vp, ci, ci, ci, ci, ci, vp, sz, vp]
L.hipdec_batch_to_rgb_scaled_all.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]
L.hipdec_batch_read_plane_scaled.argtypes = [vp, ci, ci, ci, ci, ci, vp, sz]
refused(L.hipdec_batch_to_rgb_scaled(None, 0, 10, 8, 8, 0, C.addressof(buf), 64, None))
refused(L.hipdec_batch_to_rgb_scaled_all(None, 10, None, None, 0, None, None, None))
refused(L.hipdec_batch_read_plane_scaled(None, 0, 0, 8, 8, 0, C.addressof(buf), 64))
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_validate_their_arguments_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
