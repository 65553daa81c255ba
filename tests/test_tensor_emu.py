"""Tensor output on the CPU tier: tests/test_tensor_gpu.py - unchanged, the 3840 x 2160 case included - against tests/emu/libheifhip_emu.so, the whole
library compiled for the host with the kernels under the SIMT emulator (the conversions to binary16 / bfloat16 are the integer round-to-nearest-even
helpers of color.hip there; a host compiler for baseline x86-64 has no fused multiply-add to contract the float stage into), the way
tests/test_scale_emu.py runs its module; and a host-only check that the new symbols exist and refuse bad arguments before they touch a device."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_tensor_gpu.py"]
SYMBOLS = ["hipdec_batch_to_tensor", "hipdec_image_to_tensor", "hipdec_batch_tensor_block"]
OTHER_SYMBOLS = ["hipdec_tensor_bytes", "hipdec_tensor_stats"]


def test_tensor_output_on_the_emulated_library():
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
class Desc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]
class Entry(C.Structure):
    _fields_ = [("item", C.c_int), ("left", C.c_int), ("top", C.c_int), ("width", C.c_int), ("height", C.c_int), ("flip", C.c_int)]
buf = C.create_string_buffer(64 * 64 * 12)
a = Img()
a.width, a.height, a.chroma, a.bit_depth = 64, 64, 0, 8
a.plane[0], a.stride[0] = C.addressof(buf), 64
def desc(**kw):
    d = Desc(8, 8, 2, 0, 1, 0, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
    for k, v in kw.items():
        setattr(d, k, v)
    return d
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
L.hipdec_tensor_bytes.restype = sz
L.hipdec_tensor_bytes.argtypes = [C.POINTER(Desc), ci]
L.hipdec_image_to_tensor.argtypes = [C.POINTER(Img), vp, C.POINTER(Desc), C.POINTER(Entry), ci, vp, sz, ci]
L.hipdec_batch_to_tensor.argtypes = [vp, C.POINTER(Desc), C.POINTER(Entry), ci, vp, sz, vp]
L.hipdec_batch_tensor_block.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp]
def refused(rc):
    assert rc == -1, rc
    assert L.hipdec_last_error()
assert L.hipdec_tensor_bytes(C.byref(desc()), 3) == 3 * 3 * 8 * 8 * 2
assert L.hipdec_tensor_bytes(C.byref(desc(dtype=1, layout=1)), 1) == 3 * 8 * 8 * 4
assert L.hipdec_tensor_bytes(C.byref(desc(dtype=0)), 1) == 3 * 8 * 8
assert L.hipdec_tensor_bytes(None, 1) == 0 and L.hipdec_tensor_bytes(C.byref(desc()), 0) == 0
for bad in (desc(width=0), desc(height=-1), desc(dtype=4), desc(layout=2), desc(filter=2), desc(scale=(C.c_float * 3)(1, float("nan"), 1)), desc(bias=(C.c_float * 3)(float("inf"), 0, 0))):
    assert L.hipdec_tensor_bytes(C.byref(bad), 1) == 0
    refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(bad), None, 1, C.addressof(buf), len(buf), 0))
good = desc()
refused(L.hipdec_image_to_tensor(None, None, C.byref(good), None, 1, C.addressof(buf), len(buf), 0))
refused(L.hipdec_image_to_tensor(C.byref(a), None, None, None, 1, C.addressof(buf), len(buf), 0))
refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(good), None, 1, None, len(buf), 0))
refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(good), None, 2, C.addressof(buf), len(buf), 0))
refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(good), None, 1, C.addressof(buf), 3 * 8 * 8 * 2 - 1, 0))
refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(good), (Entry * 1)(Entry(0, 60, 0, 5, 5, 0)), 1, C.addressof(buf), len(buf), 0))
refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(good), (Entry * 1)(Entry(0, 0, 0, 5, 0, 0)), 1, C.addressof(buf), len(buf), 0))
a.bit_depth = 7
refused(L.hipdec_image_to_tensor(C.byref(a), None, C.byref(good), None, 1, C.addressof(buf), len(buf), 0))
refused(L.hipdec_batch_to_tensor(None, C.byref(good), None, 1, C.addressof(buf), len(buf), None))
refused(L.hipdec_batch_tensor_block(None, 0, 0, None, None, None, None, None, None))
L.hipdec_tensor_stats.restype = None
t, e = C.c_uint64(7), C.c_uint64(7)
L.hipdec_tensor_stats(C.byref(t), C.byref(e))
assert (t.value, e.value) == (0, 0)
L.hipdec_tensor_stats(None, None)
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_validate_their_arguments_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API size_t hipdec_tensor_bytes(" in header and "HIPDEC_API void hipdec_tensor_stats(" in header
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + OTHER_SYMBOLS, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
