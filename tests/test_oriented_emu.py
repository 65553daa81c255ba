"""Oriented output on the CPU tier: tests/test_oriented_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the host
with the kernels under the SIMT emulator, the way tests/test_tensor_emu.py runs its module; and a host-only check in a fresh process: the new symbols
exist, the refusals that the arguments alone decide come back before any device is initialised, hipdec_orientation_compose and
hipdec_orientation_from_exif are pinned against NumPy, and the Python stored_window() is checked by brute force on an index image."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_oriented_gpu.py"]
SYMBOLS = ["hipdec_orientation_compose", "hipdec_orientation_from_exif", "hipdec_batch_to_tensor_oriented", "hipdec_album_to_tensor_oriented",
           "hipdec_batch_to_rgb_scaled_oriented_all", "hipdec_album_to_rgb_scaled_oriented_all"]


def test_oriented_output_on_the_emulated_library():
    _build()
    r = _run([os.path.join("tests", m) for m in MODULES], timeout=3000)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


HOST_ONLY = r"""
import ctypes as C, sys
import numpy as np
L = C.CDLL(sys.argv[1])
L.hipdec_last_error.restype = C.c_char_p
for n in sys.argv[2:]:
    assert hasattr(L, n), n
class Desc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
L.hipdec_orientation_compose.argtypes = [ci, ci, ci]
L.hipdec_orientation_from_exif.argtypes = [ci]
L.hipdec_batch_to_tensor_oriented.argtypes = [vp, C.POINTER(Desc), vp, vp, ci, vp, sz, vp]
L.hipdec_album_to_tensor_oriented.argtypes = [vp, C.POINTER(Desc), vp, vp, ci, vp, sz, vp]
L.hipdec_batch_to_rgb_scaled_oriented_all.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp]
L.hipdec_album_to_rgb_scaled_oriented_all.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp]
L.hipdec_oriented_stats.restype = None
L.hipdec_oriented_stats.argtypes = [C.POINTER(C.c_uint64)] * 3

def orient(code, a):
    a = np.rot90(a, code & 3)
    return np.fliplr(a) if code >> 2 else a
a = np.arange(6).reshape(2, 3)               # non-square, no symmetry: the eight orientations of it are all different
def code_of(x):
    m = [c for c in range(8) if orient(c, a).shape == x.shape and np.array_equal(orient(c, a), x)]
    assert len(m) == 1, m
    return m[0]
assert sorted(code_of(orient(c, a)) for c in range(8)) == list(range(8))
OPS = ((0, 90, lambda x: np.rot90(x, 1)), (0, 180, lambda x: np.rot90(x, 2)), (0, 270, lambda x: np.rot90(x, 3)), (1, 0, np.flipud), (1, 1, np.fliplr))
for c in range(8):
    for op, arg, f in OPS:
        assert L.hipdec_orientation_compose(c, op, arg) == code_of(f(orient(c, a))), (c, op, arg)
EXIF = [lambda x: x, np.fliplr, lambda x: np.rot90(x, 2), np.flipud, lambda x: x.T, lambda x: np.rot90(x, -1), lambda x: np.rot90(x.T, 2), lambda x: np.rot90(x, 1)]
for e in range(1, 9):
    assert L.hipdec_orientation_from_exif(e) == code_of(EXIF[e - 1](a)), e
def refused(rc, code=-1):
    assert rc == code, rc
    assert L.hipdec_last_error()
for bad in ((8, 0, 90), (-1, 1, 1), (0, 0, 45), (0, 0, 0), (0, 1, 2), (0, 2, 0), (0, -1, 90)):
    refused(L.hipdec_orientation_compose(*bad))
for bad in (0, 9, -1):
    refused(L.hipdec_orientation_from_exif(bad))

buf = C.create_string_buffer(4096)
p = C.addressof(buf)
good = Desc(8, 8, 0, 0, 1, 0, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
handle = p                                  # never dereferenced: every call below is refused on its other arguments first, or on the NULL handle
codes = (C.c_int * 1)(8)
refused(L.hipdec_batch_to_tensor_oriented(None, C.byref(good), None, None, 1, p, 4096, None))
refused(L.hipdec_album_to_tensor_oriented(None, C.byref(good), None, None, 1, p, 4096, None))
refused(L.hipdec_batch_to_tensor_oriented(handle, C.byref(good), None, C.addressof(codes), 1, p, 4096, None))      # code 8
refused(L.hipdec_album_to_tensor_oriented(handle, C.byref(good), None, C.addressof(codes), 1, p, 4096, None))
refused(L.hipdec_batch_to_tensor_oriented(handle, None, None, None, 1, p, 4096, None))
refused(L.hipdec_batch_to_tensor_oriented(handle, C.byref(Desc(0, 8, 0, 0, 1, 0)), None, None, 1, p, 4096, None))
one = (C.c_int * 1)(8)
stride = (C.c_size_t * 1)(24)
outs = (C.c_void_p * 1)(p)
for rgb in (L.hipdec_batch_to_rgb_scaled_oriented_all, L.hipdec_album_to_rgb_scaled_oriented_all):
    refused(rgb(None, 10, None, C.addressof(one), C.addressof(one), 1, C.addressof(outs), C.addressof(stride), None))
    refused(rgb(None, 10, None, None, C.addressof(one), 1, C.addressof(outs), C.addressof(stride), None))
s = [C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)]
L.hipdec_oriented_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0]
L.hipdec_oriented_stats(None, None, None)

# the Python helpers: displayed window -> stored window, by brute force on an index image
from libheif_amd import decoder
W, H = 7, 5
idx = np.arange(W * H).reshape(H, W)
for c in range(8):
    disp = orient(c, idx)
    dh, dw = disp.shape
    assert decoder.oriented_size(c, W, H) == (dw, dh)
    for l in range(dw):
        for t in range(dh):
            for w in range(1, dw - l + 1):
                for h in range(1, dh - t + 1):
                    sl, st, sw, sh = decoder.stored_window(c, W, H, l, t, w, h)
                    assert np.array_equal(orient(c, idx[st:st + sh, sl:sl + sw]), disp[t:t + h, l:l + w]), (c, l, t, w, h)
    for bad in ((-1, 0, 1, 1), (0, 0, dw + 1, 1), (0, dh, 1, 1), (0, 0, 0, 1)):
        try:
            decoder.stored_window(c, W, H, *bad)
            raise AssertionError(bad)
        except ValueError:
            pass
assert (decoder.ORIENT_0, decoder.ORIENT_CCW90, decoder.ORIENT_180, decoder.ORIENT_CCW270, decoder.ORIENT_MIRROR, decoder.ORIENT_CCW90_MIRROR,
        decoder.ORIENT_180_MIRROR, decoder.ORIENT_CCW270_MIRROR) == tuple(range(8))
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_host_side_is_pinned_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_oriented_stats(" in header
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_oriented_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
