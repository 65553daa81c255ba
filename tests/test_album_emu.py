"""Albums of grid photos on the CPU tier: tests/test_album_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the
host with the kernels (k_album_paste among them) under the SIMT emulator, the way tests/test_tensor_emu.py runs its module; and a host-only check that
the new symbols exist and refuse bad arguments before they touch a device."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_album_gpu.py"]
SYMBOLS = ["hipdec_album_create", "hipdec_album_count", "hipdec_album_info", "hipdec_album_run", "hipdec_album_status", "hipdec_album_canvas_plane",
           "hipdec_album_read_plane", "hipdec_album_to_rgb_all", "hipdec_album_to_rgb_scaled_all", "hipdec_album_to_tensor", "hipdec_album_paste_timing_us"]
OTHER_SYMBOLS = ["hipdec_album_free", "hipdec_album_stats"]


def test_albums_on_the_emulated_library():
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
class Photo(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("out_width", C.c_int), ("out_height", C.c_int), ("first_tile", C.c_int), ("reserved", C.c_int)]
class Desc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
L.hipdec_album_create.argtypes = [C.POINTER(vp), ci, C.POINTER(Photo), C.POINTER(C.c_char_p), C.POINTER(sz), ci, C.c_uint64]
L.hipdec_album_stats.restype = None
L.hipdec_album_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
L.hipdec_album_free.restype = None
L.hipdec_album_free.argtypes = [vp]
def refused(rc, text=None):
    assert rc == -1, rc
    msg = L.hipdec_last_error()
    assert msg, "no error text"
    if text:
        assert text in msg.decode(), msg
# the counters first: nothing has been created
a, p, k = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
L.hipdec_album_stats(C.byref(a), C.byref(p), C.byref(k))
assert (a.value, p.value, k.value) == (0, 0, 0)
L.hipdec_album_stats(None, None, None)
n = 8
tiles = (C.c_char_p * n)(*[b"\0\0\0\1x"] * n)      # never parsed: every refusal below comes before the tiles are looked at
sizes = (sz * n)(*[5] * n)
def photos(*ps):
    return (Photo * len(ps))(*[Photo(*q) for q in ps])
good = photos((2, 2, 100, 100, 0, 0))
h = vp()
refused(L.hipdec_album_create(None, 1, good, tiles, sizes, n, 0), "NULL out")
refused(L.hipdec_album_create(C.byref(h), 1, None, tiles, sizes, n, 0), "NULL")
refused(L.hipdec_album_create(C.byref(h), 1, good, None, sizes, n, 0), "NULL")
refused(L.hipdec_album_create(C.byref(h), 1, good, tiles, None, n, 0), "NULL")
refused(L.hipdec_album_create(C.byref(h), 0, good, tiles, sizes, n, 0), "0 photos")
refused(L.hipdec_album_create(C.byref(h), 1, photos((0, 2, 100, 100, 0, 0)), tiles, sizes, n, 0), "grid of 0 x 2")
refused(L.hipdec_album_create(C.byref(h), 1, photos((2, 257, 100, 100, 0, 0)), tiles, sizes, 1 << 20, 0), "grid of 2 x 257")
refused(L.hipdec_album_create(C.byref(h), 1, photos((2, 2, 100, 100, 0, 1)), tiles, sizes, n, 0), "reserved")
refused(L.hipdec_album_create(C.byref(h), 1, photos((2, 2, 100, 100, 5, 0)), tiles, sizes, n, 0), "outside the 8 tiles")
refused(L.hipdec_album_create(C.byref(h), 1, photos((2, 2, 100, 100, -1, 0)), tiles, sizes, n, 0), "outside the 8 tiles")
refused(L.hipdec_album_create(C.byref(h), 2, photos((2, 2, 100, 100, 0, 0), (1, 2, 100, 100, 3, 0)), tiles, sizes, n, 0), "share tiles")
refused(L.hipdec_album_create(C.byref(h), 2, photos((1, 2, 100, 100, 3, 0), (2, 2, 100, 100, 0, 0)), tiles, sizes, n, 0), "share tiles")
refused(L.hipdec_album_create(C.byref(h), 1, photos((2, 2, 0, 100, 0, 0)), tiles, sizes, n, 0), "output size 0 x 100")
refused(L.hipdec_album_create(C.byref(h), 1, photos((2, 2, 100, -3, 0, 0)), tiles, sizes, n, 0), "output size 100 x -3")
rc = L.hipdec_album_create(C.byref(h), 1, photos((2, 2, 100, 100, 0, 0)), tiles, sizes, n, 99 * 100)
assert rc == -5 and b"max_image_size_pixels" in L.hipdec_last_error(), rc      # HIPDEC_ERR_LIMIT
assert not h.value
# the other entry points refuse a NULL album
buf = C.create_string_buffer(4096)
L.hipdec_album_info.argtypes = [vp, ci, vp]
L.hipdec_album_run.argtypes = [vp, vp]
L.hipdec_album_status.argtypes = [vp]
L.hipdec_album_canvas_plane.argtypes = [vp, ci, ci, vp, vp]
L.hipdec_album_read_plane.argtypes = [vp, ci, ci, vp, sz]
L.hipdec_album_to_rgb_all.argtypes = [vp, ci, vp, vp, vp]
L.hipdec_album_to_rgb_scaled_all.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]
L.hipdec_album_to_tensor.argtypes = [vp, C.POINTER(Desc), vp, ci, vp, sz, vp]
L.hipdec_album_paste_timing_us.argtypes = [vp, vp]
L.hipdec_album_count.argtypes = [vp]
refused(L.hipdec_album_count(None))
refused(L.hipdec_album_info(None, 0, C.addressof(buf)))
refused(L.hipdec_album_run(None, None))
refused(L.hipdec_album_status(None))
refused(L.hipdec_album_canvas_plane(None, 0, 0, C.addressof(buf), C.addressof(buf)))
refused(L.hipdec_album_read_plane(None, 0, 0, C.addressof(buf), 64))
refused(L.hipdec_album_to_rgb_all(None, 10, C.addressof(buf), C.addressof(buf), None))
refused(L.hipdec_album_to_rgb_scaled_all(None, 10, C.addressof(buf), C.addressof(buf), 1, C.addressof(buf), C.addressof(buf), None))
d = Desc(8, 8, 2, 0, 1, 0, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
refused(L.hipdec_album_to_tensor(None, C.byref(d), None, 1, C.addressof(buf), len(buf), None))
refused(L.hipdec_album_paste_timing_us(None, C.addressof(buf)))
L.hipdec_album_free(None)
L.hipdec_album_stats(C.byref(a), C.byref(p), C.byref(k))
assert (a.value, p.value, k.value) == (0, 0, 0)
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_validate_their_arguments_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_album_free(" in header and "HIPDEC_API void hipdec_album_stats(" in header
    assert "typedef struct hipdec_album_photo { int rows, cols, out_width, out_height, first_tile, reserved; } hipdec_album_photo;" in header
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + OTHER_SYMBOLS, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
