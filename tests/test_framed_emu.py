"""Framed tensor output on the CPU tier: tests/test_framed_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the host
with the kernels under the SIMT emulator, the way tests/test_placed_emu.py runs its module; and a host-only check in a fresh process: the new symbols exist,
the refusals that the arguments alone decide come back before any device is initialised, hipdec_framed_stats reads zeros, and hipdec_resize_crop_place is
pinned against plain Python arithmetic (round() is round half to even, // rounds down)."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_framed_gpu.py"]
SYMBOLS = ["hipdec_batch_to_tensor_framed", "hipdec_album_to_tensor_framed", "hipdec_resize_crop_place"]


def test_framed_output_on_the_emulated_library():
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
class Desc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]
class Place(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]
class Fill(C.Structure):
    _fields_ = [("value", C.c_float * 3), ("domain", C.c_int), ("reserved", C.c_int)]
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_framed, L.hipdec_album_to_tensor_framed):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_resize_crop_place.argtypes = [ci, ci, ci, ci, ci, C.POINTER(Place)]
L.hipdec_framed_stats.restype = None
L.hipdec_framed_stats.argtypes = [C.POINTER(C.c_uint64)] * 4

def refused(rc, code=-1):
    assert rc == code, rc
    assert L.hipdec_last_error()

buf = C.create_string_buffer(4096)
p = C.addressof(buf)
handle = p                                  # never dereferenced: every call below is refused on its other arguments first, or on the NULL handle
ones, zeros = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
def desc(dtype=0, w=8, h=8, filt=1):
    return Desc(w, h, dtype, 0, filt, 0, ones, zeros)
def fill(values=(0, 0, 0), domain=0, reserved=0):
    return Fill((C.c_float * 3)(*values), domain, reserved)
nan, inf = float("nan"), float("inf")
M = 2 ** 24
for call in (L.hipdec_batch_to_tensor_framed, L.hipdec_album_to_tensor_framed):
    refused(call(None, C.byref(desc()), None, None, None, None, None, 1, p, 4096, None))                        # NULL handle
    refused(call(handle, None, None, None, None, None, None, 1, p, 4096, None))                                 # no description
    refused(call(handle, C.byref(desc()), None, None, None, None, None, 1, None, 4096, None))                   # no output
    refused(call(handle, C.byref(desc(w=0)), None, None, None, None, None, 1, p, 4096, None))
    refused(call(handle, C.byref(desc(dtype=4)), None, None, None, None, None, 1, p, 4096, None))
    refused(call(handle, C.byref(desc(filt=2)), None, None, None, None, None, 1, p, 4096, None))
    codes = (C.c_int * 2)(0, 8)
    refused(call(handle, C.byref(desc()), None, C.addressof(codes), None, None, None, 2, p, 4096, None))        # code 8
    assert b"entry 1" in L.hipdec_last_error()
    for bad in ((0, 0, 0, 8), (0, 0, 8, 0), (0, 0, -2, 4),                                                      # a non-positive side
                (-4, 0, 4, 4), (8, 0, 4, 4), (0, -4, 4, 4), (0, 8, 4, 4), (-100, -100, 50, 50),                 # an empty visible part
                (-M - 1, 0, M, 4), (0, -M - 1, 4, M), (0, 0, M + 1, 4), (0, 0, 4, M + 1), (2**31 - 1, 0, 1, 1), (-2**31, -2**31, 2**31 - 1, 2**31 - 1)):
        places = (Place * 2)(Place(-3, -2, 20, 20), Place(*bad))
        refused(call(handle, C.byref(desc()), None, None, C.addressof(places), None, None, 2, p, 4096, None))
        assert b"entry 1" in L.hipdec_last_error(), (bad, L.hipdec_last_error())
    for dtype, f in ((1, fill((nan, 0, 0))), (1, fill((0, inf, 0), 1)), (0, fill((0, 0, -inf))), (2, fill((114.5, 0, 0))), (0, fill((0, 256, 0))), (1, fill((0, 0, -1))),
                     (1, fill((65536, 0, 0))), (0, fill(domain=2)), (1, fill(domain=-1)), (0, fill(reserved=1)), (0, fill((1.5, 0, 0), 1)), (0, fill((0, 256, 0), 1)),
                     (0, fill((0, 0, -1), 1))):
        refused(call(handle, C.byref(desc(dtype)), None, None, None, C.byref(f), None, 1, p, 4096, None))
    entry = (C.c_int * 6)(0, 0, 0, 0, 0, 0)                                                                     # (an entry list: the item count is not asked for)
    over = (Place * 1)(Place(-3, -2, 20, 20))
    refused(call(handle, C.byref(desc()), C.addressof(entry), None, C.addressof(over), None, None, 1, p, 8 * 8 * 3 - 1, None))    # out_bytes below hipdec_tensor_bytes
    assert b"out_bytes" in L.hipdec_last_error(), L.hipdec_last_error()
s = [C.c_uint64(7) for _ in range(4)]
L.hipdec_framed_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0, 0]
L.hipdec_framed_stats(None, None, None, None)

# hipdec_resize_crop_place against plain Python arithmetic
def rule(sw, sh, r, cw, ch):
    w, h = (r, r * sh // sw) if sw <= sh else (r * sw // sh, r)
    off = lambda side, crop: -round((side - crop) / 2) if side >= crop else (crop - side) // 2
    return off(w, cw), off(h, ch), w, h
from libheif_amd import decoder
pl = Place()
n = 0
for r, cw, ch in ((256, 224, 224), (32, 33, 17), (17, 17, 33), (9, 12, 12), (1, 1, 1), (40, 37, 44)):
    for sw in range(1, 48):
        for sh in range(1, 48):
            assert L.hipdec_resize_crop_place(sw, sh, r, cw, ch, C.byref(pl)) == 0
            got = (pl.x, pl.y, pl.width, pl.height)
            assert got == rule(sw, sh, r, cw, ch), (sw, sh, r, cw, ch, got)
            x, y, w, h = got
            assert min(w, h) == r and x < cw and y < ch and x + w > 0 and y + h > 0, got                       # the visible part is not empty
            n += 1
assert n == 6 * 47 * 47
odd = sorted(set((w - 224) % 4 for sw in range(1, 48) for w in [rule(sw, 13, 256, 224, 224)[2]]))
assert odd == [0, 1, 2, 3], odd                                                                                # differences 4k + 1 (down) and 4k + 3 (up) are in the sweep
assert decoder.resize_crop_place((3840, 2160), 256, (224, 224)) == (-116, -16, 455, 256)
assert decoder.resize_crop_place((227, 500), 225, (224, 224)) == (0, -136, 225, 495)                           # (225 - 224) / 2 = 0.5 -> 0; (495 - 224) / 2 = 135.5 -> 136
assert decoder.resize_crop_place((100, 100), 10, (16, 13)) == (3, 1, 10, 10)
assert decoder.resize_crop_place((2**31 - 1, 2**31 - 1), 2**24, (224, 224))[2:] == (2**24, 2**24)              # 64-bit products
assert decoder.resize_crop_places([(3, 2), decoder.oriented_size(1, 40, 30)], 8, (8, 8)) == [rule(3, 2, 8, 8, 8), rule(30, 40, 8, 8, 8)]
for bad in ((0, 5, 8, 8, 8), (5, -1, 8, 8, 8), (5, 5, 0, 8, 8), (5, 5, 8, 0, 8), (5, 5, 8, 8, -1), (1, 2**20, 2**10, 8, 8), (5, 5, 8, 2**24 + 1, 8)):
    refused(L.hipdec_resize_crop_place(*bad, C.byref(pl)))
refused(L.hipdec_resize_crop_place(5, 5, 8, 8, 8, None))
try:
    decoder.resize_crop_place((0, 1), 8, (8, 8))
    raise AssertionError("a source without columns")
except ValueError:
    pass

# random_crop_places: torchvision's RandomCrop geometry, restated - the crop's corner lies in the padded picture, every crop pixel is picture or padding
import numpy as np
rng = np.random.default_rng(5)
sizes = [(32, 32), (20, 40), (7, 5)]
for padding, need in ((4, False), ((1, 2), True), ((0, 3, 5, 0), True)):
    pad = (padding,) * 4 if isinstance(padding, int) else (padding * 2 if len(padding) == 2 else padding)
    for _ in range(50):
        fr = decoder.random_crop_places(rng, sizes if need else sizes[:1], (28, 24), padding, need)
        for (w, h), (x, y, fw, fh) in zip(sizes, fr):
            assert (fw, fh) == (w, h)
            l, t = pad[0], pad[1]
            pw, ph = w + pad[0] + pad[2], h + pad[1] + pad[3]
            if need and pw < 28: l, pw = l + 28 - pw, pw + 2 * (28 - pw)
            if need and ph < 24: t, ph = t + 24 - ph, ph + 2 * (24 - ph)
            assert l - (pw - 28) <= x <= l and t - (ph - 24) <= y <= t, (padding, (w, h), (x, y))
assert decoder.random_crop_places(rng, [(28, 24)], (28, 24)) == [(0, 0, 28, 24)]
try:
    decoder.random_crop_places(rng, [(7, 5)], (28, 24), 4)
    raise AssertionError("a padded sample smaller than the crop")
except ValueError:
    pass
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_host_side_is_pinned_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_framed_stats(" in header
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_framed_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
