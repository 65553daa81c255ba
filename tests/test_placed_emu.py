"""Placed tensor output on the CPU tier: tests/test_placed_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the host
with the kernels under the SIMT emulator, the way tests/test_oriented_emu.py runs its module; and a host-only check in a fresh process: the new symbols
exist, the refusals that the arguments alone decide come back before any device is initialised, hipdec_placed_stats reads zeros, and
hipdec_letterbox_place is pinned against a restatement in fractions.Fraction (round half up), with the properties a letterbox has."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_placed_gpu.py"]
SYMBOLS = ["hipdec_batch_to_tensor_placed", "hipdec_album_to_tensor_placed", "hipdec_letterbox_place"]


def test_placed_output_on_the_emulated_library():
    _build()
    r = _run([os.path.join("tests", m) for m in MODULES], timeout=3000)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


HOST_ONLY = r"""
import ctypes as C, sys
from fractions import Fraction
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
for f in (L.hipdec_batch_to_tensor_placed, L.hipdec_album_to_tensor_placed):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_letterbox_place.argtypes = [ci, ci, ci, ci, ci, ci, C.POINTER(Place)]
L.hipdec_placed_stats.restype = None
L.hipdec_placed_stats.argtypes = [C.POINTER(C.c_uint64)] * 3

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
for call in (L.hipdec_batch_to_tensor_placed, L.hipdec_album_to_tensor_placed):
    refused(call(None, C.byref(desc()), None, None, None, None, None, 1, p, 4096, None))                        # NULL handle
    refused(call(handle, None, None, None, None, None, None, 1, p, 4096, None))                                 # no description
    refused(call(handle, C.byref(desc()), None, None, None, None, None, 1, None, 4096, None))                   # no output
    refused(call(handle, C.byref(desc(w=0)), None, None, None, None, None, 1, p, 4096, None))
    refused(call(handle, C.byref(desc(dtype=4)), None, None, None, None, None, 1, p, 4096, None))
    refused(call(handle, C.byref(desc(filt=2)), None, None, None, None, None, 1, p, 4096, None))
    codes = (C.c_int * 2)(0, 8)
    refused(call(handle, C.byref(desc()), None, C.addressof(codes), None, None, None, 2, p, 4096, None))        # code 8
    assert b"entry 1" in L.hipdec_last_error()
    for bad in ((0, 0, 0, 8), (0, 0, 8, 0), (0, 0, -2, 4), (1, 0, 8, 8), (0, 1, 8, 8), (-1, 0, 4, 4), (0, -1, 4, 4), (7, 7, 2, 1), (2**31 - 1, 0, 1, 1)):
        places = (Place * 2)(Place(0, 0, 8, 8), Place(*bad))
        refused(call(handle, C.byref(desc()), None, None, C.addressof(places), None, None, 2, p, 4096, None))
        assert b"entry 1" in L.hipdec_last_error(), L.hipdec_last_error()
    for dtype, f in ((1, fill((nan, 0, 0))), (1, fill((0, inf, 0), 1)), (0, fill((0, 0, -inf))), (2, fill((114.5, 0, 0))), (0, fill((0, 256, 0))), (1, fill((0, 0, -1))),
                     (1, fill((65536, 0, 0))), (0, fill(domain=2)), (1, fill(domain=-1)), (0, fill(reserved=1)), (0, fill((1.5, 0, 0), 1)), (0, fill((0, 256, 0), 1)),
                     (0, fill((0, 0, -1), 1))):
        refused(call(handle, C.byref(desc(dtype)), None, None, None, C.byref(f), None, 1, p, 4096, None))
    entry = (C.c_int * 6)(0, 0, 0, 0, 0, 0)                                                                     # (an entry list: the item count is not asked for)
    refused(call(handle, C.byref(desc()), C.addressof(entry), None, None, None, None, 1, p, 8 * 8 * 3 - 1, None))    # out_bytes below hipdec_tensor_bytes
    assert b"out_bytes" in L.hipdec_last_error(), L.hipdec_last_error()
s = [C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)]
L.hipdec_placed_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0]
L.hipdec_placed_stats(None, None, None)

# hipdec_letterbox_place against exact rational arithmetic, rounding half up
def half_up(q):
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)
def letterbox(sw, sh, cw, ch, upscale, anchor):
    if not upscale and sw <= cw and sh <= ch:
        w, h = sw, sh
    elif Fraction(sw, sh) >= Fraction(cw, ch):      # the source is at least as wide as the canvas: the width is the canvas'
        w, h = cw, max(1, half_up(Fraction(sh * cw, sw)))
    else:
        w, h = max(1, half_up(Fraction(sw * ch, sh))), ch
    return ((cw - w) // 2, (ch - h) // 2, w, h) if anchor else (0, 0, w, h)
from libheif_amd import decoder
pl = Place()
n = 0
for cw, ch in ((32, 32), (33, 17), (17, 33), (1, 1), (640, 640)):
    for sw in range(1, 41):
        for sh in range(1, 41):
            for upscale in (0, 1):
                for anchor in (0, 1):
                    assert L.hipdec_letterbox_place(sw, sh, cw, ch, upscale, anchor, C.byref(pl)) == 0
                    got = (pl.x, pl.y, pl.width, pl.height)
                    assert got == letterbox(sw, sh, cw, ch, upscale, anchor), (sw, sh, cw, ch, upscale, anchor, got)
                    x, y, w, h = got
                    assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= cw and y + h <= ch, got        # inside the canvas
                    scaled = upscale or sw > cw or sh > ch
                    assert (w == cw or h == ch) if scaled else (w, h) == (sw, sh), got                          # one side is the canvas' when scaling happens
                    if anchor:
                        assert 0 <= (cw - w) - 2 * x <= 1 and 0 <= (ch - h) - 2 * y <= 1
                    assert decoder.letterbox_place((sw, sh), (cw, ch), bool(upscale), "center" if anchor else "topleft") == got      # the Python helper, every case
                    n += 1
assert n == 5 * 40 * 40 * 4
assert decoder.letterbox_places([(3, 2), (2, 3), (40, 40)], (32, 32)) == [letterbox(3, 2, 32, 32, 1, 1), letterbox(2, 3, 32, 32, 1, 1), (0, 0, 32, 32)]
assert decoder.letterbox_places([decoder.oriented_size(1, 40, 30)], (20, 20), upscale=False, anchor="topleft") == [(0, 0, 15, 20)]
assert decoder.letterbox_place((1920, 1080), (640, 640)) == (0, 140, 640, 360)
assert decoder.letterbox_place((2**31 - 1, 1), (2**31 - 1, 2**31 - 1)) == (0, (2**31 - 2) // 2, 2**31 - 1, 1)      # 64-bit products
for bad in ((0, 5, 8, 8, 1, 1), (5, -1, 8, 8, 1, 1), (5, 5, 0, 8, 1, 1), (5, 5, 8, 0, 1, 1), (5, 5, 8, 8, 1, 2), (5, 5, 8, 8, 1, -1)):
    refused(L.hipdec_letterbox_place(*bad, C.byref(pl)))
refused(L.hipdec_letterbox_place(5, 5, 8, 8, 1, 1, None))
for bad in (dict(anchor="middle"), dict(src_size=(0, 1))):
    try:
        decoder.letterbox_place(**dict(dict(src_size=(4, 4), canvas_size=(8, 8)), **bad))
        raise AssertionError(bad)
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
    assert "HIPDEC_API void hipdec_placed_stats(" in header
    for t in ("hipdec_tensor_place", "hipdec_fill_domain", "hipdec_tensor_fill"):
        assert "} %s;" % t in header, t
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_placed_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
