"""Warped tensor output on the CPU tier: tests/test_warp_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the host
with the kernels under the SIMT emulator, the way tests/test_packed_emu.py runs its module; and a host-only check in a fresh process: the new symbols
exist, every refusal the arguments alone decide comes back before any device is initialised (naming the entry where one is at fault),
hipdec_rotate_map gives the coefficients of decoder.rotate_matrix, and hipdec_warp_stats reads zeros."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_warp_gpu.py"]
SYMBOLS = ["hipdec_tensor_warp", "hipdec_batch_to_tensor_warped", "hipdec_album_to_tensor_warped", "hipdec_rotate_map"]


def test_warped_output_on_the_emulated_library():
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
class Map(C.Structure):
    _fields_ = [("m", C.c_double * 6)]
class Warp(C.Structure):
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("filter", C.c_int), ("reserved", C.c_int)]
class Fill(C.Structure):
    _fields_ = [("value", C.c_float * 3), ("domain", C.c_int), ("reserved", C.c_int)]
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_warped, L.hipdec_album_to_tensor_warped):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_tensor_warp.argtypes = [vp, sz, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_warp_stats.restype = None
L.hipdec_warp_stats.argtypes = [C.POINTER(C.c_uint64)] * 2

def refused(rc, code=-1, names=None, says=None):
    assert rc == code, (rc, L.hipdec_last_error())
    assert L.hipdec_last_error()
    if names is not None:
        assert (b"entry %d" % names) in L.hipdec_last_error(), L.hipdec_last_error()
    if says is not None:
        assert says in L.hipdec_last_error(), L.hipdec_last_error()

buf = C.create_string_buffer(8192)
p = C.addressof(buf)
handle = p                                  # never dereferenced: every call below is refused on its other arguments first, or on the NULL handle
ones, zeros = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
def desc(dtype=0, w=16, h=8, filt=1, layout=0):
    return Desc(w, h, dtype, layout, filt, 0, ones, zeros)
def maps(*ms):
    return (Map * len(ms))(*(Map((C.c_double * 6)(*m)) for m in ms))
def fill(v=(0, 0, 0), domain=0, reserved=0):
    return Fill((C.c_float * 3)(*v), domain, reserved)
ident = (1, 0, 0, 0, 1, 0)
nan, inf = float("nan"), float("inf")
ROOM = 2 * 16 * 8 * 3

def go(call, stage, d=None, w=None, ms=None, f=None, n=2, codes=None, out=p, room=ROOM, h=handle, no_maps=False, no_warp=False):
    d = d if d is not None else desc()
    w = w if w is not None else Warp(9, 7, 16, 0)
    ms = ms if ms is not None else maps(ident, ident)
    wp, mp, fp = (None if no_warp else C.addressof(w)), (None if no_maps else C.addressof(ms)), (C.addressof(f) if f is not None else None)
    if stage:
        return call(h, 8192, wp, mp, fp, C.addressof(d), n, out, room, None)
    return call(h, C.byref(d), None, codes, wp, mp, fp, n, out, room, None)

for call, stage in ((L.hipdec_batch_to_tensor_warped, False), (L.hipdec_album_to_tensor_warped, False), (L.hipdec_tensor_warp, True)):
    g = lambda **k: go(call, stage, **k)
    for bad in ((nan,) + ident[1:], (1, 0, inf, 0, 1, 0), (1, 0, 0, 0, -inf, 0)):
        refused(g(ms=maps(ident, bad)), names=1, says=b"not finite")
    for bad in ((32000.0, 0, 0, 0, 1, 0), (1, -32000.0, 0, 0, 1, 0), (1, 0, 0, 0, 1, 40000.0)):
        refused(g(ms=maps(bad, ident)), names=0, says=b"32000")
    for bad in ((1, 0, 31985.0, 0, 1, 0), (1, 0, 0, 0, 1, 31993.0), (-2000.0, 0, 0, 0, 1, 0), (1, 0, 0, 0, 3999.9, 10.0)):
        refused(g(ms=maps(ident, bad)), names=1, says=b"corner")
    for ssz in ((32768, 7), (9, 32768), (0, 7), (9, -1)):
        refused(g(w=Warp(ssz[0], ssz[1], 16, 0)), says=b"source size")
    for wf in (1, 2, -1, 18):
        refused(g(w=Warp(9, 7, wf, 0)), says=b"warp filter")
    refused(g(w=Warp(9, 7, 16, 1)))
    refused(g(no_maps=True))
    refused(g(no_warp=True))
    for dt, f in ((1, fill((nan, 0, 0))), (1, fill((0, inf, 0), 1)), (2, fill((114.5, 0, 0))), (0, fill((0, 256, 0))), (1, fill((0, 0, -1))), (1, fill((0, 256, 0))),
                  (0, fill(domain=2)), (0, fill(reserved=1)), (0, fill((1.5, 0, 0), 1)), (0, fill((0, 256, 0), 1))):
        refused(g(d=desc(dtype=dt), f=f, room=4 * ROOM))
    refused(g(room=ROOM - 1))
    refused(g(d=desc(dtype=4)))
    refused(g(d=desc(layout=2)))
    refused(g(d=desc(w=0)))
    refused(g(d=desc(h=-1)))
    refused(g(out=None))
    refused(g(n=-1))
    if stage:
        refused(g(h=None))                                                              # no source
        w0, m0, d0 = Warp(9, 7, 16, 0), maps(ident, ident), desc()
        refused(call(p, 2 * 9 * 7 * 3 - 1, C.addressof(w0), C.addressof(m0), None, C.addressof(d0), 2, p, ROOM, None))                  # src_bytes
        assert g(n=0) == 0 and call(None, 0, C.addressof(w0), None, None, C.addressof(d0), 0, None, 0, None) == 0                        # n = 0: nothing to do
    else:
        refused(g(n=0))
        refused(g(d=desc(filt=2)))
        for bad in (-1, 8):
            codes = (C.c_int * 2)(0, bad)
            refused(g(codes=C.addressof(codes)), names=1)
        refused(g(h=None), says=b"bad arguments")                                      # everything else is in order: the NULL handle is what is left
# hipdec_rotate_map against the Python helper (which tests/test_warp_ref.py pins to PIL.Image.rotate), coefficient for coefficient
from libheif_amd import decoder
L.hipdec_rotate_map.argtypes = [C.c_double, ci, ci, vp]
for angle in (0.0, -0.0, 30.0, -17.5, 123.4, 90.0, 180.0, 270.0, 360.0, 405.0, -720.25, 1e-7, 359.99999, 12345.678):
    for size in ((13, 9), (224, 224), (1, 1), (4095, 3)):
        m = Map()
        assert L.hipdec_rotate_map(angle, size[0], size[1], C.addressof(m)) == 0
        assert tuple(m.m) == decoder.rotate_matrix(angle, size), (angle, size, tuple(m.m), decoder.rotate_matrix(angle, size))
m = Map()
for bad in ((nan, 4, 4), (inf, 4, 4), (30.0, 0, 4), (30.0, 4, -1)):
    refused(L.hipdec_rotate_map(bad[0], bad[1], bad[2], C.addressof(m)))
refused(L.hipdec_rotate_map(30.0, 4, 4, None))
s = [C.c_uint64(7), C.c_uint64(7)]
L.hipdec_warp_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0]
L.hipdec_warp_stats(None, None)
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_refusals_come_back_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_warp_stats(" in header
    for t in ("hipdec_tensor_map", "hipdec_warp_desc"):
        assert "} %s;" % t in header, t
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_warp_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
