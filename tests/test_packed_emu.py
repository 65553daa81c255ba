"""Packed tensor output on the CPU tier: tests/test_packed_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the host
with the kernels under the SIMT emulator, the way tests/test_placed_emu.py runs its module; and a host-only check in a fresh process: the new symbols
exist, every refusal the arguments alone decide comes back before any device is initialised (naming the entry where one is at fault),
hipdec_packed_stats reads zeros, and hipdec_tensor_packed_layout is pinned against a plain Python restatement, its own refusals included."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_packed_gpu.py"]
SYMBOLS = ["hipdec_batch_to_tensor_packed", "hipdec_album_to_tensor_packed", "hipdec_tensor_packed_layout"]


def test_packed_output_on_the_emulated_library():
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
class Sample(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("offset", C.c_uint64)]
class Patches(C.Structure):
    _fields_ = [("patch", C.c_int), ("merge", C.c_int), ("reserved", C.c_int * 2)]
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_packed, L.hipdec_album_to_tensor_packed):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_tensor_packed_layout.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
L.hipdec_packed_stats.restype = None
L.hipdec_packed_stats.argtypes = [C.POINTER(C.c_uint64)] * 3

def refused(rc, code=-1, names=None):
    assert rc == code, rc
    assert L.hipdec_last_error()
    if names is not None:
        assert (b"entry %d" % names) in L.hipdec_last_error(), L.hipdec_last_error()

buf = C.create_string_buffer(4096)
p = C.addressof(buf)
handle = p                                  # never dereferenced: every call below is refused on its other arguments first, or on the NULL handle
ones, zeros = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
def desc(dtype=0, w=0, h=0, filt=1, layout=0):
    return Desc(w, h, dtype, layout, filt, 0, ones, zeros)
def samples(*s):
    return (Sample * len(s))(*(Sample(*x) for x in s))
def patches(patch=0, merge=1, r0=0, r1=0):
    return Patches(patch, merge, (C.c_int * 2)(r0, r1))
good = samples((8, 8, 0), (8, 8, 192))
for call in (L.hipdec_batch_to_tensor_packed, L.hipdec_album_to_tensor_packed):
    def go(d=None, s=good, pt=None, n=2, codes=None, out=p, room=4096, h=handle):
        return call(h, C.byref(d if d is not None else desc()), None, codes, C.addressof(s) if s is not None else None,
                    C.byref(pt) if pt is not None else None, n, out, room, None)
    refused(go(h=None))                                                                 # NULL handle
    refused(call(handle, None, None, None, C.addressof(good), None, 2, p, 4096, None))  # no description
    refused(go(out=None))                                                               # no output
    refused(go(s=None))                                                                 # samples is NULL
    refused(go(d=desc(w=8)))                                                            # the sizes are per sample
    refused(go(d=desc(h=8)))
    refused(go(d=desc(w=8, h=8)))
    refused(go(d=desc(dtype=4)))
    refused(go(d=desc(filt=2)))
    refused(go(d=desc(layout=2)))
    refused(go(n=0))
    for bad in ((0, 8, 192), (8, 0, 192), (-8, 8, 192), (8, -1, 192)):                  # a non-positive side
        refused(go(s=samples((8, 8, 0), bad)), names=1)
    for pt in (patches(-1), patches(257), patches(4, 0), patches(4, 17), patches(4, -1), patches(0, 2), patches(4, 1, 1, 0), patches(4, 1, 0, 1)):
        refused(go(pt=pt))
    refused(go(s=samples((8, 8, 0), (8, 12, 192)), pt=patches(8, 1)), names=1)          # a side that is no multiple of patch * merge
    refused(go(s=samples((8, 8, 0), (12, 8, 192)), pt=patches(4, 2)), names=1)
    refused(go(s=samples((12, 8, 0), (8, 8, 288)), pt=patches(4, 2)), names=0)
    assert go(s=samples((12, 8, 0), (8, 8, 288)), pt=patches(4, 1), h=None) == -1       # (the same sizes pass with merge 1: the NULL handle is what is left)
    refused(go(s=samples((8, 8, 0), (8, 8, 4096 - 191))), names=1)                      # offset + 3wh above out_bytes / sizeof(element)
    refused(go(s=samples((8, 8, 0), (8, 8, 2**64 - 1))), names=1)
    refused(go(d=desc(dtype=1), s=samples((8, 8, 0), (8, 8, 1024 - 191))), names=1)     # float32: 1024 elements of room
    refused(go(d=desc(dtype=2), s=samples((8, 8, 0), (8, 8, 2048 - 191))), names=1)
    refused(go(room=383), names=1)
    for s, named in ((samples((8, 8, 0), (8, 8, 191)), (0, 1)), (samples((8, 8, 100), (8, 8, 0)), (0, 1)), (samples((8, 8, 0), (8, 8, 0)), (0, 1)),
                     (samples((8, 8, 400), (8, 8, 0), (8, 8, 300)), (0, 2))):           # two samples' element ranges overlap
        refused(go(s=s, n=len(s)))
        assert b"overlap" in L.hipdec_last_error() and any((b"entry %d:" % e) in L.hipdec_last_error() for e in named), L.hipdec_last_error()
    for bad in (-1, 8):                                                                 # a code outside 0 .. 7
        codes = (C.c_int * 2)(0, bad)
        refused(go(codes=C.addressof(codes)), names=1)
s = [C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)]
L.hipdec_packed_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0]
L.hipdec_packed_stats(None, None, None)

# hipdec_tensor_packed_layout against a plain restatement
def layout(sizes, P, m):
    offs, toks, at = [], [], 0
    for w, h in sizes:
        if w < 1 or h < 1 or (P and (w % (P * m) or h % (P * m))):
            return None
        offs.append(at); toks.append((w // P) * (h // P) if P else 0); at += 3 * w * h
    return offs, toks, at
from libheif_amd import decoder
cases = 0
for P in (0, 1, 4, 6, 14, 16):
    for m in (1, 2, 3):
        if P == 0 and m != 1:
            continue
        unit = max(P, 1) * m
        sweep = [[(unit * a, unit * b) for a in range(1, 5) for b in (1, 3, 7)], [(w, h) for w in range(1, 40) for h in (unit, 29, 30)], [(28, 28), (27, 28)],
                 [(unit, unit)], [(2**31 - 1 - (2**31 - 1) % unit, unit)] * 3]
        for sizes in sweep:
            n = len(sizes)
            ws, hs = (ci * n)(*[w for w, _ in sizes]), (ci * n)(*[h for _, h in sizes])
            offs, toks, total = (C.c_uint64 * n)(), (C.c_uint32 * n)(), C.c_uint64()
            pt = patches(P, m)
            rc = L.hipdec_tensor_packed_layout(C.byref(pt), ws, hs, n, offs, toks, C.byref(total))
            want = layout(sizes, P, m)
            if want is not None and max(want[1]) >= 2**32:
                want = None                                                             # (a token count that does not fit uint32_t is refused)
            if want is None:
                refused(rc)
                try:
                    decoder.packed_layout(sizes, P, m)
                    raise AssertionError(sizes)
                except ValueError:
                    pass
            else:
                assert rc == 0 and (list(offs), list(toks), total.value) == want, (P, m, sizes)
                assert decoder.packed_layout(sizes, P, m) == want
                assert L.hipdec_tensor_packed_layout(C.byref(pt), ws, hs, n, None, None, None) == 0
            cases += 1
assert cases == 16 * 5
one = (ci * 1)(8)
assert L.hipdec_tensor_packed_layout(None, one, one, 1, None, None, C.byref(total)) == 0 and total.value == 192     # patches NULL: dense
for pt in (patches(-1), patches(257), patches(4, 0), patches(4, 17), patches(0, 2), patches(4, 1, 1, 0)):
    refused(L.hipdec_tensor_packed_layout(C.byref(pt), one, one, 1, None, None, None))
refused(L.hipdec_tensor_packed_layout(None, None, one, 1, None, None, None))
refused(L.hipdec_tensor_packed_layout(None, one, None, 1, None, None, None))
refused(L.hipdec_tensor_packed_layout(None, one, one, 0, None, None, None))
refused(L.hipdec_tensor_packed_layout(None, (ci * 1)(0), one, 1, None, None, None))
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_host_side_is_pinned_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_packed_stats(" in header
    for t in ("hipdec_tensor_sample", "hipdec_tensor_patches"):
        assert "} %s;" % t in header, t
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_packed_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
