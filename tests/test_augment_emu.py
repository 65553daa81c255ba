"""Augmented tensor output on the CPU tier: tests/test_augment_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the
host with the kernels under the SIMT emulator, the way tests/test_photo_emu.py runs its module; and a host-only check in a fresh process: the new symbols
exist, every refusal the arguments alone decide comes back before any device is initialised (naming the entry and the operation where one is at fault),
and hipdec_augment_stats reads zeros.  (tests/test_augment_exhaustive_gpu.py is not given to the emulator: 16 M pixels under coroutine lanes is minutes.)"""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_augment_gpu.py"]
SYMBOLS = ["hipdec_tensor_augment", "hipdec_batch_to_tensor_augmented", "hipdec_album_to_tensor_augmented", "hipdec_gaussian_box"]


def test_augmented_output_on_the_emulated_library():
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
class Op(C.Structure):
    _fields_ = [("op", C.c_int), ("reserved", C.c_int), ("value", C.c_double)]
class Chain(C.Structure):
    _fields_ = [("n_ops", C.c_int), ("reserved", C.c_int), ("ops", Op * 8)]
class Photo(C.Structure):
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("reserved", C.c_int * 2)]
assert C.sizeof(Op) == 16 and C.sizeof(Chain) == 136 and C.sizeof(Photo) == 16
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_augmented, L.hipdec_album_to_tensor_augmented):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_tensor_augment.argtypes = [vp, sz, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_augment_stats.restype = None
L.hipdec_augment_stats.argtypes = [C.POINTER(C.c_uint64)] * 3
L.hipdec_gaussian_box.argtypes = [C.c_double, vp, vp, vp]

def refused(rc, says=()):
    assert rc == -1, (rc, L.hipdec_last_error())
    assert L.hipdec_last_error()
    for text in says:
        assert text in L.hipdec_last_error(), (text, L.hipdec_last_error())

buf = C.create_string_buffer(8192)
p = C.addressof(buf)
handle = p                                  # never dereferenced: every call below is refused on its other arguments first, or on the NULL handle
nan, inf = float("nan"), float("inf")
ones, zeros = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
def desc(dtype=0, w=16, h=8, filt=1, layout=0, scale=ones):
    return Desc(w, h, dtype, layout, filt, 0, scale, zeros)
def chain(*ops, n_ops=None, reserved=0):
    ch = Chain()
    ch.n_ops = len(ops) if n_ops is None else n_ops
    ch.reserved = reserved
    for k, o in enumerate(ops):
        ch.ops[k] = Op(o[0], o[2] if len(o) > 2 else 0, o[1])
    return ch
def chains(*cs):
    return (Chain * len(cs))(*cs)
good = chain((3, 1.2), (16, 200), (17, 2.0), (7, 0), (7, 0), (7, 0), (7, 0), (17, 8.0))
ROOM = 2 * 16 * 8 * 3

def go(call, stage, d=None, ph=None, cs=None, n=2, codes=None, out=p, room=ROOM, h=handle, no_chains=False, no_photo=False, no_desc=False, sbytes=8192):
    d = d if d is not None else desc()
    ph = ph if ph is not None else Photo(16, 8, (C.c_int * 2)(0, 0))
    cs = cs if cs is not None else chains(good, good)
    pp, cp = (None if no_photo else C.addressof(ph)), (None if no_chains else C.addressof(cs))
    if stage:
        return call(h, sbytes, pp, cp, None if no_desc else C.addressof(d), n, out, room, None)
    return call(h, None if no_desc else C.byref(d), None, codes, pp, cp, n, out, room, None)

for call, stage in ((L.hipdec_batch_to_tensor_augmented, False), (L.hipdec_album_to_tensor_augmented, False), (L.hipdec_tensor_augment, True)):
    g = lambda **k: go(call, stage, **k)
    for n_ops in (-1, 9):
        refused(g(cs=chains(good, chain(n_ops=n_ops))), (b"entry 1", b"n_ops"))
    for op in (0, 10, 15, 18, -3):
        refused(g(cs=chains(chain((7, 0), (op, 1.0)), good)), (b"entry 0", b"operation 1", b"unknown op"))
    refused(g(cs=chains(good, chain((17, 1.0, 7)))), (b"entry 1", b"operation 0", b"GAUSSIAN_BLUR", b"reserved"))
    refused(g(cs=chains(good, chain(reserved=1))), (b"entry 1", b"reserved"))
    for v in (0.5, -1.0, 256.0):
        refused(g(cs=chains(good, chain((1, 1.0), (16, v)))), (b"entry 1", b"operation 1", b"HUE", b"0 .. 255"))
    for v in (nan, inf, -inf):
        refused(g(cs=chains(good, chain((16, v)))), (b"entry 1", b"operation 0", b"HUE", b"not finite"))
        refused(g(cs=chains(chain((7, 0), (7, 0), (7, 0), (7, 0), (7, 0), (7, 0), (7, 0), (17, v)), good)), (b"entry 0", b"operation 7", b"GAUSSIAN_BLUR", b"not finite"))
    for v in (-0.1, 8.01):
        refused(g(cs=chains(chain((17, v)), good)), (b"entry 0", b"operation 0", b"GAUSSIAN_BLUR", b"radius"))
    for v in (65536.5, -1e9):
        refused(g(cs=chains(chain((6, v)), good)), (b"entry 0", b"operation 0", b"SOLARIZE", b"65536"))
    for v in (2.5, -1.0, 9.0):
        refused(g(cs=chains(good, chain((5, v)))), (b"entry 1", b"operation 0", b"POSTERIZE"))
    for ssz in ((32768, 8), (16, 32768), (0, 8), (16, -1)):
        refused(g(ph=Photo(ssz[0], ssz[1], (C.c_int * 2)(0, 0))), (b"source size",))
    refused(g(ph=Photo(16, 9, (C.c_int * 2)(0, 0))), (b"not the source size",))
    refused(g(ph=Photo(16, 8, (C.c_int * 2)(0, 1))), (b"reserved",))
    refused(g(no_chains=True))
    refused(g(no_photo=True))
    refused(g(no_desc=True))
    refused(g(room=ROOM - 1))
    refused(g(d=desc(dtype=4)))
    refused(g(d=desc(layout=2)))
    refused(g(d=desc(w=0)))
    refused(g(d=desc(h=-1)))
    refused(g(d=desc(dtype=1, scale=(C.c_float * 3)(1, nan, 1)), room=4 * ROOM))
    refused(g(out=None))
    refused(g(n=-1))
    if stage:
        refused(g(h=None))                                                              # no source
        refused(g(sbytes=2 * 16 * 8 * 3 - 1), (b"src_bytes",))
        ph0, d0 = Photo(16, 8, (C.c_int * 2)(0, 0)), desc()
        assert g(n=0) == 0 and call(None, 0, C.addressof(ph0), None, C.addressof(d0), 0, None, 0, None) == 0      # n = 0: nothing to do
    else:
        refused(g(n=0))
        refused(g(d=desc(filt=2)))
        for bad in (-1, 8):
            codes = (C.c_int * 2)(0, bad)
            refused(g(codes=C.addressof(codes)), (b"entry 1",))
        refused(g(h=None), (b"bad arguments",))                                        # everything else is in order: the NULL handle is what is left
r, ww, fw = C.c_int(), C.c_uint32(), C.c_uint32()
for v in (nan, inf, -0.5, 8.5):
    refused(L.hipdec_gaussian_box(v, C.addressof(r), C.addressof(ww), C.addressof(fw)), (b"radius",))
refused(L.hipdec_gaussian_box(1.0, None, None, None))
assert L.hipdec_gaussian_box(0.0, C.addressof(r), C.addressof(ww), C.addressof(fw)) == 0 and (r.value, ww.value, fw.value) == (0, 1 << 24, 0)
assert L.hipdec_gaussian_box(8.0, C.addressof(r), C.addressof(ww), C.addressof(fw)) == 0 and r.value == 7
s = [C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)]
L.hipdec_augment_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0]
L.hipdec_augment_stats(None, None, None)
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_refusals_come_back_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_augment_stats(" in header
    assert "} hipdec_augment_chain;" in header and "#define HIPDEC_AUGMENT_MAX_OPS 8" in header
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_augment_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
