"""Recipe tensor output on the CPU tier: tests/test_recipe_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the
host with the kernels under the SIMT emulator, the way tests/test_augment_emu.py runs its module; and a host-only check in a fresh process: the new symbols
and the record's size are in the header and the library, every refusal the arguments alone decide comes back before any device is initialised (naming the
entry and the operation where one is at fault), hipdec_tensor_augment still answers "unknown op" for opcode 32, and hipdec_recipe_stats reads zeros."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_recipe_gpu.py"]
SYMBOLS = ["hipdec_tensor_recipe", "hipdec_batch_to_tensor_recipe", "hipdec_album_to_tensor_recipe"]


def test_recipe_output_on_the_emulated_library():
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
class Affine(C.Structure):
    _fields_ = [("m", C.c_double * 6), ("filter", C.c_int), ("fill", C.c_int * 3)]
assert C.sizeof(Op) == 16 and C.sizeof(Chain) == 136 and C.sizeof(Photo) == 16 and C.sizeof(Affine) == 64
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_recipe, L.hipdec_album_to_tensor_recipe):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, vp, ci, ci, vp, sz, vp]
L.hipdec_tensor_recipe.argtypes = [vp, sz, vp, vp, vp, ci, vp, ci, vp, sz, vp]
L.hipdec_tensor_augment.argtypes = [vp, sz, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_recipe_stats.restype = None
L.hipdec_recipe_stats.argtypes = [C.POINTER(C.c_uint64)] * 4

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
def affine(m=(1, 0.25, 0, 0, 1, 0), filt=16, fill=(3, 114, 250)):
    return Affine((C.c_double * 6)(*m), filt, (C.c_int * 3)(*fill))
def affines(*a):
    return (Affine * len(a))(*a)
good = chain((3, 1.2), (32, 0), (17, 2.0), (32, 1), (7, 0), (16, 200), (32, 2), (17, 8.0))
GOOD3 = (affine(), affine((0.5, 0, 4, 0, 0.5, 2), 0, (0, 0, 0)), affine((0.9, -0.3, 2, 0.3, 0.9, -1), 17, (255, 255, 255)))
ROOM = 2 * 16 * 8 * 3

def go(call, stage, d=None, ph=None, cs=None, af=GOOD3, n_aff=None, n=2, codes=None, out=p, room=ROOM, h=handle, no_chains=False, no_photo=False, no_desc=False,
       no_affines=False, sbytes=8192):
    d = d if d is not None else desc()
    ph = ph if ph is not None else Photo(16, 8, (C.c_int * 2)(0, 0))
    cs = cs if cs is not None else chains(good, good)
    aa = affines(*af) if af else None
    n_aff = len(af) if n_aff is None else n_aff
    pp, cp = (None if no_photo else C.addressof(ph)), (None if no_chains else C.addressof(cs))
    ap = None if (no_affines or aa is None) else C.addressof(aa)
    if stage:
        return call(h, sbytes, pp, cp, ap, n_aff, None if no_desc else C.addressof(d), n, out, room, None)
    return call(h, None if no_desc else C.byref(d), None, codes, pp, cp, ap, n_aff, n, out, room, None)

for call, stage in ((L.hipdec_batch_to_tensor_recipe, False), (L.hipdec_album_to_tensor_recipe, False), (L.hipdec_tensor_recipe, True)):
    g = lambda **k: go(call, stage, **k)
    # the affine step's own refusals
    for v in (3.0, -1.0, 0.5, 1e9):
        refused(g(cs=chains(good, chain((7, 0), (32, v)))), (b"entry 1", b"operation 1", b"AFFINE", b"index"))
    for v in (nan, inf, -inf):
        refused(g(cs=chains(good, chain((32, v)))), (b"entry 1", b"operation 0", b"AFFINE", b"not finite"))
    refused(g(n_aff=2), (b"entry 0", b"operation 6", b"AFFINE", b"index"))
    refused(g(n_aff=0, af=()), (b"entry 0", b"operation 1", b"AFFINE", b"index"))
    refused(g(no_affines=True), (b"entry 0", b"operation 1", b"AFFINE", b"NULL"))
    refused(g(n_aff=-1), (b"n_affines",))
    refused(g(n_aff=-1, cs=chains(chain(), chain())), (b"n_affines",))
    refused(g(cs=chains(good, chain((32, 1, 5)))), (b"entry 1", b"operation 0", b"AFFINE", b"reserved"))
    for i in range(6):
        for v in (nan, inf):
            m = [1, 0, 0, 0, 1, 0]; m[i] = v
            refused(g(af=(affine(), affine(m), GOOD3[2])), (b"entry 0", b"operation 3", b"AFFINE", b"not finite"))
        m = [1, 0, 0, 0, 1, 0]; m[i] = -32000.0
        refused(g(af=(affine(), GOOD3[1], affine(m))), (b"entry 0", b"operation 6", b"AFFINE", b"32000"))
    refused(g(af=(affine((1999.0, 0, 20, 0, 1, 0)),) + GOOD3[1:]), (b"entry 0", b"operation 1", b"AFFINE", b"corner (16, 0)"))       # 1999 * 16 + 20
    refused(g(af=(affine((1, 0, 0, 0, 3999.0, 9)),) + GOOD3[1:]), (b"entry 0", b"operation 1", b"AFFINE", b"corner (0, 8)"))         # 3999 * 8 + 9
    assert g(af=(affine((1999.0, 0, 15, 0, 3999.0, 7)),) + GOOD3[1:], h=None) == -1 and b"bad arguments" in L.hipdec_last_error()   # just inside: taken
    for f in (1, 2, 15, 18, -1):
        refused(g(af=(affine(filt=f),) + GOOD3[1:]), (b"entry 0", b"operation 1", b"AFFINE", b"filter"))
    for c in range(3):
        for v in (-1, 256, 1 << 20):
            fill = [0, 0, 0]; fill[c] = v
            refused(g(af=GOOD3[:2] + (affine(fill=fill),)), (b"entry 0", b"operation 6", b"AFFINE", b"fill", b"0 .. 255"))
    # a record no chain names is not read
    assert g(af=GOOD3 + (affine(filt=99, fill=(-5, 0, 0)),), h=None) == -1 and b"bad arguments" in L.hipdec_last_error()
    # everything hipdec_tensor_augment refuses
    for n_ops in (-1, 9):
        refused(g(cs=chains(good, chain(n_ops=n_ops))), (b"entry 1", b"n_ops"))
    for op in (0, 10, 15, 18, 31, 33, -3):
        refused(g(cs=chains(chain((7, 0), (op, 1.0)), good)), (b"entry 0", b"operation 1", b"unknown op"))
    refused(g(cs=chains(good, chain((17, 1.0, 7)))), (b"entry 1", b"operation 0", b"GAUSSIAN_BLUR", b"reserved"))
    refused(g(cs=chains(good, chain(reserved=1))), (b"entry 1", b"reserved"))
    for v in (0.5, -1.0, 256.0):
        refused(g(cs=chains(good, chain((1, 1.0), (16, v)))), (b"entry 1", b"operation 1", b"HUE", b"0 .. 255"))
    for v in (nan, inf, -inf):
        refused(g(cs=chains(good, chain((16, v)))), (b"entry 1", b"operation 0", b"HUE", b"not finite"))
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
        refused(g(sbytes=2 * 16 * 8 * 3 - 1), (b"tensor_recipe", b"src_bytes"))
        ph0, d0 = Photo(16, 8, (C.c_int * 2)(0, 0)), desc()
        assert g(n=0) == 0 and call(None, 0, C.addressof(ph0), None, None, 0, C.addressof(d0), 0, None, 0, None) == 0      # n = 0: nothing to do
    else:
        refused(g(n=0))
        refused(g(d=desc(filt=2)))
        for bad in (-1, 8):
            codes = (C.c_int * 2)(0, bad)
            refused(g(codes=C.addressof(codes)), (b"entry 1",))
        refused(g(h=None), (b"bad arguments",))                                        # everything else is in order: the NULL handle is what is left
# the augment stage keeps refusing opcode 32
cs, ph, d = chains(chain((7, 0), (32, 0)), chain()), Photo(16, 8, (C.c_int * 2)(0, 0)), desc()
refused(L.hipdec_tensor_augment(p, 8192, C.addressof(ph), C.addressof(cs), C.addressof(d), 2, p, ROOM, None), (b"tensor_augment", b"entry 0", b"operation 1", b"unknown op 32"))
s = [C.c_uint64(7) for _ in range(4)]
L.hipdec_recipe_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0, 0]
L.hipdec_recipe_stats(None, None, None, None)
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_refusals_come_back_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_recipe_stats(" in header
    assert "} hipdec_recipe_affine;" in header and "#define HIPDEC_RECIPE_AFFINE 32" in header
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_recipe_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
