"""Projective tensor output on the CPU tier: tests/test_project_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the
host with the kernels under the SIMT emulator, the way tests/test_warp_emu.py runs its module; a host-only check in a fresh process: the new symbols exist,
every refusal the arguments alone decide comes back before any device is initialised (naming the entry where one is at fault), hipdec_quad_map gives the
coefficients of tests/project_ref.py bit for bit, and hipdec_project_stats reads zeros; and the accuracy of hipdec_perspective_map."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import project_ref as pr
from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_project_gpu.py"]
SYMBOLS = ["hipdec_tensor_project", "hipdec_batch_to_tensor_projected", "hipdec_album_to_tensor_projected", "hipdec_perspective_map", "hipdec_quad_map"]


def test_projected_output_on_the_emulated_library():
    _build()
    r = _run([os.path.join("tests", m) for m in MODULES], timeout=3000)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


HOST_ONLY = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[2])
import project_ref as pr
L = C.CDLL(sys.argv[1])
L.hipdec_last_error.restype = C.c_char_p
for n in sys.argv[3:]:
    assert hasattr(L, n), n
class Desc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]
class Map(C.Structure):
    _fields_ = [("a", C.c_double * 8), ("kind", C.c_int), ("reserved", C.c_int)]
class Warp(C.Structure):
    _fields_ = [("src_width", C.c_int), ("src_height", C.c_int), ("filter", C.c_int), ("reserved", C.c_int)]
class Fill(C.Structure):
    _fields_ = [("value", C.c_float * 3), ("domain", C.c_int), ("reserved", C.c_int)]
assert C.sizeof(Map) == 72
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_projected, L.hipdec_album_to_tensor_projected):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_tensor_project.argtypes = [vp, sz, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_project_stats.restype = None
L.hipdec_project_stats.argtypes = [C.POINTER(C.c_uint64)] * 2

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
    return (Map * len(ms))(*(Map((C.c_double * 8)(*m[1]), m[0], m[2] if len(m) > 2 else 0) for m in ms))
def fill(v=(0, 0, 0), domain=0, reserved=0):
    return Fill((C.c_float * 3)(*v), domain, reserved)
I8 = (1, 0, 0, 0, 1, 0, 0, 0)
ident = (0, I8)
def coeff(i, v, kind=0):
    m = list(I8); m[i] = v
    return (kind, tuple(m))
nan, inf = float("nan"), float("inf")
ROOM = 2 * 16 * 8 * 3
SIZE = (16, 8)

def go(call, stage, d=None, w=None, ms=None, f=None, n=2, codes=None, out=p, room=ROOM, h=handle, no_maps=False, no_warp=False):
    d = d if d is not None else desc()
    w = w if w is not None else Warp(9, 7, 16, 0)
    ms = ms if ms is not None else maps(ident, ident)
    wp, mp, fp = (None if no_warp else C.addressof(w)), (None if no_maps else C.addressof(ms)), (C.addressof(f) if f is not None else None)
    if stage:
        return call(h, 8192, wp, mp, fp, C.addressof(d), n, out, room, None)
    return call(h, C.byref(d), None, codes, wp, mp, fp, n, out, room, None)

for call, stage in ((L.hipdec_batch_to_tensor_projected, False), (L.hipdec_album_to_tensor_projected, False), (L.hipdec_tensor_project, True)):
    g = lambda **k: go(call, stage, **k)
    for kind in (0, 1):
        for i, bad in ((0, nan), (2, inf), (4, -inf), (6, nan), (7, -inf)):
            assert pr.refused(coeff(i, bad)[1], kind, SIZE)
            refused(g(ms=maps(ident, coeff(i, bad, kind))), names=1, says=b"not finite")
        for i, bad in ((0, 32000.0), (1, -32000.0), (5, 40000.0), (6, -32000.0), (7, 1e300)):
            assert pr.refused(coeff(i, bad)[1], kind, SIZE)
            refused(g(ms=maps(coeff(i, bad, kind), ident)), names=0, says=b"32000")
    for bad in ((0, (1, 0, 31985.0, 0, 1, 0, 0, 0)), (0, (1, 0, 0, 0, 1, 31993.0, 0, 0)), (0, (-2000.0, 0, 0, 0, 1, 0, 0, 0)), (0, (1, 0, 0, 0, 3999.9, 10.0, 0, 0)),
                (0, (1, 0, 0, 0, 1, 0, -1.0 / 16.001, 0)), (1, (31985.0, 1, 0, 0, 0, 0, 1, 0)), (1, (0, 0, 0, 250.0, 0, 0, 0, 1.0)), (1, (0, 0, 0, 0, 31993.0, 0, 1, 0))):
        assert pr.refused(bad[1], bad[0], SIZE)
        refused(g(ms=maps(ident, bad)), names=1, says=b"corner")
    for bad in ((1, 0, 0, 0, 1, 0, -1.0 / 16, 0), (1, 0, 0, 0, 1, 0, -1.0 / 16.00001, 0), (1, 0, 0, 0, 1, 0, 0, -0.2), (1, 0, 0, 0, 1, 0, -0.1, -0.1), (1, 0, 0, 0, 1, 0, 0, -0.125)):
        assert pr.refused(bad, 0, SIZE)
        refused(g(ms=maps(ident, (0, bad))), names=1, says=b"denominator")
    for kind in (2, -1, 7):
        refused(g(ms=maps(ident, (kind, I8))), names=1, says=b"kind")
    refused(g(ms=maps((1, I8, 1), ident)), names=0, says=b"reserved")
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
    small = (0, (0.001, 0, 0, 0, 0.001, 0, 0, 0))                                       # 46341 x 46341 pixels are 725 x 2897 tiles; times 1023 entries: 2^31 or more
    refused(g(d=desc(w=46341, h=46341), ms=maps(*([small] * 1023)), n=1023, room=1 << 62), code=-5, says=b"tiles")
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
        refused(g(h=None, ms=maps(ident, (1, (1, 0, 0, 0, 1, 0, -1.0 / 16, 0)))), says=b"bad arguments")   # (QUAD has no denominator)
# hipdec_quad_map against the restatement (which tests/test_project_ref.py pins to Pillow's QUAD from the corners), bit for bit
import numpy as np
L.hipdec_quad_map.argtypes = [C.POINTER(C.c_double), ci, ci, vp]
L.hipdec_perspective_map.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
rng = np.random.default_rng(12)
cases = [(c, s) for s in ((1, 1), (5, 7), (65, 17), (224, 224), (4095, 3)) for _, c in pr.quad_classes((33, 17), s)]
cases += [(tuple(rng.uniform(-300, 300, 8)), (int(rng.integers(1, 3000)), int(rng.integers(1, 3000)))) for _ in range(200)]
for corners, size in cases:
    m = Map()
    assert L.hipdec_quad_map((C.c_double * 8)(*corners), size[0], size[1], C.addressof(m)) == 0
    assert m.kind == 1 and m.reserved == 0
    want = pr.quad_map(corners, size)
    assert [v.hex() for v in m.a] == [float(v).hex() for v in want], (corners, size, tuple(m.a), want)
m = Map()
c8 = (C.c_double * 8)(0, 0, 0, 7, 9, 7, 9, 0)
for bad in ((0, 4), (4, -1)):
    refused(L.hipdec_quad_map(c8, bad[0], bad[1], C.addressof(m)))
refused(L.hipdec_quad_map(c8, 4, 4, None))
refused(L.hipdec_quad_map(None, 4, 4, C.addressof(m)))
refused(L.hipdec_quad_map((C.c_double * 8)(0, 0, nan, 7, 9, 7, 9, 0), 4, 4, C.addressof(m)))
e8 = (C.c_double * 8)(0, 0, 15, 0, 15, 7, 0, 7)
assert L.hipdec_perspective_map(e8, e8, C.addressof(m)) == 0 and m.kind == 0 and m.reserved == 0
assert np.allclose(tuple(m.a), (1, 0, 0, 0, 1, 0, 0, 0), rtol=0, atol=1e-12)
refused(L.hipdec_perspective_map((C.c_double * 8)(*([0.0] * 8)), e8, C.addressof(m)))             # singular
refused(L.hipdec_perspective_map(e8, (C.c_double * 8)(0, 0, 1, 1, 2, 2, 3, 3), C.addressof(m)))    # collinear end points
refused(L.hipdec_perspective_map(e8, (C.c_double * 8)(0, 0, inf, 0, 15, 7, 0, 7), C.addressof(m)))
refused(L.hipdec_perspective_map(None, e8, C.addressof(m)))
refused(L.hipdec_perspective_map(e8, e8, None))
s = [C.c_uint64(7), C.c_uint64(7)]
L.hipdec_project_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0]
L.hipdec_project_stats(None, None)
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_refusals_come_back_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header, n
    assert "HIPDEC_API void hipdec_project_stats(" in header
    assert "} hipdec_tensor_projection;" in header and "#define HIPDEC_PROJECT_PERSPECTIVE 0" in header and "#define HIPDEC_PROJECT_QUAD        1" in header
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB, os.path.join(ROOT, "tests")] + SYMBOLS + ["hipdec_project_stats"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]


class _Map(C.Structure):
    _fields_ = [("a", C.c_double * 8), ("kind", C.c_int), ("reserved", C.c_int)]


def _jittered_pairs(side, count, seed):
    """RandomPerspective's points with the jitter taken up to half the side: the picture's corners as start points, each end point moved inwards by whole
    pixels drawn from 0 .. side / 2 - 1 on either axis (so no two end points meet)"""
    rng = np.random.default_rng(seed)
    s = side - 1
    start = [(0.0, 0.0), (float(s), 0.0), (float(s), float(s)), (0.0, float(s))]
    out = []
    for _ in range(count):
        j = rng.integers(0, side // 2, 8)
        end = [(float(j[0]), float(j[1])), (float(s - j[2]), float(j[3])), (float(s - j[4]), float(s - j[5])), (float(j[6]), float(s - j[7]))]
        out.append((start, end))
    return out


def _error(a, exact, side):
    """The error of eight coefficients in source pixels at the far corner of a side x side output: a0, a1, a3, a4 multiply a coordinate of up to `side`, a2
    and a5 are offsets, a6 and a7 multiply a coordinate and scale a source coordinate of up to `side`.  One number per map: the largest weighted difference."""
    w = np.array([side, side, 1.0, side, side, 1.0, side * side, side * side], np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(exact, np.float64)) * w))


def test_perspective_map_is_as_accurate_as_lu_in_double():
    """hipdec_perspective_map against the exact solution of the same 8 x 8 system (fractions.Fraction, each coefficient rounded once to double) for corner
    jitter up to half the side at sizes 224 and 1024, 40 maps each.  The bound is not chosen: it is 4 x the error numpy.linalg.solve in float64 reaches
    against the exact solution on the same inputs - both are LU in double with partial pivoting, the factor covers the pivot order and the order of the
    sums.  The error of a map is _error above (source pixels at the far corner); a side's figure is the largest over its maps.
    Measured (x86-64; the bound is taken anew from NumPy on every run):
      side  224: hipdec_perspective_map 2.228e-11, numpy.linalg.solve 3.820e-11, bound 1.528e-10
      side 1024: hipdec_perspective_map 4.802e-10, numpy.linalg.solve 3.274e-10, bound 1.310e-09"""
    _build()
    L = C.CDLL(EMU_LIB)
    L.hipdec_perspective_map.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
    for side in (224, 1024):
        helper, lapack = [], []
        for start, end in _jittered_pairs(side, 40, 1000 + side):
            exact = pr.perspective_map_exact(start, end)
            m = _Map()
            sp, ep = [v for p in start for v in p], [v for p in end for v in p]
            assert L.hipdec_perspective_map((C.c_double * 8)(*sp), (C.c_double * 8)(*ep), C.addressof(m)) == 0, (start, end)
            assert m.kind == pr.PERSPECTIVE
            helper.append(_error(tuple(m.a), exact, side))
            lapack.append(_error(pr.perspective_map(start, end), exact, side))
        bound = 4.0 * max(lapack)
        print("side %d: hipdec_perspective_map %.3e, numpy.linalg.solve %.3e, bound %.3e" % (side, max(helper), max(lapack), bound))
        assert max(lapack) > 0.0
        assert max(helper) <= bound, (side, max(helper), max(lapack))
