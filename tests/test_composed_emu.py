"""Composed tensor output on the CPU tier: tests/test_composed_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the
host with the kernels under the SIMT emulator, the way tests/test_framed_emu.py runs its module; and a host-only check in a fresh process: the new symbols
exist, every refusal that the arguments alone decide comes back before any device is initialised with the entry named, hipdec_composed_stats reads zeros, and
the three helpers - hipdec_mosaic_tiles, hipdec_sheet_tiles, hipdec_compose_visible_area - are pinned against plain Python restatements over sweeps."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_composed_gpu.py"]
SYMBOLS = ["hipdec_batch_to_tensor_composed", "hipdec_album_to_tensor_composed", "hipdec_compose_visible_area", "hipdec_mosaic_tiles", "hipdec_sheet_tiles"]


def test_composed_output_on_the_emulated_library():
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
class Place(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]
class Tile(C.Structure):
    _fields_ = [("canvas", C.c_int), ("place", Place), ("clip", Place)]
class Fill(C.Structure):
    _fields_ = [("value", C.c_float * 3), ("domain", C.c_int), ("reserved", C.c_int)]
assert C.sizeof(Tile) == 36
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in (L.hipdec_batch_to_tensor_composed, L.hipdec_album_to_tensor_composed):
    f.argtypes = [vp, C.POINTER(Desc), vp, vp, vp, vp, vp, ci, ci, vp, sz, vp]
L.hipdec_compose_visible_area.argtypes = [ci, ci, vp, ci, ci, C.POINTER(C.c_uint64)]
L.hipdec_mosaic_tiles.argtypes = [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(Tile)]
L.hipdec_sheet_tiles.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), ci, ci, ci, C.POINTER(Tile)]
L.hipdec_letterbox_place.argtypes = [ci, ci, ci, ci, ci, ci, C.POINTER(Place)]
L.hipdec_composed_stats.restype = None
L.hipdec_composed_stats.argtypes = [C.POINTER(C.c_uint64)] * 5

def refused(rc, code=-1):
    assert rc == code, rc
    assert L.hipdec_last_error()

def tiles_of(ts):
    arr = (Tile * len(ts))()
    for k, (cv, pl, cl) in enumerate(ts):
        arr[k] = Tile(cv, Place(*pl), Place(*cl))
    return arr

buf = C.create_string_buffer(1 << 16)
p = C.addressof(buf)
handle = p                                  # never dereferenced: every call below is refused on its other arguments first, or on the NULL handle
ones, zeros = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
def desc(dtype=0, w=8, h=8, filt=1):
    return Desc(w, h, dtype, 0, filt, 0, ones, zeros)
def fill(values=(0, 0, 0), domain=0, reserved=0):
    return Fill((C.c_float * 3)(*values), domain, reserved)
nan, inf = float("nan"), float("inf")
M = 2 ** 24
ALL = (0, 0, 0, 0)
ok = (0, (-3, -2, 20, 20), ALL)
entries = (C.c_int * 12)()                                                                                          # (an entry list: the item count is not asked for)
for call in (L.hipdec_batch_to_tensor_composed, L.hipdec_album_to_tensor_composed):
    one = tiles_of([ok])
    refused(call(None, C.byref(desc()), None, None, C.addressof(one), None, None, 1, 1, p, 4096, None))             # NULL handle
    refused(call(handle, None, None, None, C.addressof(one), None, None, 1, 1, p, 4096, None))                      # no description
    refused(call(handle, C.byref(desc()), None, None, C.addressof(one), None, None, 1, 1, None, 4096, None))        # no output
    refused(call(handle, C.byref(desc()), None, None, None, None, None, 1, 1, p, 4096, None))                       # no tiles
    assert b"tiles" in L.hipdec_last_error(), L.hipdec_last_error()
    refused(call(handle, C.byref(desc()), None, None, C.addressof(one), None, None, 0, 1, p, 4096, None))           # no entry
    refused(call(handle, C.byref(desc()), None, None, C.addressof(one), None, None, 1, 0, p, 4096, None))           # no canvas
    refused(call(handle, C.byref(desc(w=0)), None, None, C.addressof(one), None, None, 1, 1, p, 4096, None))
    refused(call(handle, C.byref(desc(dtype=4)), None, None, C.addressof(one), None, None, 1, 1, p, 4096, None))
    refused(call(handle, C.byref(desc(filt=2)), None, None, C.addressof(one), None, None, 1, 1, p, 4096, None))
    codes = (C.c_int * 2)(0, 8)
    two = tiles_of([ok, ok])
    refused(call(handle, C.byref(desc()), None, C.addressof(codes), C.addressof(two), None, None, 2, 1, p, 4096, None))   # code 8
    assert b"entry 1" in L.hipdec_last_error()
    for bad in ((1, (0, 0, 4, 4), ALL), (-1, (0, 0, 4, 4), ALL),                                                    # a canvas outside 0 .. n_canvases - 1
                (0, (0, 0, 0, 8), ALL), (0, (0, 0, 8, 0), ALL), (0, (0, 0, -2, 4), ALL),                            # a non-positive side of place
                (0, (0, 0, 8, 8), (0, 0, 4, 0)), (0, (0, 0, 8, 8), (0, 0, 0, 4)), (0, (0, 0, 8, 8), (1, 1, -3, 4)), (0, (0, 0, 8, 8), (1, 1, 4, -1)),   # clip sides
                (0, (-4, 0, 4, 4), ALL), (0, (8, 0, 4, 4), ALL), (0, (0, -4, 4, 4), ALL), (0, (0, 8, 4, 4), ALL),   # place off the canvas
                (0, (0, 0, 8, 8), (8, 0, 4, 4)), (0, (0, 0, 8, 8), (-4, 2, 4, 4)), (0, (0, 0, 4, 4), (4, 4, 4, 4)), # clip off the canvas, clip beside place
                (0, (-M - 1, 0, M, 4), ALL), (0, (0, -M - 1, 4, M), ALL), (0, (0, 0, M + 1, 4), ALL), (0, (0, 0, 4, M + 1), ALL), (0, (2**31 - 1, 0, 1, 1), ALL),
                (0, (-2**31, -2**31, 2**31 - 1, 2**31 - 1), ALL),
                (0, (0, 0, 8, 8), (-M - 1, 0, M, 4)), (0, (0, 0, 8, 8), (0, M + 1, 4, 4)), (0, (0, 0, 8, 8), (0, 0, M + 1, 4)), (0, (0, 0, 8, 8), (0, 0, 4, 2**31 - 1))):
        ts = tiles_of([ok, bad])
        refused(call(handle, C.byref(desc()), None, None, C.addressof(ts), None, None, 2, 1, p, 4096, None))
        assert b"entry 1" in L.hipdec_last_error(), (bad, L.hipdec_last_error())
    many = tiles_of([(0, (k % 8, k // 8 % 8, 1, 1), ALL) for k in range(257)])                                      # more than 256 entries in one canvas
    refused(call(handle, C.byref(desc()), None, None, C.addressof(many), None, None, 257, 1, p, 4096, None))
    assert b"entry 256" in L.hipdec_last_error(), L.hipdec_last_error()
    a257 = (C.c_uint64 * 257)()
    assert L.hipdec_compose_visible_area(8, 8, C.addressof(many), 256, 1, a257) == 0 and sum(a257) == 64           # 256 are taken
    refused(L.hipdec_compose_visible_area(8, 8, C.addressof(many), 257, 1, a257))
    for dtype, f in ((1, fill((nan, 0, 0))), (1, fill((0, inf, 0), 1)), (0, fill((0, 0, -inf))), (2, fill((114.5, 0, 0))), (0, fill((0, 256, 0))), (1, fill((0, 0, -1))),
                     (1, fill((65536, 0, 0))), (0, fill(domain=2)), (1, fill(domain=-1)), (0, fill(reserved=1)), (0, fill((1.5, 0, 0), 1)), (0, fill((0, 256, 0), 1)),
                     (0, fill((0, 0, -1), 1))):
        refused(call(handle, C.byref(desc(dtype)), None, None, C.addressof(one), C.byref(f), None, 1, 1, p, 4096, None))
    spread = tiles_of([ok, (2, (0, 0, 8, 8), ALL)])
    refused(call(handle, C.byref(desc()), C.addressof(entries), None, C.addressof(spread), None, None, 2, 3, p, 3 * 8 * 8 * 3 - 1, None))   # out_bytes: n_canvases canvases
    assert b"out_bytes" in L.hipdec_last_error(), L.hipdec_last_error()
    # HIPDEC_ERR_LIMIT before a device is touched: 257 canvases of 256 disjoint entries are 65792 pieces; 256 canvases of 256 regions on rows of their own
    # are 256 tables of 2 * 514 + 2 * 256 words - more than 1 MiB
    pieces = tiles_of([(k // 256, (k % 16 * 2, k % 256 // 16 * 2, 1, 1), ALL) for k in range(257 * 256)])
    refused(call(handle, C.byref(desc(w=32, h=32)), None, None, C.addressof(pieces), None, None, 257 * 256, 257, p, 4096, None), -5)
    assert b"pieces" in L.hipdec_last_error(), L.hipdec_last_error()
    rows = tiles_of([(k // 256, (k % 4, k % 256 * 2, 1, 1), ALL) for k in range(256 * 256)])
    refused(call(handle, C.byref(desc(w=4, h=512)), None, None, C.addressof(rows), None, None, 256 * 256, 256, p, 4096, None), -5)
    assert b"cover tables" in L.hipdec_last_error(), L.hipdec_last_error()
s = [C.c_uint64(7) for _ in range(5)]
L.hipdec_composed_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0, 0, 0, 0, 0]
L.hipdec_composed_stats(None, None, None, None, None)

def flat(t):
    return (t.canvas, (t.place.x, t.place.y, t.place.width, t.place.height), (t.clip.x, t.clip.y, t.clip.width, t.clip.height))

# hipdec_mosaic_tiles: every centre of a 12 x 10 canvas, sizes 1 .. 15
def mosaic(W, H, xc, yc, sizes, cv):
    (w0, h0), (w1, h1), (w2, h2), (w3, h3) = sizes
    return [(cv, (xc - w0, yc - h0, w0, h0), (0, 0, xc, yc)), (cv, (xc, yc - h1, w1, h1), (xc, 0, W - xc, yc)),
            (cv, (xc - w2, yc, w2, h2), (0, yc, xc, H - yc)), (cv, (xc, yc, w3, h3), (xc, yc, W - xc, H - yc))]
out = (Tile * 4)()
n = 0
for xc in range(1, 12):
    for yc in range(1, 10):
        for s in range(1, 16):
            sizes = [(s, 16 - s), ((s * 7) % 15 + 1, s), (15, (s * 3) % 15 + 1), (16 - s, (s * 11) % 15 + 1)]
            assert L.hipdec_mosaic_tiles(12, 10, xc, yc, (ci * 4)(*[w for w, _ in sizes]), (ci * 4)(*[h for _, h in sizes]), 3, out) == 0
            assert [flat(t) for t in out] == mosaic(12, 10, xc, yc, sizes, 3), (xc, yc, sizes)
            n += 1
assert n == 11 * 9 * 15
w4, h4 = (ci * 4)(5, 5, 5, 5), (ci * 4)(5, 5, 5, 5)
for bad in ((12, 10, 0, 5), (12, 10, 12, 5), (12, 10, 5, 0), (12, 10, 5, 10), (0, 10, 0, 5), (12, -1, 5, 5), (M + 1, 10, 5, 5)):
    refused(L.hipdec_mosaic_tiles(*bad, w4, h4, 0, out))
refused(L.hipdec_mosaic_tiles(12, 10, 5, 5, (ci * 4)(5, 0, 5, 5), h4, 0, out))
refused(L.hipdec_mosaic_tiles(12, 10, 5, 5, w4, (ci * 4)(5, 5, 5, M + 1), 0, out))
refused(L.hipdec_mosaic_tiles(12, 10, 5, 5, w4, h4, -1, out))
refused(L.hipdec_mosaic_tiles(12, 10, 5, 5, w4, h4, 0, None))

# hipdec_sheet_tiles: sheets of 1 .. 4 x 1 .. 3 cells, gaps 0 .. 2, through hipdec_letterbox_place (pinned by tests/test_placed_emu.py)
def sheet(cols, rows, cw, ch, gap, sizes, up, cv):
    res = []
    for k, (w, h) in enumerate(sizes):
        pl = Place()
        assert L.hipdec_letterbox_place(w, h, cw, ch, up, 1, C.byref(pl)) == 0
        cx, cy = (k % cols) * (cw + gap), (k // cols) * (ch + gap)
        res.append((cv, (cx + pl.x, cy + pl.y, pl.width, pl.height), (cx, cy, cw, ch)))
    return res
n = 0
for cols in range(1, 5):
    for rows in range(1, 4):
        for gap in range(3):
            for count in sorted({1, cols * rows - 1, cols * rows} - {0}):
                for up in (0, 1):
                    sizes = [((k * 5) % 13 + 1, (k * 3) % 11 + 1) for k in range(count)]
                    o = (Tile * count)()
                    assert L.hipdec_sheet_tiles(cols, rows, 9, 7, gap, (ci * count)(*[w for w, _ in sizes]), (ci * count)(*[h for _, h in sizes]), count, up, 1, o) == 0
                    assert [flat(t) for t in o] == sheet(cols, rows, 9, 7, gap, sizes, up, 1), (cols, rows, gap, count, up)
                    n += 1
assert n >= 4 * 3 * 3 * 2 * 2
o = (Tile * 8)()
w8, h8 = (ci * 8)(*[5] * 8), (ci * 8)(*[5] * 8)
for bad in ((0, 2, 9, 7, 0, 1), (2, 0, 9, 7, 0, 1), (2, 2, 0, 7, 0, 1), (2, 2, 9, -1, 0, 1), (2, 2, 9, 7, -1, 1), (2, 2, 9, 7, 0, 0), (2, 2, 9, 7, 0, 5), (4, 2, M, 7, 0, 1)):
    refused(L.hipdec_sheet_tiles(*bad[:5], w8, h8, bad[5], 1, 0, o))
refused(L.hipdec_sheet_tiles(2, 2, 9, 7, 0, (ci * 8)(5, 0, 5, 5, 5, 5, 5, 5), h8, 2, 1, 0, o))
refused(L.hipdec_sheet_tiles(2, 2, 9, 7, 0, w8, h8, 2, 1, -1, o))
refused(L.hipdec_sheet_tiles(2, 2, 9, 7, 0, w8, h8, 2, 1, 0, None))

# hipdec_compose_visible_area: 200 seeded random tile lists against a NumPy painter
rng = np.random.default_rng(11)
for trial in range(200):
    W, H, nc = int(rng.integers(1, 24)), int(rng.integers(1, 18)), int(rng.integers(1, 4))
    ts = []
    while len(ts) < int(rng.integers(1, 20)) or not ts:
        pl = (int(rng.integers(-8, W + 4)), int(rng.integers(-8, H + 4)), int(rng.integers(1, 20)), int(rng.integers(1, 20)))
        cl = ALL if rng.integers(0, 2) else (int(rng.integers(-4, W + 2)), int(rng.integers(-4, H + 2)), int(rng.integers(1, 16)), int(rng.integers(1, 16)))
        x0, y0, x1, y1 = max(pl[0], 0), max(pl[1], 0), min(pl[0] + pl[2], W), min(pl[1] + pl[3], H)
        if cl != ALL:
            x0, y0, x1, y1 = max(x0, cl[0]), max(y0, cl[1]), min(x1, cl[0] + cl[2]), min(y1, cl[1] + cl[3])
        if x0 < x1 and y0 < y1:
            ts.append((int(rng.integers(0, nc)), pl, cl, (x0, y0, x1, y1)))
    owner = np.full((nc, H, W), -1)
    for e, (cv, _, _, (x0, y0, x1, y1)) in enumerate(ts):
        owner[cv, y0:y1, x0:x1] = e
    arr = tiles_of([t[:3] for t in ts])
    area = (C.c_uint64 * len(ts))()
    assert L.hipdec_compose_visible_area(W, H, C.addressof(arr), len(ts), nc, area) == 0, L.hipdec_last_error()
    assert list(area) == [int((owner == e).sum()) for e in range(len(ts))], (trial, W, H, ts)
area = (C.c_uint64 * 2)()
one = tiles_of([ok])
refused(L.hipdec_compose_visible_area(0, 8, C.addressof(one), 1, 1, area))
refused(L.hipdec_compose_visible_area(8, 8, None, 1, 1, area))
refused(L.hipdec_compose_visible_area(8, 8, C.addressof(one), 1, 1, None))
refused(L.hipdec_compose_visible_area(8, 8, C.addressof(one), 1, 0, area))
off = tiles_of([ok, (0, (8, 0, 4, 4), ALL)])
refused(L.hipdec_compose_visible_area(8, 8, C.addressof(off), 2, 1, area))
assert b"entry 1" in L.hipdec_last_error()

from libheif_amd import decoder
assert decoder.mosaic_tiles((12, 10), (5, 4), [(3, 3)] * 4, 2) == mosaic(12, 10, 5, 4, [(3, 3)] * 4, 2)
assert decoder.sheet_tiles((2, 2), (9, 7), [(5, 5), (20, 3), (1, 9)], gap=2, canvas=1) == sheet(2, 2, 9, 7, 2, [(5, 5), (20, 3), (1, 9)], 1, 1)
assert decoder.sheet_size((2, 2), (9, 7), 2) == (20, 16)
t, order = decoder.cutmix_tiles((8, 6), [(1, 1, 3, 2), (6, 4, 5, 5)])
assert t == [(0, (0, 0, 8, 6), ALL), (0, (0, 0, 8, 6), (1, 1, 3, 2)), (1, (0, 0, 8, 6), ALL), (1, (0, 0, 8, 6), (6, 4, 5, 5))] and order == [(0, 0), (0, 1), (1, 0), (1, 1)]
assert decoder.compose_visible_area((8, 6), t) == [42, 6, 44, 4]
assert decoder.composed_stats() == (0, 0, 0, 0, 0)
for bad in (lambda: decoder.mosaic_tiles((12, 10), (0, 4), [(3, 3)] * 4), lambda: decoder.mosaic_tiles((12, 10), (5, 4), [(3, 3)] * 3),
            lambda: decoder.sheet_tiles((2, 2), (9, 7), [(5, 5)] * 5), lambda: decoder.compose_visible_area((8, 6), [(0, (9, 0, 2, 2), ALL)])):
    try:
        bad()
        raise AssertionError("a bad argument was taken")
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
    assert "HIPDEC_API void hipdec_composed_stats(" in header and "} hipdec_tensor_tile;" in header
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_composed_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
