"""Clips on the CPU tier: tests/test_clips_gpu.py - unchanged - against tests/emu/libheifhip_emu.so, the whole library compiled for the host with the kernels
under the SIMT emulator, the way tests/test_packed_emu.py runs its module; and a host-only check in a fresh process: the new symbols exist, every refusal
the arguments alone decide comes back before any device is initialised (naming the entry, or the track, where one is at fault), hipdec_clips_stats reads
zeros, and hipdec_clip_packed_layout is pinned against a plain Python restatement, its own refusals included."""
import os
import subprocess
import sys

from test_product_on_emulator import EMU_LIB, ROOT, _build, _run

MODULES = ["test_clips_gpu.py"]
SYMBOLS = ["hipdec_clips_create", "hipdec_clips_free", "hipdec_clips_run", "hipdec_clips_status", "hipdec_clips_track_count", "hipdec_clips_frame_count",
           "hipdec_clips_frame", "hipdec_clips_frame_plane", "hipdec_clips_read_plane", "hipdec_clips_batch", "hipdec_clips_to_tensor",
           "hipdec_clips_to_tensor_packed", "hipdec_clip_packed_layout"]


def test_clips_on_the_emulated_library():
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
class Clip(C.Structure):
    _fields_ = [("frames", C.c_int), ("order", C.c_int), ("temporal_patch", C.c_int), ("reserved", C.c_int)]
class Entry(C.Structure):
    _fields_ = [("item", C.c_int), ("left", C.c_int), ("top", C.c_int), ("width", C.c_int), ("height", C.c_int), ("flip", C.c_int)]
class Sample(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("offset", C.c_uint64)]
class Patches(C.Structure):
    _fields_ = [("patch", C.c_int), ("merge", C.c_int), ("reserved", C.c_int * 2)]
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
L.hipdec_clips_to_tensor.argtypes = [vp, C.POINTER(Desc), C.POINTER(Clip), vp, vp, vp, ci, vp, sz, vp]
L.hipdec_clips_to_tensor_packed.argtypes = [vp, C.POINTER(Desc), C.POINTER(Clip), vp, vp, vp, vp, vp, ci, vp, sz, vp]
L.hipdec_clip_packed_layout.argtypes = [C.POINTER(Clip), vp, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
L.hipdec_clips_create.argtypes = [C.POINTER(vp), ci, C.POINTER(ci), C.POINTER(C.c_char_p), C.POINTER(sz), C.c_uint64]
L.hipdec_clips_stats.restype = None
L.hipdec_clips_stats.argtypes = [C.POINTER(C.c_uint64)] * 5

def refused(rc, code=-1, names=None, word=None):
    assert rc == code, (rc, L.hipdec_last_error())
    assert L.hipdec_last_error()
    if names is not None:
        assert (b"entry %d" % names) in L.hipdec_last_error(), L.hipdec_last_error()
    if word is not None:
        assert word in L.hipdec_last_error(), L.hipdec_last_error()

buf = C.create_string_buffer(1 << 16)
p = C.addressof(buf)
ones, zeros = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
def desc(dtype=0, w=8, h=8, filt=1, layout=0):
    return Desc(w, h, dtype, layout, filt, 0, ones, zeros)
entries = (Entry * 2)(Entry(0, 0, 0, 0, 0, 0), Entry(0, 0, 0, 0, 0, 0))
E = C.addressof(entries)
def ints(*v):
    return (ci * len(v))(*v)
good_frames = ints(0, 1, 2, 3)

# ---- hipdec_clips_to_tensor: everything below is decided before the handle is read (it is NULL, or never dereferenced)
def go(d=None, clip=None, fr=good_frames, codes=None, n=2, out=p, room=1 << 16, h=None, e=E):
    return L.hipdec_clips_to_tensor(h, C.byref(d if d is not None else desc()), C.byref(clip) if clip is not None else None, e,
                                    C.addressof(fr) if fr is not None else None, C.addressof(codes) if codes is not None else None, n, out, room, None)
two = Clip(2, 0, 0, 0)
refused(go(clip=two))                                                                   # NULL handle
refused(go(clip=two, h=p, out=None))
refused(go(clip=two, h=p, e=None))
refused(go(clip=None, h=p), word=b"clip")
refused(go(clip=two, h=p, fr=None), word=b"frame")                                      # frames NULL
refused(go(clip=Clip(0, 0, 0, 0), h=p), word=b"frames")                                 # T < 1
refused(go(clip=Clip(-2, 0, 0, 0), h=p), word=b"frames")
refused(go(clip=Clip(2, 0, 0, 1), h=p), word=b"reserved")
refused(go(clip=Clip(2, 0, 2, 0), h=p), word=b"temporal_patch")                         # temporal_patch > 1 in the dense call
refused(go(clip=Clip(2, 0, -1, 0), h=p), word=b"temporal_patch")
refused(go(clip=Clip(2, 2, 0, 0), h=p), word=b"order")
refused(go(clip=Clip(2, 1, 0, 0), d=desc(layout=1), h=p), word=b"channel-major")        # channel-major + NHWC
refused(go(clip=two, h=p, fr=ints(0, 1, 2, -1)), names=1, word=b"frame index -1")      # a negative frame index names the entry
refused(go(clip=two, h=p, fr=ints(-5, 1, 2, 3)), names=0)
refused(go(clip=two, h=p, codes=ints(0, 8)), names=1)                                   # a code outside 0 .. 7
refused(go(clip=two, h=p, d=desc(w=0)))
refused(go(clip=two, h=p, d=desc(dtype=4)))
refused(go(clip=two, h=p, d=desc(filt=9)))
refused(go(clip=two, h=p, d=desc(layout=2)))
refused(go(clip=two, h=p, n=0))
refused(go(clip=two, h=p, room=2 * 2 * 3 * 64 - 1), word=b"out_bytes")                  # n * T * 3 * H * W elements
refused(go(clip=two, h=p, d=desc(dtype=1), room=4 * 2 * 2 * 3 * 64 - 1), word=b"out_bytes")

# ---- hipdec_clips_to_tensor_packed
def samples(*s):
    return (Sample * len(s))(*(Sample(*x) for x in s))
def patches(patch=0, merge=1, r0=0, r1=0):
    return Patches(patch, merge, (C.c_int * 2)(r0, r1))
good = samples((8, 8, 0), (8, 8, 384))
def gop(d=None, clip=two, fr=good_frames, codes=None, s=good, pt=None, n=2, out=p, room=1 << 16, h=p):
    return L.hipdec_clips_to_tensor_packed(h, C.byref(d if d is not None else desc(w=0, h=0)), C.byref(clip) if clip is not None else None, E,
                                           C.addressof(fr) if fr is not None else None, C.addressof(codes) if codes is not None else None,
                                           C.addressof(s) if s is not None else None, C.byref(pt) if pt is not None else None, n, out, room, None)
refused(gop(h=None))
refused(gop(s=None), word=b"samples")
refused(gop(d=desc(w=8, h=0)))                                                          # the sizes are per clip
refused(gop(fr=None), word=b"frame")
refused(gop(clip=Clip(2, 0, 2, 0)), word=b"temporal_patch")                             # dense clips take 0 or 1
refused(gop(clip=Clip(3, 0, 2, 0), pt=patches(4)), word=b"temporal_patch 2")            # T % Tp
refused(gop(clip=Clip(2, 0, 17, 0), pt=patches(4)), word=b"temporal_patch")
refused(gop(clip=Clip(2, 0, -1, 0), pt=patches(4)), word=b"temporal_patch")
refused(gop(clip=Clip(2, 1, 2, 0), pt=patches(4)), word=b"channel-major")               # channel-major order with patches
refused(gop(clip=Clip(2, 1, 0, 0), d=desc(w=0, h=0, layout=1)), word=b"channel-major")
for pt in (patches(-1), patches(257), patches(4, 0), patches(4, 17), patches(0, 2), patches(4, 1, 1, 0), patches(4, 1, 0, 1)):
    refused(gop(pt=pt))
for bad in ((0, 8, 384), (8, -1, 384)):
    refused(gop(s=samples((8, 8, 0), bad)), names=1)
refused(gop(s=samples((8, 8, 0), (12, 8, 384)), pt=patches(4, 2)), names=1)             # a side that is no multiple of patch * merge
refused(gop(s=samples((8, 8, 0), (8, 8, 383))), names=1, word=b"overlap")               # 3 * T * w * h = 384 elements per clip
refused(gop(s=samples((8, 8, 200), (8, 8, 0))), word=b"overlap")
refused(gop(s=samples((8, 8, 0), (8, 8, (1 << 16) - 383))), names=1)                    # offset + 3Twh above out_bytes / sizeof(element)
refused(gop(s=samples((8, 8, 0), (8, 8, 2**64 - 1))), names=1)
refused(gop(d=desc(dtype=2, w=0, h=0), s=samples((8, 8, 0), (8, 8, (1 << 15) - 383))), names=1)
refused(gop(fr=ints(0, 1, -1, 3)), names=1)
refused(gop(codes=ints(9, 0)), names=0)

# ---- hipdec_clips_create: what the arguments alone decide
h = vp()
blob = b"\x00\x00\x00\x02\x40\x01"
arr = (C.c_char_p * 2)(blob, blob)
sizes = (sz * 2)(len(blob), len(blob))
refused(L.hipdec_clips_create(None, 1, ints(1), arr, sizes, 0))
refused(L.hipdec_clips_create(C.byref(h), 0, ints(1), arr, sizes, 0))
refused(L.hipdec_clips_create(C.byref(h), 1, None, arr, sizes, 0))
refused(L.hipdec_clips_create(C.byref(h), 1, ints(1), None, sizes, 0))
refused(L.hipdec_clips_create(C.byref(h), 1, ints(1), arr, None, 0))
refused(L.hipdec_clips_create(C.byref(h), 2, ints(1, 0), arr, sizes, 0), word=b"track 1")
refused(L.hipdec_clips_create(C.byref(h), 2, ints(1, 1), arr, (sz * 2)(len(blob), 0), 0), word=b"track 1, sample 0")
refused(L.hipdec_clips_create(C.byref(h), 2, ints(1, 1), arr, (sz * 2)(len(blob), 5), 0), code=-2, word=b"track 1, sample 0")     # truncated framing
refused(L.hipdec_clips_create(C.byref(h), 1, ints(2), arr, sizes, 0), code=-3, word=b"track 0, sample 0")                          # a sample without a coded picture
refused(L.hipdec_clips_create(C.byref(h), 2, ints(1000, 25), arr, sizes, 0), code=-5, word=b"track 1")                             # the chain limit, before a sample is read
assert not h.value
refused(L.hipdec_clips_track_count(None))
refused(L.hipdec_clips_frame_count(None, 0))
L.hipdec_clips_free(None)

s = [C.c_uint64(7) for _ in range(5)]
L.hipdec_clips_stats(*[C.byref(x) for x in s])
assert [x.value for x in s] == [0] * 5
L.hipdec_clips_stats(None, None, None, None, None)

# ---- hipdec_clip_packed_layout against a plain restatement
def layout(sizes, T, P, m, Tp):
    if T < 1 or Tp < 0 or Tp > 16 or (not P and Tp > 1):
        return None
    tp = max(Tp, 1)
    if T % tp:
        return None
    offs, toks, at = [], [], 0
    for w, h in sizes:
        if w < 1 or h < 1 or (P and (w % (P * m) or h % (P * m))):
            return None
        offs.append(at); toks.append((T // tp) * (w // P) * (h // P) if P else 0); at += 3 * T * w * h
    return offs, toks, at
from libheif_amd import decoder
cases = 0
for P in (0, 1, 4, 14):
    for m in (1, 2):
        if P == 0 and m != 1:
            continue
        for T, Tp in ((1, 0), (1, 1), (4, 2), (3, 2), (6, 3), (16, 2), (2, 17), (0, 1), (4, -1)):
            unit = max(P, 1) * m
            for sizes in ([(unit * a, unit * b) for a in range(1, 4) for b in (1, 5)], [(w, h) for w in range(1, 30) for h in (unit, 29)], [(unit, unit)]):
                n = len(sizes)
                ws, hs = (ci * n)(*[w for w, _ in sizes]), (ci * n)(*[h for _, h in sizes])
                offs, toks, total = (C.c_uint64 * n)(), (C.c_uint32 * n)(), C.c_uint64()
                pt, cd = patches(P, m), Clip(T, 0, Tp, 0)
                rc = L.hipdec_clip_packed_layout(C.byref(cd), C.byref(pt), ws, hs, n, offs, toks, C.byref(total))
                want = layout(sizes, T, P, m, Tp)
                if want is None:
                    refused(rc)
                    try:
                        decoder.clip_packed_layout(sizes, T, P, m, Tp)
                        raise AssertionError((sizes, T, P, m, Tp))
                    except ValueError:
                        pass
                else:
                    assert rc == 0 and (list(offs), list(toks), total.value) == want, (P, m, T, Tp, sizes)
                    assert decoder.clip_packed_layout(sizes, T, P, m, Tp) == want
                    assert L.hipdec_clip_packed_layout(C.byref(cd), C.byref(pt), ws, hs, n, None, None, None) == 0
                cases += 1
assert cases == 7 * 9 * 3
one = (ci * 1)(8)
cd = Clip(4, 0, 0, 0)
assert L.hipdec_clip_packed_layout(C.byref(cd), None, one, one, 1, None, None, C.byref(total)) == 0 and total.value == 4 * 192     # patches NULL: dense
refused(L.hipdec_clip_packed_layout(None, None, one, one, 1, None, None, None))
refused(L.hipdec_clip_packed_layout(C.byref(cd), None, None, one, 1, None, None, None))
refused(L.hipdec_clip_packed_layout(C.byref(cd), None, one, one, 0, None, None, None))
refused(L.hipdec_clip_packed_layout(C.byref(Clip(4, 0, 0, 1)), None, one, one, 1, None, None, None))
refused(L.hipdec_clip_packed_layout(C.byref(Clip(4, 1, 2, 0)), C.byref(patches(4)), one, one, 1, None, None, None))                # channel-major with patches
print("HOST ONLY OK")
"""


def test_new_symbols_exist_and_the_host_side_is_pinned_without_a_device():
    """in a fresh process, so that nothing has initialised a device before the refusals"""
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    for n in SYMBOLS:
        assert "HIPDEC_API int %s(" % n in header or "HIPDEC_API void %s(" % n in header or "HIPDEC_API hipdec_batch* %s(" % n in header, n
    assert "HIPDEC_API void hipdec_clips_stats(" in header
    for t in ("hipdec_clip_frame", "hipdec_clip_desc", "hipdec_clip_order"):
        assert "} %s;" % t in header, t
    env = dict(os.environ, HIPDEC_LIBRARY=EMU_LIB, HIPDEC_DEV_AB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB] + SYMBOLS + ["hipdec_clips_stats"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
