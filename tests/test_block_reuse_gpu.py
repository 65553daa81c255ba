"""The colour stage's launch kit (libheif_amd/csrc/color.hip: blocks_reserve / blocks_upload, launch_z_chunks) as the output forms use it on ONE handle.

Reuse: a form keeps its block array on the device between calls and uploads it only when its bytes change.  One Batch of two SMALL stills goes through
    A, A again (nothing to upload: same arguments, same output buffer), B (as many entries, other windows / codes / maps / chains / sizes: changed in
    place), C (four times the entries: the array grows), A again (inside the grown capacity)
for each form, and after every call the WHOLE poisoned output buffer - the mask of the placed form too - equals what a fresh Batch writes for the same
arguments.  The two RGB forms have one entry per item of the batch, so their sequence is A, A, B, A (B: other sizes, or another out_chroma).

Second chunk: a grid's z extent is 65535, so a call of 65537 entries is two launches of every kernel.  Entry k of such a call equals entry k mod 8 of an
eight-entry call on a fresh handle; the entries from index 65535 on are compared on their own.  All three forms passed on the commit before the launch kit.

Runs on the MI355X (`-m gpu`) and, through tests/test_block_reuse_emu.py, against the library compiled for the host."""
import ctypes as C
import functools
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer, check
from libheif_amd.color import SCALE_BILINEAR, SCALE_BOX, SCALE_NEAREST
from test_oriented_gpu import SMALL
from test_scale_gpu import _batch, _still
from test_tensor_gpu import BIAS, SCALE, _lib

pytestmark = pytest.mark.gpu

POISON = 0xA5
ES = {"uint8": 1, "float16": 2}
WINDOWS = [(0, 0, 0, 0), (5, 7, 33, 17), (1, 3, 35, 21), (37, 11, 31, 29)]   # (left, top, width, height) in the 72 x 40 stills; zeros: the whole picture
SIZE = (16, 12)
CALLS = "AABCA"


def _streams():
    cf, bits, vui, size = SMALL
    return [_still(cf, bits, vui, size, seed=s) for s in (11, 12)]


def _fresh():
    return _batch(_streams())


def entries_of(v):
    """A and B: two entries, C: eight - item, window, flip"""
    n, shift = {"A": (2, 0), "B": (2, 1), "C": (8, 2)}[v]
    return [((e + shift) % 2,) + WINDOWS[(e + shift) % 4] + ((e + shift) // 2 % 2,) for e in range(n)]


def codes_of(v):
    return {"A": (1, 6), "B": (4, 3), "C": tuple(range(8))}[v]


def _poisoned(keep, key, nbytes):
    """the output buffer of (form, variant) on this handle - the SAME device memory every time, so that a repeated call repeats its blocks - filled with POISON"""
    if key not in keep:
        keep[key] = DeviceBuffer(nbytes)
    src = np.full(nbytes, POISON, np.uint8)
    check(_lib().hipdec_memcpy_h2d(keep[key].ptr, src.ctypes.data, nbytes))
    return keep[key]


def _whole(b, buf):
    check(b._lib.hipdec_stream_synchronize(None))
    return buf.to_numpy((buf.nbytes,), np.uint8)


def _tensor_form(dtype="float16", layout="NCHW", **kw):
    def form(b, v, keep):
        entries = entries_of(v)
        out = _poisoned(keep, v, len(entries) * 3 * SIZE[0] * SIZE[1] * ES[dtype] + 256)
        call_kw = {k: (f(v) if callable(f) else f) for k, f in kw.items()}
        b.to_tensor(SIZE, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out, **call_kw)
        return _whole(b, out)
    return form


def _placed(b, v, keep):
    entries = entries_of(v)
    n, canvas = len(entries), (16, 16)
    places = [[(2, 1, 13, 9), (0, 3, 16, 11), (7, 5, 9, 6), (1, 0, 5, 16)][(e + ord(v)) % 4] for e in range(n)]
    out = _poisoned(keep, v, n * 3 * canvas[0] * canvas[1] * 2 + 256)
    mask = _poisoned(keep, v + "-mask", n * canvas[0] * canvas[1] + 64)
    b.to_tensor(canvas, entries, dtype="bfloat16", layout="NHWC", scale=SCALE, bias=BIAS, filter=SCALE_BOX, out=out, orientations=codes_of(v), places=places, fill=114, mask=mask)
    return np.concatenate([_whole(b, out), _whole(b, mask)])


def _packed(b, v, keep):
    entries = entries_of(v)
    sizes = [[(8, 16), (16, 8), (8, 8), (16, 16)][(e + ord(v)) % 4] for e in range(len(entries))]
    offsets, at = [], 16
    for w, h in sizes:
        offsets.append(at)
        at += 3 * w * h + 16
    out = _poisoned(keep, v, at * 2)
    b.to_tensor_packed(sizes, entries, patch=4, merge=2, dtype="float16", layout="NCHW", scale=SCALE, bias=BIAS, filter=SCALE_BOX, orientations=codes_of(v), offsets=offsets,
                       out=out)
    return _whole(b, out)


def _warped(b, v, keep):
    entries = entries_of(v)
    angle = {"A": 30.0, "B": -75.0, "C": 11.0}[v]
    maps = [decoder.rotate_matrix(angle * (e + 1), SIZE) if e % 3 else (0.5, 0.0, 1.0 + e, 0.0, 0.5, 2.0) for e in range(len(entries))]   # (e % 3 == 0: Pillow's scale path)
    out = _poisoned(keep, v, len(entries) * 3 * SIZE[0] * SIZE[1] * 2 + 256)
    b.to_tensor_warped(SIZE, maps, entries, warp_filter=SCALE_NEAREST if v == "B" else SCALE_BILINEAR, fill=(3, 200, 77), orientations=codes_of(v), filter=SCALE_BOX,
                       dtype="float16", layout="NHWC", scale=SCALE, bias=BIAS, out=out)
    return _whole(b, out)


def _photo(b, v, keep):
    entries = entries_of(v)
    pool = [[("contrast", 1.4), ("sharpness", 1.6)], [("equalize",)], [], [("color", 0.0), ("autocontrast",), ("posterize", 5), ("brightness", 0.7)], [("solarize", 100)]]
    chains = [pool[(e + ord(v)) % len(pool)] for e in range(len(entries))]
    out = _poisoned(keep, v, len(entries) * 3 * SIZE[0] * SIZE[1] + 256)
    b.to_tensor_photo(SIZE, chains, entries, filter=SCALE_BILINEAR, orientations=codes_of(v), dtype="uint8", layout="NCHW", out=out)
    return _whole(b, out)


def _rgb_all(b, v, keep):
    if v not in keep:
        b.alloc_rgb({"A": 10, "B": 11}[v])
        keep[v] = b.rgb_state()
    b.use_rgb(keep[v])
    for buf, stride, h in b._rgb:
        check(_lib().hipdec_memcpy_h2d(buf.ptr, np.full(buf.nbytes, POISON, np.uint8).ctypes.data, buf.nbytes))
    b.to_rgb_all()
    return np.concatenate([b.rgb(i).ravel() for i in range(b.n)])


_SCALED_STATE = ("_srgb", "_srgb_chroma", "_srgb_w", "_srgb_h", "_srgb_ptrs", "_srgb_strides")


def _rgb_scaled_all(b, v, keep):
    if v not in keep:
        b.alloc_rgb_scaled({"A": [(16, 9), (7, 16)], "B": [(5, 3), (16, 16)]}[v], 10)
        keep[v] = {k: getattr(b, k) for k in _SCALED_STATE}
    for k, value in keep[v].items():
        setattr(b, k, value)
    for buf, stride, h in b._srgb:
        check(_lib().hipdec_memcpy_h2d(buf.ptr, np.full(buf.nbytes, POISON, np.uint8).ctypes.data, buf.nbytes))
    b.to_rgb_scaled_all(SCALE_BOX)
    return np.concatenate([b.rgb_scaled(i).ravel() for i in range(b.n)])


FORMS = {
    "box": (_tensor_form(filter=SCALE_BOX), CALLS),
    "box-oriented": (_tensor_form(layout="NHWC", filter=SCALE_BOX, orientations=codes_of), CALLS),
    "bilinear": (_tensor_form(dtype="uint8", filter=SCALE_BILINEAR), CALLS),
    "placed": (_placed, CALLS),
    "packed": (_packed, CALLS),
    "warped": (_warped, CALLS),
    "photo": (_photo, CALLS),
    "rgb-all": (_rgb_all, "AABA"),
    "rgb-scaled-all": (_rgb_scaled_all, "AABA"),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_a_block_array_is_reused_changed_in_place_and_grown(name):
    form, calls = FORMS[name]
    want = {}
    for v in sorted(set(calls)):
        fresh = _fresh()
        try:
            want[v] = form(fresh, v, {})
        finally:
            fresh.free()
        assert (want[v] != POISON).any(), "the fresh call wrote nothing"
    b, keep = _fresh(), {}
    try:
        for k, v in enumerate(calls):
            got = form(b, v, keep)
            assert got.shape == want[v].shape
            assert np.array_equal(got, want[v]), (name, calls[:k + 1], int((got != want[v]).sum()))
    finally:
        b.free()


N_MANY = 65537


def _many(b, n, filt, margin, keep):
    """n entries that cycle over the two stills and the four windows, 4 x 4 uint8 NCHW, through the C ABI (the entry array is built in one step);
    margin: the placed form, a 2 x 2 rectangle inside a one-pixel margin"""
    k = np.arange(n)
    arr = np.zeros((n, 6), np.int32)
    arr[:, 0] = k % 2
    arr[:, 1:5] = np.array(WINDOWS, np.int32)[(k // 2) % 4]
    entries = (decoder.TensorEntry * n).from_buffer(arr)
    desc = decoder.tensor_desc((4, 4), "uint8", "NCHW", filt)
    out = _poisoned(keep, "out", n * 48 + 256)
    if margin:
        places = (decoder.TensorPlace * n).from_buffer(np.tile(np.array([1, 1, 2, 2], np.int32), (n, 1)))
        fill = decoder.tensor_fill(114)
        check(b._lib.hipdec_batch_to_tensor_placed(b._h, C.byref(desc), entries, None, places, fill, None, n, out.ptr, out.nbytes, None))
    else:
        check(b._lib.hipdec_batch_to_tensor(b._h, C.byref(desc), entries, n, out.ptr, out.nbytes, None))
    raw = _whole(b, out)
    assert (raw[n * 48:] == POISON).all(), "bytes behind the tensor were written"
    return raw[:n * 48].reshape(n, 48)


@functools.lru_cache(maxsize=None)
def _eight(filt, margin):
    fresh = _fresh()
    try:
        return _many(fresh, 8, filt, margin, {})
    finally:
        fresh.free()


@pytest.mark.parametrize("filt,margin", [(SCALE_BOX, False), (SCALE_BILINEAR, False), (SCALE_BOX, True)], ids=["box", "bilinear", "placed"])
def test_entries_beyond_the_z_extent_of_a_grid_go_out_in_a_second_launch(filt, margin):
    ref = _eight(filt, margin)
    assert len({r.tobytes() for r in ref}) == 8, "the eight entries do not differ: a misplaced one would pass"
    b = _fresh()
    try:
        got = _many(b, N_MANY, filt, margin, {})
    finally:
        b.free()
    idx = np.arange(N_MANY) % 8
    assert np.array_equal(got[65535:], ref[idx[65535:]]), "the entries of the second launch"
    bad = np.flatnonzero((got != ref[idx]).any(axis=1))
    assert bad.size == 0, (bad[:8], bad.size)
