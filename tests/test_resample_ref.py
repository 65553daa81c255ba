"""HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC on the CPU tier: (a) the NumPy restatement tests/resample_ref.py against PIL.Image.resize, bit for bit;
(b) the coefficient tables the kernel receives (hipdec_resample_taps, host only) against the restatement's, tap for tap; (c) the refusals of the new
filter values, in a fresh process, before a device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_ref as rr
from test_product_on_emulator import EMU_LIB, ROOT, _build

FILTERS = [rr.BILINEAR, rr.BICUBIC]

# (input w, h, output w, h, channels, crop window or None)
PIL_CASES = [
    (200, 136, 100, 66, 3, None), (200, 136, 37, 23, 3, None), (141, 93, 300, 200, 3, None), (256, 256, 224, 224, 3, None),
    (200, 136, 200, 23, 3, None), (200, 136, 7, 136, 3, None), (200, 136, 1, 1, 3, None), (1, 1, 5, 4, 3, None), (1, 1, 1, 1, 1, None),
    (17, 9, 224, 31, 1, None), (256, 200, 64, 48, 1, None), (200, 136, 64, 64, 3, (3, 5, 100, 81)), (141, 93, 50, 50, 3, (37, 1, 51, 45)),
]


def test_the_restatement_is_pillow_bit_for_bit():
    if os.path.isdir("/root/reference"):   # the development machine: skipping here would hide the pin
        import PIL   # noqa: F401
    Image = pytest.importorskip("PIL.Image")
    pil = {rr.BILINEAR: Image.BILINEAR, rr.BICUBIC: Image.BICUBIC}
    rng = np.random.default_rng(2024)
    n = 0
    for (w, h, ow, oh, ch, win) in PIL_CASES:
        a = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        if ch == 1:
            a = a[:, :, 0]
        for f in FILTERS:
            im = Image.fromarray(a)   # (h, w) -> mode L, (h, w, 3) -> RGB
            src = a
            if win:
                l, t, cw, chh = win
                im = im.crop((l, t, l + cw, t + chh))
                src = a[t:t + chh, l:l + cw]
            exp = np.asarray(im.resize((ow, oh), pil[f]))
            got = rr.resample(src, ow, oh, f)
            assert got.shape == exp.shape and np.array_equal(got, exp), (w, h, ow, oh, ch, win, f, int(np.abs(got.astype(int) - exp.astype(int)).max()))
            n += 1
    assert n >= 25


AXES = [(200, 100), (200, 37), (200, 1), (141, 300), (93, 93), (4096, 224), (17, 224), (1, 4)]


def _lib():
    from libheif_amd._capi import library_path
    L = C.CDLL(library_path())
    L.hipdec_resample_taps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int]
    L.hipdec_resample_taps.restype = C.c_int
    return L


@pytest.mark.parametrize("filt", FILTERS)
def test_the_kernels_tables_are_the_restatements_tap_for_tap(filt):
    L = _lib()
    cap = 512
    buf = (C.c_int32 * cap)()
    first = C.c_int(-1)
    for n_in, n_out in AXES:
        t = rr.table(n_in, n_out, filt)
        for xx, (xmin, k) in enumerate(t):
            n = L.hipdec_resample_taps(n_in, n_out, filt, xx, C.byref(first), buf, cap)
            assert n == len(k) and n <= cap and first.value == xmin, (n_in, n_out, xx, n, len(k), first.value, xmin)
            assert tuple(buf[:n]) == k, (n_in, n_out, xx)
    # a capacity below the count: the count is still returned and nothing behind the capacity is written
    buf[3] = 12345
    n = L.hipdec_resample_taps(4096, 224, filt, 100, C.byref(first), buf, 3)
    assert n > 3 and buf[3] == 12345 and tuple(buf[:3]) == rr.table(4096, 224, filt)[100][1][:3]
    assert L.hipdec_resample_taps(200, 100, filt, 5, C.byref(first), None, 0) == len(rr.table(200, 100, filt)[5][1])
    for bad in ((0, 4, filt, 0), (4, 0, filt, 0), (4, 4, filt, 4), (4, 4, filt, -1), (4, 4, 1, 0), (4, 4, 0, 0), (4, 4, 18, 0)):
        assert L.hipdec_resample_taps(bad[0], bad[1], bad[2], bad[3], C.byref(first), buf, cap) < 0, bad
    assert L.hipdec_resample_taps(4, 4, filt, 0, None, buf, cap) < 0


def test_the_int32_accumulator_bound_of_the_header_holds():
    """2^21 + 255 * sum |k| over the axes above stays below 2^31 (the kernel accumulates in int32)"""
    worst = 0
    for filt in FILTERS:
        for n_in, n_out in AXES + [(4096, 1), (4096, 4095), (3, 4096)]:
            for _, k in rr.table(n_in, n_out, filt):
                worst = max(worst, (1 << 21) + 255 * sum(abs(v) for v in k))
    assert worst < (1 << 31), worst


HOST_ONLY = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
L.hipdec_last_error.restype = C.c_char_p
class Img(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("chroma", C.c_int), ("bit_depth", C.c_int), ("plane", C.c_void_p * 4), ("stride", C.c_size_t * 4), ("on_device", C.c_int)]
class Desc(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("filter", C.c_int), ("reserved", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]
buf = C.create_string_buffer(64 * 64 * 12)
a = Img()
a.width, a.height, a.chroma, a.bit_depth = 64, 64, 0, 8
a.plane[0], a.stride[0] = C.addressof(buf), 128
def desc(**kw):
    d = Desc(8, 8, 2, 0, 16, 0, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
    for k, v in kw.items():
        setattr(d, k, v)
    return d
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
L.hipdec_tensor_bytes.restype = sz
L.hipdec_tensor_bytes.argtypes = [C.POINTER(Desc), ci]
L.hipdec_image_to_tensor.argtypes = [C.POINTER(Img), vp, C.POINTER(Desc), vp, ci, vp, sz, ci]
L.hipdec_batch_to_rgb_scaled.argtypes = [vp, ci, ci, ci, ci, ci, vp, sz, vp]
L.hipdec_batch_to_rgb_scaled_all.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]
L.hipdec_album_to_rgb_scaled_all.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]
for f in (16, 17):
    assert L.hipdec_tensor_bytes(C.byref(desc(filter=f)), 3) == 3 * 3 * 8 * 8 * 2
    assert L.hipdec_tensor_bytes(C.byref(desc(filter=f, dtype=0)), 1) == 3 * 8 * 8
for f in (2, 15, 18, -1):
    assert L.hipdec_tensor_bytes(C.byref(desc(filter=f)), 1) == 0, f
    rc = L.hipdec_image_to_tensor(C.byref(a), None, C.byref(desc(filter=f)), None, 1, C.addressof(buf), len(buf), 0)
    assert rc == -1 and b"unknown filter" in L.hipdec_last_error(), (f, rc)
# a float dtype from a source above 8 bits: refused as unsupported, for every float dtype; U8 is the form that exists
a.bit_depth = 10
for f in (16, 17):
    for dt in (1, 2, 3):
        rc = L.hipdec_image_to_tensor(C.byref(a), None, C.byref(desc(filter=f, dtype=dt)), None, 1, C.addressof(buf), len(buf), 0)
        assert rc == -4 and b"HIPDEC_TENSOR_U8" in L.hipdec_last_error(), (f, dt, rc, L.hipdec_last_error())
# another out_chroma with a new filter: unsupported, decided from the arguments alone
one = (C.c_int * 1)(8)
outs = (C.c_void_p * 1)(C.addressof(buf))
strides = (C.c_size_t * 1)(64)
for f in (16, 17):
    for oc in (11, 12, 14, 0):
        for rc in (L.hipdec_batch_to_rgb_scaled(None, 0, oc, 8, 8, f, C.addressof(buf), 64, None),
                   L.hipdec_batch_to_rgb_scaled_all(None, oc, one, one, f, outs, strides, None),
                   L.hipdec_album_to_rgb_scaled_all(None, oc, one, one, f, outs, strides, None)):
            assert rc == -4 and b"out_chroma" in L.hipdec_last_error(), (f, oc, rc, L.hipdec_last_error())
    assert L.hipdec_batch_to_rgb_scaled(None, 0, 10, 8, 8, f, C.addressof(buf), 64, None) == -1
print("HOST ONLY OK")
"""


def test_the_new_filter_values_are_refused_where_they_have_no_meaning_without_a_device():
    _build()
    header = open(os.path.join(ROOT, "include", "heif_hipdec.h")).read()
    assert "HIPDEC_SCALE_BILINEAR = 16" in header and "HIPDEC_SCALE_BICUBIC = 17" in header
    assert "HIPDEC_API int hipdec_resample_taps(" in header
    r = subprocess.run([sys.executable, "-c", HOST_ONLY, EMU_LIB], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "HOST ONLY OK" in r.stdout, r.stdout[-2000:]
