"""Tensor output on the device: hipdec_batch_to_tensor / hipdec_image_to_tensor (crop window, scale, flip, normalise, dense NCHW / NHWC tensor).

Everything is bit-exact, there are no tolerances, and no expected value comes from the code under test:
  NEAREST  V(x, y) = full(left + x * rw // ow, top + y * rh // oh), `full` = Batch.to_rgb (out_chroma 10, or 14 for the native-depth value of float
           dtypes from sources above 8 bits), hipdec_color_convert for the image form; the whole picture additionally equals Batch.to_rgb_scaled
           NEAREST, which tests/test_scale_gpu.py pins to the compiled reference.
  BOX      Batch.planes cropped by the window rule (luma [left, left + rw), chroma [left >> sH, ((left + rw - 1) >> sH) + 1), the same in y), each
           plane through `box_plane` of tests/test_scale_gpu.py (the definition of include/heif_hipdec.h in int64 NumPy), then hipdec_color_convert of
           the three planes as a 4:4:4 image (out_chroma 10 / 14); the whole picture additionally equals Batch.to_rgb_scaled BOX.
  floats   np.float32(V) * scale + bias in float32 (a multiply, then an add), .astype(np.float16) for F16, (bits + 0x7fff + ((bits >> 16) & 1)) >> 16
           on the float32 bits for BF16; bit patterns are compared.

Box alignment: a window at an odd `left` takes the aligned row loads because the window travels to the kernel as an offset and the plane pointer is not
moved.  The evidence here is a kernel-argument inspection (hipdec_batch_tensor_block: the parameter block as it was uploaded): the pointer is the
plane's own, 4-sample aligned, and the odd offset is in the block.  box_columns (color.hip) takes the 32- / 64-bit loads exactly when pointer, stride
and the group's first column are aligned, and box_tile starts the groups at (offset + first column) & ~3.

Runs on the MI355X (`-m gpu`) and, through tests/test_tensor_emu.py, against the library compiled for the host."""
import ctypes as C
import os
import numpy as np
import pytest

import libheif_amd
from libheif_amd import color, decoder
from libheif_amd._capi import DeviceBuffer, HipDecError, Nclx, check
from libheif_amd.color import ColorImage, SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import TensorDesc, TensorEntry
from oracle import pyoracle as orc
from test_scale_gpu import STILLS, VUI_FULL, VUI_LIMITED, _batch, _color_convert_444, _lib as _scale_lib, _random_image, _still, box_plane, full_shape

pytestmark = pytest.mark.gpu

DTYPES = ("uint8", "float32", "float16", "bfloat16")
LAYOUTS = ("NCHW", "NHWC")
SCALE = np.array([1.0 / 255.0 / 0.229, 0.017507, 3.0], np.float32)       # nothing that is exact in binary16 / bfloat16
BIAS = np.array([-0.485 / 0.229, -2.0357141, 0.25], np.float32)


def _lib():
    L = _scale_lib()
    decoder._bind(L)
    return L


def _shifts(cf):
    return (1 if cf in (1, 2) else 0), (1 if cf == 1 else 0)


def _whole(e, w, h):
    item, left, top, rw, rh, flip = e
    return (item, 0, 0, w, h, flip) if (left, top, rw, rh) == (0, 0, 0, 0) else e


def nearest_V(full, win, ow, oh):
    """full: (h, w, 3); the formula of the header, 64-bit products"""
    left, top, rw, rh = win
    iy = top + np.arange(oh, dtype=np.int64) * rh // oh
    ix = left + np.arange(ow, dtype=np.int64) * rw // ow
    return full[iy[:, None], ix[None, :], :]


def crop_planes(planes, cf, win):
    left, top, rw, rh = win
    sH, sV = _shifts(cf)
    out = [planes[0][top:top + rh, left:left + rw]]
    for p in planes[1:]:
        out.append(p[top >> sV:((top + rh - 1) >> sV) + 1, left >> sH:((left + rw - 1) >> sH) + 1])
    return out


def box_V(L, planes, cf, bits, nclx, win, ow, oh, native):
    scaled = [box_plane(np.ascontiguousarray(p), ow, oh) for p in crop_planes(planes, cf, win)]
    rows = _color_convert_444(L, scaled, cf, bits, nclx, 14 if native else 10)
    return (rows.view(np.uint16) if native else rows).reshape(oh, ow, 3)


def bf16_bits(f32):
    bits = f32.view(np.uint32).astype(np.uint64)
    return ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def elements(V, dtype, scale, bias):
    """V: (..., 3) integers -> the tensor's elements as comparable bit patterns"""
    if dtype == "uint8":
        return V.astype(np.uint8)
    f = V.astype(np.float32) * scale.astype(np.float32) + bias.astype(np.float32)
    assert f.dtype == np.float32
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)
    return bf16_bits(f)


def as_bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def expected_tensor(Vs, flips, dtype, layout, scale, bias):
    """Vs: one (oh, ow, 3) array per entry"""
    out = []
    for V, flip in zip(Vs, flips):
        e = elements(V, dtype, scale, bias)
        if flip:
            e = e[:, ::-1, :]
        out.append(e.transpose(2, 0, 1) if layout == "NCHW" else e)
    return np.stack(out)


def run_tensor(b, size, entries, dtype, layout, filt, scale=SCALE, bias=BIAS):
    n = b.n if entries is None else len(entries)
    nbytes = n * 3 * size[0] * size[1] * {"uint8": 1, "float32": 4}.get(dtype, 2)
    out = DeviceBuffer(nbytes)
    assert b.to_tensor(size, entries, dtype=dtype, layout=layout, scale=scale, bias=bias, filter=filt, out=out) is out
    got = b.tensor_to_host()
    assert got.shape == ((n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3))
    return as_bits(got)


def windows_of(w, h):
    """entries of one item: whole, flipped whole, odd offset to the right / bottom edge, odd offset + even size, even offset + odd size (flipped), 1 x 1"""
    return [(0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1), (0, 1, 1, w - 1, h - 1, 0), (0, 37, 21, 64, 40, 0), (0, 36, 20, 63, 41, 1), (0, w - 1, h - 1, 1, 1, 0),
            (0, 5, 7, 1, 1, 1), (0, 3, 2, 2, 1, 0)]


SIZES = [(50, 34), (48, 32), (1, 1), (7, 3), (100, 90)]     # widths that are / are not multiples of 4, 1 x 1, up-scaling for most windows


def _full_rgb(b, i, native):
    d = b.info(i)
    rows = b.to_rgb(i, 14 if native else 10)
    return (rows.view(np.uint16) if native else rows).reshape(d["height"], d["width"], 3)


def _nclx_of(d):
    return (d["colour_primaries"], d["transfer_characteristics"], d["matrix_coeffs"], d["full_range_flag"])


STILLS_12 = [(1, 12, VUI_LIMITED, (142, 94)), (3, 12, VUI_FULL, (141, 93))]


@pytest.mark.parametrize("filt", [SCALE_NEAREST, SCALE_BOX])
@pytest.mark.parametrize("cf,bits,vui,size", STILLS + STILLS_12)
def test_to_tensor_is_the_definition(cf, bits, vui, size, filt):
    """every chroma format and bit depth, both filters and layouts, all four dtypes; several entries of one item in one call"""
    L = _lib()
    b = _batch([_still(cf, bits, vui, size)])
    try:
        d = b.info(0)
        w, h = d["width"], d["height"]
        planes, nclx = b.planes(0), _nclx_of(d)
        entries = windows_of(w, h)
        wins = [_whole(e, w, h)[1:5] for e in entries]
        flips = [e[5] for e in entries]
        full = {False: _full_rgb(b, 0, False)}
        if bits > 8:
            full[True] = _full_rgb(b, 0, True)
        for ow, oh in SIZES:
            Vs = {}
            for native in full:
                if filt == SCALE_NEAREST:
                    Vs[native] = [nearest_V(full[native], win, ow, oh) for win in wins]
                else:
                    Vs[native] = [box_V(L, planes, cf, bits, nclx, win, ow, oh, native) for win in wins]
            for dtype in DTYPES:
                native = bits > 8 and dtype != "uint8"
                for layout in LAYOUTS:
                    want = expected_tensor(Vs[native], flips, dtype, layout, SCALE, BIAS)
                    got = run_tensor(b, (ow, oh), entries, dtype, layout, filt)
                    assert np.array_equal(got, want), ((ow, oh), dtype, layout, int((got != want).sum()))
    finally:
        b.free()


@pytest.mark.parametrize("cf,bits,vui,size", [STILLS[0], STILLS[3], STILLS[4], STILLS[6], STILLS[7]])
def test_whole_picture_is_to_rgb_scaled_and_identity_is_to_rgb(cf, bits, vui, size):
    """uint8 NHWC of the whole picture is hipdec_batch_to_rgb_scaled byte for byte, both filters; at the picture's own size NEAREST is hipdec_batch_to_rgb;
    a window at its own size is that crop of hipdec_batch_to_rgb"""
    b = _batch([_still(cf, bits, vui, size)])
    try:
        w, h = size
        for filt in (SCALE_NEAREST, SCALE_BOX):
            for ow, oh in ((50, 34), (48, 32), (1, 1), (w, h), (w + 9, h + 5)):
                want = b.to_rgb_scaled(0, ow, oh, filt, 10).reshape(1, oh, ow, 3)
                got = run_tensor(b, (ow, oh), None, "uint8", "NHWC", filt)
                assert np.array_equal(got, want), (filt, (ow, oh))
        full = _full_rgb(b, 0, False)
        assert np.array_equal(run_tensor(b, (w, h), [(0, 0, 0, 0, 0, 0)], "uint8", "NHWC", SCALE_NEAREST)[0], full)
        got = run_tensor(b, (64, 40), [(0, 37, 21, 64, 40, 0), (0, 37, 21, 64, 40, 1)], "uint8", "NHWC", SCALE_NEAREST)
        assert np.array_equal(got[0], full[21:61, 37:101]) and np.array_equal(got[1], full[21:61, 37:101][:, ::-1])
        if cf in (0, 3):   # no subsampled plane: the box filter at the window's own size is a copy as well
            got = run_tensor(b, (63, 41), [(0, 37, 21, 63, 41, 0)], "uint8", "NHWC", SCALE_BOX)
            assert np.array_equal(got[0], full[21:62, 37:100])
    finally:
        b.free()


def test_entries_over_several_items_and_entries_null():
    sizes_in = [(200, 136), (142, 94), (64, 64), (136, 200)]
    streams = [_still(1, 8, VUI_FULL if k % 2 else VUI_LIMITED, s, seed=30 + k) for k, s in enumerate(sizes_in)]
    L = _lib()
    b = _batch(streams)
    try:
        fulls = [_full_rgb(b, i, False) for i in range(b.n)]
        planes = [b.planes(i) for i in range(b.n)]
        nclx = [_nclx_of(b.info(i)) for i in range(b.n)]
        entries = [(3, 1, 3, 99, 150, 1), (0, 0, 0, 0, 0, 0), (2, 11, 13, 32, 32, 0), (0, 101, 35, 99, 101, 0), (1, 0, 0, 0, 0, 1), (3, 0, 0, 0, 0, 0), (0, 7, 9, 50, 30, 1)]
        for filt in (SCALE_NEAREST, SCALE_BOX):
            for (ow, oh), dtype, layout in (((56, 56), "float16", "NCHW"), ((30, 21), "bfloat16", "NHWC"), ((30, 21), "float32", "NCHW")):
                def V(i, win):
                    if filt == SCALE_NEAREST:
                        return nearest_V(fulls[i], win, ow, oh)
                    return box_V(L, planes[i], 1, 8, nclx[i], win, ow, oh, False)
                wins = [_whole(e, *sizes_in[e[0]])[1:5] for e in entries]
                want = expected_tensor([V(e[0], win) for e, win in zip(entries, wins)], [e[5] for e in entries], dtype, layout, SCALE, BIAS)
                got = run_tensor(b, (ow, oh), entries, dtype, layout, filt)
                assert np.array_equal(got, want), (filt, dtype, layout)
                # entries == NULL: entry i is the whole of item i
                want = expected_tensor([V(i, (0, 0) + sizes_in[i]) for i in range(b.n)], [0] * b.n, dtype, layout, SCALE, BIAS)
                got = run_tensor(b, (ow, oh), None, dtype, layout, filt)
                assert np.array_equal(got, want), ("NULL entries", filt, dtype, layout)
    finally:
        b.free()


def test_scales_that_land_in_the_f16_subnormal_range_and_on_exact_zeros():
    b = _batch([_still(1, 8, VUI_FULL, (200, 136))])
    try:
        full = _full_rgb(b, 0, False)
        entries = [(0, 0, 0, 0, 0, 0), (0, 33, 17, 101, 77, 1)]
        wins = [(0, 0, 200, 136), (33, 17, 101, 77)]
        Vs = [nearest_V(full, win, 50, 34) for win in wins]
        cases = [(np.array([1.7e-7, 2.9e-8, 5.96e-8], np.float32), np.zeros(3, np.float32)),         # 255 * 1.7e-7 = 4.3e-5 < 2^-14: binary16 subnormals, and ties
                 (np.array([0.0, 1.0, -1.0], np.float32), np.array([0.0, 0.0, 0.0], np.float32)),        # +0, V, -V with -0.0 where V = 0
                 (np.array([3.0e4, 1.0e36, -1.0e36], np.float32), np.array([1.0, 0.0, 0.0], np.float32))]   # binary16 overflow; float32 overflow to +-inf
        for sc, bi in cases:
            for dtype in ("float16", "bfloat16", "float32"):
                with np.errstate(over="ignore"):
                    want = expected_tensor(Vs, [0, 1], dtype, "NCHW", sc, bi)
                got = run_tensor(b, (50, 34), entries, dtype, "NCHW", SCALE_NEAREST, sc, bi)
                assert np.array_equal(got, want), (sc, dtype, int((got != want).sum()))
        sub = expected_tensor(Vs, [0, 1], "float16", "NCHW", cases[0][0], cases[0][1])
        assert ((sub & 0x7c00) == 0).all() and (sub & 0x3ff).any(), "the first case is meant to sit in the binary16 subnormal range"
        zero = expected_tensor(Vs, [0, 1], "float16", "NCHW", cases[1][0], cases[1][1])
        assert (zero[:, 0] == 0).all()
    finally:
        b.free()


def test_mean_std_are_folded_as_the_docstring_states():
    b = _batch([_still(1, 10, VUI_FULL, (142, 94))])
    try:
        mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        full8, full10 = _full_rgb(b, 0, False), _full_rgb(b, 0, True)
        for dtype, full, maxv in (("float16", full10, 1023), ("float32", full10, 1023), ("uint8", full8, 255)):
            sc = np.float32(1) / (np.float32(maxv) * np.array(std, np.float32))
            bi = -np.array(mean, np.float32) / np.array(std, np.float32)
            assert np.array_equal(np.stack(decoder.tensor_scale_bias(mean, std, max_value=maxv)), np.stack([sc, bi]))
            out = DeviceBuffer(3 * 40 * 30 * 4)
            b.to_tensor((40, 30), None, dtype=dtype, layout="NCHW", mean=mean, std=std, filter=SCALE_NEAREST, out=out)
            got = as_bits(b.tensor_to_host())
            want = expected_tensor([nearest_V(full, (0, 0, 142, 94), 40, 30)], [0], dtype, "NCHW", sc, bi)
            assert np.array_equal(got, want), dtype
        with pytest.raises(ValueError):
            b.to_tensor((40, 30), None, mean=mean, scale=1.0, out=DeviceBuffer(3 * 40 * 30 * 2))
    finally:
        b.free()


# ---- the image form ------------------------------------------------------------------------------------------------------------------------------

def _color_convert(L, planes, cf, bits, nclx, out_chroma):
    """hipdec_color_convert of the image as it is, nearest-neighbour chroma"""
    h, w = planes[0].shape
    img = ColorImage()
    img.width, img.height, img.chroma, img.bit_depth, img.on_device = w, h, cf, bits, 0
    keep = [np.ascontiguousarray(p) for p in planes]
    for c, p in enumerate(keep):
        img.plane[c], img.stride[c] = p.ctypes.data, p.strides[0]
    bpp = {10: 3, 14: 6}[out_chroma]
    out = np.empty((h, w * bpp), np.uint8)
    n = Nclx(1, *nclx)
    check(L.hipdec_color_convert(C.byref(img), C.byref(n), out_chroma, 1, 0, out.ctypes.data, w * bpp, 0))
    return (out.view(np.uint16) if out_chroma == 14 else out).reshape(h, w, 3)


IMAGES = [(1, 8, (1, 13, 6, 1)), (1, 8, (1, 13, 1, 0)), (2, 8, (1, 13, 6, 1)), (3, 8, (1, 13, 2, 1)), (0, 8, (1, 13, 6, 1)),
          (1, 10, (9, 16, 9, 1)), (1, 10, (9, 16, 9, 0)), (2, 12, (1, 13, 1, 0)), (3, 12, (1, 13, 6, 1)), (1, 12, (2, 2, 2, 1))]


@pytest.mark.parametrize("cf,bits,nclx", IMAGES)
def test_image_to_tensor_on_an_odd_sized_image(cf, bits, nclx):
    """381 x 251 (SHAPES of tests/test_scale_gpu.py): odd sizes for the subsampled formats too, windows that touch the right and the bottom edge"""
    L = _lib()
    w, h = 381, 251
    planes, _ = _random_image(w, h, cf, bits, False, seed=7 * cf + bits)
    full = {False: _color_convert(L, planes, cf, bits, nclx, 10)}
    if bits > 8:
        full[True] = _color_convert(L, planes, cf, bits, nclx, 14)
    entries = [(0, 0, 0, 0, 0), (1, 1, 380, 250, 1), (379, 249, 2, 2, 0), (380, 250, 1, 1, 0), (37, 21, 64, 40, 1), (36, 20, 301, 41, 0), (0, 250, 381, 1, 0)]
    wins = [(0, 0, w, h) if e[:4] == (0, 0, 0, 0) else e[:4] for e in entries]
    flips = [e[4] for e in entries]
    for filt in (SCALE_NEAREST, SCALE_BOX):
        for ow, oh in ((50, 34), (48, 32), (1, 1)):
            for dtype, layout in (("uint8", "NHWC"), ("float16", "NCHW"), ("bfloat16", "NCHW"), ("float32", "NHWC")):
                native = bits > 8 and dtype != "uint8"
                if filt == SCALE_NEAREST:
                    Vs = [nearest_V(full[native], win, ow, oh) for win in wins]
                else:
                    Vs = [box_V(L, planes, cf, bits, nclx, win, ow, oh, native) for win in wins]
                want = expected_tensor(Vs, flips, dtype, layout, SCALE, BIAS)
                got = as_bits(color.image_to_tensor(planes, bits, cf, nclx, (ow, oh), entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt))
                assert np.array_equal(got, want), (filt, (ow, oh), dtype, layout, int((got != want).sum()))
    # entries == NULL: one entry, the whole image
    got = as_bits(color.image_to_tensor(planes, bits, cf, nclx, (48, 32), None, dtype="uint8", layout="NHWC", filter=SCALE_NEAREST))
    assert np.array_equal(got[0], nearest_V(full[False], (0, 0, w, h), 48, 32))


def test_image_to_tensor_takes_device_planes_and_a_device_destination():
    L = _lib()
    w, h = 128, 96
    planes, _ = _random_image(w, h, 1, 8, False, seed=3)
    nclx = (1, 13, 6, 1)
    want = as_bits(color.image_to_tensor(planes, 8, 1, nclx, (40, 30), [(3, 5, 100, 80, 1)], dtype="float16", layout="NCHW", scale=SCALE, bias=BIAS))
    img = ColorImage()
    img.width, img.height, img.chroma, img.bit_depth, img.on_device = w, h, 1, 8, 1
    keep = []
    for c, p in enumerate(planes):
        pad = np.zeros((p.shape[0], p.shape[1] + 3), np.uint8)       # odd strides: the byte loop of the row loads
        pad[:, :p.shape[1]] = p
        keep.append(DeviceBuffer.from_numpy(pad))
        img.plane[c], img.stride[c] = keep[-1].ptr, pad.shape[1]
    desc = decoder.tensor_desc((40, 30), "float16", "NCHW", SCALE_BOX, SCALE, BIAS)
    ent = decoder.tensor_entries([(0, 3, 5, 100, 80, 1)])
    out = DeviceBuffer(3 * 40 * 30 * 2)
    n = Nclx(1, *nclx)
    check(L.hipdec_image_to_tensor(C.byref(img), C.byref(n), C.byref(desc), ent, 1, out.ptr, out.nbytes, 1))
    assert np.array_equal(out.to_numpy((1, 3, 30, 40), np.uint16), want)


# ---- the full shape ------------------------------------------------------------------------------------------------------------------------------

@full_shape
def test_full_shape_random_resized_crop_to_224():
    """a decoded 3840 x 2160 still to 224 x 224 from random-resized-crop windows (and the whole picture, which takes the chunk loop: 3840 / 224 > 4 tiles
    of boxes 17 columns wide), float16 NCHW"""
    L = _lib()
    w, h = 3840, 2160
    b = _batch([_still(1, 8, VUI_LIMITED, (w, h), seed=77)])
    try:
        d = b.info(0)
        assert (d["width"], d["height"]) == (w, h)
        rng = np.random.default_rng(2024)
        entries = decoder.random_resized_crop_entries(rng, [(w, h)] * 3, items=[0, 0, 0]) + [(0, 0, 0, 0, 0, 0)]
        assert entries == decoder.random_resized_crop_entries(np.random.default_rng(2024), [(w, h)] * 3, items=[0, 0, 0]) + [(0, 0, 0, 0, 0, 0)]
        for e in entries[:3]:
            assert 0 <= e[1] and e[1] + e[3] <= w and 0 <= e[2] and e[2] + e[4] <= h and e[3] > 0 and e[4] > 0
        planes, nclx, full = b.planes(0), _nclx_of(d), _full_rgb(b, 0, False)
        wins = [_whole(e, w, h)[1:5] for e in entries]
        flips = [e[5] for e in entries]
        want = expected_tensor([box_V(L, planes, 1, 8, nclx, win, 224, 224, False) for win in wins], flips, "float16", "NCHW", SCALE, BIAS)
        got = run_tensor(b, (224, 224), entries, "float16", "NCHW", SCALE_BOX)
        assert np.array_equal(got, want), int((got != want).sum())
        want = expected_tensor([nearest_V(full, win, 224, 224) for win in wins], flips, "float16", "NCHW", SCALE, BIAS)
        got = run_tensor(b, (224, 224), entries, "float16", "NCHW", SCALE_NEAREST)
        assert np.array_equal(got, want), int((got != want).sum())
    finally:
        b.free()


def test_example_host_writes_a_tensor(tmp_path):
    """examples/decode_batch.c --tensor N end to end: float16 NCHW of the centred squares, its checksum is Batch.to_tensor's; a bad N prints the usage"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.abspath(libheif_amd.library_path())
    exe = str(tmp_path / "decode_batch")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    r = subprocess.run([exe, "--tensor", "0", "x.hevc"], capture_output=True, text=True)
    assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    items = [((200, 136), VUI_FULL), ((136, 200), VUI_LIMITED), ((64, 64), VUI_FULL)]
    files = []
    for k, (size, vui) in enumerate(items):
        f = tmp_path / ("item%d.hevc" % k)
        f.write_bytes(_still(1, 8, vui, size, seed=60 + k))
        files.append(str(f))
    r = subprocess.run([exe, "--tensor", "56"] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    b = _batch([_still(1, 8, vui, size, seed=60 + k) for k, (size, vui) in enumerate(items)])
    try:
        entries = [decoder.center_crop_entry(k, w, h, min(w, h)) for k, ((w, h), _) in enumerate(items)]
        out = DeviceBuffer(3 * 3 * 56 * 56 * 2)
        b.to_tensor((56, 56), entries, dtype="float16", layout="NCHW", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=out)
        want = int(b.tensor_to_host().view(np.uint16).astype(np.uint64).sum())
        assert "tensor 3x3x56x56 float16, sum of the bit patterns %d\n" % want in r.stdout, r.stdout
    finally:
        b.free()


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------------

def test_crop_helpers_are_plain_host_arithmetic():
    assert decoder.center_crop_entry(2, 381, 251, 224) == (2, 78, 13, 224, 224, 0)
    assert decoder.center_crop_entry(0, 200, 136, 100, 36, flip=True) == (0, 50, 50, 100, 36, 1)
    with pytest.raises(ValueError):
        decoder.center_crop_entry(0, 200, 136, 224)
    sizes = [(200, 136), (3840, 2160), (64, 64), (5, 900)]
    a = decoder.random_resized_crop_entries(np.random.default_rng(5), sizes)
    assert a == decoder.random_resized_crop_entries(np.random.default_rng(5), sizes)
    assert a != decoder.random_resized_crop_entries(np.random.default_rng(6), sizes)
    for k, ((w, h), e) in enumerate(zip(sizes, a)):
        assert e[0] == k and e[3] >= 1 and e[4] >= 1 and e[1] >= 0 and e[2] >= 0 and e[1] + e[3] <= w and e[2] + e[4] <= h and e[5] in (0, 1)
    ratio = a[3][3] / a[3][4]      # 5 x 900 admits no window inside the ratio range: the centred fall-back, clamped to 3 / 4
    assert a[3][3] == 5 and abs(ratio - 0.75) < 0.2


# ---- box alignment -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cf,bits,vui,size", [STILLS[0], STILLS[6]])
def test_a_box_window_at_an_odd_offset_keeps_the_plane_pointer(cf, bits, vui, size):
    """kernel-argument inspection (see the module docstring): the blocks the box kernel received carry the PLANE's pointer and the window as an offset"""
    L = _lib()
    b = _batch([_still(cf, bits, vui, size)])
    try:
        es = 2 if bits > 8 else 1
        run_tensor(b, (48, 32), [(0, 37, 21, 101, 77, 0), (0, 0, 0, 0, 0, 0)], "float16", "NCHW", SCALE_BOX)
        for plane in range(3):
            p, st = C.c_void_p(), C.c_size_t()
            check(L.hipdec_batch_device_plane(b._h, 0, plane, C.byref(p), C.byref(st)))
            ptr, stride, x, y, w, h = b.tensor_block(0, plane)
            assert (ptr, stride) == (p.value, st.value), plane
            assert ptr % (4 * es) == 0 and stride % (4 * es) == 0, "the decoder's planes are aligned to the vector loads"
            assert (x, y, w, h) == ((37, 21, 101, 77) if plane == 0 else (18, 10, 51, 39)), plane
            assert b.tensor_block(1, plane)[2:] == ((0, 0) + size if plane == 0 else (0, 0, size[0] // 2, size[1] // 2))
        with pytest.raises(HipDecError):
            b.tensor_block(2, 0)
    finally:
        b.free()


# ---- refusals, life cycle, counters ----------------------------------------------------------------------------------------------------------------

def _refused(L, rc, code):
    assert rc == code, (rc, L.hipdec_last_error())
    assert L.hipdec_last_error(), "hipdec_last_error() is empty after a refusal"


def _desc(size=(40, 30), dtype="float16", layout="NCHW", filt=SCALE_BOX, scale=1.0, bias=0.0):
    return decoder.tensor_desc(size, dtype, layout, filt, scale, bias)


def test_tensor_calls_refuse_bad_arguments_with_a_message():
    L = _lib()
    b = _batch([_still(1, 8, VUI_FULL, (200, 136))])
    try:
        out = DeviceBuffer(3 * 40 * 30 * 4 * 2)
        call = lambda desc, entries, n, nbytes=out.nbytes: L.hipdec_batch_to_tensor(b._h, C.byref(desc), decoder.tensor_entries(entries) if entries else None, n, out.ptr, nbytes, None)
        good = _desc()
        assert L.hipdec_tensor_bytes(C.byref(good), 2) == 2 * 3 * 40 * 30 * 2
        for e in ((0, 150, 0, 51, 10, 0), (0, 0, 100, 10, 37, 0), (0, -1, 0, 10, 10, 0), (0, 0, -1, 10, 10, 0), (0, 200, 0, 1, 1, 0),      # leaves the picture
                  (0, 5, 5, 0, 10, 0), (0, 5, 5, 10, -2, 0), (0, 0, 0, 0, 10, 0), (0, 2 ** 31 - 1, 0, 2 ** 31 - 1, 1, 0),                  # non-positive / overflowing
                  (1, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0)):                                                                               # no such item
            _refused(L, call(good, [e], 1), -1)
        for bad in (_desc(size=(0, 30)), _desc(size=(40, -1))):
            _refused(L, call(bad, None, 1), -1)
            assert L.hipdec_tensor_bytes(C.byref(bad), 1) == 0
        for field, value in (("dtype", 4), ("dtype", -1), ("layout", 2), ("layout", -1), ("filter", 2), ("filter", -1)):
            bad = _desc()
            setattr(bad, field, value)
            _refused(L, call(bad, None, 1), -1)
            assert L.hipdec_tensor_bytes(C.byref(bad), 1) == 0
        _refused(L, call(good, None, 1, 3 * 40 * 30 * 2 - 1), -1)                         # short out_bytes
        _refused(L, call(good, [(0, 0, 0, 0, 0, 0)] * 2, 2, 3 * 40 * 30 * 2 * 2 - 1), -1)
        for sc, bi in ((float("nan"), 0.0), (1.0, float("nan")), (float("inf"), 0.0), (1.0, float("-inf"))):
            for dtype in ("float16", "bfloat16", "float32"):
                _refused(L, call(_desc(dtype=dtype, scale=(1.0, sc, 1.0), bias=(bi, 0.0, 0.0)), None, 1), -1)
        assert call(_desc(dtype="uint8", scale=float("nan"), bias=float("nan")), None, 1) == 0      # uint8 ignores scale and bias
        _refused(L, call(good, None, 2), -1)                                              # NULL entries: n_entries must be the item count
        _refused(L, call(good, None, 0), -1)
        _refused(L, call(good, [(0, 0, 0, 0, 0, 0)], -1), -1)
        _refused(L, L.hipdec_batch_to_tensor(None, C.byref(good), None, 1, out.ptr, out.nbytes, None), -1)
        _refused(L, L.hipdec_batch_to_tensor(b._h, None, None, 1, out.ptr, out.nbytes, None), -1)
        _refused(L, L.hipdec_batch_to_tensor(b._h, C.byref(good), None, 1, None, out.nbytes, None), -1)
        assert call(good, None, 1) == 0                                                   # a good call still works afterwards
        b.status()
    finally:
        b.free()
    # the image form
    y = np.zeros((20, 30), np.uint8)
    host = np.zeros(3 * 8 * 8 * 4, np.uint8)
    img = ColorImage()
    img.width, img.height, img.chroma, img.bit_depth = 30, 20, 0, 8
    img.plane[0], img.stride[0] = y.ctypes.data, 30
    d8 = _desc(size=(8, 8))
    icall = lambda im, desc, entries, n, nbytes=host.nbytes: L.hipdec_image_to_tensor(C.byref(im) if im is not None else None, None, C.byref(desc),
                                                                                      decoder.tensor_entries(entries) if entries else None, n, host.ctypes.data, nbytes, 0)
    assert icall(img, d8, None, 1) == 0
    _refused(L, icall(None, d8, None, 1), -1)
    _refused(L, icall(img, d8, None, 2), -1)
    _refused(L, icall(img, d8, [(0, 25, 0, 6, 5, 0)], 1), -1)
    _refused(L, icall(img, d8, None, 1, 3 * 8 * 8 * 2 - 1), -1)
    _refused(L, icall(img, _desc(size=(8, 8), scale=float("nan")), None, 1), -1)
    img.stride[0] = 29
    _refused(L, icall(img, d8, None, 1), -1)
    img.stride[0], img.bit_depth = 30, 10                                                 # wider monochrome goes nowhere, as in hipdec_batch_to_rgb
    y16 = np.zeros((20, 30), np.uint16)
    img.plane[0], img.stride[0] = y16.ctypes.data, 60
    _refused(L, icall(img, d8, None, 1), -4)


def test_tensor_output_is_held_against_the_limit_given_at_creation():
    L = _lib()
    b = _batch([_still(1, 8, VUI_FULL, (200, 136))], max_image_size_pixels=200 * 136)
    try:
        out = DeviceBuffer(3 * 400 * 300)
        big, fits = _desc(size=(400, 300), dtype="uint8"), _desc(size=(200, 136), dtype="uint8")
        _refused(L, L.hipdec_batch_to_tensor(b._h, C.byref(big), None, 1, out.ptr, out.nbytes, None), -5)
        assert L.hipdec_batch_to_tensor(b._h, C.byref(fits), None, 1, out.ptr, out.nbytes, None) == 0     # at the limit
        b.status()
    finally:
        b.free()


def test_life_cycle_timing_slot_and_counters():
    L = _lib()
    s = _still(1, 8, VUI_FULL, (200, 136))
    a = _batch([s])
    n0 = decoder.tensor_stats()
    first = run_tensor(a, (48, 32), [(0, 3, 5, 100, 80, 0), (0, 0, 0, 0, 0, 1)], "float16", "NCHW", SCALE_BOX)
    again = run_tensor(a, (48, 32), [(0, 3, 5, 100, 80, 0), (0, 0, 0, 0, 0, 1)], "float16", "NCHW", SCALE_BOX)      # twice in a row: the blocks are not uploaded again
    assert np.array_equal(first, again)
    other = run_tensor(a, (48, 32), [(0, 4, 5, 100, 80, 0)], "float16", "NCHW", SCALE_BOX)
    assert not np.array_equal(other[0], first[0])
    assert a.slot_kernel_timing_us(0)["colour"] > 0.0
    n1 = decoder.tensor_stats()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (3, 5)
    color.image_to_tensor([np.zeros((20, 30), np.uint8)], 8, 0, None, (8, 8), [(0, 0, 10, 10), (1, 1, 5, 5), (0, 0, 0, 0)])
    n2 = decoder.tensor_stats()
    assert (n2[0] - n1[0], n2[1] - n1[1]) == (1, 3)
    b = decoder.Batch([s], recycle=a)
    try:
        out = DeviceBuffer(3 * 48 * 32 * 2)
        d = _desc(size=(48, 32))
        _refused(L, L.hipdec_batch_to_tensor(a._h, C.byref(d), None, 1, out.ptr, out.nbytes, None), -1)     # a recycled batch
        assert decoder.tensor_stats() == n2                                                                 # (refusals do not count)
        b.run(); b.status()
        got = run_tensor(b, (48, 32), [(0, 3, 5, 100, 80, 0), (0, 0, 0, 0, 0, 1)], "float16", "NCHW", SCALE_BOX)
        assert np.array_equal(got, first)
    finally:
        b.free()
        a.free()


def test_free_right_behind_to_tensor_waits_for_it():
    """as tests/test_scale_gpu.py states it for the scaled calls: the work is marked on the batch, hipdec_batch_free waits for it"""
    streams = [_still(1, 8, VUI_FULL, (200, 136), seed=40 + k) for k in range(4)]
    for filt in (SCALE_NEAREST, SCALE_BOX):
        b = decoder.Batch(streams)
        b.run()
        out = DeviceBuffer(4 * 3 * 64 * 44 * 2)
        b.to_tensor((64, 44), None, dtype="float16", filter=filt, out=out)
        b.free()
        want = _batch(streams)
        assert np.array_equal(out.to_numpy((4, 3, 44, 64), np.uint16), run_tensor(want, (64, 44), None, "float16", "NCHW", filt, np.ones(3, np.float32), np.zeros(3, np.float32)))
        want.free()
