"""Scaled output on the device: hipdec_image_scale, hipdec_batch_to_rgb_scaled(_all), hipdec_batch_read_plane_scaled.

HIPDEC_SCALE_NEAREST is pinned to the compiled reference: heif_image objects are built in oracle/_ref/libheif.so, heif_image_scale_image()
(HeifPixelImage::scale_nearest_neighbor, libheif/image/pixelimage.cc:1783-1972) scales them, and every plane / every interleaved row has to come
out of the device byte for byte.  HIPDEC_SCALE_BOX is not in the reference: its definition (include/heif_hipdec.h) is restated below in plain
integer arithmetic over int64 (`box_plane`), independent of the code under test; the fused box RGB has to equal hipdec_color_convert of those
expected planes presented as a 4:4:4 image.  Everything is bit-exact, there are no tolerances.

The module runs on the MI355X (`-m gpu`) and, through tests/test_scale_emu.py, against the library compiled for the host.  The full-shape case
(3840 x 2160) runs in both; HIPDEC_SCALE_SKIP_FULL_SHAPE=1 is the switch test_scale_emu.py would use if the emulator ever needed more than about a
minute for it (it needs seconds: it does not set it)."""
import ctypes as C
import os
import numpy as np
import pytest

import libheif_amd
from libheif_amd import color, decoder
from libheif_amd._capi import DeviceBuffer, HipDecError, Nclx, check
from libheif_amd.color import ColorImage, SCALE_BOX, SCALE_NEAREST, subsampled_size
from oracle import pyoracle as orc
import libheif_host as lh

pytestmark = pytest.mark.gpu

needs_reference = pytest.mark.skipif(not lh.available(), reason="oracle/_ref/libheif.so is not built (build() compiles it where the reference sources are): "
                                                                "no reference to pin the nearest-neighbour filter to")

CHANNEL_ALPHA = 6
CHROMA_INTERLEAVED = {10: (3, 8), 11: (4, 8), 12: (3, 10), 14: (3, 10)}   # heif_chroma -> components per pixel, bit depth of the plane

# (source size), then the sizes it is scaled to: down (odd and even), 1 x 1, identity, up
SHAPES = [((381, 251), [(100, 66), (77, 51), (1, 1), (381, 251), (500, 400)]),
          ((128, 96), [(100, 66), (33, 17), (1, 1), (128, 96), (500, 400)])]


def _lib():
    L = libheif_amd.load_library()
    decoder._bind(L)
    vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
    L.hipdec_image_scale.argtypes = [C.POINTER(ColorImage), ci, ci, ci, C.POINTER(ColorImage)]
    L.hipdec_color_convert.argtypes = [C.POINTER(ColorImage), C.POINTER(Nclx), ci, ci, ci, vp, sz, ci]
    L.hipdec_plane_scale.argtypes = [vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, sz, vp]
    assert L.hipdec_init(0) == 0, L.hipdec_last_error()
    return L


def _ref():
    L = lh.lib()
    vp, ci = C.c_void_p, C.c_int
    L.heif_image_create.restype = lh.HeifError
    L.heif_image_create.argtypes = [ci, ci, ci, ci, C.POINTER(vp)]
    L.heif_image_add_plane.restype = lh.HeifError
    L.heif_image_add_plane.argtypes = [vp, ci, ci, ci, ci]
    L.heif_image_get_plane2.restype = C.POINTER(C.c_uint8)
    L.heif_image_get_plane2.argtypes = [vp, ci, C.POINTER(C.c_size_t)]
    L.heif_image_scale_image.restype = lh.HeifError
    L.heif_image_scale_image.argtypes = [vp, C.POINTER(vp), ci, ci, vp]
    return L


def _ref_fill(L, img, channel, rows):
    """rows: (h, row bytes) uint8"""
    stride = C.c_size_t()
    p = L.heif_image_get_plane2(img, channel, C.byref(stride))
    assert p
    dst = np.ctypeslib.as_array(p, shape=(rows.shape[0] * stride.value,)).reshape(rows.shape[0], stride.value)
    dst[:, :rows.shape[1]] = rows


def _ref_read(L, img, channel, h, row_bytes):
    stride = C.c_size_t()
    p = L.heif_image_get_plane_readonly2(img, channel, C.byref(stride))
    assert p
    return np.ctypeslib.as_array(p, shape=(h * stride.value,)).reshape(h, stride.value)[:, :row_bytes].copy()


def ref_scale_planes(planes, alpha, chroma, bits, ow, oh):
    """heif_image_scale_image() on a planar image; returns the scaled planes in the order given (alpha last)"""
    L = _ref()
    h, w = planes[0].shape
    es = 2 if bits > 8 else 1
    img = C.c_void_p()
    lh.check(L.heif_image_create(w, h, lh.COLORSPACE_MONO if chroma == 0 else lh.COLORSPACE_YCBCR, chroma, C.byref(img)))
    chans = [lh.CHANNEL_Y, lh.CHANNEL_CB, lh.CHANNEL_CR][:len(planes)] + ([CHANNEL_ALPHA] if alpha is not None else [])
    src = list(planes) + ([alpha] if alpha is not None else [])
    out = C.c_void_p()
    try:
        for ch, p in zip(chans, src):
            lh.check(L.heif_image_add_plane(img, ch, p.shape[1], p.shape[0], bits))
            _ref_fill(L, img, ch, np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1))
        lh.check(L.heif_image_scale_image(img, C.byref(out), ow, oh, None))
        res = []
        for ch in chans:
            pw, ph = L.heif_image_get_width(out, ch), L.heif_image_get_height(out, ch)
            rows = _ref_read(L, out, ch, ph, pw * es)
            res.append(rows.view(np.uint16) if es == 2 else rows)
        return res
    finally:
        if out:
            L.heif_image_release(out)
        L.heif_image_release(img)


def ref_scale_interleaved(rows, w, h, out_chroma, ow, oh):
    """the reference's scaling of an interleaved image (pixelimage.cc:1858-1913)"""
    L = _ref()
    comps, bits = CHROMA_INTERLEAVED[out_chroma]
    bpp = comps * (2 if bits > 8 else 1)
    img, out = C.c_void_p(), C.c_void_p()
    lh.check(L.heif_image_create(w, h, lh.COLORSPACE_RGB, out_chroma, C.byref(img)))
    try:
        lh.check(L.heif_image_add_plane(img, lh.CHANNEL_INTERLEAVED, w, h, bits))
        _ref_fill(L, img, lh.CHANNEL_INTERLEAVED, rows[:, :w * bpp])
        lh.check(L.heif_image_scale_image(img, C.byref(out), ow, oh, None))
        assert L.heif_image_get_width(out, lh.CHANNEL_INTERLEAVED) == ow and L.heif_image_get_height(out, lh.CHANNEL_INTERLEAVED) == oh
        return _ref_read(L, out, lh.CHANNEL_INTERLEAVED, oh, ow * bpp)
    finally:
        if out:
            L.heif_image_release(out)
        L.heif_image_release(img)


def box_plane(p, qw, qh):
    """HIPDEC_SCALE_BOX as include/heif_hipdec.h defines it, in integer arithmetic over int64 (an integral image gives the sums)"""
    ph, pw = p.shape
    integral = np.zeros((ph + 1, pw + 1), np.int64)
    integral[1:, 1:] = np.cumsum(np.cumsum(p.astype(np.int64), axis=0), axis=1)
    x0 = np.array([ox * pw // qw for ox in range(qw)], np.int64)
    x1 = np.array([(ox + 1) * pw // qw for ox in range(qw)], np.int64)
    x1 = np.where(x1 <= x0, x0 + 1, x1)
    y0 = np.array([oy * ph // qh for oy in range(qh)], np.int64)
    y1 = np.array([(oy + 1) * ph // qh for oy in range(qh)], np.int64)
    y1 = np.where(y1 <= y0, y0 + 1, y1)
    s = integral[y1[:, None], x1[None, :]] - integral[y0[:, None], x1[None, :]] - integral[y1[:, None], x0[None, :]] + integral[y0[:, None], x0[None, :]]
    n = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    return ((s + n // 2) // n).astype(p.dtype)


def box_planes(planes, alpha, chroma, ow, oh):
    """every plane with ITS OWN sizes; chroma planes to the subsampled size of the output image"""
    cw, ch = subsampled_size(ow, oh, chroma)
    res = [box_plane(planes[0], ow, oh)] + [box_plane(p, cw, ch) for p in planes[1:]]
    return res + ([box_plane(alpha, ow, oh)] if alpha is not None else [])


def _random_image(w, h, chroma, bits, alpha, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bits > 8 else np.uint8
    cw, ch = subsampled_size(w, h, chroma)
    planes = [rng.integers(0, 1 << bits, (h, w)).astype(dt)]
    if chroma:
        planes += [rng.integers(0, 1 << bits, (ch, cw)).astype(dt) for _ in range(2)]
    return planes, (rng.integers(0, 1 << bits, (h, w)).astype(dt) if alpha else None)


def image_scale_device(L, planes, alpha, chroma, bits, ow, oh, filt):
    """hipdec_image_scale with on_device = 1 on both sides; odd strides on the input so that the unaligned row loads run too"""
    dt = planes[0].dtype
    es = dt.itemsize
    h, w = planes[0].shape
    cw, ch = subsampled_size(ow, oh, chroma)
    src = list(planes) + ([alpha] if alpha is not None else [])
    slots = list(range(len(planes))) + ([3] if alpha is not None else [])
    inp, out = ColorImage(), ColorImage()
    inp.width, inp.height, inp.chroma, inp.bit_depth, inp.on_device = w, h, chroma, bits, 1
    out.on_device = 1
    keep, outs = [], []
    for a, c in zip(src, slots):
        pad = np.zeros((a.shape[0], a.shape[1] + 3), dt)     # stride = (width + 3) samples
        pad[:, :a.shape[1]] = a
        b = DeviceBuffer.from_numpy(pad)
        qw, qh = (cw, ch) if c in (1, 2) else (ow, oh)
        o = DeviceBuffer(qw * qh * es)
        keep += [b, o]
        inp.plane[c], inp.stride[c] = b.ptr, pad.shape[1] * es
        out.plane[c], out.stride[c] = o.ptr, qw * es
        outs.append((o, qw, qh))
    check(L.hipdec_image_scale(C.byref(inp), ow, oh, filt, C.byref(out)))
    assert (out.width, out.height, out.chroma, out.bit_depth) == (ow, oh, chroma, bits)
    return [o.to_numpy((qh, qw), dt) for o, qw, qh in outs]


FORMATS = [(chroma, bits, alpha) for chroma in (0, 1, 2, 3) for bits in (8, 10) for alpha in (False, True)]


@needs_reference
@pytest.mark.parametrize("chroma,bits,alpha", FORMATS)
def test_image_scale_nearest_is_the_reference_plane_by_plane(chroma, bits, alpha):
    L = _lib()
    for k, ((w, h), targets) in enumerate(SHAPES):
        planes, a = _random_image(w, h, chroma, bits, alpha, seed=100 * chroma + bits + k)
        for ow, oh in targets:
            want = ref_scale_planes(planes, a, chroma, bits, ow, oh)
            got_host = color.image_scale(planes, bits, chroma, ow, oh, SCALE_NEAREST, alpha=a)
            got_dev = image_scale_device(L, planes, a, chroma, bits, ow, oh, SCALE_NEAREST)
            assert len(want) == len(got_host) == len(got_dev)
            for c, (x, y, z) in enumerate(zip(want, got_host, got_dev)):
                assert x.shape == y.shape == z.shape, (c, x.shape, y.shape, z.shape)
                assert np.array_equal(x, y), ("host planes", (w, h), (ow, oh), c)
                assert np.array_equal(x, z), ("device planes", (w, h), (ow, oh), c)


@pytest.mark.parametrize("chroma,bits,alpha", FORMATS)
def test_image_scale_box_is_the_definition_plane_by_plane(chroma, bits, alpha):
    L = _lib()
    for k, ((w, h), targets) in enumerate(SHAPES):
        planes, a = _random_image(w, h, chroma, bits, alpha, seed=200 * chroma + bits + k)
        for ow, oh in targets:
            want = box_planes(planes, a, chroma, ow, oh)
            got_host = color.image_scale(planes, bits, chroma, ow, oh, SCALE_BOX, alpha=a)
            got_dev = image_scale_device(L, planes, a, chroma, bits, ow, oh, SCALE_BOX)
            for c, (x, y, z) in enumerate(zip(want, got_host, got_dev)):
                assert x.shape == y.shape == z.shape, (c, x.shape, y.shape, z.shape)
                assert np.array_equal(x, y), ("host planes", (w, h), (ow, oh), c)
                assert np.array_equal(x, z), ("device planes", (w, h), (ow, oh), c)


def test_box_identity_is_a_copy_and_a_constant_plane_stays_constant():
    planes, _ = _random_image(97, 55, 1, 8, False, seed=5)
    got = color.image_scale(planes, 8, 1, 97, 55, SCALE_BOX)
    for x, y in zip(planes, got):
        assert np.array_equal(x, y)
    flat = [np.full((55, 97), 201, np.uint8), np.full((28, 49), 17, np.uint8), np.full((28, 49), 250, np.uint8)]
    for ow, oh in ((13, 7), (1, 1), (200, 111)):
        got = color.image_scale(flat, 8, 1, ow, oh, SCALE_BOX)
        assert [int(g.min()) for g in got] == [201, 17, 250] and [int(g.max()) for g in got] == [201, 17, 250]


VUI_FULL = dict(vui_primaries=1, vui_transfer=13, vui_matrix=6, vui_full_range=1)
VUI_LIMITED = dict(vui_primaries=1, vui_transfer=13, vui_matrix=1, vui_full_range=0)
# (chroma format, bit depth, VUI, picture size): full range takes the integer op for 4:2:0, limited range the float chain.  The generator codes odd
# picture sizes for 4:0:0 and 4:4:4 only; the subsampled formats get sizes that are no multiple of the coding block instead (142 x 94)
STILLS = [(1, 8, VUI_FULL, (200, 136)), (1, 8, VUI_LIMITED, (142, 94)), (2, 8, VUI_FULL, (142, 94)), (3, 8, VUI_LIMITED, (141, 93)), (0, 8, {}, (141, 93)),
          (1, 10, VUI_FULL, (142, 94)), (1, 10, VUI_LIMITED, (200, 136)), (2, 10, VUI_LIMITED, (200, 136)), (3, 10, VUI_FULL, (141, 93))]
RGB_TARGETS = [(100, 66), (37, 23), (1, 1), None, (300, 200)]    # None: identity


def _out_chromas(cf, bits):
    if cf == 0:
        return (10, 11)
    return (10, 11) if bits == 8 else (10, 11, 12, 14)


_STREAMS = {}


def _still(cf, bits, vui, size, seed=11):
    key = (cf, bits, tuple(sorted(vui.items())), size, seed)
    if key not in _STREAMS:
        _STREAMS[key] = orc.encode(orc.synth_image(size[0], size[1], bits, cf, seed=seed), bit_depth=bits, **vui)
    return _STREAMS[key]


def _batch(streams, **kw):
    b = decoder.Batch(streams, **kw)
    b.run()
    b.status()
    return b


@needs_reference
@pytest.mark.parametrize("cf,bits,vui,size", STILLS)
def test_to_rgb_scaled_nearest_is_to_rgb_followed_by_the_reference_scaling(cf, bits, vui, size):
    b = _batch([_still(cf, bits, vui, size)])
    w, h = size
    try:
        for oc in _out_chromas(cf, bits):
            full = b.to_rgb(0, oc)
            for t in RGB_TARGETS:
                ow, oh = t or size
                want = ref_scale_interleaved(full, w, h, oc, ow, oh)
                got = b.to_rgb_scaled(0, ow, oh, SCALE_NEAREST, oc)
                assert got.shape == want.shape
                assert np.array_equal(got, want), (oc, (ow, oh), int((got != want).sum()))
    finally:
        b.free()


def _color_convert_444(L, planes, cf, bits, nclx, out_chroma):
    """hipdec_color_convert of planes presented as a 4:4:4 image (monochrome: as it is)"""
    h, w = planes[0].shape
    img = ColorImage()
    img.width, img.height, img.chroma, img.bit_depth, img.on_device = w, h, (3 if cf else 0), bits, 0
    keep = [np.ascontiguousarray(p) for p in planes]
    for c, p in enumerate(keep):
        img.plane[c], img.stride[c] = p.ctypes.data, p.strides[0]
    bpp = {10: 3, 11: 4, 12: 6, 14: 6}[out_chroma]
    out = np.empty((h, w * bpp), np.uint8)
    n = Nclx(1, *nclx)
    check(L.hipdec_color_convert(C.byref(img), C.byref(n), out_chroma, 1, 0, out.ctypes.data, w * bpp, 0))
    return out


@pytest.mark.parametrize("cf,bits,vui,size", STILLS)
def test_to_rgb_scaled_box_is_color_convert_of_the_box_scaled_planes(cf, bits, vui, size):
    L = _lib()
    b = _batch([_still(cf, bits, vui, size)])
    try:
        planes = b.planes(0)
        d = b.info(0)
        nclx = (d["colour_primaries"], d["transfer_characteristics"], d["matrix_coeffs"], d["full_range_flag"])
        for t in RGB_TARGETS:
            ow, oh = t or size
            scaled = [box_plane(p, ow, oh) for p in planes]          # each plane with its own size, all to ow x oh
            for oc in _out_chromas(cf, bits):
                want = _color_convert_444(L, scaled, cf, bits, nclx, oc)
                got = b.to_rgb_scaled(0, ow, oh, SCALE_BOX, oc)
                assert np.array_equal(got, want), (oc, (ow, oh), int((got != want).sum()))
    finally:
        b.free()


@pytest.mark.parametrize("cf,bits,vui,size", [STILLS[0], STILLS[2], STILLS[4], STILLS[6]])
def test_planes_scaled_of_a_batch_item_are_image_scale_of_its_planes(cf, bits, vui, size):
    b = _batch([_still(cf, bits, vui, size)])
    try:
        planes = b.planes(0)
        for filt in (SCALE_NEAREST, SCALE_BOX):
            for ow, oh in ((100, 66), (37, 23), (1, 1), (300, 200)):
                want = color.image_scale(planes, bits, cf, ow, oh, filt)
                got = b.planes_scaled(0, ow, oh, filt)
                for x, y in zip(want, got):
                    assert x.shape == y.shape and np.array_equal(x, y), (filt, (ow, oh))
    finally:
        b.free()


@pytest.mark.parametrize("filt", [SCALE_NEAREST, SCALE_BOX])
def test_to_rgb_scaled_all_with_mixed_sizes_is_the_per_item_calls(filt):
    sizes_in = [(200, 136), (142, 94), (64, 64), (136, 200), (96, 80), (142, 94), (200, 136), (72, 56), (64, 64), (120, 40)]
    streams = [_still(1, 8, VUI_FULL if k % 2 else VUI_LIMITED, s, seed=30 + k) for k, s in enumerate(sizes_in)]
    b = _batch(streams)
    try:
        sizes_out = [decoder.fit_within(w, h, 48 + 7 * k) if k % 3 else (w + 9, h + 5) for k, (w, h) in enumerate(sizes_in)]
        for oc in (10, 11):
            b.alloc_rgb_scaled(sizes_out, oc)
            b.to_rgb_scaled_all(filt)
            b.status()
            for k, (ow, oh) in enumerate(sizes_out):
                want = b.to_rgb_scaled(k, ow, oh, filt, oc)
                assert np.array_equal(b.rgb_scaled(k), want), (oc, k)
        t = b.slot_kernel_timing_us(0)
        assert t["colour"] >= 0.0
    finally:
        b.free()


def test_fit_within_is_the_thumbnailer_rule():
    assert decoder.fit_within(3840, 2160, 512) == (512, 288)
    assert decoder.fit_within(2160, 3840, 512) == (288, 512)
    assert decoder.fit_within(300, 200, 512) == (300, 200)
    assert decoder.fit_within(1000, 1000, 256) == (256, 256)
    assert decoder.fit_within(4000, 3, 256) == (256, 0)         # the thumbnailer refuses a zero size; so do the entry points


full_shape = pytest.mark.skipif(os.environ.get("HIPDEC_SCALE_SKIP_FULL_SHAPE") == "1", reason="HIPDEC_SCALE_SKIP_FULL_SHAPE=1")


@full_shape
def test_full_shape_box():
    """the plane scaler at full shape: 3840 x 2160 8-bit 4:2:0 to 480 x 270 and to 1 x 1 through hipdec_image_scale, and a 16-bit plane of all 0xFFFF
    to 1 x 1: the sum is 3840 * 2160 * 65535 = 5.4e11, which a 32-bit accumulator does not hold.  (The fused kernels at this shape: the next test.)"""
    L = _lib()
    w, h = 3840, 2160
    planes = [p.astype(np.uint8) for p in orc.synth_image(w, h, 8, 1, seed=77)]
    for ow, oh in ((480, 270), (1, 1)):
        want = box_planes(planes, None, 1, ow, oh)
        got = color.image_scale(planes, 8, 1, ow, oh, SCALE_BOX)
        for x, y in zip(want, got):
            assert np.array_equal(x, y), (ow, oh)
    ones = np.full((h, w), 0xFFFF, np.uint16)
    got = color.image_scale([ones], 16, 0, 1, 1, SCALE_BOX)
    assert got[0].shape == (1, 1) and int(got[0][0, 0]) == 0xFFFF
    got = color.image_scale([ones], 16, 0, 3, 2, SCALE_BOX)
    assert (got[0] == 0xFFFF).all()


@full_shape
@needs_reference
def test_full_shape_fused_rgb():
    """the fused scale + colour kernels on a decoded 3840 x 2160 8-bit 4:2:0 still - the shape whose time DESIGN.md quotes: a tile below 256 output
    pixels whose start is not 4-column aligned in the source (480 x 270), boxes wider than the 1024-column span over three planes (1 x 1, 3 x 2),
    up-scaling past the span (4000 x 2200).  BOX against hipdec_color_convert of the box-scaled planes presented as 4:4:4, NEAREST against the
    reference's scaling of the full-size to_rgb."""
    L = _lib()
    w, h = 3840, 2160
    b = _batch([_still(1, 8, VUI_LIMITED, (w, h), seed=77)])
    try:
        planes = b.planes(0)
        d = b.info(0)
        assert (d["width"], d["height"]) == (w, h)
        nclx = (d["colour_primaries"], d["transfer_characteristics"], d["matrix_coeffs"], d["full_range_flag"])
        full = {oc: b.to_rgb(0, oc) for oc in (10, 11)}
        for ow, oh in ((480, 270), (1, 1), (3, 2), (4000, 2200)):
            scaled = [box_plane(p, ow, oh) for p in planes]
            for oc in (10, 11):
                want = _color_convert_444(L, scaled, 1, 8, nclx, oc)
                got = b.to_rgb_scaled(0, ow, oh, SCALE_BOX, oc)
                assert np.array_equal(got, want), ("box", oc, (ow, oh), int((got != want).sum()))
                want = ref_scale_interleaved(full[oc], w, h, oc, ow, oh)
                got = b.to_rgb_scaled(0, ow, oh, SCALE_NEAREST, oc)
                assert np.array_equal(got, want), ("nearest", oc, (ow, oh), int((got != want).sum()))
    finally:
        b.free()


def _nearest_plane(p, qw, qh):
    """pixelimage.cc:1936-1943 for a lone plane (the image's sizes are the plane's)"""
    ph, pw = p.shape
    return p[(np.arange(qh, dtype=np.int64) * ph // qh)[:, None], (np.arange(qw, dtype=np.int64) * pw // qw)[None, :]]


@pytest.mark.parametrize("bits", [8, 12])
def test_plane_scale_on_device_planes(bits):
    """hipdec_plane_scale, the plane kernel behind a C call of its own: device pointers in and out, both filters; the call has finished when it returns"""
    L = _lib()
    dt = np.uint16 if bits > 8 else np.uint8
    es = np.dtype(dt).itemsize
    rng = np.random.default_rng(bits)
    src = rng.integers(0, 1 << bits, (173, 259)).astype(dt)
    pad = np.zeros((173, 264), dt)
    pad[:, :259] = src
    d_in = DeviceBuffer.from_numpy(pad)
    for qw, qh in ((64, 40), (1, 1), (259, 173), (300, 200)):
        d_out = DeviceBuffer(qw * qh * es)
        for filt, want in ((SCALE_NEAREST, _nearest_plane(src, qw, qh)), (SCALE_BOX, box_plane(src, qw, qh))):
            check(L.hipdec_plane_scale(d_in.ptr, 264 * es, 259, 173, es, 259, 173, qw, qh, qw, qh, filt, d_out.ptr, qw * es, None))
            assert np.array_equal(d_out.to_numpy((qh, qw), dt), want), (filt, (qw, qh))
    # a chroma plane of a 4:2:0 image: the nearest-neighbour index uses the IMAGE's sizes (517 x 345 -> 100 x 66), the plane is 259 x 173 -> 50 x 33
    d_out = DeviceBuffer(50 * 33 * es)
    check(L.hipdec_plane_scale(d_in.ptr, 264 * es, 259, 173, es, 517, 345, 100, 66, 50, 33, SCALE_NEAREST, d_out.ptr, 50 * es, None))
    want = src[(np.arange(33) * 345 // 66)[:, None], (np.arange(50) * 517 // 100)[None, :]]
    assert np.array_equal(d_out.to_numpy((33, 50), dt), want)


def test_image_scale_has_its_own_counter():
    L = _lib()
    L.hipdec_image_scale_stats.restype = None
    L.hipdec_image_scale_stats.argtypes = [C.POINTER(C.c_uint64)]
    L.hipdec_image_ops_stats.restype = None
    L.hipdec_image_ops_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    n0, x0, g0 = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L.hipdec_image_scale_stats(C.byref(n0)); L.hipdec_image_ops_stats(C.byref(x0), C.byref(g0))
    planes, _ = _random_image(40, 30, 1, 8, False, seed=1)
    color.image_scale(planes, 8, 1, 10, 8, SCALE_BOX)
    color.image_scale(planes, 8, 1, 10, 8, SCALE_NEAREST)
    n1, x1, g1 = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L.hipdec_image_scale_stats(C.byref(n1)); L.hipdec_image_ops_stats(C.byref(x1), C.byref(g1))
    assert n1.value == n0.value + 2 and x1.value == x0.value      # (hipdec_image_transform's counter keeps its meaning)


def test_example_host_makes_previews_with_thumb(tmp_path):
    """examples/decode_batch.c --thumb N end to end: its previews are Batch.to_rgb_scaled(BOX) at the thumbnailer's sizes; a bad N prints the usage"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.abspath(libheif_amd.library_path())
    exe = str(tmp_path / "decode_batch")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    r = subprocess.run([exe, "--thumb", "0", "x.hevc"], capture_output=True, text=True)
    assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    r = subprocess.run([exe, "--thumb"], capture_output=True, text=True)
    assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    items = [((200, 136), VUI_FULL), ((136, 200), VUI_LIMITED), ((64, 64), VUI_FULL)]
    files = []
    for k, (size, vui) in enumerate(items):
        f = tmp_path / ("item%d.hevc" % k)
        f.write_bytes(_still(1, 8, vui, size, seed=60 + k))
        files.append(str(f))
    r = subprocess.run([exe, "--thumb", "96"] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    b = _batch([_still(1, 8, vui, size, seed=60 + k) for k, (size, vui) in enumerate(items)])
    try:
        for k, (size, _) in enumerate(items):
            ow, oh = decoder.fit_within(size[0], size[1], 96)
            want = int(b.to_rgb_scaled(k, ow, oh, SCALE_BOX).astype(np.uint64).sum())
            assert "%s: preview %dx%d RGB24, byte sum %d\n" % (files[k], ow, oh, want) in r.stdout, r.stdout
    finally:
        b.free()


# ---- refusals and life cycle ----------------------------------------------------------------------------------------------------------------

def _refused(L, rc, code):
    assert rc == code, (rc, L.hipdec_last_error())
    assert L.hipdec_last_error(), "hipdec_last_error() is empty after a refusal"


def test_scaled_calls_refuse_bad_arguments_with_a_message():
    L = _lib()
    b = _batch([_still(1, 8, VUI_FULL, (200, 136))])
    try:
        out = DeviceBuffer(300 * 200 * 6)
        host = np.empty((400, 400), np.uint8)
        for ow, oh in ((0, 10), (10, 0), (-3, 5)):
            _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, ow, oh, SCALE_BOX, out.ptr, 4096, None), -1)
            _refused(L, L.hipdec_batch_read_plane_scaled(b._h, 0, 0, ow, oh, SCALE_BOX, host.ctypes.data, 400), -1)
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 50, 40, 2, out.ptr, 4096, None), -1)          # unknown filter
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 50, 40, -1, out.ptr, 4096, None), -1)
        _refused(L, L.hipdec_batch_read_plane_scaled(b._h, 0, 0, 50, 40, 7, host.ctypes.data, 400), -1)
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 50, 40, SCALE_BOX, out.ptr, 50 * 3 - 1, None), -1)   # stride below a row
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 11, 50, 40, SCALE_NEAREST, out.ptr, 50 * 4 - 1, None), -1)
        _refused(L, L.hipdec_batch_read_plane_scaled(b._h, 0, 1, 50, 40, SCALE_BOX, host.ctypes.data, 24), -1)      # a chroma row is 25 bytes
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 12, 50, 40, SCALE_BOX, out.ptr, 4096, None), -4)          # RRGGBB needs > 8-bit planes, as to_rgb
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 1, 10, 50, 40, SCALE_BOX, out.ptr, 4096, None), -1)          # no such item
        ws, hs = (C.c_int * 1)(50), (C.c_int * 1)(0)
        ptrs, strides = (C.c_void_p * 1)(out.ptr), (C.c_size_t * 1)(4096)
        _refused(L, L.hipdec_batch_to_rgb_scaled_all(b._h, 10, ws, hs, SCALE_BOX, ptrs, strides, None), -1)
        _refused(L, L.hipdec_batch_to_rgb_scaled_all(b._h, 10, None, hs, SCALE_BOX, ptrs, strides, None), -1)
        # a good call still works afterwards
        assert b.to_rgb_scaled(0, 50, 40, SCALE_BOX).shape == (40, 150)
    finally:
        b.free()
    # hipdec_image_scale
    y = np.zeros((20, 30), np.uint8)
    o = np.zeros((20, 30), np.uint8)
    inp, out_img = ColorImage(), ColorImage()
    inp.width, inp.height, inp.chroma, inp.bit_depth = 30, 20, 0, 8
    inp.plane[0], inp.stride[0] = y.ctypes.data, 30
    out_img.plane[0], out_img.stride[0] = o.ctypes.data, 30
    _refused(L, L.hipdec_image_scale(C.byref(inp), 0, 5, SCALE_BOX, C.byref(out_img)), -1)
    _refused(L, L.hipdec_image_scale(C.byref(inp), 5, 5, 3, C.byref(out_img)), -1)
    out_img.stride[0] = 9
    _refused(L, L.hipdec_image_scale(C.byref(inp), 10, 5, SCALE_BOX, C.byref(out_img)), -1)
    out_img.stride[0] = 30
    out_img.plane[0] = None
    _refused(L, L.hipdec_image_scale(C.byref(inp), 10, 5, SCALE_BOX, C.byref(out_img)), -1)
    _refused(L, L.hipdec_image_scale(None, 10, 5, SCALE_BOX, C.byref(out_img)), -1)
    _refused(L, L.hipdec_plane_scale(None, 30, 30, 20, 1, 30, 20, 10, 5, 10, 5, SCALE_BOX, None, 10, None), -1)


def test_scaled_output_is_held_against_the_limit_given_at_creation():
    L = _lib()
    b = _batch([_still(1, 8, VUI_FULL, (200, 136))], max_image_size_pixels=200 * 136)
    try:
        out = DeviceBuffer(400 * 300 * 3)
        host = np.empty((300, 400), np.uint8)
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 400, 300, SCALE_NEAREST, out.ptr, 1200, None), -5)
        _refused(L, L.hipdec_batch_read_plane_scaled(b._h, 0, 0, 400, 300, SCALE_NEAREST, host.ctypes.data, 400), -5)
        assert L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 200, 136, SCALE_NEAREST, out.ptr, 600, None) == 0     # at the limit
        b.status()
    finally:
        b.free()


def test_a_retired_batch_refuses_scaled_calls():
    L = _lib()
    s = _still(1, 8, VUI_FULL, (200, 136))
    a = _batch([s])
    b = decoder.Batch([s], recycle=a)
    try:
        out = DeviceBuffer(50 * 40 * 3)
        host = np.empty((40, 50), np.uint8)
        _refused(L, L.hipdec_batch_to_rgb_scaled(a._h, 0, 10, 50, 40, SCALE_BOX, out.ptr, 150, None), -1)
        _refused(L, L.hipdec_batch_read_plane_scaled(a._h, 0, 0, 50, 40, SCALE_BOX, host.ctypes.data, 50), -1)
        ws, hs = (C.c_int * 1)(50), (C.c_int * 1)(40)
        ptrs, strides = (C.c_void_p * 1)(out.ptr), (C.c_size_t * 1)(150)
        _refused(L, L.hipdec_batch_to_rgb_scaled_all(a._h, 10, ws, hs, SCALE_BOX, ptrs, strides, None), -1)
        b.run(); b.status()
        assert b.to_rgb_scaled(0, 50, 40, SCALE_BOX).shape == (40, 150)
    finally:
        b.free()
        a.free()


def test_free_right_behind_a_scaled_call_waits_for_it():
    """work enqueued by the scaled calls is marked on the batch: hipdec_batch_free without a status call in between waits for the kernels that
    still read the arena.  What this guards: on the device a missing wait would hand the arena back to the pool while the kernel reads it (the pool
    does not unmap it, so the bytes would most likely still be right), and the emulator finishes every launch before it returns - so the comparison
    below documents the contract, and the use-after-free check proper is `bash tools/emu_asan_whole_library.sh tests/test_scale_gpu.py`
    (AddressSanitizer on the host build), which watches hipdec_batch_free's own bookkeeping: events, parameter blocks, captured state."""
    L = _lib()
    streams = [_still(1, 8, VUI_FULL, (200, 136), seed=40 + k) for k in range(4)]
    for filt in (SCALE_NEAREST, SCALE_BOX):
        b = decoder.Batch(streams)
        b.run()
        b.alloc_rgb_scaled((64, 44))
        b.to_rgb_scaled_all(filt)
        keep = b._srgb
        b.free()
        want = decoder.Batch(streams)
        want.run()
        want.status()
        for k in range(4):
            buf, stride, h = keep[k]
            assert np.array_equal(buf.to_numpy((h, stride), np.uint8), want.to_rgb_scaled(k, 64, 44, filt))
        want.free()
