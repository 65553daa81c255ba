"""Oriented output on the device: hipdec_batch_to_tensor_oriented / hipdec_batch_to_rgb_scaled_oriented_all and their album forms ('irot' / 'imir' folded
into the store of the fused tensor and scaled-RGB kernels, include/heif_hipdec.h hipdec_orientation).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code: the header defines the oriented result as
orient(code, P), P what the EXISTING unoriented call of the same library writes for the same item, window, filter and the pre-orientation size (the
displayed size, swapped for an odd number of quarter turns), and orient is np.rot90(a, r) followed by np.fliplr where m is set; a tensor entry's flip then
mirrors the displayed result.  The unoriented calls are pinned by tests/test_tensor_gpu.py and tests/test_scale_gpu.py.  One test holds the result against
the transform chain (hipdec_image_transform, then hipdec_color_convert), which tests/test_transform_gpu.py and tests/test_color_boundary.py pin to the
compiled reference.

Block height of the quarter-turn store (k_oriented_box, color.hip): RB = 64 rows of the pre-orientation picture where the component values are 8 bits wide
(8-bit sources, and the uint8 dtype from any source), RB = 32 for native-depth values (float dtypes from sources above 8 bits); the column tile is 96 / 64.
SHAPES below has RB - 1, RB, RB + 1 and 2 * RB + 1 of both on both sides of the result.

Runs on the MI355X (`-m gpu`) and, through tests/test_oriented_emu.py, against the library compiled for the host."""
import ctypes as C
import functools
import numpy as np
import pytest

from libheif_amd import color, decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import Album, TensorDesc
from test_scale_gpu import VUI_FULL, VUI_LIMITED, _batch, _refused, _still
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits, run_tensor
from test_transform_gpu import ColorImage, XF_MIRROR, XF_ROTATE

pytestmark = pytest.mark.gpu

FILTERS = (SCALE_NEAREST, SCALE_BOX)
CODES = tuple(range(8))
SMALL = (1, 8, VUI_FULL, (72, 40))                       # the even-sized 4:2:0 8-bit still most cases use
# 4:2:2, 4:4:4 and 4:0:0 with odd width and height, 10-bit 4:2:0
FORMATS = [(2, 8, VUI_FULL, (72, 40)), (3, 8, VUI_LIMITED, (41, 23)), (0, 8, {}, (41, 23)), (1, 10, VUI_LIMITED, (72, 40))]


def orient(code, a):
    """a: (H, W, ...) - the definition of the header"""
    a = np.rot90(a, code & 3)
    return np.fliplr(a) if code >> 2 else a


def pre_size(code, size):
    return (size[1], size[0]) if code & 1 else tuple(size)


@functools.lru_cache(maxsize=None)
def _shared_batch(still):
    cf, bits, vui, size = still
    return _batch([_still(cf, bits, dict(vui), size)])


def _b(still):
    cf, bits, vui, size = still
    return _shared_batch((cf, bits, tuple(sorted(vui.items())), size))


@pytest.fixture(scope="module", autouse=True)
def _free_batches():
    yield
    _shared_batch.cache_clear()


def _hwc(t, layout):
    return t.transpose(0, 2, 3, 1) if layout == "NCHW" else t


def expected_oriented(b, size, entries, codes, dtype, layout, filt, call=run_tensor):
    """entry by entry: the unoriented call without the flip at the pre-orientation size, oriented, flipped"""
    n = b.n if entries is None else len(entries)
    entries = [(i, 0, 0, 0, 0, 0) for i in range(n)] if entries is None else entries
    out = [None] * n
    for parity in (0, 1):
        idx = [e for e in range(n) if (codes[e] & 1) == parity]
        if not idx:
            continue
        P = _hwc(call(b, pre_size(parity, size), [tuple(entries[e][:5]) + (0,) for e in idx], dtype, layout, filt), layout)
        for k, e in enumerate(idx):
            a = orient(codes[e], P[k])
            out[e] = a[:, ::-1] if entries[e][5] else a
    exp = np.stack(out)
    assert exp.shape == (n, size[1], size[0], 3)
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def run_oriented(b, size, entries, codes, dtype, layout, filt):
    n = b.n if entries is None else len(entries)
    out = DeviceBuffer(n * 3 * size[0] * size[1] * {"uint8": 1, "float32": 4}.get(dtype, 2))
    assert b.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out, orientations=codes) is out
    got = b.tensor_to_host()
    assert got.shape == ((n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3))
    return as_bits(got)


def check(b, size, entries, codes, dtype, layout, filt):
    got = run_oriented(b, size, entries, codes, dtype, layout, filt)
    exp = expected_oriented(b, size, entries, codes, dtype, layout, filt)
    bad = [(e, codes[e], int((got[e] != exp[e]).sum())) for e in range(len(codes)) if not np.array_equal(got[e], exp[e])]
    assert not bad, (size, dtype, layout, filt, bad)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", FILTERS)
def test_all_eight_codes(filt, dtype, layout):
    check(_b(SMALL), (22, 13), [(0, 0, 0, 0, 0, 0)] * 8, CODES, dtype, layout, filt)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("still", FORMATS, ids=lambda s: "cf%d-%dbit" % (s[0], s[1]))
def test_chroma_formats_and_depths(still, filt):
    b = _b(still)
    for dtype, layout in (("uint8", "NHWC"), ("float32", "NCHW")):     # 10-bit: uint8 is the to-SDR value, float32 the native-depth one
        check(b, (19, 14), [(0, 0, 0, 0, 0, 0)] * 8, CODES, dtype, layout, filt)


# displayed sizes: widths that are no multiple of 4, 1 x N and N x 1, RB - 1 / RB / RB + 1 / 2 RB + 1 for RB = 32 and 64 on either side
SHAPES = [(7, 5), (1, 9), (9, 1), (2, 3)] + [s for n in (31, 32, 33, 63, 64, 65, 129) for s in ((n, 3), (5, n))]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_output_shapes_where_the_store_can_go_wrong(size, filt):
    e = [(0, 0, 0, 0, 0, 0)] * 8
    check(_b(SMALL), size, e, CODES, "uint8", "NCHW", filt)
    check(_b(SMALL), size, e, CODES, "float16", "NHWC", filt)
    check(_b(FORMATS[3]), size, e, CODES, "float32", "NCHW", filt)     # native depth: the 64-bit stage, RB = 32
    check(_b(FORMATS[3]), size, e, CODES, "bfloat16", "NHWC", filt)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("size", [(261, 67), (67, 261)], ids=lambda s: "%dx%d" % s)
def test_up_scaled_output_wider_than_a_tile(size, filt):
    """pre-orientation widths of 261 (more than one 256-pixel tile of the unoriented kernel, three of the oriented one) and 67"""
    codes = (1, 2, 7, 4, 3)
    check(_b(SMALL), size, [(0, 0, 0, 0, 0, 0)] * len(codes), codes, "uint8", "NHWC", filt)
    check(_b(SMALL), size, [(0, 0, 0, 0, 0, 0)] * len(codes), codes, "float16", "NCHW", filt)


WINDOWS = [(0, 1, 3, 35, 21, 0), (0, 5, 7, 33, 17, 1), (0, 0, 0, 0, 0, 1), (0, 37, 11, 31, 29, 0), (0, 71, 39, 1, 1, 1), (0, 3, 1, 69, 39, 1), (0, 9, 5, 7, 3, 0),
           (0, 1, 1, 71, 39, 1)]
WINDOW_CODES = (1, 5, 4, 3, 6, 7, 2, 0)                  # flip together with m: entries 1, 2, 4, 5


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype,layout", [("uint8", "NCHW"), ("float16", "NHWC")])
def test_windows_flips_and_several_codes_on_one_item(dtype, layout, filt):
    """windows at odd left / top with odd sizes stay in luma samples of the STORED picture"""
    check(_b(SMALL), (21, 10), WINDOWS, WINDOW_CODES, dtype, layout, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_mixed_codes_share_one_launch(filt):
    b = _b(SMALL)
    before = decoder.oriented_stats()
    got = run_oriented(b, (24, 10), [(0, 0, 0, 0, 0, 0)] * 8, CODES, "float32", "NCHW", filt)
    after = decoder.oriented_stats()
    assert tuple(a - c for a, c in zip(after, before)) == (1, 8, 4)
    assert np.array_equal(got, expected_oriented(b, (24, 10), [(0, 0, 0, 0, 0, 0)] * 8, CODES, "float32", "NCHW", filt))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype,layout", [("uint8", "NHWC"), ("bfloat16", "NCHW")])
def test_identity_is_the_unoriented_call_byte_for_byte(dtype, layout, filt):
    L = _lib()
    b = _b(SMALL)
    size = (30, 17)
    entries = [(0, 0, 0, 0, 0, 0), (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)]
    want = run_tensor(b, size, entries, dtype, layout, filt)
    assert np.array_equal(run_oriented(b, size, entries, (0, 0, 0), dtype, layout, filt), want)
    desc = decoder.tensor_desc(size, dtype, layout, filt, SCALE, BIAS)                 # orientations = NULL through the C ABI
    out = DeviceBuffer(want.nbytes)
    decoder.check(L.hipdec_batch_to_tensor_oriented(b._h, C.byref(desc), decoder.tensor_entries(entries), None, 3, out.ptr, out.nbytes, None))
    decoder.check(L.hipdec_stream_synchronize(None))
    assert np.array_equal(out.to_numpy(want.shape, want.dtype), want)


def _rgb_oriented(L, call, handle, codes, sizes, filt, pad, fill=0xA5):
    """the RGB form into rows `pad` bytes longer than the pixels, pre-filled; returns the (h, stride) arrays"""
    n = len(sizes)
    strides = [w * 3 + pad for w, _ in sizes]
    bufs = [DeviceBuffer.from_numpy(np.full((h, st), fill, np.uint8)) for (_, h), st in zip(sizes, strides)]
    rc = call(handle, 10, (C.c_int * n)(*codes), (C.c_int * n)(*[w for w, _ in sizes]), (C.c_int * n)(*[h for _, h in sizes]), filt,
              (C.c_void_p * n)(*[x.ptr for x in bufs]), (C.c_size_t * n)(*strides), None)
    decoder.check(rc)
    decoder.check(L.hipdec_stream_synchronize(None))
    return [x.to_numpy((h, st), np.uint8) for x, (_, h), st in zip(bufs, sizes, strides)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("still", [SMALL, FORMATS[3], FORMATS[2]], ids=lambda s: "cf%d-%dbit" % (s[0], s[1]))
def test_rgb_form_with_a_stride_larger_than_the_row(still, filt):
    L = _lib()
    cf, bits, vui, size = still
    streams = [_still(cf, bits, vui, size)] * 8
    b = _batch(streams)
    try:
        sizes = [(23, 9), (9, 23), (64, 5), (5, 64), (31, 11), (13, 35), (1, 7), (70, 3)]
        got = _rgb_oriented(L, L.hipdec_batch_to_rgb_scaled_oriented_all, b._h, CODES, sizes, filt, pad=13)
        for i, (code, (w, h)) in enumerate(zip(CODES, sizes)):
            pw, ph = pre_size(code, (w, h))
            want = orient(code, b.to_rgb_scaled(i, pw, ph, filt, 10).reshape(ph, pw, 3)).reshape(h, w * 3)
            assert np.array_equal(got[i][:, :w * 3], want), (i, code, filt)
            assert (got[i][:, w * 3:] == 0xA5).all(), "bytes between the row's end and the stride were written"
    finally:
        b.free()


@pytest.mark.parametrize("still", [SMALL, FORMATS[1]], ids=lambda s: "cf%d" % s[0])
def test_nearest_at_displayed_full_size_is_the_oriented_full_picture_and_the_transform_chain(still):
    """... = orient(Batch.to_rgb), and = hipdec_color_convert (nearest-neighbour chroma, out_chroma 10) of the planes after hipdec_image_transform
    ROTATE_CCW, then MIRROR horizontal: the order libheif applies the properties in, planes first"""
    L = _lib()
    cf, bits, vui, (w, h) = still
    b = _batch([_still(cf, bits, vui, (w, h))] * 8)
    try:
        sizes = [pre_size(c, (w, h)) for c in CODES]
        got = _rgb_oriented(L, L.hipdec_batch_to_rgb_scaled_oriented_all, b._h, CODES, sizes, SCALE_NEAREST, pad=0)
        full = b.to_rgb(0, 10).reshape(h, w, 3)
        d = b.info(0)
        nclx = (d["colour_primaries"], d["transfer_characteristics"], d["matrix_coeffs"], d["full_range_flag"])
        for code, (dw, dh), g in zip(CODES, sizes, got):
            assert np.array_equal(g.reshape(dh, dw, 3), orient(code, full)), code
            planes, pw, ph = b.planes(0), w, h
            for op, arg in ([(XF_ROTATE, 90 * (code & 3))] if code & 3 else []) + ([(XF_MIRROR, 1)] if code >> 2 else []):
                planes, pw, ph = _transform(L, planes, pw, ph, cf, op, arg)
            assert (pw, ph) == (dw, dh)
            chain = color.convert_colorspace(planes, 8, cf, nclx, color.CHROMA_RGB, upsampling=color.UPSAMPLING_NEAREST)
            assert np.array_equal(g, chain.reshape(dh, dw * 3)), ("transform chain", code)
    finally:
        b.free()


def _transform(L, planes, w, h, cf, op, arg):
    """hipdec_image_transform on host planes of an 8-bit image; returns the planes and the new size"""
    L.hipdec_image_transform.argtypes = [C.POINTER(ColorImage), C.c_int, C.POINTER(C.c_int), C.POINTER(ColorImage)]
    src, dst = ColorImage(w, h, cf, 8), ColorImage()
    keep = [np.ascontiguousarray(p) for p in planes]
    ow, oh = (h, w) if op == XF_ROTATE and arg != 180 else (w, h)
    sx, sy = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    outs = []
    for c, p in enumerate(keep):
        src.plane[c], src.stride[c] = p.ctypes.data, p.strides[0]
        o = np.zeros((oh, ow) if c == 0 else ((oh + sy - 1) // sy, (ow + sx - 1) // sx), np.uint8)
        outs.append(o)
        dst.plane[c], dst.stride[c] = o.ctypes.data, o.strides[0]
    decoder.check(L.hipdec_image_transform(C.byref(src), op, (C.c_int * 4)(arg, 0, 0, 0), C.byref(dst)))
    assert (dst.width, dst.height) == (ow, oh)
    return outs, ow, oh


def _album_tensor(a, size, entries, dtype, layout, filt):
    n = len(entries)
    out = DeviceBuffer(n * 3 * size[0] * size[1] * {"uint8": 1, "float32": 4}.get(dtype, 2))
    a.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out)
    return as_bits(a.tensor_to_host())


@pytest.mark.parametrize("filt", FILTERS)
def test_album_forms_against_the_unoriented_album_calls(filt):
    """two photos of different grid geometry with different codes, tensor and RGB forms"""
    from test_album_gpu import _photos
    L = _lib()
    a = Album(_photos("mixed8")[:2])                      # 2 x 3 tiles of 72 x 48 clipped to 200 x 90, and 1 x 1 of 64 x 64
    try:
        a.run()
        a.status()
        entries, codes, size = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 101, 57, 0), (1, 1, 1, 63, 63, 0)], (3, 5, 6, 1), (37, 18)
        for dtype, layout in (("uint8", "NHWC"), ("float16", "NCHW")):
            out = DeviceBuffer(4 * 3 * size[0] * size[1] * 2)
            a.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out, orientations=codes)
            got = as_bits(a.tensor_to_host())
            assert np.array_equal(got, expected_oriented(a, size, entries, codes, dtype, layout, filt, call=_album_tensor)), (dtype, layout)
        sizes, rgb_codes = [(45, 100), (32, 32)], (7, 2)
        got = _rgb_oriented(L, L.hipdec_album_to_rgb_scaled_oriented_all, a._h, rgb_codes, sizes, filt, pad=5)
        a.alloc_rgb_scaled([pre_size(c, s) for c, s in zip(rgb_codes, sizes)])
        a.to_rgb_scaled_all(filt)
        for p, (code, (w, h)) in enumerate(zip(rgb_codes, sizes)):
            pw, ph = pre_size(code, (w, h))
            want = orient(code, a.rgb_scaled(p).reshape(ph, pw, 3)).reshape(h, w * 3)
            assert np.array_equal(got[p][:, :w * 3], want) and (got[p][:, w * 3:] == 0xA5).all(), (p, code)
        a.alloc_rgb_scaled(sizes)                           # the Python keyword: displayed sizes into alloc_rgb_scaled
        a.to_rgb_scaled_all(filt, orientations=rgb_codes)
        for p, (w, h) in enumerate(sizes):
            assert np.array_equal(a.rgb_scaled(p), got[p][:, :w * 3]), p
    finally:
        a.free()


def test_refusals_have_a_status_and_a_message():
    L = _lib()
    b = _b(SMALL)
    desc = decoder.tensor_desc((16, 8), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
    out = DeviceBuffer(16 * 8 * 3 + 64)
    for bad in (-1, 8):
        _refused(L, L.hipdec_batch_to_tensor_oriented(b._h, C.byref(desc), None, (C.c_int * 1)(bad), 1, out.ptr, out.nbytes, None), -1)
        assert b"entry 0" in L.hipdec_last_error()
    _refused(L, L.hipdec_batch_to_tensor_oriented(b._h, C.byref(desc), None, (C.c_int * 1)(1), 1, out.ptr, 16 * 8 * 3 - 1, None), -1)       # a short out_bytes
    _refused(L, L.hipdec_batch_to_tensor_oriented(b._h, C.byref(desc), decoder.tensor_entries([(0, 70, 0, 5, 5, 0)]), (C.c_int * 1)(1), 1, out.ptr, out.nbytes, None), -1)
    one = lambda v, t=C.c_int: (t * 1)(v)
    ptrs = (C.c_void_p * 1)(out.ptr)
    rgb = L.hipdec_batch_to_rgb_scaled_oriented_all
    for bad in (-1, 8):
        _refused(L, rgb(b._h, 10, one(bad), one(8), one(16), SCALE_BOX, ptrs, one(24, C.c_size_t), None), -1)
        assert b"item 0" in L.hipdec_last_error()
    _refused(L, rgb(b._h, 11, one(1), one(8), one(16), SCALE_BOX, ptrs, one(32, C.c_size_t), None), -4)       # out_chroma 11: unsupported
    _refused(L, rgb(b._h, 10, one(1), one(8), one(16), SCALE_BOX, ptrs, one(23, C.c_size_t), None), -1)       # a short stride
    _refused(L, rgb(b._h, 10, one(1), one(0), one(16), SCALE_BOX, ptrs, one(24, C.c_size_t), None), -1)
    _refused(L, rgb(b._h, 10, one(1), one(8), one(16), 2, ptrs, one(24, C.c_size_t), None), -1)
    _refused(L, rgb(None, 10, one(1), one(8), one(16), SCALE_BOX, ptrs, one(24, C.c_size_t), None), -1)
    assert rgb(b._h, 10, one(1), one(8), one(16), SCALE_BOX, ptrs, one(24, C.c_size_t), None) == 0
    decoder.check(L.hipdec_stream_synchronize(None))
    with pytest.raises(ValueError):
        b.to_tensor((16, 8), None, dtype="uint8", out=out, orientations=(0, 1))      # two codes for one entry


def test_example_host_makes_oriented_previews(tmp_path):
    """examples/decode_batch.c --thumb N --orient CODE end to end: the size rule sees the displayed picture, so a quarter turn makes the preview at the swapped
    pre-orientation size (an orientation keeps the byte sum of that); a bad CODE prints the usage"""
    import os
    import subprocess
    import libheif_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.abspath(libheif_amd.library_path())
    exe = str(tmp_path / "decode_batch")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    for bad in (["--orient", "8"], ["--orient", "-1"], ["--orient"]):
        r = subprocess.run([exe, "--thumb", "32"] + bad + ["x.hevc"][:len(bad) - 1], capture_output=True, text=True)
        assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    f = tmp_path / "item.hevc"
    f.write_bytes(_still(*SMALL))
    r = subprocess.run([exe, "--thumb", "32", "--orient", "5", str(f)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    dw, dh = decoder.fit_within(40, 72, 32)                     # the displayed picture of the 72 x 40 still is 40 x 72
    want = int(_b(SMALL).to_rgb_scaled(0, dh, dw, SCALE_BOX).astype(np.uint64).sum())
    assert "%s: preview %dx%d RGB24, byte sum %d\n" % (f, dw, dh, want) in r.stdout, r.stdout
