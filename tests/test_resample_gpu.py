"""HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC on the device (k_resample, color.hip) through every call that takes them.

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code: the header defines the integer stage as
V = resample(full[window], ow, oh), `full` the interleaved 8-bit RGB picture of hipdec_batch_to_rgb (out_chroma 10; hipdec_color_convert for the image
form) and resample Pillow's 8-bit resampler, which tests/resample_ref.py restates in NumPy and tests/test_resample_ref.py pins to PIL.Image.resize.  The
float stage, the flip and the layouts are `expected_tensor` of tests/test_tensor_gpu.py, the orientation is np.rot90 / np.fliplr as tests/test_oriented_gpu.py
states it.

The kernel's tile is 16 output rows x at most 64 output columns, it stages 4 source rows x at most 1024 source columns at a time: the shapes below have
outputs below, at and above 16 / 64, up- and down-scaling, one-axis identity, 1 x 1, and taps wider than one staged chunk (1024 columns to 1).

Runs on the MI355X (`-m gpu`) and, through tests/test_resample_emu.py, against the library compiled for the host."""
import ctypes as C
import functools

import numpy as np
import pytest

import resample_ref as rr
from libheif_amd import color, decoder
from libheif_amd._capi import DeviceBuffer, HipDecError
from libheif_amd.color import SCALE_BICUBIC, SCALE_BILINEAR
from libheif_amd.decoder import Album
from test_album_gpu import ALBUMS, _album, _color_convert as _album_color_convert, _free_albums, _nclx as _album_nclx, expected_canvases   # noqa: F401 (_free_albums: the fixture)
from test_oriented_gpu import orient, pre_size
from test_scale_gpu import STILLS, VUI_FULL, VUI_LIMITED, _batch, _random_image, _refused, _still
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, STILLS_12, _color_convert, _full_rgb, _lib, _whole, as_bits, expected_tensor, run_tensor, windows_of

pytestmark = pytest.mark.gpu

FILTERS = (SCALE_BILINEAR, SCALE_BICUBIC)
assert (SCALE_BILINEAR, SCALE_BICUBIC) == (rr.BILINEAR, rr.BICUBIC) == (decoder.SCALE_BILINEAR, decoder.SCALE_BICUBIC) == (16, 17)


def resample_V(full, win, ow, oh, filt, stats=None):
    left, top, rw, rh = win
    return rr.resample(np.ascontiguousarray(full[top:top + rh, left:left + rw]), ow, oh, filt, stats)


_SHARED = {}


def _b(cf, bits, vui, size):
    """the decoded still, shared by the tests that only read it"""
    key = (cf, bits, tuple(sorted(vui.items())), size)
    if key not in _SHARED:
        _SHARED[key] = _batch([_still(cf, bits, vui, size)])
    return _SHARED[key]


@pytest.fixture(scope="module", autouse=True)
def _free_batches():
    yield
    for b in _SHARED.values():
        b.free()
    _SHARED.clear()


def _sizes(w, h):
    """down-scaling, 1 x 1, identity, up-scaling, x identity, y identity"""
    return [(100, 66), (37, 23), (1, 1), (w, h), (300, 200), (w, 23), (7, h)]


COMBOS = [(dt, lo) for dt in DTYPES for lo in LAYOUTS]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("cf,bits,vui,size", STILLS + STILLS_12)
def test_to_tensor_is_pillows_resize_of_the_window(cf, bits, vui, size, filt):
    """every chroma format and bit depth; the whole picture and windows at odd offsets with flips, several entries of one item per call; all four dtypes
    and both layouts for 8-bit sources (all eight at 37 x 23, two of them - a different pair each time - at the other sizes), uint8 for wider sources"""
    b = _b(cf, bits, vui, size)
    d = b.info(0)
    w, h = d["width"], d["height"]
    entries = windows_of(w, h)
    wins = [_whole(e, w, h)[1:5] for e in entries]
    flips = [e[5] for e in entries]
    full = _full_rgb(b, 0, False)
    for k, (ow, oh) in enumerate(_sizes(w, h)):
        Vs = [resample_V(full, win, ow, oh, filt) for win in wins]
        if bits > 8:
            combos = [("uint8", LAYOUTS[k & 1])]
        else:
            combos = COMBOS if (ow, oh) == (37, 23) else [COMBOS[(2 * k) % 8], COMBOS[(2 * k + 5) % 8]]
        for dtype, layout in combos:
            want = expected_tensor(Vs, flips, dtype, layout, SCALE, BIAS)
            got = run_tensor(b, (ow, oh), entries, dtype, layout, filt)
            assert np.array_equal(got, want), ((ow, oh), dtype, layout, int((got != want).sum()))


def _checker(w, h, cell):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // cell + xx // cell) & 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("cf", [3, 1])
def test_sums_below_zero_and_above_255_are_clipped(cf):
    """a 0 / 255 luma checkerboard of 3-pixel cells with neutral chroma, 96 x 64: bicubic's negative lobes push sums past both ends of the range, in the
    horizontal pass and in the vertical one (asserted on the reference's own pre-clip sums: otherwise the clamp went untested)"""
    L = _lib()
    w, h = 96, 64
    y = _checker(w, h, 3)
    cw, ch = (w, h) if cf == 3 else (w // 2, h // 2)
    planes = [y, np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)]
    nclx = (1, 13, 6, 1)
    full = _color_convert(L, planes, cf, 8, nclx, 10)
    assert np.array_equal(full[:, :, 0], y)
    for ow, oh in ((250, 170), (41, 27)):
        stats = {}
        V = resample_V(full, (0, 0, w, h), ow, oh, SCALE_BICUBIC, stats)
        assert stats["min"] < 0 and stats["max"] > (255 << 22), stats
        for dtype, layout in (("uint8", "NHWC"), ("float32", "NCHW")):
            want = expected_tensor([V], [0], dtype, layout, SCALE, BIAS)
            got = as_bits(color.image_to_tensor(planes, 8, cf, nclx, (ow, oh), None, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=SCALE_BICUBIC))
            assert np.array_equal(got, want), (cf, (ow, oh), dtype, int((got != want).sum()))


MANY_TAPS = (1024, 768)


@functools.lru_cache(maxsize=None)
def _many_taps_image(size):
    L = _lib()
    planes, _ = _random_image(size[0], size[1], 1, 8, False, seed=5)
    nclx = (1, 13, 6, 1)
    return planes, nclx, _color_convert(L, planes, 1, 8, nclx, 10)


def _many_taps(size, cases):
    planes, nclx, full = _many_taps_image(size)
    w, h = size
    for (ow, oh), filt, dtype, layout in cases:
        V = resample_V(full, (0, 0, w, h), ow, oh, filt)
        want = expected_tensor([V], [0], dtype, layout, SCALE, BIAS)
        got = as_bits(color.image_to_tensor(planes, 8, 1, nclx, (ow, oh), None, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt))
        assert np.array_equal(got, want), ((ow, oh), filt, dtype, int((got != want).sum()))


def test_more_taps_than_any_tile_holds():
    """1024 x 768 to 64 x 48 bicubic: 64 taps per axis and more; to 1 x 1 and 1024 x 1 bilinear: the taps are the whole row / column - the vertical sums run
    over 192 chunks of source rows.  1300 x 40 to 1 x 1 and 3 x 2: a row's taps span more than one staged chunk of 1024 columns, so the horizontal sums are
    carried across chunks."""
    assert max(len(k) for _, k in rr.table(1024, 64, SCALE_BICUBIC)) >= 64
    assert len(rr.table(1024, 1, SCALE_BILINEAR)[0][1]) == 1024 and len(rr.table(768, 1, SCALE_BILINEAR)[0][1]) == 768
    _many_taps(MANY_TAPS, [((64, 48), SCALE_BICUBIC, "uint8", "NHWC"), ((1, 1), SCALE_BILINEAR, "float32", "NCHW"), ((1024, 1), SCALE_BILINEAR, "uint8", "NCHW"),
                           ((1, 1), SCALE_BICUBIC, "uint8", "NHWC")])
    assert len(rr.table(1300, 1, SCALE_BILINEAR)[0][1]) == 1300 and max(len(k) for _, k in rr.table(1300, 3, SCALE_BICUBIC)) > 1024
    _many_taps((1300, 40), [((1, 1), SCALE_BILINEAR, "uint8", "NHWC"), ((3, 2), SCALE_BICUBIC, "float16", "NCHW"), ((2, 40), SCALE_BILINEAR, "uint8", "NCHW")])


@pytest.mark.parametrize("cf,bits,nclx", [(1, 8, (1, 13, 6, 1)), (2, 8, (1, 13, 1, 0)), (3, 8, (1, 13, 2, 1)), (0, 8, (1, 13, 6, 1)), (1, 10, (9, 16, 9, 1)), (3, 12, (1, 13, 6, 1))])
def test_image_form_on_an_odd_sized_image_with_windows_at_the_edges(cf, bits, nclx):
    """381 x 251 to 224 x 224: odd sizes for the subsampled formats too, windows that touch the right and the bottom edge"""
    L = _lib()
    w, h = 381, 251
    planes, _ = _random_image(w, h, cf, bits, False, seed=7 * cf + bits)
    full = _color_convert(L, planes, cf, bits, nclx, 10)
    entries = [(0, 0, 0, 0, 0), (1, 1, 380, 250, 1), (157, 27, 224, 224, 0), (380, 250, 1, 1, 0), (36, 20, 345, 41, 1), (0, 250, 381, 1, 0), (379, 0, 2, 251, 0)]
    wins = [(0, 0, w, h) if e[:4] == (0, 0, 0, 0) else e[:4] for e in entries]
    flips = [e[4] for e in entries]
    for filt in FILTERS:
        Vs = [resample_V(full, win, 224, 224, filt) for win in wins]
        for dtype, layout in ((("uint8", "NHWC"),) if bits > 8 else (("float16", "NCHW"), ("uint8", "NHWC"))):
            want = expected_tensor(Vs, flips, dtype, layout, SCALE, BIAS)
            got = as_bits(color.image_to_tensor(planes, bits, cf, nclx, (224, 224), entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt))
            assert np.array_equal(got, want), (filt, dtype, layout, int((got != want).sum()))
    if bits > 8:   # a float dtype from a source above 8 bits has no definition here
        with pytest.raises(HipDecError) as e:
            color.image_to_tensor(planes, bits, cf, nclx, (8, 8), None, dtype="float16", filter=SCALE_BILINEAR)
        assert e.value.code == -4


# ---- orientation -------------------------------------------------------------------------------------------------------------------------------------

def _run_oriented(b, size, entries, codes, dtype, layout, filt):
    n = len(entries)
    out = DeviceBuffer(n * 3 * size[0] * size[1] * {"uint8": 1, "float32": 4}.get(dtype, 2))
    assert b.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out, orientations=codes) is out
    return as_bits(b.tensor_to_host())


def _expected_oriented(full, w, h, size, entries, codes, dtype, layout, filt):
    """entry by entry: resample at the pre-orientation size, the float stage, orient, flip"""
    out = []
    for e, code in zip(entries, codes):
        pw, ph = pre_size(code & 1, size)
        V = resample_V(full, _whole(e, w, h)[1:5], pw, ph, filt)
        a = orient(code, expected_tensor([V], [0], dtype, "NHWC", SCALE, BIAS)[0])
        out.append(a[:, ::-1] if e[5] else a)
    exp = np.stack(out)
    assert exp.shape == (len(entries), size[1], size[0], 3)
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("cf,bits,vui,size", [STILLS[0], STILLS[3]])
def test_all_eight_orientation_codes_in_one_call(cf, bits, vui, size, filt):
    """a 200 x 136 4:2:0 still and a 141 x 93 4:4:4 one; displayed sizes whose pre-orientation sides are below, at and above the kernel's 16 x 64 tile"""
    b = _b(cf, bits, vui, size)
    w, h = size
    full = _full_rgb(b, 0, False)
    entries = [(0, 0, 0, 0, 0, 0)] * 8 + [(0, 37, 21, 64, 40, 1), (0, 1, 1, w - 1, h - 1, 1)]
    codes = tuple(range(8)) + (3, 6)
    before = decoder.oriented_stats()
    runs = 0
    for dsize, dtype, layout in (((22, 13), "uint8", "NHWC"), ((70, 17), "float16", "NCHW"), ((16, 65), "float32", "NHWC"), ((33, 64), "bfloat16", "NCHW")):
        got = _run_oriented(b, dsize, entries, codes, dtype, layout, filt)
        exp = _expected_oriented(full, w, h, dsize, entries, codes, dtype, layout, filt)
        bad = [(e, codes[e], int((got[e] != exp[e]).sum())) for e in range(len(codes)) if not np.array_equal(got[e], exp[e])]
        assert not bad, (dsize, dtype, layout, bad)
        runs += 1
    after = decoder.oriented_stats()
    assert tuple(a - c for a, c in zip(after, before)) == (runs, runs * 10, runs * 5)      # one launch per call; codes 1, 3, 5, 7 and the extra 3


@pytest.mark.parametrize("filt", FILTERS)
def test_oriented_rgb_form_with_a_padded_stride(filt):
    L = _lib()
    cf, bits, vui, size = STILLS[0]
    b = _batch([_still(cf, bits, vui, size)] * 8)
    try:
        w, h = size
        full = _full_rgb(b, 0, False)
        sizes = [(23, 9), (9, 23), (64, 5), (5, 64), (31, 17), (13, 35), (1, 7), (70, 3)]
        codes = tuple(range(8))
        pad, fill, n = 13, 0xA5, 8
        strides = [sw * 3 + pad for sw, _ in sizes]
        bufs = [DeviceBuffer.from_numpy(np.full((sh, st), fill, np.uint8)) for (_, sh), st in zip(sizes, strides)]
        decoder.check(L.hipdec_batch_to_rgb_scaled_oriented_all(b._h, 10, (C.c_int * n)(*codes), (C.c_int * n)(*[s[0] for s in sizes]), (C.c_int * n)(*[s[1] for s in sizes]),
                                                                filt, (C.c_void_p * n)(*[x.ptr for x in bufs]), (C.c_size_t * n)(*strides), None))
        decoder.check(L.hipdec_stream_synchronize(None))
        for i, ((sw, sh), st) in enumerate(zip(sizes, strides)):
            got = bufs[i].to_numpy((sh, st), np.uint8)
            pw, ph = pre_size(codes[i] & 1, (sw, sh))
            want = orient(codes[i], resample_V(full, (0, 0, w, h), pw, ph, filt))
            assert np.array_equal(got[:, :sw * 3].reshape(sh, sw, 3), want), (i, codes[i])
            assert (got[:, sw * 3:] == fill).all(), "bytes beyond a row's 3 * width were written"
        assert b.slot_kernel_timing_us(0)["colour"] > 0.0
    finally:
        b.free()


# ---- the RGB24 forms ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("cf,bits,vui,size", [STILLS[1], STILLS[4], STILLS[6]])
def test_to_rgb_scaled_is_pillows_resize_of_to_rgb(cf, bits, vui, size, filt):
    """the single-item call; 4:2:0 through the float chain, monochrome, 10-bit through to-SDR"""
    L = _lib()
    b = _b(cf, bits, vui, size)
    w, h = size
    full = _full_rgb(b, 0, False)
    for ow, oh in ((50, 34), (1, 1), (w, h), (w + 9, h + 5)):
        got = b.to_rgb_scaled(0, ow, oh, filt, 10).reshape(oh, ow, 3)
        assert np.array_equal(got, resample_V(full, (0, 0, w, h), ow, oh, filt)), (ow, oh)
    out = DeviceBuffer(50 * 34 * 6)
    for oc in (11, 12, 14):
        _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, oc, 50, 34, filt, out.ptr, 50 * 6, None), -4)
    _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 50, 34, filt, out.ptr, 50 * 3 - 1, None), -1)
    _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 1, 10, 50, 34, filt, out.ptr, 50 * 3, None), -1)
    _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 0, 34, filt, out.ptr, 50 * 3, None), -1)
    # the plane-level forms keep refusing the new values
    host = np.empty((34, 50), np.uint16)
    _refused(L, L.hipdec_batch_read_plane_scaled(b._h, 0, 0, 50, 34, filt, host.ctypes.data, 100), -1)
    with pytest.raises(HipDecError):
        color.image_scale([np.zeros((20, 30), np.uint8)], 8, 0, 10, 5, filt)


@pytest.mark.parametrize("filt", FILTERS)
def test_to_rgb_scaled_all_with_per_item_sizes(filt):
    sizes_in = [(200, 136), (142, 94), (64, 64)]
    b = _batch([_still(1, 8, VUI_FULL if k % 2 else VUI_LIMITED, s, seed=30 + k) for k, s in enumerate(sizes_in)])
    try:
        sizes = [(100, 66), (150, 100), (17, 65)]
        b.alloc_rgb_scaled(sizes, 10)
        b.to_rgb_scaled_all(filt)
        b.status()
        assert b.slot_kernel_timing_us(0)["colour"] > 0.0
        for i, ((w, h), (ow, oh)) in enumerate(zip(sizes_in, sizes)):
            buf, stride, rows = b._srgb[i]
            got = buf.to_numpy((rows, stride), np.uint8).reshape(oh, ow, 3)
            assert np.array_equal(got, resample_V(_full_rgb(b, i, False), (0, 0, w, h), ow, oh, filt)), i
    finally:
        b.free()


ALBUM = "444"      # the smallest album of tests/test_album_gpu.py: two photos of 131 x 91 and 99 x 63, 4:4:4


@pytest.mark.parametrize("filt", FILTERS)
def test_album_forms(filt):
    photos, bits, cf = ALBUMS[ALBUM]
    a = _album(ALBUM)
    fulls = []
    for p, planes in enumerate(expected_canvases(ALBUM)):
        h, w = planes[0].shape
        fulls.append(_album_color_convert(planes, cf, bits, _album_nclx(ALBUM, p), 10).reshape(h, w, 3))
    sizes = [(33, 23), (150, 70)]
    a.alloc_rgb_scaled(sizes, 10)
    a.to_rgb_scaled_all(filt)
    a.status()
    for p, (ow, oh) in enumerate(sizes):
        h, w = fulls[p].shape[:2]
        assert np.array_equal(a.rgb_scaled(p).reshape(oh, ow, 3), resample_V(fulls[p], (0, 0, w, h), ow, oh, filt)), p
    entries = [(1, 0, 0, 0, 0, 0), (0, 33, 31, 70, 57, 1), (0, 0, 0, 0, 0, 1)]
    wins = [(e[1], e[2], e[3], e[4]) if e[3] else (0, 0, photos[e[0]][4], photos[e[0]][5]) for e in entries]
    Vs = [resample_V(fulls[e[0]], win, 50, 34, filt) for e, win in zip(entries, wins)]
    for dtype, layout in (("uint8", "NHWC"), ("bfloat16", "NCHW")):
        want = expected_tensor(Vs, [e[5] for e in entries], dtype, layout, SCALE, BIAS)
        assert np.array_equal(run_tensor(a, (50, 34), entries, dtype, layout, filt), want), (dtype, layout)
    # oriented, through the album
    codes = (5, 2, 0)
    out = DeviceBuffer(3 * 3 * 34 * 50)
    a.to_tensor((34, 50), entries, dtype="uint8", layout="NHWC", filter=filt, out=out, orientations=codes)
    got = a.tensor_to_host()
    for k, (e, win, code) in enumerate(zip(entries, wins, codes)):
        pw, ph = pre_size(code & 1, (34, 50))
        want = orient(code, resample_V(fulls[e[0]], win, pw, ph, filt))
        assert np.array_equal(got[k], want[:, ::-1] if e[5] else want), k


# ---- tables, life cycle, limits ------------------------------------------------------------------------------------------------------------------------

def test_two_calls_with_different_tables_then_free_right_behind_the_launch():
    """tables are per (input, output) size: a second call on the same batch with other sizes uploads other tables into the same buffer; hipdec_batch_free
    right behind the launch waits for it (as tests/test_tensor_gpu.py states it for the other filters)"""
    streams = [_still(1, 8, VUI_FULL, (200, 136), seed=40 + k) for k in range(4)]
    ones, zeros = np.ones(3, np.float32), np.zeros(3, np.float32)
    for filt in FILTERS:
        want = _batch(streams)
        n0 = decoder.tensor_stats()
        first = run_tensor(want, (64, 44), None, "float16", "NCHW", filt, ones, zeros)
        again = run_tensor(want, (64, 44), None, "float16", "NCHW", filt, ones, zeros)        # the same blocks and tables: nothing is uploaded
        other = run_tensor(want, (30, 90), [(1, 3, 5, 100, 80, 0), (2, 0, 0, 0, 0, 1)], "float16", "NCHW", filt, ones, zeros)
        back = run_tensor(want, (64, 44), None, "float16", "NCHW", filt, ones, zeros)
        assert np.array_equal(first, again) and np.array_equal(first, back)
        n1 = decoder.tensor_stats()
        assert (n1[0] - n0[0], n1[1] - n0[1]) == (4, 14)
        assert want.slot_kernel_timing_us(0)["colour"] > 0.0
        fulls = [_full_rgb(want, i, False) for i in range(4)]
        exp = expected_tensor([resample_V(f, (0, 0, 200, 136), 64, 44, filt) for f in fulls], [0] * 4, "float16", "NCHW", ones, zeros)
        assert np.array_equal(first, exp)
        exp = expected_tensor([resample_V(fulls[1], (3, 5, 100, 80), 30, 90, filt), resample_V(fulls[2], (0, 0, 200, 136), 30, 90, filt)], [0, 1], "float16", "NCHW", ones, zeros)
        assert np.array_equal(other, exp)
        want.free()
        b = decoder.Batch(streams)
        b.run()
        out = DeviceBuffer(4 * 3 * 64 * 44 * 2)
        b.to_tensor((64, 44), None, dtype="float16", filter=filt, scale=ones, bias=zeros, out=out)
        b.free()
        assert np.array_equal(out.to_numpy((4, 3, 44, 64), np.uint16), first)


def test_the_limit_given_at_creation_holds_for_the_new_filters():
    L = _lib()
    b = _batch([_still(1, 8, VUI_FULL, (200, 136))], max_image_size_pixels=200 * 136)
    try:
        out = DeviceBuffer(3 * 400 * 300)
        for filt in FILTERS:
            big, fits = decoder.tensor_desc((400, 300), "uint8", "NCHW", filt, 1.0, 0.0), decoder.tensor_desc((200, 136), "uint8", "NCHW", filt, 1.0, 0.0)
            _refused(L, L.hipdec_batch_to_tensor(b._h, C.byref(big), None, 1, out.ptr, out.nbytes, None), -5)
            _refused(L, L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 400, 300, filt, out.ptr, 1200, None), -5)
            assert L.hipdec_batch_to_tensor(b._h, C.byref(fits), None, 1, out.ptr, out.nbytes, None) == 0     # at the limit
            assert L.hipdec_batch_to_rgb_scaled(b._h, 0, 10, 200, 136, filt, out.ptr, 600, None) == 0
        b.status()
    finally:
        b.free()
