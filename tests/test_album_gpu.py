"""Albums of grid photos (hipdec_album_*, libheif_amd.decoder.Album): K photos, one launch set, one fused paste.

Everything is bit-exact and no expected value comes from the code under test: the expected canvas of a photo is the oracle's decode of every tile
(oracle.pyoracle.decode) pasted in NumPy at (col * tile_w, row * tile_h) - subsampled for chroma - and clipped to the output size, the way
HeifPixelImage::copy_image_to does it; RGB, scaled RGB and tensors are the batch forms' definitions (hipdec_color_convert, the box filter and the
nearest-neighbour formula of include/heif_hipdec.h, the tensor helpers of tests/test_tensor_gpu.py) over that expected canvas.

The tiles are a few CTBs each (72 x 48 and 64 x 64), the smallest at which the paste can go wrong: chroma tiles of 36 bytes put the destinations at
phases 0 / 4 / 8 of the 16-byte store unit (10 bit: 0 / 8), clipped right columns and bottom rows, odd output sizes, a 1 x 1 photo, a tile row of which
one luma row survives, a tile that is clipped away entirely."""
import ctypes as C
import functools

import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import HipDecError, Nclx, check
from libheif_amd.color import ColorImage, SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import Album, album_stats
from libheif_amd.grid import GridDecoderC, GridLayout
from oracle import pyoracle as orc
from tools import streamgen
from test_scale_gpu import VUI_FULL, VUI_LIMITED, _color_convert_444, box_plane
from test_tensor_gpu import BIAS, SCALE, _lib, box_V, expected_tensor, nearest_V, run_tensor

pytestmark = pytest.mark.gpu

# (rows, cols, tile_w, tile_h, out_w, out_h, VUI)
MIXED = [(2, 3, 72, 48, 200, 90, VUI_FULL),       # chroma tile rows of 36 bytes: phases 0 / 4 / 8; right column and bottom row clipped, even output width
         (1, 1, 64, 64, 64, 64, VUI_LIMITED),     # a 1 x 1 photo at full size
         (3, 2, 64, 64, 127, 129, VUI_FULL)]      # odd output: chroma sizes (w + 1) / 2; one luma row of the last tile row survives
PAIR_EVEN = [(2, 2, 72, 48, 130, 90, VUI_FULL), (1, 2, 64, 64, 100, 64, VUI_LIMITED)]     # 4:2:2: even widths
PAIR_ODD = [(2, 2, 72, 48, 131, 91, VUI_LIMITED), (1, 2, 64, 64, 99, 63, VUI_FULL)]       # 4:4:4 and 4:0:0: odd sizes
CLIPPED = [(1, 3, 64, 64, 128, 64, VUI_FULL), (2, 2, 64, 64, 64, 70, VUI_LIMITED)]        # out_w = (cols - 1) * tile_w: the last column is clipped away
ALBUMS = {"mixed8": (MIXED, 8, 1), "mixed10": (MIXED, 10, 1), "mono": (PAIR_ODD, 8, 0), "422": (PAIR_EVEN, 8, 2), "444": (PAIR_ODD, 8, 3),
          "clipped": (CLIPPED, 8, 1)}


def _specs(name):
    photos, bits, cf = ALBUMS[name]
    out = []
    for p, (rows, cols, tw, th, _, _, vui) in enumerate(photos):
        for t in range(rows * cols):
            cfg = dict(chroma_format_idc=cf, stress=t & 1, wpp=(t >> 1) & 1, qp=26 + 2 * (t % 3), **(vui if cf else {}))
            out.append((tw, th, 900 + 50 * p + t, bits, cfg))
    return out


@functools.lru_cache(maxsize=None)
def _all_streams():
    """every tile of every album of this module, generated (or read from the stream cache) in one go"""
    names = sorted(ALBUMS)
    flat = streamgen.make_streams([s for n in names for s in _specs(n)])
    out, k = {}, 0
    for n in names:
        out[n] = []
        for rows, cols, *_ in ALBUMS[n][0]:
            out[n].append(flat[k:k + rows * cols])
            k += rows * cols
    return out


@functools.lru_cache(maxsize=None)
def _oracle(stream):
    return orc.decode(stream)


@functools.lru_cache(maxsize=None)
def expected_canvases(name):
    """per photo: the oracle's tiles pasted and clipped, plane by plane"""
    photos, bits, cf = ALBUMS[name]
    out = []
    for (rows, cols, tw, th, ow, oh, _), tiles in zip(photos, _all_streams()[name]):
        refs = [_oracle(t) for t in tiles]
        assert all((r["width"], r["height"]) == (tw, th) for r in refs)
        planes = []
        for c in range(3 if cf else 1):
            ph, pw = refs[0]["planes"][c].shape
            sw, sh = tw // pw, th // ph
            canvas = np.zeros((rows * ph, cols * pw), np.uint16 if bits > 8 else np.uint8)      # (the oracle hands out uint16 whatever the depth)
            for t, r in enumerate(refs):
                y, x = divmod(t, cols)
                canvas[y * ph:(y + 1) * ph, x * pw:(x + 1) * pw] = r["planes"][c]
            planes.append(np.ascontiguousarray(canvas[:(oh + sh - 1) // sh, :(ow + sw - 1) // sw]))
        out.append(planes)
    return out


def _photos(name):
    return [(tiles, rows, cols, ow, oh) for (rows, cols, _, _, ow, oh, _), tiles in zip(ALBUMS[name][0], _all_streams()[name])]


_LIVE = {}


def _album(name):
    """the album `name`, decoded once and shared by the tests that only read it"""
    if name not in _LIVE:
        a = Album(_photos(name))
        a.run()
        a.status()
        _LIVE[name] = a
    return _LIVE[name]


@pytest.fixture(scope="module", autouse=True)
def _free_albums():
    yield
    for a in _LIVE.values():
        a.free()
    _LIVE.clear()


def _nclx(name, p):
    vui = ALBUMS[name][0][p][6]
    return (vui["vui_primaries"], vui["vui_transfer"], vui["vui_matrix"], vui["vui_full_range"])


def _color_convert(planes, cf, bits, nclx, out_chroma):
    """hipdec_color_convert of the planes uploaded as a ColorImage of their own chroma format, nearest-neighbour chroma: rows of (h, w * bytes per pixel)"""
    L = _lib()
    h, w = planes[0].shape
    img = ColorImage()
    img.width, img.height, img.chroma, img.bit_depth, img.on_device = w, h, cf, bits, 0
    keep = [np.ascontiguousarray(q) for q in planes]
    for c, q in enumerate(keep):
        img.plane[c], img.stride[c] = q.ctypes.data, q.strides[0]
    bpp = {10: 3, 11: 4, 14: 6}[out_chroma]
    out = np.empty((h, w * bpp), np.uint8)
    n = Nclx(1, *nclx)
    check(L.hipdec_color_convert(C.byref(img), C.byref(n), out_chroma, 1, 0, out.ctypes.data, w * bpp, 0))
    return out


def _assert_planes(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, c, g.shape, w.shape)
        assert np.array_equal(g, w), (what, "plane %d" % c, int((g != w).sum()))


@pytest.mark.parametrize("name", ["mixed8", "mixed10", "mono", "422", "444", "clipped"])
def test_canvases_are_the_oracle_tiles_pasted_and_clipped(name):
    photos, bits, cf = ALBUMS[name]
    a = _album(name)
    want = expected_canvases(name)
    assert a.n == len(photos)
    for p, (rows, cols, tw, th, ow, oh, _) in enumerate(photos):
        d = a.info(p)
        assert (d["width"], d["height"], d["coded_width"], d["coded_height"]) == (ow, oh, cols * tw, rows * th)
        assert (d["bit_depth_luma"], d["chroma_format_idc"]) == (bits, cf)
        if cf:
            assert (d["chroma_width"], d["chroma_height"]) == want[p][1].shape[::-1]
            assert (d["colour_primaries"], d["transfer_characteristics"], d["matrix_coeffs"], d["full_range_flag"]) == _nclx(name, p)
        _assert_planes(a.planes(p), want[p], (name, p))
        ptr, stride = a.canvas_plane(p, 0)
        assert ptr and stride % 256 == 0 and stride >= ow * (2 if bits > 8 else 1)


def test_monochrome_album_has_no_chroma_planes():
    a = _album("mono")
    for c in (1, 2):
        with pytest.raises(HipDecError, match="monochrome"):
            a.canvas_plane(0, c)
        buf = np.empty((64, 64), np.uint8)
        with pytest.raises(HipDecError, match="monochrome"):
            check(a._lib.hipdec_album_read_plane(a._h, 0, c, buf.ctypes.data, 64))


@pytest.mark.parametrize("name", ["mixed8", "mixed10", "422", "clipped"])
def test_same_pixels_as_the_grid_path(name):
    """(hipdec_grid_create takes an output that clips a whole tile column away: so does the album, with the same pixels)"""
    photos, bits, cf = ALBUMS[name]
    a = _album(name)
    for p, ((rows, cols, tw, th, ow, oh, _), tiles) in enumerate(zip(photos, _all_streams()[name])):
        g = GridDecoderC(tiles, GridLayout(rows, cols, tw, th, ow, oh, bit_depth=bits), [0])
        try:
            g.decode()
            g.wait()
            _assert_planes(a.planes(p), g.planes(), (name, p))
        finally:
            g.free()


@pytest.mark.parametrize("name,out_chroma", [("mixed8", 10), ("mixed8", 11), ("mixed10", 10), ("mixed10", 11), ("mixed10", 14), ("422", 10), ("444", 11),
                                             ("mono", 10), ("clipped", 10)])
def test_rgb_at_full_size_is_color_convert_of_the_expected_canvas(name, out_chroma):
    photos, bits, cf = ALBUMS[name]
    a = _album(name)
    a.alloc_rgb(out_chroma)
    a.to_rgb_all()
    a.status()
    for p, planes in enumerate(expected_canvases(name)):
        want = _color_convert(planes, cf, bits, _nclx(name, p), out_chroma)
        got = a.rgb(p)
        assert got.shape == want.shape and np.array_equal(got, want), (name, out_chroma, p, int((got != want).sum()))
        if (bits, cf, out_chroma) == (8, 1, 10) and _nclx(name, p)[3] == 1:      # 8-bit full-range 4:2:0: the colour oracle as well
            h, w = planes[0].shape
            assert np.array_equal(got, orc.color_420_to_rgb24(planes[0], planes[1], planes[2], _nclx(name, p)).reshape(h, -1)), (name, p)


SCALED_SIZES = {"mixed8": [(50, 23), (100, 90), (64, 65)], "mixed10": [(50, 23), (100, 90), (64, 65)], "444": [(33, 23), (150, 70)]}   # (the second: an up-scale)


@pytest.mark.parametrize("filt", [SCALE_NEAREST, SCALE_BOX])
@pytest.mark.parametrize("name,out_chroma", [("mixed8", 10), ("mixed8", 11), ("mixed10", 14), ("444", 10)])
def test_scaled_rgb_is_the_batch_definition_over_the_expected_canvas(name, out_chroma, filt):
    L = _lib()
    photos, bits, cf = ALBUMS[name]
    a = _album(name)
    sizes = SCALED_SIZES[name]
    a.alloc_rgb_scaled(sizes, out_chroma)
    a.to_rgb_scaled_all(filt)
    a.status()
    bpp = {10: 3, 11: 4, 14: 6}[out_chroma]
    for p, (planes, (ow, oh)) in enumerate(zip(expected_canvases(name), sizes)):
        h, w = planes[0].shape
        if filt == SCALE_BOX:      # every plane with its own size to ow x oh, then the colour conversion of the 4:4:4 image
            want = _color_convert_444(L, [box_plane(q, ow, oh) for q in planes], cf, bits, _nclx(name, p), out_chroma)
        else:                      # the full-size rows, then pixel (x, y) <- (x * w / ow, y * h / oh)
            full = _color_convert(planes, cf, bits, _nclx(name, p), out_chroma)
            want = nearest_V(full.reshape(h, w, bpp), (0, 0, w, h), ow, oh).reshape(oh, ow * bpp)
        got = a.rgb_scaled(p)
        assert got.shape == want.shape and np.array_equal(got, want), (name, out_chroma, filt, p, int((got != want).sum()))


# photo 2 named twice; a window across the tile border of photo 2 (x = 64, y = 64) at odd left / top; flipped entries; whole photos
ENTRIES = [(0, 0, 0, 0, 0, 0), (2, 33, 31, 70, 67, 0), (2, 0, 0, 0, 0, 1), (0, 71, 47, 61, 40, 1), (1, 3, 5, 20, 30, 0)]


@pytest.mark.parametrize("filt", [SCALE_NEAREST, SCALE_BOX])
@pytest.mark.parametrize("name,dtype", [("mixed8", "uint8"), ("mixed8", "bfloat16"), ("mixed10", "uint8"), ("mixed10", "bfloat16")])
def test_tensor_is_the_batch_definition_over_the_expected_canvas(name, dtype, filt):
    L = _lib()
    photos, bits, cf = ALBUMS[name]
    a = _album(name)
    canv = expected_canvases(name)
    native = bits > 8 and dtype != "uint8"
    fulls = []
    for p, planes in enumerate(canv):
        h, w = planes[0].shape
        rows = _color_convert(planes, cf, bits, _nclx(name, p), 14 if native else 10)
        fulls.append((rows.view(np.uint16) if native else rows).reshape(h, w, 3))
    wins = [(e[1], e[2], e[3], e[4]) if e[3] else (0, 0, photos[e[0]][4], photos[e[0]][5]) for e in ENTRIES]
    ow, oh = 50, 34
    if filt == SCALE_NEAREST:
        Vs = [nearest_V(fulls[e[0]], win, ow, oh) for e, win in zip(ENTRIES, wins)]
    else:
        Vs = [box_V(L, canv[e[0]], cf, bits, _nclx(name, e[0]), win, ow, oh, native) for e, win in zip(ENTRIES, wins)]
    for layout in ("NCHW", "NHWC"):
        want = expected_tensor(Vs, [e[5] for e in ENTRIES], dtype, layout, SCALE, BIAS)
        got = run_tensor(a, (ow, oh), ENTRIES, dtype, layout, filt)
        assert np.array_equal(got, want), (name, dtype, layout, filt, int((got != want).sum()))
    # entries == NULL: entry p is the whole of photo p
    whole = [(0, 0, q[4], q[5]) for q in photos]
    if filt == SCALE_NEAREST:
        Vs = [nearest_V(fulls[p], win, ow, oh) for p, win in enumerate(whole)]
    else:
        Vs = [box_V(L, canv[p], cf, bits, _nclx(name, p), win, ow, oh, native) for p, win in enumerate(whole)]
    want = expected_tensor(Vs, [0] * len(photos), dtype, "NCHW", SCALE, BIAS)
    assert np.array_equal(run_tensor(a, (ow, oh), None, dtype, "NCHW", filt), want), (name, dtype, "NULL entries", filt)


def test_counters_and_a_repeated_run():
    """album_stats rises by (1, photos, 1) per create + run; the tensor counters of hipdec_batch_to_tensor / hipdec_image_to_tensor and the decoder
    path's coalescer counters are not the album's and stay; a second run gives the same canvases"""
    before, tensors, coalesced = album_stats(), decoder.tensor_stats(), decoder.coalesce_stats()
    a = Album(_photos("mixed8"))
    try:
        assert album_stats() == (before[0] + 1, before[1] + 3, before[2])
        a.run()
        a.status()
        assert album_stats() == (before[0] + 1, before[1] + 3, before[2] + 1)
        first = [a.planes(p) for p in range(a.n)]
        run_tensor(a, (20, 10), None, "uint8", "NHWC", SCALE_BOX)
        assert album_stats() == (before[0] + 1, before[1] + 3, before[2] + 1)
        assert decoder.tensor_stats() == tensors and decoder.coalesce_stats() == coalesced
        a.run()
        a.status()
        assert album_stats() == (before[0] + 1, before[1] + 3, before[2] + 2)
        for p, want in enumerate(expected_canvases("mixed8")):
            _assert_planes(a.planes(p), first[p], ("second run", p))
            _assert_planes(a.planes(p), want, ("second run against the oracle", p))
        assert a.paste_timing_us() >= 0.0
    finally:
        a.free()


def test_creation_refuses_geometry_the_tiles_do_not_support():
    tiles = _all_streams()["mixed8"]
    for photos, text in (([(tiles[0], 2, 3, 217, 90)], "exceeds the tiled area"),
                         ([(tiles[0], 2, 3, 200, 97)], "exceeds the tiled area"),
                         ([(tiles[0][:5] + tiles[1], 2, 3, 200, 90)], "tiles differ in size"),
                         ([(tiles[0], 2, 3, 200, 90), (_all_streams()["mixed10"][1], 1, 1, 64, 64)], "mixes 8-bit and >8-bit"),      # (the batch's own rule)
                         ([(tiles[0], 2, 3, 200, 90), (_all_streams()["444"][1], 1, 2, 99, 63)], "bit depth or chroma format")):
        with pytest.raises(HipDecError, match=text):
            Album(photos)
    with pytest.raises(HipDecError, match="max_image_size_pixels"):
        Album(_photos("mixed8"), max_image_size_pixels=72 * 48)      # every tile fits, the first photo's output of 200 x 90 does not
