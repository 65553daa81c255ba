"""Composed tensor output on the device: hipdec_batch_to_tensor_composed / hipdec_album_to_tensor_composed (mosaic, CutMix, contact sheets: several entries
share a canvas, later entries lie on top, the fill element wherever no entry's region lies, an optional mask; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code:
  owned    the expected canvas is NumPy painter's order: what the EXISTING hipdec_batch_to_tensor_oriented (run_oriented of tests/test_oriented_gpu.py)
           writes for every entry at its place's size, pasted WITH CLIPPING to place n clip n canvas, in entry order - a later paste overwrites an earlier.
  unowned  the fill elements of tests/test_placed_gpu.py (fill_elements: the header's definition in NumPy float32).
  mask     1 where nothing was pasted, 0 elsewhere.
The tensor and the mask lie 256 bytes (plus, in one test, one element) inside buffers pre-filled with 0xA5, as in tests/test_framed_gpu.py: the bytes in
front of and behind them must come back untouched, and since every element is compared no 0xA5 element survives where another is expected (expected_composed
asserts that no expected or fill element is that pattern).

Runs on the MI355X (`-m gpu`) and, unchanged, through tests/test_composed_emu.py against the library compiled for the host."""
import ctypes as C
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album
from test_framed_gpu import GUARD, run_framed
from test_oriented_gpu import CODES, SMALL, _b, _free_batches, _hwc, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_placed_gpu import BITS, ES, FILTERS, POISON, TEN_BIT, WHOLE, _fill, fill_elements
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits

pytestmark = pytest.mark.gpu

ALL = (0, 0, 0, 0)                                       # a clip of the whole canvas


def region(tile, canvas):
    """(x0, y0, x1, y1) of place n clip n canvas, in canvas coordinates"""
    _, (x, y, w, h), clip = tile
    r = [max(x, 0), max(y, 0), min(x + w, canvas[0]), min(y + h, canvas[1])]
    if clip is not None and tuple(clip) != ALL:
        cx, cy, cw, ch = clip
        r = [max(r[0], cx), max(r[1], cy), min(r[2], cx + cw), min(r[3], cy + ch)]
    return tuple(r)


def expected_composed(b, canvas, nc, entries, codes, tiles, dtype, layout, filt, fill=None, domain="component"):
    """(canvases, mask, owner): the fill elements, and painted over them in entry order what the existing oriented call writes at every place's size"""
    n = len(tiles)
    entries = [(i,) + WHOLE for i in range(n)] if entries is None else [tuple(e) + (0,) * (6 - len(e)) for e in entries]
    codes = (0,) * n if codes is None else tuple(codes)
    W, H = canvas
    exp = np.empty((nc, H, W, 3), BITS[dtype])
    owner = np.full((nc, H, W), -1, np.int64)
    fe = fill_elements(fill, domain, dtype)
    poison = int.from_bytes(bytes([POISON]) * ES[dtype], "little")
    assert not (fe == poison).any(), "a fill element is the poison pattern: an unwritten pixel would pass"
    exp[...] = fe
    samples = {}
    for size in sorted(set(tuple(t[1][2:]) for t in tiles)):
        idx = [e for e in range(n) if tuple(tiles[e][1][2:]) == size]
        S = _hwc(run_oriented(b, size, [entries[e] for e in idx], [codes[e] for e in idx], dtype, layout, filt), layout)
        if dtype != "uint8":
            assert not (S == poison).any(), "an expected element is the poison pattern"
        for k, e in enumerate(idx):
            samples[e] = S[k]
    for e in range(n):
        cv, (x, y, w, h), _ = tiles[e]
        x0, y0, x1, y1 = region(tiles[e], canvas)
        assert x0 < x1 and y0 < y1, tiles[e]
        exp[cv, y0:y1, x0:x1] = samples[e][y0 - y:y1 - y, x0 - x:x1 - x]
        owner[cv, y0:y1, x0:x1] = e
    return (exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp), (owner < 0).astype(np.uint8), owner


def _view(buf, offset, nbytes):
    v = DeviceBuffer.__new__(DeviceBuffer)
    v.ptr, v.nbytes, v.free = buf.ptr + offset, nbytes, lambda: None
    return v


def _untouched(buf, offset, nbytes, what):
    raw = buf.to_numpy((buf.nbytes,), np.uint8)
    assert (raw[:offset] == POISON).all(), "bytes in front of the %s were written" % what
    assert (raw[offset + nbytes:] == POISON).all(), "bytes behind the %s were written" % what


def run_composed(b, canvas, nc, entries, codes, tiles, dtype, layout, filt, fill=None, domain="component", mask=None, shift=0):
    """the composed call into poisoned buffers with 256 guard bytes on either side of the tensor and of the mask (shift: further bytes in front of the
    tensor); returns the tensor's bit patterns (and the mask)"""
    nbytes = nc * 3 * canvas[0] * canvas[1] * ES[dtype]
    buf = DeviceBuffer.from_numpy(np.full(nbytes + 2 * GUARD + shift, POISON, np.uint8))
    out = _view(buf, GUARD + shift, nbytes)
    mbytes = nc * canvas[0] * canvas[1]
    mbuf = DeviceBuffer.from_numpy(np.full(mbytes + 2 * GUARD + 1, POISON, np.uint8)) if mask else None
    assert b.to_tensor_composed(canvas, tiles, entries, n_canvases=nc, orientations=codes, fill=fill, fill_domain=domain, mask=_view(mbuf, GUARD + 1, mbytes) if mask else None,
                                filter=filt, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out) is out
    got = as_bits(b.tensor_to_host())
    assert got.shape == ((nc, 3, canvas[1], canvas[0]) if layout == "NCHW" else (nc, canvas[1], canvas[0], 3))
    _untouched(buf, GUARD + shift, nbytes, "tensor")
    if not mask:
        return got
    m = b.tensor_mask_to_host()
    _untouched(mbuf, GUARD + 1, mbytes, "mask")
    return got, m


def check(b, canvas, nc, entries, codes, tiles, dtype, layout, filt, fill=114, domain="component", mask=False, shift=0):
    got = run_composed(b, canvas, nc, entries, codes, tiles, dtype, layout, filt, fill, domain, mask, shift)
    exp, emask, owner = expected_composed(b, canvas, nc, entries, codes, tiles, dtype, layout, filt, fill, domain)
    if mask:
        got, m = got
        assert np.array_equal(m, emask), (canvas, tiles)
    bad = [(c, int((got[c] != exp[c]).sum())) for c in range(nc) if not np.array_equal(got[c], exp[c])]
    assert not bad, (canvas, tiles, dtype, layout, filt, bad)
    return owner


E0 = (0,) + WHOLE


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cw", (24, 25))
def test_two_entries_abut_at_every_column_of_a_group_and_a_block(cw, dtype, layout):
    """canvas x - 8 holds two entries that abut at column x = 8 .. 13: the first is the whole-canvas sample clipped to the columns left of x, the second a
    sample of its own placed from x on; codes 0, 1, 4 and 7.  The inner edge cuts a 4-pixel group and a 16-byte block at every position, and in every
    other canvas the second entry starts one row lower, so that a run of fill remains above it"""
    tiles, codes = [], []
    for k, x in enumerate(range(8, 14)):
        tiles += [(k, (0, 0, cw, 9), (0, 0, x, 9)), (k, (x, k & 1, cw - x, 9 - (k & 1)), ALL)]
        codes += [(0, 1, 4, 7)[k % 4], (0, 1, 4, 7)[(k + 1) % 4]]
    for filt in (SCALE_BOX, SCALE_NEAREST, SCALE_BILINEAR):
        check(_b(SMALL), (cw, 9), 6, [E0] * 12, codes, tiles, dtype, layout, filt, fill=(3, 114, 250))


@pytest.mark.parametrize("filt", FILTERS)
def test_a_later_entry_punches_a_hole_into_an_earlier_one(filt):
    """four pieces around the hole, for all eight codes; the earlier entry leaves the canvas on two sides and fill remains on the other two"""
    tiles, codes = [], []
    for k in range(8):
        tiles += [(k, (-3, -2, 30, 19), ALL), (k, (10, 6, 12, 8), ALL)]
        codes += [CODES[k], CODES[(k + 3) % 8]]
    b = _b(SMALL)
    s0 = decoder.composed_stats()
    check(b, (33, 21), 8, [E0] * 16, codes, tiles, "uint8", "NCHW", filt, mask=True)
    s1 = decoder.composed_stats()
    assert tuple(a - c for a, c in zip(s1, s0)) == (1, 16, 8 * 5, 0, 1)          # four pieces and the hole's own, per canvas
    check(b, (33, 21), 8, [E0] * 16, codes, tiles, "float16", "NHWC", filt, mask=True)


@pytest.mark.parametrize("domain", ("component", "element"))
@pytest.mark.parametrize("dtype,layout", [("uint8", "NHWC"), ("float32", "NCHW"), ("bfloat16", "NCHW")])
def test_mosaic_of_four_around_odd_and_even_centres(dtype, layout, domain):
    """samples larger and smaller than their quadrants: the large ones are clipped by the quadrant, the small ones leave grey between them and the edge"""
    sizes = [(30, 20), (12, 9), (25, 22), (10, 30)]
    tiles = decoder.mosaic_tiles((40, 30), (17, 13), sizes, 0) + decoder.mosaic_tiles((40, 30), (20, 14), sizes[::-1], 1)
    assert tiles[0] == (0, (17 - 30, 13 - 20, 30, 20), (0, 0, 17, 13)) and tiles[3] == (0, (17, 13, 10, 30), (17, 13, 23, 17))
    entries = [E0, (0, 1, 3, 35, 21, 0), (0, 5, 7, 33, 17, 1), E0] * 2
    for filt in (SCALE_BOX, SCALE_BILINEAR):
        check(_b(SMALL), (40, 30), 2, entries, (0, 0, 4, 2, 0, 6, 0, 0), tiles, dtype, layout, filt, fill=(3, 114, 250), domain=domain, mask=True)


@pytest.mark.parametrize("gap", (1, 3))
def test_contact_sheet_of_three_by_two_with_an_empty_cell(gap):
    """five letterboxed thumbnails in six cells: fill runs between the cells in every row, beside and above the thumbnails, and over the whole last cell;
    hipdec_compose_visible_area against a NumPy count"""
    entries = [E0, (0, 1, 3, 35, 21, 0), (0, 5, 7, 33, 17, 1), E0, (0, 37, 11, 31, 29, 0)]
    codes = (0, 0, 1, 3, 6)
    shown = [decoder.oriented_size(c, e[3] or 72, e[4] or 40) for e, c in zip(entries, codes)]
    tiles = decoder.sheet_tiles((3, 2), (11, 8), shown, gap=gap)
    canvas = decoder.sheet_size((3, 2), (11, 8), gap)
    assert canvas == (33 + 2 * gap, 16 + gap) and tiles[4][2] == (11 + gap, 8 + gap, 11, 8)
    b = _b(SMALL)
    for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_BICUBIC), ("float32", "NHWC", SCALE_NEAREST)):
        owner = check(b, canvas, 1, entries, codes, tiles, dtype, layout, filt, fill=(255, 255, 255) if dtype == "uint8" else 114, mask=True)
    assert decoder.compose_visible_area(canvas, tiles) == [int((owner == e).sum()) for e in range(5)]
    assert (owner[0, :, 11:11 + gap] == -1).all() and (owner[0, 8:8 + gap] == -1).all() and (owner[0, 8 + gap:, 22 + 2 * gap:] == -1).all()


def test_cutmix_over_three_canvases():
    boxes = [(5, 3, 9, 7), (-4, -2, 12, 10), (20, 10, 10, 10)]                   # inside, over the top-left corner, over the bottom-right one
    tiles, order = decoder.cutmix_tiles((24, 16), boxes)
    assert order == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)] and tiles[3] == (1, (0, 0, 24, 16), (-4, -2, 12, 10))
    windows = [E0, (0, 3, 1, 69, 39, 1), (0, 37, 11, 31, 29, 0)]
    entries = [windows[(k + role) % 3] for k, role in order]
    area = decoder.compose_visible_area((24, 16), tiles)
    assert [area[2 * k + 1] for k in range(3)] == [63, 64, 24] and all(area[2 * k] + area[2 * k + 1] == 24 * 16 for k in range(3))
    c0 = decoder.composed_stats()
    for dtype, layout, filt in (("uint8", "NCHW", SCALE_BOX), ("float16", "NHWC", SCALE_BILINEAR)):
        owner = check(_b(SMALL), (24, 16), 3, entries, (0, 4, 0, 0, 5, 1), tiles, dtype, layout, filt)
    c1 = decoder.composed_stats()
    assert c1[4] == c0[4] and not (owner < 0).any()                              # every pixel is owned: no cover launch
    assert [int((owner == e).sum()) for e in range(6)] == area


def test_a_canvas_without_entries_and_a_fully_hidden_entry():
    b = _b(SMALL)
    tiles = [(0, (5, 4, 6, 5), ALL), (2, (-1, 2, 9, 9), ALL), (0, (0, 0, 20, 12), ALL), (0, (18, 10, 9, 9), ALL)]        # entry 0 lies under entry 2
    s0 = decoder.composed_stats()
    owner = check(b, (20, 12), 3, [E0] * 4, (0, 1, 2, 3), tiles, "float32", "NCHW", SCALE_BOX, mask=True)
    s1 = decoder.composed_stats()
    assert (owner[1] == -1).all() and not (owner == 0).any()
    # entry 2 is cut by entry 3's corner into two pieces
    assert tuple(a - c for a, c in zip(s1, s0)) == (1, 4, 1 + 2 + 1, 1, 1)
    assert decoder.compose_visible_area((20, 12), tiles, 3) == [0, 8 * 9, 20 * 12 - 4, 4]
    check(b, (20, 12), 3, [E0] * 4, (0, 1, 2, 3), tiles, "uint8", "NHWC", SCALE_BILINEAR, fill=(1, 2, 3))


@pytest.mark.parametrize("dtype,layout", [("uint8", "NCHW"), ("float16", "NHWC"), ("float32", "NCHW")])
def test_seventeen_small_regions_scattered_in_one_canvas(dtype, layout):
    """2 x 2 regions cut out of 9 x 7 samples, five or six in one row of the canvas and their rows staggered - a band of the cover table holds many
    intervals, and the last region abuts the first and merges with it - and a second canvas whose regions are 2 x 2 samples themselves"""
    at = [((k * 7) % 38, (k % 3) * 2 + (k % 2)) for k in range(16)] + [(2, 1)]
    tiles = [(0, (x - 3, y - 2, 9, 7), (x, y, 2, 2)) for x, y in at] + [(1, (x, 28 - y, 2, 2), ALL) for x, y in at]
    codes = [k % 8 for k in range(34)]
    for filt in (SCALE_BOX, SCALE_NEAREST):
        owner = check(_b(SMALL), (40, 30), 2, [E0] * 34, codes, tiles, dtype, layout, filt, fill=(10, 114, 200), mask=True)
    assert max(len(set(owner[0, y]) - {-1}) for y in range(30)) >= 4              # a row with at least four intervals


@pytest.mark.parametrize("filt", FILTERS)
def test_three_entries_overlap_in_a_staircase(filt):
    tiles = [(0, (0, 0, 20, 14), ALL), (0, (8, 5, 20, 14), ALL), (0, (16, 10, 20, 14), ALL), (1, (16, 10, 20, 14), ALL), (1, (8, 5, 20, 14), ALL), (1, (0, 0, 20, 14), ALL)]
    for dtype, layout in (("uint8", "NHWC"), ("bfloat16", "NCHW")):
        check(_b(SMALL), (37, 25), 2, [E0, (0, 5, 7, 33, 17, 1), (0, 1, 3, 35, 21, 0)] * 2, (0, 3, 5, 6, 1, 4), tiles, dtype, layout, filt, mask=True)


def test_one_entry_per_canvas_gives_the_framed_calls_bytes():
    """... and launches no cover kernel when no canvas has a margin and no mask is asked for"""
    b = _b(SMALL)
    e, codes = [E0, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)], (1, 6, 0)
    margins = [(-1, -1, 18, 11), (-4, 0, 16, 9), (-30, -20, 80, 50)]               # canvas 1 has a margin
    covered = [(-1, -1, 18, 11), (0, 0, 16, 9), (-30, -20, 80, 50)]
    for frames, launches in ((margins, 1), (covered, 0)):
        tiles = [(k, f, ALL) for k, f in enumerate(frames)]
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_NEAREST), ("float16", "NCHW", SCALE_BICUBIC), ("float32", "NCHW", SCALE_BOX)):
            want = run_framed(b, (16, 9), e, codes, frames, dtype, layout, filt, fill=7)
            s0, f0, p0 = decoder.composed_stats(), decoder.framed_stats(), decoder.placed_stats()
            got = run_composed(b, (16, 9), 3, e, codes, tiles, dtype, layout, filt, fill=7)
            s1, f1, p1 = decoder.composed_stats(), decoder.framed_stats(), decoder.placed_stats()
            assert np.array_equal(got, want), (frames, dtype, layout, filt)
            assert tuple(a - c for a, c in zip(s1, s0)) == (1, 3, 3, 0, launches)
            assert f1 == f0 and p1 == p0                                           # neither the framed nor the placed surface counts a composed call
    s0 = decoder.composed_stats()
    _, m = run_composed(b, (16, 9), 3, e, codes, [(k, f, ALL) for k, f in enumerate(covered)], "uint8", "NHWC", SCALE_NEAREST, mask=True)
    assert not m.any() and decoder.composed_stats()[4] - s0[4] == 1                # (the mask alone takes the cover launch)


@pytest.mark.parametrize("dtype,layout,cw", [("uint8", "NCHW", 24), ("float16", "NCHW", 24), ("bfloat16", "NHWC", 24), ("float32", "NCHW", 24), ("uint8", "NHWC", 25)])
def test_a_tensor_that_starts_one_element_behind_a_16_byte_boundary(dtype, layout, cw):
    tiles = [(0, (2, 1, 9, 5), ALL), (0, (13, 3, 30, 13), (13, 3, 7, 4)), (1, (-5, -3, 16, 9), ALL), (1, (cw - 4, 2, 4, 7), ALL)]
    for filt in (SCALE_BOX, SCALE_BILINEAR):
        check(_b(SMALL), (cw, 9), 2, [E0] * 4, (0, 1, 4, 7), tiles, dtype, layout, filt, fill=(3, 114, 250), mask=True, shift=ES[dtype])


def test_a_ten_bit_source_with_a_component_fill_above_255():
    b = _b(TEN_BIT)
    tiles = decoder.mosaic_tiles((19, 14), (9, 6), [(12, 9), (7, 4), (5, 11), (30, 19)])
    for filt in (SCALE_BOX, SCALE_NEAREST):
        check(b, (19, 14), 1, [E0] * 4, (0, 3, 5, 6), tiles, "float16", "NCHW", filt, fill=(1023, 512, 256), mask=True)
    check(b, (19, 14), 1, [E0] * 4, (0, 3, 5, 6), tiles, "uint8", "NHWC", SCALE_BILINEAR, fill=255)


def test_album_form_with_two_photos():
    from test_album_gpu import _photos
    a = Album(_photos("444"))                              # photos of 131 x 91 and 99 x 63
    try:
        a.run()
        a.status()
        entries, codes = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 71, 57, 0), (1, 1, 1, 63, 61, 0)], (3, 0, 6, 5)
        tiles = [(0, (-4, -16, 48, 69), ALL), (0, (21, -5, 38, 36), (25, 0, 15, 20)), (1, (-11, 2, 37, 48), ALL), (1, (30, 20, 62, 40), ALL)]
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_NEAREST), ("uint8", "NCHW", SCALE_BILINEAR)):
            check(a, (40, 36), 2, entries, codes, tiles, dtype, layout, filt, fill=(114, 114, 0), mask=True)
    finally:
        a.free()


def test_refusals_that_need_the_handle_leave_the_output_untouched():
    from test_scale_gpu import VUI_FULL, _batch, _still
    L = _lib()
    b = _b(SMALL)
    canvas = (16, 8)
    nbytes = 2 * 16 * 8 * 3 * 4
    out = DeviceBuffer.from_numpy(np.full(nbytes + 2 * GUARD, POISON, np.uint8))
    mask = DeviceBuffer.from_numpy(np.full(2 * 16 * 8 + 2 * GUARD, POISON, np.uint8))
    good = [(0, (-3, -2, 30, 14), ALL), (1, (0, 0, 16, 8), (2, 2, 5, 5)), (1, (4, 1, 8, 4), ALL)]

    def call(dtype="uint8", tiles=good, entries=[E0] * 3, fill=None, codes=(0, 1, 2), handle=b._h, room=nbytes, filt=SCALE_BOX, nc=2, fn=L.hipdec_batch_to_tensor_composed):
        desc = decoder.tensor_desc(canvas, dtype, "NCHW", filt, SCALE, BIAS)
        return fn(handle, C.byref(desc), decoder.tensor_entries(entries) if entries else None, (C.c_int * 3)(*codes), decoder.tensor_tiles(tiles),
                  C.byref(fill) if fill is not None else None, mask.ptr + GUARD, 3, nc, out.ptr + GUARD, room, None)

    _refused(L, call(entries=[E0, E0, (1,) + WHOLE]), -1)                              # the batch has one item
    assert b"entry 2" in L.hipdec_last_error(), L.hipdec_last_error()
    _refused(L, call(entries=None), -1)                                                # three entries without a list, one item
    _refused(L, call(entries=[E0, E0, (0, 70, 0, 8, 8, 0)]), -1)                       # a window that leaves the picture
    assert b"entry 2" in L.hipdec_last_error()
    _refused(L, call(tiles=[good[0], good[1], (2, (0, 0, 4, 4), ALL)]), -1)            # canvas 2 of 2
    assert b"entry 2" in L.hipdec_last_error()
    _refused(L, call(tiles=[good[0], good[1], (1, (0, 0, 16, 8), (3, 3, 4, 0))]), -1)  # a clip with one zero side
    _refused(L, call(tiles=[good[0], good[1], (1, (0, 0, 4, 4), (8, 0, 4, 4))]), -1)   # place and clip share no pixel
    _refused(L, call(room=2 * 16 * 8 * 3 - 1), -1)
    _refused(L, call(codes=(0, 1, 8)), -1)
    _refused(L, call("float32", fill=_fill((0, 256, 0))), -1)                          # a component fill above the 8-bit source's largest value
    _refused(L, call(handle=None), -1)
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_composed), -1)
    # what the oriented call refuses for a sample of the place's size: bilinear into a float dtype from a 10-bit source is HIPDEC_ERR_UNSUPPORTED
    _refused(L, call("float32", handle=_b(TEN_BIT)._h, filt=SCALE_BILINEAR), -4)
    small = _batch([_still(1, 8, VUI_FULL, (72, 40))], max_image_size_pixels=72 * 40)
    try:
        _refused(L, call(handle=small._h, tiles=[good[0], good[1], (1, (-3, -2, 80, 40), ALL)]), -5)     # place.width * place.height above max_image_size_pixels
        assert b"entry 2" in L.hipdec_last_error()
    finally:
        small.free()
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((out.nbytes,), np.uint8) == POISON).all() and (mask.to_numpy((mask.nbytes,), np.uint8) == POISON).all()
    assert call() == 0                                                                 # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    with pytest.raises(ValueError):
        b.to_tensor_composed(canvas, good[:2], [E0] * 3, dtype="uint8")                # two tiles for three entries


def test_example_host_makes_a_contact_sheet(tmp_path):
    """examples/decode_batch.c --thumb N --sheet COLS ROWS end to end: the 72 x 40 still, displayed with a quarter turn, letterboxed into the first of 2 x 1
    cells of 32 x 32 with 2 pixels between them, white elsewhere, as one uint8 NHWC picture whose byte sum is the expected canvas'; bad COLS / ROWS or too
    many items print the usage"""
    import os
    import subprocess
    import libheif_amd
    from test_scale_gpu import _still
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.abspath(libheif_amd.library_path())
    exe = str(tmp_path / "decode_batch")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    f = tmp_path / "item.hevc"
    f.write_bytes(_still(*SMALL))
    for bad in (["--sheet", "0", "1"], ["--sheet", "2", "-1"], ["--sheet", "2"], ["--sheet"], ["--sheet", "1", "1", str(f), str(f)]):
        r = subprocess.run([exe, "--thumb", "32"] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    r = subprocess.run([exe, "--thumb", "32", "--orient", "5", "--filter", "bilinear", "--sheet", "2", "1", str(f)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    tiles = decoder.sheet_tiles((2, 1), (32, 32), [(40, 72)], gap=2)        # the displayed picture of the 72 x 40 still is 40 x 72
    assert tiles == [(0, (7, 0, 18, 32), (0, 0, 32, 32))]
    exp, _, _ = expected_composed(_b(SMALL), (66, 32), 1, [E0], (5,), tiles, "uint8", "NHWC", SCALE_BILINEAR, fill=255)
    assert "%s: cell 0, 18x32 at (7, 0)\n" % f in r.stdout, r.stdout
    assert "contact sheet 32x66x3 uint8, 2 x 1 cells: 1 pieces, 1 cover launch(es), byte sum %d\n" % int(exp.astype(np.uint64).sum()) in r.stdout, r.stdout
