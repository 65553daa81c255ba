"""Framed tensor output on the device: hipdec_batch_to_tensor_framed / hipdec_album_to_tensor_framed (resize-then-crop and crop-with-padding: the
rectangle of every entry's resized, displayed sample may leave its canvas on any side, only the part on the canvas is computed and written, the fill element
everywhere else, an optional mask; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code, exactly as in tests/test_placed_gpu.py:
  inside   the visible part holds what the EXISTING hipdec_batch_to_tensor_oriented (Batch.to_tensor(..., orientations=)) writes for the same entry at the
           rectangle's size, pasted into a NumPy canvas WITH CLIPPING.  That call is pinned by tests/test_oriented_gpu.py and tests/test_resample_gpu.py.
  outside  the fill elements of tests/test_placed_gpu.py (fill_elements: the header's definition in NumPy float32).
  mask     1 outside the visible part, 0 inside.
The tensor and the mask lie 256 bytes inside buffers pre-filled with 0xA5: the bytes IN FRONT OF them - where a rectangle with a negative offset would
start - and behind them must come back untouched, and since every element is compared no 0xA5 element survives where another is expected (expected_framed
asserts that no expected or fill element is that pattern).

The pieces of work hipdec_framed_stats counts are restated here from the header: box - a column tile of P (96 columns for 8-bit samples, 64 for wider ones;
every rectangle below is up-scaled, so the tile is the cap) x 16 rows, or x 64 / 32 rows for a quarter turn; bilinear / bicubic - 64 columns x 16 rows of P;
nearest - 256 x 4 displayed pixels.

Runs on the MI355X (`-m gpu`) and, for a handful of cases, through tests/test_framed_emu.py against the library compiled for the host."""
import ctypes as C
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album
from test_oriented_gpu import CODES, FORMATS, SMALL, _b, _free_batches, _hwc, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_placed_gpu import BITS, ES, FILTERS, POISON, TEN_BIT, WHOLE, _defaults, _fill, fill_elements, run_placed
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits

pytestmark = pytest.mark.gpu

GUARD = 256


def visible(frame, canvas):
    """(x0, y0, x1, y1) of the rectangle's part on the canvas, in canvas coordinates"""
    x, y, w, h = frame
    return max(x, 0), max(y, 0), min(x + w, canvas[0]), min(y + h, canvas[1])


def expected_framed(b, canvas, entries, codes, frames, dtype, layout, filt, fill=None, domain="component", existing=run_oriented):
    """the canvas of every entry: the fill elements, and pasted into them WITH CLIPPING what the existing oriented call writes at the rectangle's size"""
    n, entries, codes, frames = _defaults(b, canvas, entries, codes, frames)
    W, H = canvas
    exp = np.empty((n, H, W, 3), BITS[dtype])
    fe = fill_elements(fill, domain, dtype)
    poison = int.from_bytes(bytes([POISON]) * ES[dtype], "little")
    assert not (fe == poison).any(), "a fill element is the poison pattern: an unwritten margin would pass"
    exp[...] = fe
    for size in sorted(set(f[2:] for f in frames)):
        idx = [e for e in range(n) if frames[e][2:] == size]
        S = _hwc(existing(b, size, [entries[e] for e in idx], [codes[e] for e in idx], dtype, layout, filt), layout)
        if dtype != "uint8":
            assert not (S == poison).any(), "an expected element is the poison pattern"
        for k, e in enumerate(idx):
            x, y = frames[e][:2]
            x0, y0, x1, y1 = visible(frames[e], canvas)
            assert x0 < x1 and y0 < y1, frames[e]
            exp[e, y0:y1, x0:x1] = S[k][y0 - y:y1 - y, x0 - x:x1 - x]
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def expected_mask(canvas, frames, n):
    m = np.ones((n, canvas[1], canvas[0]), np.uint8)
    for e in range(n):
        x0, y0, x1, y1 = visible(frames[e], canvas)
        m[e, y0:y1, x0:x1] = 0
    return m


def _inside(buf, nbytes):
    """the nbytes behind the first GUARD bytes of buf as a DeviceBuffer that does not own them"""
    v = DeviceBuffer.__new__(DeviceBuffer)
    v.ptr, v.nbytes, v.free = buf.ptr + GUARD, nbytes, lambda: None
    return v


def _guards_untouched(buf, nbytes, what):
    raw = buf.to_numpy((nbytes + 2 * GUARD,), np.uint8)
    assert (raw[:GUARD] == POISON).all(), "bytes in front of the %s were written" % what
    assert (raw[GUARD + nbytes:] == POISON).all(), "bytes behind the %s were written" % what


def run_framed(b, canvas, entries, codes, frames, dtype, layout, filt, fill=None, domain="component", mask=None):
    """the framed call into poisoned buffers with 256 guard bytes on either side of the tensor and of the mask; returns the tensor's bit patterns (and the mask)"""
    n = b.n if entries is None else len(entries)
    nbytes = n * 3 * canvas[0] * canvas[1] * ES[dtype]
    buf = DeviceBuffer.from_numpy(np.full(nbytes + 2 * GUARD, POISON, np.uint8))
    out = _inside(buf, nbytes)
    mbytes = n * canvas[0] * canvas[1]
    mbuf = DeviceBuffer.from_numpy(np.full(mbytes + 2 * GUARD, POISON, np.uint8)) if mask else None
    assert b.to_tensor(canvas, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out, orientations=codes, frames=frames, fill=fill,
                       fill_domain=domain, mask=_inside(mbuf, mbytes) if mask else None) is out
    got = as_bits(b.tensor_to_host())
    assert got.shape == ((n, 3, canvas[1], canvas[0]) if layout == "NCHW" else (n, canvas[1], canvas[0], 3))
    _guards_untouched(buf, nbytes, "tensor")
    if not mask:
        return got
    m = b.tensor_mask_to_host()
    _guards_untouched(mbuf, mbytes, "mask")
    return got, m


def check(b, canvas, entries, codes, frames, dtype, layout, filt, fill=114, domain="component", mask=False):
    got = run_framed(b, canvas, entries, codes, frames, dtype, layout, filt, fill, domain, mask)
    n = b.n if entries is None else len(entries)
    if mask:
        got, m = got
        assert np.array_equal(m, expected_mask(canvas, frames, n)), (canvas, frames)
    exp = expected_framed(b, canvas, entries, codes, frames, dtype, layout, filt, fill, domain)
    bad = [(e, int((got[e] != exp[e]).sum())) for e in range(n) if not np.array_equal(got[e], exp[e])]
    assert not bad, (canvas, frames, dtype, layout, filt, bad)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cw", (24, 25))
def test_every_cut_of_a_four_pixel_group(cw, dtype, layout):
    """x = -1 .. -5 against canvas widths 4k and 4k + 1, for codes 0, 1, 4 and 7 (forward, quarter turn, reversed, reversed quarter turn): the left edge cuts a
    group at every position, the right edge of the 30-wide rectangle cuts one as well"""
    frames = [(x, -1 - (x & 1), 30, 13) for x in range(-1, -6, -1) for _ in range(4)]
    codes = [(0, 1, 4, 7)[k % 4] for k in range(len(frames))]
    for filt in (SCALE_BOX, SCALE_NEAREST, SCALE_BILINEAR):
        check(_b(SMALL), (cw, 9), [(0,) + WHOLE] * len(frames), codes, frames, dtype, layout, filt, fill=(3, 114, 250))


@pytest.mark.parametrize("filt", FILTERS)
def test_all_eight_codes_overhanging_on_all_four_sides(filt):
    e, frames = [(0,) + WHOLE] * 8, [(-19, -11, 70, 44)] * 8
    check(_b(SMALL), (33, 21), e, CODES, frames, "uint8", "NCHW", filt, mask=True)
    check(_b(SMALL), (33, 21), e, CODES, frames, "float16", "NHWC", filt)


@pytest.mark.parametrize("dtype,layout", [("uint8", "NHWC"), ("float32", "NCHW")])
def test_one_side_only_for_each_of_the_four_sides(dtype, layout):
    W, H = 21, 14
    frames = [(-4, 2, 12, 9), (13, 2, 12, 9), (5, -3, 12, 9), (5, 8, 12, 9)]                # left, right, top, bottom
    for filt in FILTERS:
        check(_b(SMALL), (W, H), [(0,) + WHOLE] * 4, (0, 3, 5, 6), frames, dtype, layout, filt, fill=(114, 0, 255), mask=True)


@pytest.mark.parametrize("filt", FILTERS)
def test_a_rectangle_inside_the_canvas_gives_the_placed_calls_bytes(filt):
    b = _b(SMALL)
    e, frames = [(0,) + WHOLE] * 8, [(5, 4, 13, 9)] * 8
    for dtype, layout in (("uint8", "NHWC"), ("bfloat16", "NCHW")):
        s0 = decoder.framed_stats()
        got = run_framed(b, (23, 19), e, CODES, frames, dtype, layout, filt, fill=7)
        s1 = decoder.framed_stats()
        assert np.array_equal(got, run_placed(b, (23, 19), e, CODES, frames, dtype, layout, filt, fill=7))
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 8) and s1[2] > s0[2] and s1[3] == s0[3]     # nothing is skipped


def _pieces(filt, code, size, wide=False, dtype="uint8"):
    """the pieces of work of an unclipped, up-scaled sample of the displayed `size` (the module's docstring)"""
    dw, dh = size
    pw, ph = (dh, dw) if code & 1 else (dw, dh)
    up = lambda n, u: (n + u - 1) // u
    if filt == SCALE_NEAREST:
        return up(dw, 256) * up(dh, 4)
    if filt == SCALE_BOX:
        rb = (32 if wide and dtype != "uint8" else 64) if code & 1 else 16
        return up(pw, 64 if wide else 96) * up(ph, rb)
    return up(pw, 64) * up(ph, 16)


@pytest.mark.parametrize("filt", FILTERS)
def test_whole_tiles_and_bands_clipped_away(filt):
    """a 200 x 70 rectangle at x = -130 leaves column tiles of 64 and 96 columns (and, for a quarter turn, blocks of rows) without a visible pixel, a 70 x 120
    one at y = -100 bands of 16 rows; the nearest kernel's pieces are 256 x 4 pixels: it skips rows of them above and below either canvas"""
    for still, dtype, layout in ((SMALL, "uint8", "NCHW"), (SMALL, "float16", "NHWC"), (TEN_BIT, "uint8", "NHWC")):
        b = _b(still)
        for canvas, frame in (((40, 30), (-130, -20, 200, 70)), ((30, 12), (-20, -100, 70, 120))):
            s0 = decoder.framed_stats()
            check(b, canvas, [(0,) + WHOLE] * 8, CODES, [frame] * 8, dtype, layout, filt, mask=True)
            s1 = decoder.framed_stats()                                               # (the one framed call of check(): the expected value is the oriented call's)
            tiles, skipped = s1[2] - s0[2], s1[3] - s0[3]
            assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, 8)
            assert tiles + skipped == sum(_pieces(filt, c, frame[2:], still is TEN_BIT, dtype) for c in CODES), (filt, frame, tiles, skipped)
            assert tiles > 0 and skipped > 0, (filt, frame, tiles, skipped)


@pytest.mark.parametrize("dtype,layout", [("uint8", "NHWC"), ("float16", "NCHW"), ("float32", "NHWC")])
def test_one_visible_pixel_a_canvas_of_one_row_and_of_one_column(dtype, layout):
    b = _b(SMALL)
    corners = [(-29, -12, 30, 13), (8, -12, 30, 13), (-29, 6, 30, 13), (8, 6, 30, 13)]       # one pixel of the rectangle in each corner of a 9 x 7 canvas
    for filt in FILTERS:
        check(b, (9, 7), [(0,) + WHOLE] * 4, (0, 3, 5, 6), corners, dtype, layout, filt, mask=True)
    for canvas, frames in (((1, 9), [(-7, -2, 30, 13), (0, 3, 1, 4), (-29, 8, 30, 13), (0, -4, 1, 30)]), ((9, 1), [(-7, -5, 30, 13), (2, 0, 5, 1), (8, -12, 30, 13), (-3, 0, 30, 1)])):
        for filt in (SCALE_BOX, SCALE_NEAREST, SCALE_BILINEAR):
            check(b, canvas, [(0,) + WHOLE] * 4, (0, 3, 5, 6), frames, dtype, layout, filt, mask=True)


MIXED_ENTRIES = [(0, 1, 3, 35, 21, 0), (0, 5, 7, 33, 17, 1), (0, 0, 0, 0, 0, 1), (0, 37, 11, 31, 29, 0), (0, 71, 39, 1, 1, 1), (0, 3, 1, 69, 39, 1)]
MIXED_CODES = (1, 5, 4, 3, 6, 0)
MIXED_FRAMES = [(-2, 1, 13, 9), (-40, -30, 100, 60), (7, 5, 33, 6), (1, -9, 5, 31), (19, 10, 1, 1), (3, 2, 13, 9)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype,layout", [("uint8", "NCHW"), ("float16", "NHWC"), ("float32", "NCHW")])
def test_rectangles_windows_flips_and_codes_differ_inside_one_call(dtype, layout, filt):
    check(_b(SMALL), (20, 11), MIXED_ENTRIES, MIXED_CODES, MIXED_FRAMES, dtype, layout, filt, fill=(10, 114, 200), mask=True)


@pytest.mark.parametrize("still", FORMATS, ids=lambda s: "cf%d-%dbit" % (s[0], s[1]))
def test_chroma_formats_and_depths(still):
    b = _b(still)
    e, frames = [(0,) + WHOLE] * 8, [(-6, -3, 30, 19)] * 8
    for filt in (SCALE_NEAREST, SCALE_BOX):
        check(b, (19, 14), e, CODES, frames, "uint8", "NHWC", filt)
        check(b, (19, 14), e, CODES, frames, "float32", "NCHW", filt, fill=255, mask=True)   # 10-bit: float32 holds the native-depth value
    check(b, (19, 14), e, CODES, frames, "uint8", "NCHW", SCALE_BICUBIC)
    if still is TEN_BIT:
        check(b, (19, 14), e, CODES, frames, "float32", "NCHW", SCALE_BOX, fill=(1023, 512, 256))   # a component fill above 255


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_fill_domains(dtype):
    b = _b(SMALL)
    e, codes, frames = [(0,) + WHOLE] * 2, (0, 3), [(-2, 1, 9, 5), (10, -2, 5, 9)]
    for layout in LAYOUTS:
        check(b, (14, 12), e, codes, frames, dtype, layout, SCALE_BOX, (0, 114, 255), "component")
        check(b, (14, 12), e, codes, frames, dtype, layout, SCALE_BOX, (0, 7, 255) if dtype == "uint8" else (1.0 + 2.0 ** -11, -1.5, 70000.0), "element")
        check(b, (14, 12), e, codes, frames, dtype, layout, SCALE_BOX, None)                  # fill None: component 0


def test_album_form_with_two_photos():
    from test_album_gpu import _photos
    a = Album(_photos("444"))                              # photos of 131 x 91 and 99 x 63
    try:
        a.run()
        a.status()
        entries, codes = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 71, 57, 0), (1, 1, 1, 63, 61, 0)], (3, 0, 6, 5)
        frames = [decoder.resize_crop_place(decoder.oriented_size(3, 131, 91), 48, (40, 36)), decoder.resize_crop_place((99, 63), 40, (40, 36)), (-11, 2, 37, 48), (21, -5, 38, 36)]
        assert frames[0] == (-4, -16, 48, 69) and frames[1] == (-11, -2, 62, 40)
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_NEAREST), ("uint8", "NCHW", SCALE_BILINEAR)):
            check(a, (40, 36), entries, codes, frames, dtype, layout, filt, fill=(114, 114, 0), mask=True)
    finally:
        a.free()


def test_a_frame_of_a_clip_through_its_borrowed_batch():
    from libheif_amd.decoder import Clips
    from test_clips_gpu import track
    c = Clips([track("ippp")[0]])                          # 200 x 136, IPPP
    try:
        c.run()
        c.status()
        b = c.batch
        frames = [decoder.resize_crop_place((200, 136), 24, (16, 16)), (-3, 5, 20, 20)]
        assert frames[0] == (-10, -4, 35, 24)
        items = [c.frame(0, f)["item"] for f in (0, c.frame_count(0) - 1)]
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_BILINEAR)):
            check(b, (16, 16), [(items[0],) + WHOLE, (items[1],) + WHOLE], (0, 1), frames, dtype, layout, filt, mask=True)
    finally:
        c.free()


def test_places_null_is_the_oriented_call_byte_for_byte_and_launch_for_launch():
    L = _lib()
    b = _b(SMALL)
    size, entries, codes = (30, 17), [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)], (1, 6, 0)
    for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("bfloat16", "NCHW", SCALE_NEAREST), ("float16", "NCHW", SCALE_BICUBIC)):
        o0 = decoder.oriented_stats()
        want = run_oriented(b, size, entries, codes, dtype, layout, filt)
        o1 = decoder.oriented_stats()
        desc = decoder.tensor_desc(size, dtype, layout, filt, SCALE, BIAS)
        out = DeviceBuffer.from_numpy(np.full(want.nbytes + 2 * GUARD, POISON, np.uint8))
        p1, f1 = decoder.placed_stats(), decoder.framed_stats()
        decoder.check(L.hipdec_batch_to_tensor_framed(b._h, C.byref(desc), decoder.tensor_entries(entries), (C.c_int * 3)(*codes), None, None, None, 3, out.ptr + GUARD,
                                                      want.nbytes, None))
        decoder.check(L.hipdec_stream_synchronize(None))
        o2, p2, f2 = decoder.oriented_stats(), decoder.placed_stats(), decoder.framed_stats()
        assert tuple(a - c for a, c in zip(o2, o1)) == tuple(a - c for a, c in zip(o1, o0))      # the oriented kernels' launches, entries and quarter turns
        assert p2 == p1 and tuple(a - c for a, c in zip(f2, f1)) == (1, 3, 0, 0)                 # no margin launch, no k_frame_* piece of work
        raw = out.to_numpy((want.nbytes + 2 * GUARD,), np.uint8)
        assert np.array_equal(raw[GUARD:GUARD + want.nbytes], want.reshape(-1).view(np.uint8)), (dtype, layout, filt)
        assert (raw[:GUARD] == POISON).all() and (raw[GUARD + want.nbytes:] == POISON).all()


def test_the_margin_kernel_is_one_launch_per_call_or_none():
    b = _b(SMALL)
    e = [(0,) + WHOLE] * 3
    s0 = decoder.placed_stats()
    run_framed(b, (16, 9), e, CODES[:3], [(-1, -1, 18, 11), (-4, 0, 16, 9), (-30, -20, 80, 50)], "uint8", "NHWC", SCALE_NEAREST, fill=7)      # entry 1 has a margin
    s1 = decoder.placed_stats()
    run_framed(b, (16, 9), e, CODES[:3], [(-1, -1, 18, 11), (0, 0, 16, 9), (-30, -20, 80, 50)], "uint8", "NHWC", SCALE_NEAREST, fill=7)       # every canvas is covered
    s2 = decoder.placed_stats()
    _, m = run_framed(b, (16, 9), e, CODES[:3], [(-1, -1, 18, 11), (0, 0, 16, 9), (-30, -20, 80, 50)], "uint8", "NHWC", SCALE_NEAREST, mask=True)
    s3 = decoder.placed_stats()
    assert not m.any()
    assert [s1[2] - s0[2], s2[2] - s1[2], s3[2] - s2[2]] == [1, 0, 1]                          # (the mask alone takes the margin launch)
    assert s3[:2] == s0[:2]                                                                    # none of them is a placed call


def test_refusals_have_a_status_a_message_and_leave_the_output_untouched():
    from test_scale_gpu import VUI_FULL, _batch, _still
    L = _lib()
    b = _b(SMALL)
    canvas = (16, 8)
    nbytes = 2 * 16 * 8 * 3 * 4
    out = DeviceBuffer.from_numpy(np.full(nbytes + 2 * GUARD, POISON, np.uint8))
    mask = DeviceBuffer.from_numpy(np.full(2 * 16 * 8 + 2 * GUARD, POISON, np.uint8))
    good = [(-3, -2, 30, 14), (0, 0, 16, 8)]
    entries = decoder.tensor_entries([(0,) + WHOLE] * 2)

    def call(dtype="uint8", frames=good, fill=None, codes=(0, 1), handle=b._h, room=nbytes, filt=SCALE_BOX, desc=None, fn=L.hipdec_batch_to_tensor_framed):
        desc = desc or decoder.tensor_desc(canvas, dtype, "NCHW", filt, SCALE, BIAS)
        return fn(handle, C.byref(desc), entries, (C.c_int * 2)(*codes), decoder.tensor_places(frames), C.byref(fill) if fill is not None else None, mask.ptr + GUARD, 2,
                  out.ptr + GUARD, room, None)

    for bad in ((1, 1, 0, 4), (1, 1, 8, -1),                                           # a non-positive side
                (-8, 1, 8, 4), (16, 1, 8, 4), (1, -4, 8, 4), (1, 8, 8, 4),             # an empty visible part: the rectangle ends at the canvas' edge on each side
                (-2 ** 24 - 1, 0, 2 ** 24, 4), (0, 2 ** 24 + 1, 4, 4), (0, 0, 2 ** 24 + 1, 4), (0, 0, 4, 2 ** 24 + 1), (2 ** 31 - 1, 0, 2, 2), (-2 ** 31, 0, 2 ** 31 - 1, 2)):
        _refused(L, call(frames=[good[0], bad]), -1)
        assert b"entry 1" in L.hipdec_last_error(), L.hipdec_last_error()
    nan, inf = float("nan"), float("inf")
    for dtype, fill in (("float32", _fill((nan, 0, 0))), ("float32", _fill((0, inf, 0), 1)), ("float16", _fill((114.5, 0, 0))), ("uint8", _fill((0, 256, 0))),
                        ("float32", _fill((0, 256, 0))), ("uint8", _fill(domain=2)), ("uint8", _fill(reserved=1)), ("uint8", _fill((1.5, 0, 0), 1))):
        _refused(L, call(dtype, fill=fill), -1)
    _refused(L, call(room=2 * 16 * 8 * 3 - 1), -1)                                     # out_bytes below hipdec_tensor_bytes
    _refused(L, call(codes=(0, 8)), -1)
    assert b"entry 1" in L.hipdec_last_error()
    _refused(L, call(handle=None), -1)
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_framed), -1)
    _refused(L, call(filt=2), -1)
    # what the oriented call refuses for a sample of the rectangle's size: bilinear into a float dtype from a 10-bit source is HIPDEC_ERR_UNSUPPORTED
    _refused(L, call("float32", handle=_b(TEN_BIT)._h, filt=SCALE_BILINEAR), -4)
    small = _batch([_still(1, 8, VUI_FULL, (72, 40))] * 2, max_image_size_pixels=72 * 40)
    try:
        _refused(L, call(handle=small._h, frames=[good[0], (-3, -2, 80, 40)]), -5)     # pl.width * pl.height above max_image_size_pixels
        assert b"entry 1" in L.hipdec_last_error()
        assert call(handle=small._h, frames=[good[0], (-3, -2, 72, 40)]) == 0
        decoder.check(L.hipdec_stream_synchronize(None))
        decoder.check(L.hipdec_memset(out.ptr, POISON, out.nbytes))
        decoder.check(L.hipdec_memset(mask.ptr, POISON, mask.nbytes))
    finally:
        small.free()
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((out.nbytes,), np.uint8) == POISON).all() and (mask.to_numpy((mask.nbytes,), np.uint8) == POISON).all()
    assert call() == 0                                                                 # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    with pytest.raises(ValueError):
        b.to_tensor(canvas, None, dtype="uint8", frames=good)                          # two rectangles for one entry
    with pytest.raises(ValueError):
        b.to_tensor(canvas, None, dtype="uint8", frames=good[:1], places=good[1:])     # mutually exclusive


def test_example_host_makes_a_resize_then_crop_batch(tmp_path):
    """examples/decode_batch.c --thumb N --frame RESIZE CROP end to end: Resize(24) -> CenterCrop(16) of the 72 x 40 still, displayed with a quarter turn, as one
    uint8 NHWC tensor whose byte sum is the slice's of the oriented call at the resized size; a bad RESIZE or CROP prints the usage"""
    import os
    import subprocess
    import libheif_amd
    from test_scale_gpu import _still
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.abspath(libheif_amd.library_path())
    exe = str(tmp_path / "decode_batch")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    for bad in (["--frame", "0", "16"], ["--frame", "24", "-1"], ["--frame", "24"], ["--frame"]):
        r = subprocess.run([exe, "--thumb", "32"] + bad, capture_output=True, text=True)
        assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    f = tmp_path / "item.hevc"
    f.write_bytes(_still(*SMALL))
    r = subprocess.run([exe, "--thumb", "32", "--orient", "5", "--filter", "bilinear", "--frame", "24", "16", str(f)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    x, y, w, h = decoder.resize_crop_place((40, 72), 24, (16, 16))          # the displayed picture of the 72 x 40 still is 40 x 72
    assert (x, y, w, h) == (-4, -14, 24, 43)
    full = _b(SMALL).to_tensor((w, h), [(0,) + WHOLE], dtype="uint8", layout="NHWC", filter=SCALE_BILINEAR, orientations=(5,), out=DeviceBuffer(w * h * 3))
    want = int(full.to_numpy((h, w, 3), np.uint8)[-y:-y + 16, -x:-x + 16].astype(np.uint64).sum())
    assert "%s: 16x16 of the sample resized to %dx%d, at (%d, %d), byte sum %d\n" % (f, w, h, -x, -y, want) in r.stdout, r.stdout
