"""Placed tensor output on the device: hipdec_batch_to_tensor_placed / hipdec_album_to_tensor_placed (letterbox and pad-to-size: every entry's displayed
sample in a rectangle of a larger canvas, the fill element everywhere else, an optional padding mask; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code:
  inside   the header defines the rectangle's content as what the EXISTING hipdec_batch_to_tensor_oriented writes for the same entry, code, filter, dtype,
           scale and bias at the rectangle's size; that call (Batch.to_tensor(..., orientations=)) is run for the entries of each rectangle size and its
           result pasted into a NumPy canvas.  It is pinned by tests/test_oriented_gpu.py and tests/test_resample_gpu.py.
  outside  the fill element is restated here in NumPy float32 arithmetic: float32(V) * scale + bias - one multiply, one add - for the component domain, the
           value itself for the element domain; .astype(float16) for F16, (bits + 0x7fff + ((bits >> 16) & 1)) >> 16 on the float32 bits for BF16.
  mask     1 outside the rectangle, 0 inside.
The output buffer is 256 bytes longer than the tensor and pre-filled with 0xA5: the tail must come back untouched, and since every element is compared with
its expected value no 0xA5 element survives where another is expected (SCALE / BIAS of tests/test_tensor_gpu.py give no float element of that pattern,
which expected_placed asserts).

Runs on the MI355X (`-m gpu`) and, through tests/test_placed_emu.py, against the library compiled for the host."""
import ctypes as C
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album, TensorFill
from test_oriented_gpu import CODES, FORMATS, SMALL, _b, _free_batches, _hwc, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits, bf16_bits

pytestmark = pytest.mark.gpu

FILTERS = (SCALE_NEAREST, SCALE_BOX, SCALE_BILINEAR, SCALE_BICUBIC)
POISON = 0xA5
ES = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
BITS = {"uint8": np.uint8, "float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}
WHOLE = (0, 0, 0, 0, 0)
TEN_BIT = FORMATS[3]


def fill_elements(fill, domain, dtype, scale=SCALE, bias=BIAS):
    """the three fill elements as bit patterns: the definition of the header in NumPy float32"""
    v = np.broadcast_to(np.asarray(0 if fill is None else fill, np.float32), (3,)).copy()
    if dtype == "uint8":
        return v.astype(np.uint8)
    f = v * scale.astype(np.float32) + bias.astype(np.float32) if domain == "component" else v
    assert f.dtype == np.float32
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16)
    return bf16_bits(f)


def _defaults(b, canvas, entries, codes, places):
    n = b.n if entries is None else len(entries)
    entries = [(i,) + WHOLE for i in range(n)] if entries is None else [tuple(e) + (0,) * (6 - len(e)) for e in entries]
    codes = (0,) * n if codes is None else tuple(codes)
    places = [(0, 0) + tuple(canvas)] * n if places is None else [tuple(p) for p in places]
    return n, entries, codes, places


def expected_placed(b, canvas, entries, codes, places, dtype, layout, filt, fill=None, domain="component", existing=run_oriented):
    """the canvas of every entry: the fill elements, and pasted into them what the existing oriented call writes at the rectangle's size"""
    n, entries, codes, places = _defaults(b, canvas, entries, codes, places)
    W, H = canvas
    exp = np.empty((n, H, W, 3), BITS[dtype])
    fe = fill_elements(fill, domain, dtype)
    assert not (fe == int.from_bytes(bytes([POISON]) * ES[dtype], "little")).any(), "a fill element is the poison pattern: an unwritten margin would pass"
    exp[...] = fe
    for size in sorted(set(p[2:] for p in places)):
        idx = [e for e in range(n) if places[e][2:] == size]
        S = _hwc(existing(b, size, [entries[e] for e in idx], [codes[e] for e in idx], dtype, layout, filt), layout)
        if dtype != "uint8":
            assert not (S == int.from_bytes(bytes([POISON]) * ES[dtype], "little")).any(), "an expected element is the poison pattern"
        for k, e in enumerate(idx):
            x, y, w, h = places[e]
            exp[e, y:y + h, x:x + w] = S[k]
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def expected_mask(canvas, places, n):
    m = np.ones((n, canvas[1], canvas[0]), np.uint8)
    for e in range(n):
        x, y, w, h = places[e] if places is not None else (0, 0) + tuple(canvas)
        m[e, y:y + h, x:x + w] = 0
    return m


def run_placed(b, canvas, entries, codes, places, dtype, layout, filt, fill=None, domain="component", mask=None):
    """the placed call into a poisoned buffer 256 bytes longer than the tensor; returns the tensor's bit patterns (and the mask, where one is asked for)"""
    n = b.n if entries is None else len(entries)
    nbytes = n * 3 * canvas[0] * canvas[1] * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    mbuf = DeviceBuffer.from_numpy(np.full(n * canvas[0] * canvas[1] + 64, POISON, np.uint8)) if mask else None
    places = [(0, 0) + tuple(canvas)] * n if places is None else places      # (places = NULL goes through the C ABI in its own test)
    assert b.to_tensor(canvas, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out, orientations=codes, places=places, fill=fill,
                       fill_domain=domain, mask=mbuf) is out
    got = as_bits(b.tensor_to_host())
    assert got.shape == ((n, 3, canvas[1], canvas[0]) if layout == "NCHW" else (n, canvas[1], canvas[0], 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    if not mask:
        return got
    m = b.tensor_mask_to_host()
    assert (mbuf.to_numpy((m.size + 64,), np.uint8)[m.size:] == POISON).all(), "bytes behind the mask were written"
    return got, m


def check(b, canvas, entries, codes, places, dtype, layout, filt, fill=114, domain="component", mask=False):
    got = run_placed(b, canvas, entries, codes, places, dtype, layout, filt, fill, domain, mask)
    n = b.n if entries is None else len(entries)
    if mask:
        got, m = got
        assert np.array_equal(m, expected_mask(canvas, places, n)), (canvas, places)
    exp = expected_placed(b, canvas, entries, codes, places, dtype, layout, filt, fill, domain)
    bad = [(e, int((got[e] != exp[e]).sum())) for e in range(n) if not np.array_equal(got[e], exp[e])]
    assert not bad, (canvas, places, dtype, layout, filt, bad)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", FILTERS)
def test_all_eight_codes_in_a_rectangle_lower_than_the_canvas(filt, dtype, layout):
    """NCHW with a rectangle height different from the canvas height: what a plane stride derived from the sample gets wrong"""
    check(_b(SMALL), (23, 19), [(0,) + WHOLE] * 8, CODES, [(5, 4, 13, 9)] * 8, dtype, layout, filt, mask=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cw", (24, 25))
def test_vector_store_alignment_of_every_offset_and_width(cw, dtype, layout):
    """x = 0 .. 3 and widths 4k - 1, 4k, 4k + 1 against canvas widths 4k and 4k + 1; codes 0 .. 7 in turn"""
    places = [(x, 1 + (x & 1), w, 5) for x in range(4) for w in (7, 8, 9)]
    codes = [k % 8 for k in range(len(places))]
    for filt in (SCALE_BOX, SCALE_NEAREST, SCALE_BILINEAR):
        check(_b(SMALL), (cw, 9), [(0,) + WHOLE] * len(places), codes, places, dtype, layout, filt, fill=(3, 114, 250))


def test_places_null_is_the_oriented_call_byte_for_byte_and_launch_for_launch():
    L = _lib()
    b = _b(SMALL)
    size, entries, codes = (30, 17), [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)], (1, 6, 0)
    for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("bfloat16", "NCHW", SCALE_NEAREST), ("float16", "NCHW", SCALE_BICUBIC)):
        want = run_oriented(b, size, entries, codes, dtype, layout, filt)
        desc = decoder.tensor_desc(size, dtype, layout, filt, SCALE, BIAS)
        out = DeviceBuffer.from_numpy(np.full(want.nbytes + 256, POISON, np.uint8))
        o0, p0 = decoder.oriented_stats(), decoder.placed_stats()
        decoder.check(L.hipdec_batch_to_tensor_placed(b._h, C.byref(desc), decoder.tensor_entries(entries), (C.c_int * 3)(*codes), None, None, None, 3, out.ptr,
                                                      out.nbytes, None))
        decoder.check(L.hipdec_stream_synchronize(None))
        o1, p1 = decoder.oriented_stats(), decoder.placed_stats()
        assert (o1[0] - o0[0], o1[1] - o0[1]) == (1, 3) and tuple(a - c for a, c in zip(p1, p0)) == (1, 3, 0)
        raw = out.to_numpy((want.nbytes + 256,), np.uint8)
        assert np.array_equal(raw[:want.nbytes], want.reshape(-1).view(np.uint8)) and (raw[want.nbytes:] == POISON).all(), (dtype, layout, filt)
        # ... and so is a rectangle list that names the whole canvas, whatever the fill
        assert np.array_equal(run_placed(b, size, entries, codes, [(0, 0) + size] * 3, dtype, layout, filt, fill=200), want)


@pytest.mark.parametrize("dtype,layout", [("uint8", "NCHW"), ("float16", "NHWC"), ("float32", "NCHW"), ("bfloat16", "NHWC")])
def test_rectangles_at_the_edges_one_pixel_and_one_pixel_margins(dtype, layout):
    W, H = 21, 14
    places = [(0, 3, 9, 7), (12, 3, 9, 7), (4, 0, 9, 7), (4, 7, 9, 7),            # touching the left, right, top and bottom edge only
              (0, 0, 9, 7), (12, 7, 9, 7), (0, 2, 21, 5), (6, 0, 5, 14),          # two corners, full width, full height
              (10, 6, 1, 1), (0, 0, 1, 1), (20, 13, 1, 1), (1, 1, 19, 12)]        # 1 x 1 in the middle and in two corners, a 1-pixel margin all round
    codes = [k % 8 for k in range(len(places))]
    for filt in (SCALE_BOX, SCALE_NEAREST):
        check(_b(SMALL), (W, H), [(0,) + WHOLE] * len(places), codes, places, dtype, layout, filt, fill=(114, 0, 255), mask=True)


@pytest.mark.parametrize("dtype,layout", [("uint8", "NHWC"), ("float16", "NCHW"), ("float32", "NHWC")])
def test_canvases_of_one_column_and_of_one_row(dtype, layout):
    for canvas, places in (((1, 9), [(0, 3, 1, 4), (0, 0, 1, 1), (0, 8, 1, 1), (0, 0, 1, 9)]), ((9, 1), [(2, 0, 5, 1), (0, 0, 1, 1), (8, 0, 1, 1), (0, 0, 9, 1)])):
        for filt in (SCALE_BOX, SCALE_NEAREST, SCALE_BILINEAR):
            check(_b(SMALL), canvas, [(0,) + WHOLE] * 4, (0, 3, 5, 6), places, dtype, layout, filt, mask=True)


# rectangle sizes with RB - 1 / RB / RB + 1 / 2 RB + 1 for RB = 32 and 64 on either side (k_oriented_box's quarter-turn store, tests/test_oriented_gpu.py)
RB_SIZES = [s for n in (31, 32, 33, 63, 64, 65, 129) for s in ((n, 3), (5, n))]


@pytest.mark.parametrize("filt", (SCALE_NEAREST, SCALE_BOX))
@pytest.mark.parametrize("size", RB_SIZES, ids=lambda s: "%dx%d" % s)
def test_quarter_turn_runs_inside_a_canvas_at_an_odd_offset(size, filt):
    canvas, places, e = (size[0] + 5, size[1] + 5), [(3, 1) + size] * 8, [(0,) + WHOLE] * 8
    check(_b(SMALL), canvas, e, CODES, places, "uint8", "NCHW", filt)
    check(_b(SMALL), canvas, e, CODES, places, "float16", "NHWC", filt)
    check(_b(TEN_BIT), canvas, e, CODES, places, "float32", "NCHW", filt)     # native depth: the 64-bit stage, RB = 32
    check(_b(TEN_BIT), canvas, e, CODES, places, "bfloat16", "NHWC", filt)


MIXED_ENTRIES = [(0, 1, 3, 35, 21, 0), (0, 5, 7, 33, 17, 1), (0, 0, 0, 0, 0, 1), (0, 37, 11, 31, 29, 0), (0, 71, 39, 1, 1, 1), (0, 3, 1, 69, 39, 1)]
MIXED_CODES = (1, 5, 4, 3, 6, 0)
MIXED_PLACES = [(2, 1, 13, 9), (0, 0, 20, 11), (7, 5, 13, 6), (1, 0, 5, 11), (19, 10, 1, 1), (3, 2, 13, 9)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype,layout", [("uint8", "NCHW"), ("float16", "NHWC"), ("float32", "NCHW")])
def test_rectangles_windows_flips_and_codes_differ_inside_one_call(dtype, layout, filt):
    """several entries of one item, with windows at odd offsets, flips together with mirrored codes, and rectangles of different sizes"""
    check(_b(SMALL), (20, 11), MIXED_ENTRIES, MIXED_CODES, MIXED_PLACES, dtype, layout, filt, fill=(10, 114, 200), mask=True)


def test_entries_none_and_orientations_none():
    from test_scale_gpu import VUI_FULL, _batch, _still
    b = _batch([_still(1, 8, VUI_FULL, (72, 40)), _still(3, 8, VUI_FULL, (41, 23))])
    try:
        places = [decoder.letterbox_place((72, 40), (32, 32)), decoder.letterbox_place((41, 23), (32, 32), anchor="topleft")]
        assert places == [(0, 7, 32, 18), (0, 0, 32, 18)]
        for dtype, layout, filt in (("float16", "NCHW", SCALE_BOX), ("uint8", "NHWC", SCALE_BILINEAR)):
            check(b, (32, 32), None, None, places, dtype, layout, filt, mask=True)
    finally:
        b.free()


@pytest.mark.parametrize("still", FORMATS, ids=lambda s: "cf%d-%dbit" % (s[0], s[1]))
def test_chroma_formats_and_depths(still):
    b = _b(still)
    e, places = [(0,) + WHOLE] * 8, [(3, 2, 14, 9)] * 8
    for filt in (SCALE_NEAREST, SCALE_BOX):
        check(b, (19, 14), e, CODES, places, "uint8", "NHWC", filt)
        check(b, (19, 14), e, CODES, places, "float32", "NCHW", filt, fill=255)      # 10-bit: float32 holds the native-depth value
    check(b, (19, 14), e, CODES, places, "uint8", "NCHW", SCALE_BILINEAR)


def test_a_component_fill_is_held_against_the_depth_of_the_source():
    L = _lib()
    check(_b(TEN_BIT), (19, 14), [(0,) + WHOLE], (1,), [(3, 2, 14, 9)], "float32", "NCHW", SCALE_BOX, fill=(1023, 512, 256))
    for still, dtype in ((TEN_BIT, "uint8"), (SMALL, "float32")):
        b = _b(still)
        desc = decoder.tensor_desc((19, 14), dtype, "NCHW", SCALE_BOX, SCALE, BIAS)
        out = DeviceBuffer.from_numpy(np.full(19 * 14 * 3 * 4, POISON, np.uint8))
        fill = decoder.tensor_fill(1023)
        _refused(L, L.hipdec_batch_to_tensor_placed(b._h, C.byref(desc), None, None, decoder.tensor_places([(3, 2, 14, 9)]), C.byref(fill), None, 1, out.ptr, out.nbytes,
                                                    None), -1)
        decoder.check(L.hipdec_stream_synchronize(None))
        assert (out.to_numpy((out.nbytes,), np.uint8) == POISON).all()


# element fills: a binary16 tie to even (down, and up), a binary16 subnormal tie, a negative value, both zeros, and a value that overflows binary16
ELEMENT_FILLS = [(1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.5 * 2.0 ** -24), (-1.5, 0.0, -0.0), (70000.0, -3.0e-8, 0.1)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_both_fill_domains_and_fills_that_differ_per_channel(dtype, layout):
    b = _b(SMALL)
    e, codes, places = [(0,) + WHOLE] * 2, (0, 3), [(2, 1, 9, 5), (1, 2, 5, 9)]
    for fill in (0, 114, 255, (0, 114, 255), (1, 2, 3)):
        check(b, (14, 12), e, codes, places, dtype, layout, SCALE_BOX, fill, "component")
    fills = [(0, 7, 255), 164] if dtype == "uint8" else ELEMENT_FILLS + [0.0]
    for fill in fills:
        check(b, (14, 12), e, codes, places, dtype, layout, SCALE_BOX, fill, "element")
    if dtype == "float16":      # the restatement itself, against the values the comment above promises
        assert list(fill_elements(ELEMENT_FILLS[0], "element", dtype)) == [0x3c00, 0x3c02, 0x0002]
        assert list(fill_elements(ELEMENT_FILLS[1], "element", dtype)) == [0xbe00, 0x0000, 0x8000]
        assert int(fill_elements(ELEMENT_FILLS[2], "element", dtype)[0]) == 0x7c00
    # fill = None through the C ABI: component 0 in every channel
    L = _lib()
    desc = decoder.tensor_desc((14, 12), dtype, layout, SCALE_BOX, SCALE, BIAS)
    nbytes = 2 * 3 * 14 * 12 * ES[dtype]
    out = DeviceBuffer(nbytes)
    decoder.check(L.hipdec_batch_to_tensor_placed(b._h, C.byref(desc), decoder.tensor_entries(e), (C.c_int * 2)(*codes), decoder.tensor_places(places), None, None, 2,
                                                  out.ptr, out.nbytes, None))
    decoder.check(L.hipdec_stream_synchronize(None))
    want = expected_placed(b, (14, 12), e, codes, places, dtype, layout, SCALE_BOX, 0, "component")
    assert np.array_equal(out.to_numpy(want.shape, want.dtype), want)


def test_the_mask_is_written_when_no_entry_has_a_margin():
    b = _b(SMALL)
    before = decoder.placed_stats()
    got, m = run_placed(b, (16, 9), [(0,) + WHOLE] * 2, (0, 1), None, "float16", "NCHW", SCALE_BOX, mask=True)
    after = decoder.placed_stats()
    assert m.shape == (2, 9, 16) and not m.any()
    assert np.array_equal(got, run_oriented(b, (16, 9), [(0,) + WHOLE] * 2, (0, 1), "float16", "NCHW", SCALE_BOX))
    assert tuple(a - c for a, c in zip(after, before)) == (1, 2, 1)           # the mask alone takes the margin launch


def test_tensor_mask_to_host_is_the_mask_of_the_last_call_or_an_error():
    b = _b(SMALL)
    e, places = [(0,) + WHOLE], [(1, 1, 6, 4)]
    _, m = run_placed(b, (9, 7), e, (0,), places, "uint8", "NHWC", SCALE_BOX, mask=True)
    assert np.array_equal(m, expected_mask((9, 7), places, 1)) and np.array_equal(b.tensor_mask_to_host(), m)
    run_placed(b, (9, 7), e, (0,), places, "uint8", "NHWC", SCALE_BOX)        # a placed call without a mask: the earlier mask is not handed back
    with pytest.raises(RuntimeError, match="no mask"):
        b.tensor_mask_to_host()
    run_placed(b, (9, 7), e, (0,), places, "uint8", "NHWC", SCALE_BOX, mask=True)
    assert np.array_equal(b.tensor_mask_to_host(), m)
    run_oriented(b, (6, 4), e, (0,), "uint8", "NHWC", SCALE_BOX)              # ... nor after a call of another form
    with pytest.raises(RuntimeError, match="no mask"):
        b.tensor_mask_to_host()


def test_the_margin_kernel_is_one_launch_per_call_with_margins_and_none_without():
    b = _b(SMALL)
    e = [(0,) + WHOLE] * 5
    s0 = decoder.placed_stats()
    run_placed(b, (16, 9), e, CODES[:5], [(1, 1, 8, 4), (0, 0, 16, 9), (3, 0, 13, 9), (0, 0, 16, 8), (15, 8, 1, 1)], "uint8", "NHWC", SCALE_NEAREST, fill=7)
    s1 = decoder.placed_stats()
    run_placed(b, (16, 9), e, CODES[:5], [(0, 0, 16, 9)] * 5, "uint8", "NHWC", SCALE_NEAREST, fill=7)
    s2 = decoder.placed_stats()
    assert tuple(a - c for a, c in zip(s1, s0)) == (1, 5, 1)
    assert tuple(a - c for a, c in zip(s2, s1)) == (1, 5, 0)


def test_album_form_with_two_photos_in_different_rectangles():
    from test_album_gpu import _photos
    a = Album(_photos("444"))                              # 2 x 2 tiles of 72 x 48 clipped to 131 x 91, and 1 x 2 of 64 x 64 clipped to 99 x 63
    try:
        a.run()
        a.status()
        entries, codes = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 71, 57, 0), (1, 1, 1, 63, 61, 0)], (3, 0, 6, 5)
        places = [decoder.letterbox_place(decoder.oriented_size(3, 131, 91), (40, 36)), decoder.letterbox_place((99, 63), (40, 36)), (1, 2, 37, 18), (21, 0, 18, 36)]
        assert places[0][2:] == (25, 36) and places[1][2:] == (40, 25)
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_NEAREST), ("uint8", "NCHW", SCALE_BILINEAR)):
            check(a, (40, 36), entries, codes, places, dtype, layout, filt, fill=(114, 114, 0), mask=True)
    finally:
        a.free()


def _fill(values=(0, 0, 0), domain=0, reserved=0):
    f = TensorFill()
    for c in range(3):
        f.value[c] = values[c]
    f.domain, f.reserved = domain, reserved
    return f


def test_refusals_have_a_status_a_message_and_leave_the_output_untouched():
    from test_scale_gpu import VUI_FULL, _batch, _still
    L = _lib()
    b = _b(SMALL)
    canvas = (16, 8)
    nbytes = 2 * 16 * 8 * 3 * 4
    room = max(nbytes, 2 * 80 * 40 * 3)                                                # (the buffer holds the largest tensor any call below names)
    out = DeviceBuffer.from_numpy(np.full(room, POISON, np.uint8))
    mask = DeviceBuffer.from_numpy(np.full(2 * 80 * 40, POISON, np.uint8))
    good_places = [(1, 1, 8, 4), (0, 0, 16, 8)]
    entries = decoder.tensor_entries([(0,) + WHOLE] * 2)

    def call(dtype="uint8", places=good_places, fill=None, codes=(0, 1), handle=b._h, room=nbytes, filt=SCALE_BOX, desc=None, fn=L.hipdec_batch_to_tensor_placed):
        desc = desc or decoder.tensor_desc(canvas, dtype, "NCHW", filt, SCALE, BIAS)
        return fn(handle, C.byref(desc), entries, (C.c_int * 2)(*codes), decoder.tensor_places(places) if places is not None else None,
                    C.byref(fill) if fill is not None else None, mask.ptr, 2, out.ptr, room, None)

    for bad in ((1, 1, 0, 4), (1, 1, 8, -1), (9, 1, 8, 4), (1, 5, 8, 4), (-1, 1, 8, 4), (1, -1, 8, 4), (0, 0, 17, 8), (2 ** 31 - 1, 0, 2, 2)):
        _refused(L, call(places=[good_places[0], bad]), -1)
        assert b"entry 1" in L.hipdec_last_error(), L.hipdec_last_error()
    nan, inf = float("nan"), float("inf")
    for dtype, fill in (("float32", _fill((nan, 0, 0))), ("float32", _fill((0, inf, 0), 1)), ("uint8", _fill((0, 0, -inf))),        # a fill that is not finite
                        ("float16", _fill((114.5, 0, 0))), ("uint8", _fill((0, 256, 0))), ("float32", _fill((0, 0, -1))),          # component: integral, in range
                        ("float32", _fill((0, 0, 65536))), ("float32", _fill((0, 256, 0))),                                        # (256 from an 8-bit source)
                        ("uint8", _fill(domain=2)), ("float32", _fill(domain=-1)), ("uint8", _fill(reserved=1)),                   # domain, reserved
                        ("uint8", _fill((1.5, 0, 0), 1)), ("uint8", _fill((0, 256, 0), 1)), ("uint8", _fill((0, 0, -1), 1))):      # a U8 element
        _refused(L, call(dtype, fill=fill), -1)
    _refused(L, call(room=2 * 16 * 8 * 3 - 1), -1)                                     # out_bytes below hipdec_tensor_bytes
    for bad in (-1, 8):
        _refused(L, call(codes=(0, bad)), -1)
        assert b"entry 1" in L.hipdec_last_error()
    _refused(L, call(handle=None), -1)
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_placed), -1)
    _refused(L, call(filt=2), -1)                                                      # what the sibling calls refuse: an unknown filter ...
    d = decoder.tensor_desc((0, 8), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
    _refused(L, call(desc=d), -1)                                                      # ... a canvas without columns
    # ... and what they refuse for a sample of the rectangle's size: bilinear into a float dtype from a 10-bit source is HIPDEC_ERR_UNSUPPORTED
    wide = _b(TEN_BIT)
    _refused(L, call("float32", handle=wide._h, filt=SCALE_BILINEAR), -4)
    small = _batch([_still(1, 8, VUI_FULL, (72, 40))] * 2, max_image_size_pixels=72 * 40)
    try:
        big = decoder.tensor_desc((80, 40), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
        _refused(L, L.hipdec_batch_to_tensor_placed(small._h, C.byref(big), None, None, decoder.tensor_places(good_places), None, None, 2, out.ptr, 2 * 80 * 40 * 3, None), -5)
    finally:
        small.free()
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((room,), np.uint8) == POISON).all() and (mask.to_numpy((2 * 80 * 40,), np.uint8) == POISON).all()
    assert call() == 0                                                                 # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    with pytest.raises(ValueError):
        b.to_tensor(canvas, None, dtype="uint8", out=out, places=good_places)          # two rectangles for one entry
    with pytest.raises(ValueError):
        b.to_tensor(canvas, None, dtype="uint8", out=out, fill=0, fill_domain="pixel")
