"""Warped tensor output on the device: hipdec_tensor_warp, hipdec_batch_to_tensor_warped, hipdec_album_to_tensor_warped (Pillow-exact affine transforms
of the resized 8-bit picture, normalised; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code:
  intermediate  what the library's EXISTING hipdec_batch_to_tensor_oriented returns for the same entries and codes with dtype U8, layout NHWC, the source
                size and the resize filter (Batch.to_tensor(..., orientations=)).  That call is pinned by tests/test_oriented_gpu.py and
                tests/test_resample_gpu.py and is not under test here.
  warp          tests/warp_ref.py applied to it: the NumPy float64 restatement that tests/test_warp_ref.py pins to PIL.Image.transform bit for bit.
  float stage   float32(V) * scale + bias in NumPy float32, .astype(float16) / the bfloat16 rounding on the bits (tests/test_tensor_gpu.py elements);
                the fill elements as tests/test_placed_gpu.py fill_elements states them.
The output buffer is 256 bytes longer than the tensor and pre-filled with 0xA5: the tail must come back untouched.

The kernel's tile is 64 x 16 output pixels (warp_kernels.h kWarpTC x kWarpTR): output sizes 1 x 1, 5 x 7 and 65 x 17 - one column and one row more than
the tile; source sizes 1 x 1, 1 x 7, 7 x 5, 33 x 17 and 64 x 48.

Runs on the MI355X (`-m gpu`) and, through tests/test_warp_emu.py, against the library compiled for the host."""
import ctypes as C
import functools

import numpy as np
import pytest

import warp_ref as wr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album, TensorFill
from test_oriented_gpu import CODES, FORMATS, SMALL, _b, _free_batches, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_placed_gpu import fill_elements
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits, elements

pytestmark = pytest.mark.gpu

WARP_FILTERS = (SCALE_NEAREST, SCALE_BILINEAR, SCALE_BICUBIC)
RESIZE_FILTERS = (SCALE_NEAREST, SCALE_BOX, SCALE_BILINEAR, SCALE_BICUBIC)
SRC_SIZES = [(1, 1), (1, 7), (7, 5), (33, 17), (64, 48)]
OUT_SIZES = [(1, 1), (5, 7), (65, 17)]
POISON = 0xA5
ES = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
WHOLE = (0, 0, 0, 0, 0)
TEN_BIT = FORMATS[3]
FILL3 = (3, 114, 250)


def _key(still):
    cf, bits, vui, size = still
    return (cf, bits, tuple(sorted(vui.items())), size)


@functools.lru_cache(maxsize=None)
def _intermediate(key, src_size, entries, codes, filt):
    """the U8 / NHWC picture the maps read: the existing oriented call, computed once per (still, entries, codes, size, filter) and never modified"""
    cf, bits, vui, size = key
    mid = run_oriented(_b((cf, bits, dict(vui), size)), src_size, list(entries), codes, "uint8", "NHWC", filt)
    mid.setflags(write=False)
    return mid


def expected_warped(mid, maps, size, wf, dtype, layout, fill=None, domain="component"):
    n = len(maps)
    fe = fill_elements(fill, domain, dtype)
    out = []
    for e in range(n):
        V, inside = wr.warp(mid[e], maps[e], size, wf)
        el = elements(V, dtype, SCALE, BIAS)
        out.append(np.where(inside[..., None], el, fe[None, None, :].astype(el.dtype)))
    exp = np.stack(out) if n else np.empty((0, size[1], size[0], 3), fe.dtype)
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def run_warped(h, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=0, domain="component"):
    """the warped call into a poisoned buffer 256 bytes longer than the tensor; returns the tensor's bit patterns"""
    n = len(maps)
    nbytes = n * 3 * size[0] * size[1] * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    assert h.to_tensor_warped(size, maps, entries, src_size=src_size, warp_filter=wf, fill=fill, fill_domain=domain, orientations=codes, filter=filt, dtype=dtype,
                              layout=layout, scale=SCALE, bias=BIAS, out=out) is out
    got = as_bits(h.tensor_to_host())
    assert got.shape == ((n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    return got


def check(still, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=0, domain="component"):
    n = len(maps)
    ent = tuple((i,) + WHOLE for i in range(n)) if entries is None else tuple(tuple(e) for e in entries)
    cds = (0,) * n if codes is None else tuple(codes)
    mid = _intermediate(_key(still), src_size, ent, cds, filt)
    got = run_warped(_b(still), size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill, domain)
    exp = expected_warped(mid, maps, size, wf, dtype, layout, fill, domain)
    bad = [(e, int((got[e] != exp[e]).sum())) for e in range(n) if not np.array_equal(got[e], exp[e])]
    assert not bad, (src_size, size, wf, dtype, layout, filt, bad)


def _maps(src_size, size):
    return [m for _, m, _ in wr.map_classes(src_size, size)]


@pytest.mark.parametrize("wf", WARP_FILTERS)
@pytest.mark.parametrize("src_size", SRC_SIZES, ids=lambda s: "src%dx%d" % s)
def test_every_map_class_at_every_size(src_size, wf):
    """identity, translations, scales, a negative scale, shear, three rotations and a map that is outside everywhere: one entry each, one call per size"""
    for size in OUT_SIZES:
        maps = _maps(src_size, size)
        check(SMALL, size, maps, [(0,) + WHOLE] * len(maps), None, src_size, wf, "uint8", "NHWC", SCALE_BILINEAR, fill=FILL3)


def test_the_centred_maps_are_not_fill_alone():
    for src_size in SRC_SIZES:
        mid = np.zeros((src_size[1], src_size[0], 3), np.uint8)
        for name, m, centred in wr.map_classes(src_size, src_size):
            if centred:
                inside = wr.warp(mid, m, src_size, SCALE_BILINEAR)[1]
                assert 2 * int(inside.sum()) >= inside.size, (name, src_size)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_dtypes_layouts_and_both_fill_domains(dtype, layout):
    src_size = (33, 17)
    for size in ((13, 9), (65, 17), (8, 3)):
        cls = dict((n, m) for n, m, _ in wr.map_classes(src_size, size))
        maps = [cls["rotate_30"], cls["translate_half"], cls["all_outside"], cls["shear"], cls["scale_two"]]
        for wf in WARP_FILTERS:
            check(SMALL, size, maps, [(0,) + WHOLE] * 5, None, src_size, wf, dtype, layout, SCALE_BOX, fill=FILL3, domain="component")
        efill = (5, 0, 255) if dtype == "uint8" else (-1.5, 0.0, 3.25e-5)
        check(SMALL, size, maps, [(0,) + WHOLE] * 5, None, src_size, SCALE_BILINEAR, dtype, layout, SCALE_BOX, fill=efill, domain="element")


@pytest.mark.parametrize("filt", RESIZE_FILTERS)
def test_orientation_codes_flips_and_every_resize_filter(filt):
    src_size, size = (7, 5), (5, 7)
    rot = dict((n, m) for n, m, _ in wr.map_classes(src_size, size))["rotate_-17.5"]
    entries = [(0, 0, 0, 0, 0, k & 1) for k in range(8)]
    for wf in (SCALE_NEAREST, SCALE_BICUBIC):
        check(SMALL, size, [rot] * 8, entries, CODES, src_size, wf, "float16", "NCHW", filt, fill=114)


def test_entries_that_differ_in_window_code_flip_and_map():
    src_size, size = (33, 17), (65, 17)
    cls = wr.map_classes(src_size, size)
    entries = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0), (0, 36, 20, 31, 19, 1)]
    maps = [cls[8][1], cls[2][1], cls[6][1], cls[10][1]]
    for wf in WARP_FILTERS:
        check(SMALL, size, maps, entries, (1, 6, 0, 3), src_size, wf, "bfloat16", "NHWC", SCALE_BICUBIC, fill=FILL3)


@pytest.mark.parametrize("still", FORMATS[:3], ids=lambda s: "cf%d" % s[0])
def test_entries_none_is_every_item_whole(still):
    src_size, size = (7, 5), (5, 7)
    m = dict((n, m) for n, m, _ in wr.map_classes(src_size, size))["rotate_30"]
    check(still, size, [m], None, None, src_size, SCALE_BILINEAR, "float32", "NCHW", SCALE_NEAREST)


@pytest.mark.parametrize("wf", WARP_FILTERS)
def test_the_identity_map_at_the_source_size_is_the_oriented_call_byte_for_byte(wf):
    b = _b(SMALL)
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    entries, codes = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)], (1, 6, 0)
    for size in ((30, 17), (65, 17)):
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("bfloat16", "NCHW", SCALE_NEAREST), ("float16", "NCHW", SCALE_BICUBIC), ("float32", "NHWC", SCALE_BILINEAR)):
            want = run_oriented(b, size, entries, codes, dtype, layout, filt)
            got = run_warped(b, size, [ident] * 3, entries, codes, None, wf, dtype, layout, filt, fill=200)
            assert np.array_equal(got, want), (size, dtype, layout, filt)


def test_the_stage_alone_over_a_buffer_of_the_tests_own():
    L = _lib()
    rng = np.random.default_rng(5)
    src_size, size, n = (33, 17), (65, 17), 3
    src = rng.integers(0, 256, (n, src_size[1], src_size[0], 3), dtype=np.uint8)
    sbuf = DeviceBuffer.from_numpy(src)
    cls = wr.map_classes(src_size, size)
    maps = [cls[8][1], cls[5][1], cls[2][1]]
    for wf in WARP_FILTERS:
        for dtype, layout in (("uint8", "NCHW"), ("float16", "NHWC"), ("float32", "NCHW")):
            nbytes = n * 3 * size[0] * size[1] * ES[dtype]
            out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
            got = as_bits(decoder.tensor_warp(sbuf, size, maps, src_size=src_size, warp_filter=wf, fill=FILL3, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out,
                                              to_host=True))
            assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all()
            assert np.array_equal(got, expected_warped(src, maps, size, wf, dtype, layout, FILL3)), (wf, dtype, layout)
    # n = 0: taken, nothing written, nothing counted
    out = DeviceBuffer.from_numpy(np.full(64, POISON, np.uint8))
    s0 = decoder.warp_stats()
    desc = decoder.tensor_desc(size, "uint8", "NCHW", 0, SCALE, BIAS)
    wd = decoder.warp_desc(src_size, SCALE_BILINEAR)
    assert L.hipdec_tensor_warp(sbuf.ptr, sbuf.nbytes, C.byref(wd), None, None, C.byref(desc), 0, out.ptr, 64, None) == 0
    assert L.hipdec_tensor_warp(None, 0, C.byref(wd), None, None, C.byref(desc), 0, None, 0, None) == 0
    decoder.check(L.hipdec_stream_synchronize(None))
    assert decoder.warp_stats() == s0 and (out.to_numpy((64,), np.uint8) == POISON).all()
    assert decoder.tensor_warp(sbuf, size, [], src_size=src_size, dtype="uint8", to_host=True).shape == (0, 3, size[1], size[0])
    _refused(L, L.hipdec_tensor_warp(sbuf.ptr, sbuf.nbytes - 1, C.byref(wd), decoder.tensor_maps(maps), None, C.byref(desc), n, out.ptr, 1 << 20, None), -1)   # src_bytes
    _refused(L, L.hipdec_tensor_warp(sbuf.ptr, sbuf.nbytes, C.byref(wd), decoder.tensor_maps(maps), None, C.byref(desc), -1, out.ptr, 1 << 20, None), -1)
    _refused(L, L.hipdec_tensor_warp(None, sbuf.nbytes, C.byref(wd), decoder.tensor_maps(maps), None, C.byref(desc), n, out.ptr, 1 << 20, None), -1)


def test_album_form_with_two_photos():
    from test_album_gpu import _photos
    a = Album(_photos("444"))                              # 2 x 2 tiles of 72 x 48 clipped to 131 x 91, and 1 x 2 of 64 x 64 clipped to 99 x 63
    try:
        a.run()
        a.status()
        src_size, size = (33, 17), (20, 13)
        entries, codes = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 71, 57, 0), (1, 1, 1, 63, 61, 0)], (3, 0, 6, 5)
        cls = wr.map_classes(src_size, size)
        maps = [cls[8][1], cls[9][1], cls[6][1], cls[0][1]]
        for wf, dtype, layout, filt in ((SCALE_BILINEAR, "uint8", "NHWC", SCALE_BOX), (SCALE_BICUBIC, "float16", "NCHW", SCALE_BILINEAR), (SCALE_NEAREST, "float32", "NCHW", SCALE_NEAREST)):
            out = DeviceBuffer(4 * 3 * src_size[0] * src_size[1])
            a.to_tensor(src_size, entries, dtype="uint8", layout="NHWC", filter=filt, out=out, orientations=codes)
            mid = a.tensor_to_host()
            got = run_warped(a, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=FILL3)
            assert np.array_equal(got, expected_warped(mid, maps, size, wf, dtype, layout, FILL3)), (wf, dtype, layout, filt)
    finally:
        a.free()


def test_a_ten_bit_still_is_warped_as_uint8_and_refused_as_float():
    L = _lib()
    src_size, size = (33, 17), (13, 9)
    m = dict((n, m) for n, m, _ in wr.map_classes(src_size, size))["rotate_30"]
    for wf in WARP_FILTERS:
        check(TEN_BIT, size, [m, m], [(0,) + WHOLE, (0, 2, 2, 31, 21, 1)], (0, 5), src_size, wf, "uint8", "NCHW", SCALE_BILINEAR, fill=9)
    b = _b(TEN_BIT)
    out = DeviceBuffer.from_numpy(np.full(4096, POISON, np.uint8))
    for dtype in ("float32", "float16", "bfloat16"):
        with pytest.raises(decoder.HipDecError) as ei:
            b.to_tensor_warped(size, [m], src_size=src_size, dtype=dtype, out=out)
        assert ei.value.code == -4 and "10-bit" in ei.value.message, ei.value
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((4096,), np.uint8) == POISON).all()


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
    size, src_size = (16, 8), (9, 7)
    nbytes = 2 * 16 * 8 * 3 * 4
    out = DeviceBuffer.from_numpy(np.full(nbytes, POISON, np.uint8))
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    entries = decoder.tensor_entries([(0,) + WHOLE] * 2)

    def call(dtype="uint8", maps=(ident, ident), fill=None, codes=(0, 1), handle=b._h, room=nbytes, filt=SCALE_BOX, desc=None, warp=None, fn=L.hipdec_batch_to_tensor_warped,
             no_maps=False):
        desc = desc or decoder.tensor_desc(size, dtype, "NCHW", filt, SCALE, BIAS)
        warp = warp or decoder.warp_desc(src_size, SCALE_BILINEAR)
        return fn(handle, C.byref(desc), entries, (C.c_int * 2)(*codes), C.byref(warp), None if no_maps else decoder.tensor_maps(maps), C.byref(fill) if fill is not None else None,
                  2, out.ptr, room, None)

    def names(text):
        assert text in L.hipdec_last_error(), L.hipdec_last_error()

    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 0, 0, 0, 1, 0), (1, 0, inf, 0, 1, 0), (1, 0, 0, 0, -inf, 0)):                 # a coefficient that is not finite
        _refused(L, call(maps=(ident, bad)), -1)
        names(b"entry 1"); names(b"not finite")
    for bad in ((32000.0, 0, 0, 0, 1, 0), (1, -32000.0, 0, 0, 1, 0), (1, 0, 0, 0, 1, 40000.0)):      # |m[i]| >= 32000
        _refused(L, call(maps=(bad, ident)), -1)
        names(b"entry 0"); names(b"32000")
    for bad in ((1, 0, 31985.0, 0, 1, 0), (1, 0, 0, 0, 1, 31993.0), (-2000.0, 0, 0, 0, 1, 0), (1, 0, 0, 0, 3999.9, 10.0)):   # a corner of [0, 16] x [0, 8]
        _refused(L, call(maps=(ident, bad)), -1)
        names(b"entry 1"); names(b"corner")
    assert call(maps=(ident, (1, 0, 31983.5, 0, 1, 0)), handle=None) == -1                         # (a corner at 31999.5 passes: the NULL handle is what is left)
    names(b"bad arguments")
    for ssz in ((32768, 7), (9, 32768), (0, 7), (9, -1)):                                          # the source size
        _refused(L, call(warp=decoder.warp_desc(ssz, SCALE_BILINEAR)), -1)
        names(b"source size")
    for wf in (SCALE_BOX, 2, -1, 18):                                                              # BOX has no warp; unknown filters
        _refused(L, call(warp=decoder.warp_desc(src_size, wf)), -1)
        names(b"warp filter")
    _refused(L, call(warp=decoder.WarpDesc(9, 7, SCALE_BILINEAR, 1)), -1)
    _refused(L, call(no_maps=True), -1)
    for dtype, fill in (("float32", _fill((nan, 0, 0))), ("float32", _fill((0, inf, 0), 1)), ("float16", _fill((114.5, 0, 0))), ("uint8", _fill((0, 256, 0))),
                        ("float32", _fill((0, 0, -1))), ("float32", _fill((0, 256, 0))), ("uint8", _fill(domain=2)), ("uint8", _fill(reserved=1)),
                        ("uint8", _fill((1.5, 0, 0), 1)), ("uint8", _fill((0, 256, 0), 1))):
        _refused(L, call(dtype, fill=fill), -1)
    _refused(L, call(room=2 * 16 * 8 * 3 - 1), -1)                                                 # out_bytes below hipdec_tensor_bytes
    for bad in (-1, 8):
        _refused(L, call(codes=(0, bad)), -1)
        names(b"entry 1")
    _refused(L, call(handle=None), -1)
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_warped), -1)
    _refused(L, call(filt=2), -1)                                                                  # what the sibling calls refuse: an unknown resize filter ...
    _refused(L, call(desc=decoder.tensor_desc((0, 8), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)), -1)
    bad_entries = decoder.tensor_entries([(0,) + WHOLE, (0, 70, 0, 10, 10, 0)])                     # ... a window that leaves the picture ...
    _refused(L, L.hipdec_batch_to_tensor_warped(b._h, C.byref(decoder.tensor_desc(size, "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)), bad_entries, None,
                                                C.byref(decoder.warp_desc(src_size)), decoder.tensor_maps((ident, ident)), None, 2, out.ptr, nbytes, None), -1)
    names(b"entry 1")
    _refused(L, call("float32", handle=_b(TEN_BIT)._h), -4)                                        # ... and a float dtype from a 10-bit source
    small = _batch([_still(1, 8, VUI_FULL, (72, 40))] * 2, max_image_size_pixels=72 * 40)
    try:
        big = decoder.tensor_desc((80, 40), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
        room = DeviceBuffer(2 * 80 * 40 * 3)
        _refused(L, L.hipdec_batch_to_tensor_warped(small._h, C.byref(big), None, None, C.byref(decoder.warp_desc(src_size)), decoder.tensor_maps((ident, ident)), None, 2,
                                                    room.ptr, room.nbytes, None), -5)
    finally:
        small.free()
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((nbytes,), np.uint8) == POISON).all()
    s0 = decoder.warp_stats()
    assert call() == 0                                                                             # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    assert decoder.warp_stats() == (s0[0] + 1, s0[1] + 2)
    with pytest.raises(ValueError):
        b.to_tensor_warped(size, [ident, ident], dtype="uint8")                                    # two maps for one entry
    with pytest.raises(ValueError):
        b.to_tensor_warped(size, [ident[:5]], dtype="uint8")
    with pytest.raises(ValueError):
        b.to_tensor_warped(size, [ident], dtype="uint8", fill_domain="pixel")


@pytest.mark.parametrize("wf", WARP_FILTERS)
def test_one_resize_launch_and_one_warp_launch_per_call_and_the_stats_advance_by_the_entries(wf):
    """hipdec_warp_stats counts launches of the warp kernel as its calls; hipdec_oriented_stats counts the launches of the resize stage"""
    b = _b(SMALL)
    src_size, size = (33, 17), (65, 17)
    maps = _maps(src_size, size)                           # eleven entries with eleven different maps (both NEAREST paths among them)
    n = len(maps)
    o0, w0, t0 = decoder.oriented_stats(), decoder.warp_stats(), decoder.tensor_stats()
    run_warped(b, size, maps, [(0,) + WHOLE] * n, [k % 8 for k in range(n)], src_size, wf, "float16", "NCHW", SCALE_BOX)
    o1, w1, t1 = decoder.oriented_stats(), decoder.warp_stats(), decoder.tensor_stats()
    assert (o1[0] - o0[0], o1[1] - o0[1]) == (1, n)
    assert (w1[0] - w0[0], w1[1] - w0[1]) == (1, n)
    assert (t1[0] - t0[0], t1[1] - t0[1]) == (1, n)
