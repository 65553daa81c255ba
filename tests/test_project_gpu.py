"""Projective tensor output on the device: hipdec_tensor_project, hipdec_batch_to_tensor_projected, hipdec_album_to_tensor_projected (Pillow-exact
PERSPECTIVE and QUAD transforms of the resized 8-bit picture, normalised; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code:
  intermediate  what the library's EXISTING hipdec_batch_to_tensor_oriented returns for the same entries and codes with dtype U8, layout NHWC, the source
                size and the resize filter (tests/test_warp_gpu.py _intermediate).  That call is pinned elsewhere and is not under test here.
  projection    tests/project_ref.py applied to it: the NumPy float64 restatement that tests/test_project_ref.py pins to PIL.Image.transform bit for bit.
  float stage   tests/test_tensor_gpu.py elements; the fill elements as tests/test_placed_gpu.py fill_elements states them.
  equalities    against the EXISTING warped call (a6 = a7 = 0), the existing stages (chaining) and the existing oriented call.
The output buffer is 256 bytes longer than the tensor and pre-filled with 0xA5: the tail must come back untouched.

The kernel's tile is 64 x 16 output pixels: output sizes 1 x 1, 5 x 7 and 65 x 17 - one column and one row more than the tile; source sizes 1 x 1, 1 x 7,
7 x 5, 33 x 17 and 64 x 48.

Runs on the MI355X (`-m gpu`) and, through tests/test_project_emu.py, against the library compiled for the host."""
import ctypes as C

import numpy as np
import pytest

import project_ref as pr
import warp_ref as wr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album, TensorProjection
from test_oriented_gpu import CODES, FORMATS, SMALL, _b, _free_batches, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_placed_gpu import fill_elements
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits, elements
from test_warp_gpu import ES, FILL3, OUT_SIZES, POISON, RESIZE_FILTERS, SRC_SIZES, TEN_BIT, WARP_FILTERS, WHOLE, _fill, _intermediate, _key, run_warped

pytestmark = pytest.mark.gpu

IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def expected_projected(mid, maps, size, wf, dtype, layout, fill=None, domain="component"):
    """maps: (kind, eight coefficients) per entry"""
    n = len(maps)
    fe = fill_elements(fill, domain, dtype)
    out = []
    for e in range(n):
        V, inside = pr.project(mid[e], maps[e][1], maps[e][0], size, wf)
        el = elements(V, dtype, SCALE, BIAS)
        out.append(np.where(inside[..., None], el, fe[None, None, :].astype(el.dtype)))
    exp = np.stack(out) if n else np.empty((0, size[1], size[0], 3), fe.dtype)
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def run_projected(h, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=0, domain="component"):
    """the projected call into a poisoned buffer 256 bytes longer than the tensor; returns the tensor's bit patterns"""
    n = len(maps)
    nbytes = n * 3 * size[0] * size[1] * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    assert h.to_tensor_projected(size, maps, entries, src_size=src_size, warp_filter=wf, fill=fill, fill_domain=domain, orientations=codes, filter=filt,
                                 dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out) is out
    got = as_bits(h.tensor_to_host())
    assert got.shape == ((n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    return got


def check(still, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=0, domain="component"):
    n = len(maps)
    ent = tuple((i,) + WHOLE for i in range(n)) if entries is None else tuple(tuple(e) for e in entries)
    cds = (0,) * n if codes is None else tuple(codes)
    mid = _intermediate(_key(still), src_size, ent, cds, filt)
    got = run_projected(_b(still), size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill, domain)
    exp = expected_projected(mid, maps, size, wf, dtype, layout, fill, domain)
    bad = [(e, int((got[e] != exp[e]).sum())) for e in range(n) if not np.array_equal(got[e], exp[e])]
    assert not bad, (src_size, size, wf, dtype, layout, filt, bad)


def _maps(src_size, size):
    return [(k, m) for _, k, m in pr.map_classes(src_size, size)]


def _cls(src_size, size):
    return dict((n, (k, m)) for n, k, m in pr.map_classes(src_size, size))


@pytest.mark.parametrize("wf", WARP_FILTERS)
@pytest.mark.parametrize("src_size", SRC_SIZES, ids=lambda s: "src%dx%d" % s)
def test_every_map_class_at_every_size(src_size, wf):
    """eight PERSPECTIVE classes and four QUAD classes, one entry each - both kinds in one call -, one call per output size"""
    for size in OUT_SIZES:
        maps = _maps(src_size, size)
        check(SMALL, size, maps, [(0,) + WHOLE] * len(maps), None, src_size, wf, "uint8", "NHWC", SCALE_BILINEAR, fill=FILL3)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_dtypes_layouts_and_both_fill_domains(dtype, layout):
    src_size = (33, 17)
    for size in ((13, 9), (65, 17), (8, 3)):
        cls = _cls(src_size, size)
        maps = [cls["perspective_keystone_both"], cls["quad_jittered"], cls["perspective_all_outside"], cls["perspective_partly_outside"], cls["quad_non_convex"]]
        for wf in WARP_FILTERS:
            check(SMALL, size, maps, [(0,) + WHOLE] * 5, None, src_size, wf, dtype, layout, SCALE_BOX, fill=FILL3, domain="component")
        efill = (5, 0, 255) if dtype == "uint8" else (-1.5, 0.0, 3.25e-5)
        check(SMALL, size, maps, [(0,) + WHOLE] * 5, None, src_size, SCALE_BILINEAR, dtype, layout, SCALE_BOX, fill=efill, domain="element")


@pytest.mark.parametrize("filt", RESIZE_FILTERS)
def test_orientation_codes_flips_and_every_resize_filter(filt):
    src_size, size = (7, 5), (5, 7)
    cls = _cls(src_size, size)
    entries = [(0, 0, 0, 0, 0, k & 1) for k in range(8)]
    maps = [cls["perspective_keystone_both"] if k % 2 == 0 else cls["quad_jittered"] for k in range(8)]
    for wf in (SCALE_NEAREST, SCALE_BICUBIC):
        check(SMALL, size, maps, entries, CODES, src_size, wf, "float16", "NCHW", filt, fill=114)


def test_entries_that_differ_in_window_code_flip_kind_and_map():
    src_size, size = (33, 17), (65, 17)
    cls = _cls(src_size, size)
    entries = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0), (0, 36, 20, 31, 19, 1)]
    maps = [cls["perspective_keystone_x"], cls["quad_own_corners"], cls["perspective_denominator_quarter_to_four"], cls["quad_non_convex"]]
    for wf in WARP_FILTERS:
        check(SMALL, size, maps, entries, (1, 6, 0, 3), src_size, wf, "bfloat16", "NHWC", SCALE_BICUBIC, fill=FILL3)


@pytest.mark.parametrize("still", FORMATS[:3], ids=lambda s: "cf%d" % s[0])
def test_entries_none_is_every_item_whole_and_a_bare_eight_sequence_is_perspective(still):
    src_size, size = (7, 5), (5, 7)
    kind, m = _cls(src_size, size)["perspective_keystone_y"]
    ent, mid_key = ((0,) + WHOLE,), _key(still)
    got = run_projected(_b(still), size, [m], None, None, src_size, SCALE_BILINEAR, "float32", "NCHW", SCALE_NEAREST)
    mid = _intermediate(mid_key, src_size, ent, (0,), SCALE_NEAREST)
    assert np.array_equal(got, expected_projected(mid, [(kind, m)], size, SCALE_BILINEAR, "float32", "NCHW", 0))


@pytest.mark.parametrize("wf", (SCALE_BILINEAR, SCALE_BICUBIC))
def test_a_perspective_map_without_a6_a7_gives_the_warped_calls_bytes(wf):
    """against the EXISTING hipdec_batch_to_tensor_warped: division by exactly 1.0 is exact"""
    b = _b(SMALL)
    src_size = (33, 17)
    entries, codes = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)], (1, 6, 0)
    for size in ((30, 17), (65, 17)):
        affine = [m for _, m, _ in wr.map_classes(src_size, size)]
        for dtype, layout in (("uint8", "NHWC"), ("float16", "NCHW")):
            for k in range(0, len(affine) - 2, 3):
                ms = affine[k:k + 3]
                want = run_warped(b, size, ms, entries, codes, src_size, wf, dtype, layout, SCALE_BILINEAR, fill=FILL3)
                got = run_projected(b, size, [tuple(m) + (0.0, 0.0) for m in ms], entries, codes, src_size, wf, dtype, layout, SCALE_BILINEAR, fill=FILL3)
                assert np.array_equal(got, want), (size, dtype, layout, k)


@pytest.mark.parametrize("wf", WARP_FILTERS)
def test_the_decode_side_form_is_the_stage_over_the_oriented_calls_result(wf):
    """hipdec_batch_to_tensor_projected against hipdec_tensor_project over what the EXISTING hipdec_batch_to_tensor_oriented wrote"""
    b = _b(SMALL)
    src_size, size = (33, 17), (65, 17)
    cls = _cls(src_size, size)
    entries, codes = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)], (1, 6, 0)
    maps = [cls["perspective_keystone_both"], cls["quad_jittered"], cls["perspective_partly_outside"]]
    for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("bfloat16", "NCHW", SCALE_NEAREST), ("float32", "NHWC", SCALE_BICUBIC)):
        mid = DeviceBuffer(3 * 3 * src_size[0] * src_size[1])
        b.to_tensor(src_size, entries, dtype="uint8", layout="NHWC", filter=filt, out=mid, orientations=codes)
        b.tensor_to_host()                                                                          # (waits)
        want = as_bits(decoder.tensor_project(mid, size, maps, src_size=src_size, warp_filter=wf, fill=FILL3, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS,
                                              to_host=True))
        got = run_projected(b, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=FILL3)
        assert np.array_equal(got, want), (dtype, layout, filt)
    ident = run_projected(b, (30, 17), [IDENT] * 3, entries, codes, None, wf, "float16", "NCHW", SCALE_BICUBIC, fill=200)
    assert np.array_equal(ident, run_oriented(b, (30, 17), entries, codes, "float16", "NCHW", SCALE_BICUBIC))   # the identity at the source size


def test_the_stage_alone_over_a_buffer_of_the_tests_own():
    L = _lib()
    rng = np.random.default_rng(5)
    src_size, size, n = (33, 17), (65, 17), 3
    src = rng.integers(0, 256, (n, src_size[1], src_size[0], 3), dtype=np.uint8)
    sbuf = DeviceBuffer.from_numpy(src)
    cls = _cls(src_size, size)
    maps = [cls["perspective_keystone_both"], cls["quad_jittered"], cls["perspective_affine_only"]]
    for wf in WARP_FILTERS:
        for dtype, layout in (("uint8", "NCHW"), ("float16", "NHWC"), ("float32", "NCHW")):
            nbytes = n * 3 * size[0] * size[1] * ES[dtype]
            out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
            got = as_bits(decoder.tensor_project(sbuf, size, maps, src_size=src_size, warp_filter=wf, fill=FILL3, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS,
                                                 out=out, to_host=True))
            assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all()
            assert np.array_equal(got, expected_projected(src, maps, size, wf, dtype, layout, FILL3)), (wf, dtype, layout)
    # n = 0: taken, nothing written, nothing counted
    out = DeviceBuffer.from_numpy(np.full(64, POISON, np.uint8))
    s0 = decoder.project_stats()
    desc = decoder.tensor_desc(size, "uint8", "NCHW", 0, SCALE, BIAS)
    wd = decoder.warp_desc(src_size, SCALE_BILINEAR)
    assert L.hipdec_tensor_project(sbuf.ptr, sbuf.nbytes, C.byref(wd), None, None, C.byref(desc), 0, out.ptr, 64, None) == 0
    assert L.hipdec_tensor_project(None, 0, C.byref(wd), None, None, C.byref(desc), 0, None, 0, None) == 0
    decoder.check(L.hipdec_stream_synchronize(None))
    assert decoder.project_stats() == s0 and (out.to_numpy((64,), np.uint8) == POISON).all()
    assert decoder.tensor_project(sbuf, size, [], src_size=src_size, dtype="uint8", to_host=True).shape == (0, 3, size[1], size[0])
    marr = decoder.tensor_projections(maps)
    _refused(L, L.hipdec_tensor_project(sbuf.ptr, sbuf.nbytes - 1, C.byref(wd), marr, None, C.byref(desc), n, out.ptr, 1 << 20, None), -1)   # src_bytes
    _refused(L, L.hipdec_tensor_project(sbuf.ptr, sbuf.nbytes, C.byref(wd), marr, None, C.byref(desc), -1, out.ptr, 1 << 20, None), -1)
    _refused(L, L.hipdec_tensor_project(None, sbuf.nbytes, C.byref(wd), marr, None, C.byref(desc), n, out.ptr, 1 << 20, None), -1)


def test_a_u8_nhwc_output_chains_with_the_other_stages():
    """project -> warp / photo / augment / recipe and warp / photo -> project through U8 / NHWC buffers; the other stages are the EXISTING calls and
    their expected bytes are tests/warp_ref.py and 255 - v (invert)"""
    rng = np.random.default_rng(6)
    src_size, size, n = (33, 17), (21, 13), 2
    src = rng.integers(0, 256, (n, src_size[1], src_size[0], 3), dtype=np.uint8)
    sbuf = DeviceBuffer.from_numpy(src)
    cls = _cls(src_size, size)
    maps = [cls["perspective_keystone_both"], cls["quad_jittered"]]
    u8 = dict(dtype="uint8", layout="NHWC")
    first = DeviceBuffer(n * size[0] * size[1] * 3)
    p1 = decoder.tensor_project(sbuf, size, maps, src_size=src_size, warp_filter=SCALE_BICUBIC, fill=FILL3, out=first, to_host=True, **u8)
    want1 = np.stack([pr.project(src[e], maps[e][1], maps[e][0], size, SCALE_BICUBIC, FILL3)[0] for e in range(n)])
    assert np.array_equal(p1, want1)
    rot = [m for nm, m, _ in wr.map_classes(size, size) if nm == "rotate_30"] * n
    got = decoder.tensor_warp(first, size, rot, src_size=size, warp_filter=SCALE_BILINEAR, fill=9, to_host=True, **u8)
    assert np.array_equal(got, np.stack([wr.warp(want1[e], rot[e], size, SCALE_BILINEAR, (9, 9, 9))[0] for e in range(n)]))
    assert np.array_equal(decoder.tensor_photo(first, [("invert",)] * n, src_size=size, to_host=True, **u8), 255 - want1)
    assert np.array_equal(decoder.tensor_augment(first, [("invert",)] * n, src_size=size, to_host=True, **u8), 255 - want1)
    got = decoder.tensor_recipe(first, [("invert", ("affine", rot[0], SCALE_BILINEAR, 9))] * n, src_size=size, to_host=True, **u8)
    assert np.array_equal(got, np.stack([wr.warp(255 - want1[e], rot[e], size, SCALE_BILINEAR, (9, 9, 9))[0] for e in range(n)]))
    # ... and the other way round: the photo stage's and the warp stage's output is a source of this stage
    inv = DeviceBuffer(n * src_size[0] * src_size[1] * 3)
    decoder.tensor_photo(sbuf, [("invert",)] * n, src_size=src_size, out=inv, to_host=True, **u8)
    got = decoder.tensor_project(inv, size, maps, src_size=src_size, warp_filter=SCALE_NEAREST, fill=FILL3, to_host=True, **u8)
    assert np.array_equal(got, np.stack([pr.project(255 - src[e], maps[e][1], maps[e][0], size, SCALE_NEAREST, FILL3)[0] for e in range(n)]))
    rot_src = [m for nm, m, _ in wr.map_classes(src_size, src_size) if nm == "rotate_-17.5"] * n
    turned = DeviceBuffer(n * src_size[0] * src_size[1] * 3)
    decoder.tensor_warp(sbuf, src_size, rot_src, src_size=src_size, warp_filter=SCALE_BICUBIC, fill=1, out=turned, to_host=True, **u8)
    mid = np.stack([wr.warp(src[e], rot_src[e], src_size, SCALE_BICUBIC, (1, 1, 1))[0] for e in range(n)])
    got = decoder.tensor_project(turned, size, maps, src_size=src_size, warp_filter=SCALE_BILINEAR, fill=FILL3, to_host=True, **u8)
    assert np.array_equal(got, np.stack([pr.project(mid[e], maps[e][1], maps[e][0], size, SCALE_BILINEAR, FILL3)[0] for e in range(n)]))


def test_album_form_with_two_photos():
    from test_album_gpu import _photos
    a = Album(_photos("444"))                              # 2 x 2 tiles of 72 x 48 clipped to 131 x 91, and 1 x 2 of 64 x 64 clipped to 99 x 63
    try:
        a.run()
        a.status()
        src_size, size = (33, 17), (20, 13)
        entries, codes = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 71, 57, 0), (1, 1, 1, 63, 61, 0)], (3, 0, 6, 5)
        cls = _cls(src_size, size)
        maps = [cls["perspective_keystone_both"], cls["quad_jittered"], cls["perspective_partly_outside"], cls["quad_own_corners"]]
        for wf, dtype, layout, filt in ((SCALE_BILINEAR, "uint8", "NHWC", SCALE_BOX), (SCALE_BICUBIC, "float16", "NCHW", SCALE_BILINEAR), (SCALE_NEAREST, "float32", "NCHW", SCALE_NEAREST)):
            out = DeviceBuffer(4 * 3 * src_size[0] * src_size[1])
            a.to_tensor(src_size, entries, dtype="uint8", layout="NHWC", filter=filt, out=out, orientations=codes)
            mid = a.tensor_to_host()
            got = run_projected(a, size, maps, entries, codes, src_size, wf, dtype, layout, filt, fill=FILL3)
            assert np.array_equal(got, expected_projected(mid, maps, size, wf, dtype, layout, FILL3)), (wf, dtype, layout, filt)
    finally:
        a.free()


def test_a_ten_bit_still_is_projected_as_uint8_and_refused_as_float():
    L = _lib()
    src_size, size = (33, 17), (13, 9)
    cls = _cls(src_size, size)
    maps = [cls["perspective_keystone_both"], cls["quad_jittered"]]
    for wf in WARP_FILTERS:
        check(TEN_BIT, size, maps, [(0,) + WHOLE, (0, 2, 2, 31, 21, 1)], (0, 5), src_size, wf, "uint8", "NCHW", SCALE_BILINEAR, fill=9)
    b = _b(TEN_BIT)
    out = DeviceBuffer.from_numpy(np.full(4096, POISON, np.uint8))
    for dtype in ("float32", "float16", "bfloat16"):
        with pytest.raises(decoder.HipDecError) as ei:
            b.to_tensor_projected(size, maps[:1], src_size=src_size, dtype=dtype, out=out)
        assert ei.value.code == -4 and "10-bit" in ei.value.message, ei.value
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((4096,), np.uint8) == POISON).all()


def test_refusals_have_a_status_a_message_and_leave_the_output_untouched():
    from test_scale_gpu import VUI_FULL, _batch, _still
    L = _lib()
    b = _b(SMALL)
    size, src_size = (16, 8), (9, 7)
    nbytes = 2 * 16 * 8 * 3 * 4
    out = DeviceBuffer.from_numpy(np.full(nbytes, POISON, np.uint8))
    entries = decoder.tensor_entries([(0,) + WHOLE] * 2)
    P, Q = pr.PERSPECTIVE, pr.QUAD

    def call(dtype="uint8", maps=(IDENT, IDENT), fill=None, codes=(0, 1), handle=b._h, room=nbytes, filt=SCALE_BOX, desc=None, warp=None,
             fn=L.hipdec_batch_to_tensor_projected, no_maps=False):
        desc = desc or decoder.tensor_desc(size, dtype, "NCHW", filt, SCALE, BIAS)
        warp = warp or decoder.warp_desc(src_size, SCALE_BILINEAR)
        marr = maps if not isinstance(maps, tuple) else decoder.tensor_projections(maps)
        return fn(handle, C.byref(desc), entries, (C.c_int * 2)(*codes), C.byref(warp), None if no_maps else marr, C.byref(fill) if fill is not None else None,
                  2, out.ptr, room, None)

    def names(text):
        assert text in L.hipdec_last_error(), L.hipdec_last_error()

    def with_coefficient(i, v):
        m = list(IDENT)
        m[i] = v
        return tuple(m)

    nan, inf = float("nan"), float("inf")
    for kind in (P, Q):
        for i, bad in ((0, nan), (2, inf), (4, -inf), (6, nan), (7, inf)):                           # a coefficient that is not finite
            _refused(L, call(maps=(IDENT, (kind, with_coefficient(i, bad)))), -1)
            names(b"entry 1"); names(b"not finite")
        for i, bad in ((0, 32000.0), (1, -32000.0), (5, 40000.0), (6, 32000.0), (7, -1e9)):          # |a[i]| >= 32000
            _refused(L, call(maps=((kind, with_coefficient(i, bad)), IDENT)), -1)
            names(b"entry 0"); names(b"32000")
    for m in pr.map_classes(src_size, size):                                                        # (what the restatement says of the maps used below)
        assert not pr.refused(m[2], m[1], size)
    corner_maps = [(P, (1, 0, 31985.0, 0, 1, 0, 0, 0)), (P, (1, 0, 0, 0, 1, 31993.0, 0, 0)), (P, (-2000.0, 0, 0, 0, 1, 0, 0, 0)), (P, (1, 0, 0, 0, 1, 0, -1.0 / 16.001, 0)),
                   (Q, (31985.0, 1, 0, 0, 0, 0, 1, 0)), (Q, (0, 0, 0, 250.0, 0, 0, 0, 1.0)), (Q, (0, 0, 0, 0, 31993.0, 0, 1, 0))]
    for bad in corner_maps:                                                                         # a corner of [0, 16] x [0, 8]
        assert pr.refused(bad[1], bad[0], size)
        _refused(L, call(maps=(IDENT, bad)), -1)
        names(b"entry 1"); names(b"corner"); names(b"32000")
    for bad in ((1, 0, 0, 0, 1, 0, -1.0 / 16, 0), (1, 0, 0, 0, 1, 0, -1.0 / 16.00001, 0), (1, 0, 0, 0, 1, 0, 0, -0.2), (1, 0, 0, 0, 1, 0, -0.1, -0.1)):   # the denominator
        assert pr.refused(bad, P, size)
        _refused(L, call(maps=(IDENT, bad)), -1)
        names(b"entry 1"); names(b"denominator")
    for kind in (2, -1, 7):                                                                         # the kind, `reserved`
        _refused(L, call(maps=(IDENT, (kind, IDENT))), -1)
        names(b"entry 1"); names(b"kind")
    marr = decoder.tensor_projections((IDENT, IDENT))
    marr[0].reserved = 1
    _refused(L, call(maps=marr), -1)
    names(b"entry 0"); names(b"reserved")
    assert call(maps=(IDENT, (1, 0, 31983.5, 0, 1, 0, 0, 0)), handle=None) == -1                    # (a corner at 31999.5 passes: the NULL handle is what is left)
    names(b"bad arguments")
    for ssz in ((32768, 7), (9, 32768), (0, 7), (9, -1)):                                          # the source size
        _refused(L, call(warp=decoder.warp_desc(ssz, SCALE_BILINEAR)), -1)
        names(b"source size")
    for wf in (SCALE_BOX, 2, -1, 18):                                                              # BOX has no projection; unknown filters
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
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_projected), -1)
    _refused(L, call(filt=2), -1)                                                                  # what the sibling calls refuse: an unknown resize filter ...
    _refused(L, call(desc=decoder.tensor_desc((0, 8), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)), -1)
    bad_entries = decoder.tensor_entries([(0,) + WHOLE, (0, 70, 0, 10, 10, 0)])                     # ... a window that leaves the picture ...
    _refused(L, L.hipdec_batch_to_tensor_projected(b._h, C.byref(decoder.tensor_desc(size, "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)), bad_entries, None,
                                                   C.byref(decoder.warp_desc(src_size)), decoder.tensor_projections((IDENT, IDENT)), None, 2, out.ptr, nbytes, None), -1)
    names(b"entry 1")
    _refused(L, call("float32", handle=_b(TEN_BIT)._h), -4)                                        # ... and a float dtype from a 10-bit source
    small = _batch([_still(1, 8, VUI_FULL, (72, 40))] * 2, max_image_size_pixels=72 * 40)
    try:
        big = decoder.tensor_desc((80, 40), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
        room = DeviceBuffer(2 * 80 * 40 * 3)
        _refused(L, L.hipdec_batch_to_tensor_projected(small._h, C.byref(big), None, None, C.byref(decoder.warp_desc(src_size)), decoder.tensor_projections((IDENT, IDENT)),
                                                       None, 2, room.ptr, room.nbytes, None), -5)
    finally:
        small.free()
    # 2^31 tiles or more: HIPDEC_ERR_LIMIT, decided on the arguments alone (46341 x 46341 pixels are 725 x 2897 tiles; times 1023 entries)
    huge = decoder.tensor_desc((46341, 46341), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
    many = decoder.tensor_projections([(0.001, 0, 0, 0, 0.001, 0, 0, 0)] * 1023)
    wd = decoder.warp_desc(src_size)
    _refused(L, L.hipdec_tensor_project(out.ptr, 1 << 40, C.byref(wd), many, None, C.byref(huge), 1023, out.ptr, 1 << 62, None), -5)
    names(b"tiles")
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((nbytes,), np.uint8) == POISON).all()
    s0, w0 = decoder.project_stats(), decoder.warp_stats()
    assert call() == 0                                                                             # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    assert decoder.project_stats() == (s0[0] + 1, s0[1] + 2) and decoder.warp_stats() == w0
    assert call(maps=(IDENT, (Q, (1, 0, 0, 0, 1, 0, -1.0 / 16, 0)))) == 0                           # (QUAD has no denominator: a6 is a coefficient of yin)
    decoder.check(L.hipdec_stream_synchronize(None))
    with pytest.raises(ValueError):
        b.to_tensor_projected(size, [IDENT, IDENT], dtype="uint8")                                 # two maps for one entry
    with pytest.raises(ValueError):
        b.to_tensor_projected(size, [IDENT[:6]], dtype="uint8")
    with pytest.raises(ValueError):
        b.to_tensor_projected(size, [("mesh", IDENT)], dtype="uint8")
    with pytest.raises(ValueError):
        b.to_tensor_projected(size, [IDENT], dtype="uint8", fill_domain="pixel")


@pytest.mark.parametrize("wf", WARP_FILTERS)
def test_one_resize_launch_and_one_project_launch_per_call_and_the_stats_advance_by_the_entries(wf):
    """hipdec_project_stats counts launches of the projective kernel as its calls; hipdec_warp_stats does not move"""
    b = _b(SMALL)
    src_size, size = (33, 17), (65, 17)
    maps = _maps(src_size, size)                           # twelve entries with twelve different maps, both kinds
    n = len(maps)
    o0, p0, t0, w0 = decoder.oriented_stats(), decoder.project_stats(), decoder.tensor_stats(), decoder.warp_stats()
    run_projected(b, size, maps, [(0,) + WHOLE] * n, [k % 8 for k in range(n)], src_size, wf, "float16", "NCHW", SCALE_BOX)
    o1, p1, t1 = decoder.oriented_stats(), decoder.project_stats(), decoder.tensor_stats()
    assert (o1[0] - o0[0], o1[1] - o0[1]) == (1, n)
    assert (p1[0] - p0[0], p1[1] - p0[1]) == (1, n)
    assert (t1[0] - t0[0], t1[1] - t0[1]) == (1, n)
    assert decoder.warp_stats() == w0


def test_the_map_helpers_of_the_package_are_the_c_helpers():
    q = decoder.quad_map([(1.5, 2.0), (0.25, 16.5), (30.0, 17.0), (33.0, -1.0)], (65, 17))
    assert isinstance(q, TensorProjection) and q.kind == pr.QUAD and tuple(q.a) == pr.quad_map((1.5, 2.0, 0.25, 16.5, 30.0, 17.0, 33.0, -1.0), (65, 17))
    start, end = [(3.0, 5.0), (210.0, 11.0), (200.0, 190.0), (17.0, 222.0)], [(0.0, 0.0), (223.0, 0.0), (223.0, 223.0), (0.0, 223.0)]
    p = decoder.perspective_map(start, end)
    assert p.kind == pr.PERSPECTIVE
    np.testing.assert_allclose(tuple(p.a), pr.perspective_map_exact(start, end), rtol=1e-9, atol=1e-12)
    with pytest.raises(decoder.HipDecError):
        decoder.perspective_map([(0.0, 0.0)] * 4, end)                                              # singular: four equal start points
    with pytest.raises(decoder.HipDecError):
        decoder.quad_map([(0.0, 0.0)] * 4, (0, 4))
