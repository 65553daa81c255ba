"""Photometric tensor output on the device: hipdec_tensor_photo, hipdec_batch_to_tensor_photo, hipdec_album_to_tensor_photo (Pillow-exact ColorJitter /
RandAugment colour operations on the resized 8-bit picture, chained, normalised; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code:
  stage         tests/photo_ref.py applied to synthetic uint8 samples: the NumPy restatement that tests/test_photo_ref.py pins to PIL.ImageEnhance / ImageOps.
  intermediate  (decode-side forms) what the library's EXISTING hipdec_batch_to_tensor_oriented returns for the same entries and codes with dtype U8, layout
                NHWC (Batch.to_tensor(..., orientations=)); pinned by tests/test_oriented_gpu.py and tests/test_resample_gpu.py, not under test here.
  float stage   float32(V) * scale + bias in NumPy float32, .astype(float16) / the bfloat16 rounding on the bits (tests/test_tensor_gpu.py elements).
The output buffer is 256 bytes longer than the tensor and pre-filled with 0xA5: the tail must come back untouched.

The kernels' constants (photo_kernels.h): k_photo_apply's tile is 64 x 16 pixels (kWarpTC x kWarpTR), four pixels per lane, SHARPNESS stages the tile
with a one-pixel halo; k_photo_hist gives a workgroup 64 rows of a sample (kPhotoHistRows), one LDS histogram copy per wave of 64 lanes.  Sizes
(width x height): 1 x 1, 1 x 7, 7 x 1, 2 x 2; 3 x 3 - the first with an interior pixel; 65 x 17 - one column and one row beyond a tile, so the halo crosses
tile edges both ways; 3 x 65 - one row more than a histogram workgroup's slice, so two workgroups add into one histogram.

Runs on the MI355X (`-m gpu`) and, through tests/test_photo_emu.py, against the library compiled for the host."""
import ctypes as C

import numpy as np
import pytest

import photo_ref as pr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album
from test_oriented_gpu import FORMATS, SMALL, _b, _free_batches, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits, elements

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (65, 17), (3, 65)]      # (width, height)
POISON = 0xA5
ES = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
WHOLE = (0, 0, 0, 0, 0)
TEN_BIT = FORMATS[3]
# every operation alone; the enhancers with a factor inside [0, 1], above 1 and below 0
ALONE = [[(pr.BRIGHTNESS, 0.4)], [(pr.BRIGHTNESS, 1.7)], [(pr.COLOR, 0.0)], [(pr.COLOR, 1.6)], [(pr.COLOR, -0.5)], [(pr.CONTRAST, 0.3)], [(pr.CONTRAST, 1.9)],
         [(pr.SHARPNESS, 0.0)], [(pr.SHARPNESS, 1.8)], [(pr.SHARPNESS, -1.0)], [(pr.POSTERIZE, 3)], [(pr.POSTERIZE, 0)], [(pr.POSTERIZE, 8)],
         [(pr.SOLARIZE, 128)], [(pr.SOLARIZE, 100.5)], [(pr.INVERT, 0)], [(pr.AUTOCONTRAST, 0)], [(pr.EQUALIZE, 0)]]


def samples(n, size, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, size[1], size[0], 3), dtype=np.uint8)


def expected(src, chains, dtype, layout):
    n = len(chains)
    exp = np.stack([elements(pr.apply_chain(src[e], chains[e]), dtype, SCALE, BIAS) for e in range(n)])
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def run_stage(src, chains, dtype="uint8", layout="NHWC"):
    """the stage alone into a poisoned buffer 256 bytes longer than the tensor; returns the tensor's bit patterns"""
    n, h, w, _ = src.shape
    nbytes = src.size * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    sbuf = DeviceBuffer.from_numpy(src)
    got = as_bits(decoder.tensor_photo(sbuf, chains, src_size=(w, h), dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out, to_host=True))
    assert got.shape == ((n, 3, h, w) if layout == "NCHW" else (n, h, w, 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    assert np.array_equal(sbuf.to_numpy(src.shape, np.uint8), src), "the source was written"
    return got


def check_stage(src, chains, dtype="uint8", layout="NHWC"):
    got, exp = run_stage(src, chains, dtype, layout), expected(src, chains, dtype, layout)
    bad = [(e, chains[e], int((got[e] != exp[e]).sum())) for e in range(len(chains)) if not np.array_equal(got[e], exp[e])]
    assert not bad, (src.shape, dtype, layout, bad)
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_operation_alone_at_every_size(dtype, layout):
    for k, size in enumerate(SIZES):
        check_stage(samples(len(ALONE), size, 10 + k), ALONE, dtype, layout)


def test_entries_with_different_chains_of_lengths_0_to_4_share_the_launches():
    chains = [[], [(pr.SHARPNESS, 1.5)], [(pr.BRIGHTNESS, 0.6), (pr.CONTRAST, 1.4)], [(pr.POSTERIZE, 3), (pr.EQUALIZE, 0), (pr.COLOR, 0.5)],
              [(pr.SHARPNESS, 1.8), (pr.AUTOCONTRAST, 0), (pr.SOLARIZE, 90.0), (pr.SHARPNESS, 0.2)], [(pr.EQUALIZE, 0), (pr.EQUALIZE, 0), (pr.INVERT, 0), (pr.CONTRAST, 0.0)], []]
    for size in ((65, 17), (3, 65), (3, 3)):
        src = samples(len(chains), size, 77)
        s0 = decoder.photo_stats()
        for dtype, layout in (("uint8", "NHWC"), ("float16", "NCHW")):
            check_stage(src, chains, dtype, layout)
        s1 = decoder.photo_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (2, 2 * len(chains))
        assert s1[2] - s0[2] == 2 * (4 + 3)            # four apply launches; statistics are needed at steps 0, 1 and 3


@pytest.mark.parametrize("chain", [[(pr.BRIGHTNESS, 0.55), (pr.CONTRAST, 1.6)], [(pr.POSTERIZE, 2), (pr.EQUALIZE, 0)], [(pr.SHARPNESS, 2.0), (pr.AUTOCONTRAST, 0)]],
                         ids=["brightness_contrast", "posterize_equalize", "sharpness_autocontrast"])
def test_later_statistics_are_those_of_the_earlier_steps_result(chain):
    for size in ((65, 17), (3, 65)):
        src = (samples(3, size, 5) // 2 + 40).astype(np.uint8)      # a range of 40 .. 167: the first step changes what the second one measures
        got = check_stage(src, [chain] * 3, "uint8", "NHWC")
        alone = np.stack([pr.apply_op(pr.apply_op(src[e], *chain[0]), chain[1][0], 0.0 if chain[1][0] != pr.CONTRAST else chain[1][1]) for e in range(3)])
        assert np.array_equal(got, alone)
        if size == (65, 17):                                       # (the second step is not the identity there, and measuring the source would differ)
            first = np.stack([pr.apply_op(src[e], *chain[0]) for e in range(3)])
            wrong = np.stack([pr.apply_op(src[e], *chain[1]) for e in range(3)])
            assert not np.array_equal(got, first) and not np.array_equal(got, wrong)


def test_a_flat_sample():
    for size in ((1, 1), (7, 1), (65, 17)):
        src = np.broadcast_to(np.array([31, 200, 117], np.uint8), (1, size[1], size[0], 3)).copy()
        got = check_stage(np.repeat(src, 3, axis=0), [[(pr.CONTRAST, 0.0)], [(pr.EQUALIZE, 0)], [(pr.AUTOCONTRAST, 0)]])
        assert np.array_equal(got[1], src[0]) and np.array_equal(got[2], src[0])
        m = pr.contrast_mean(int(pr.lum(src[0]).sum()), size[0] * size[1])
        assert (got[0] == m).all()
    grey = np.full((1, 17, 65, 3), 93, np.uint8)
    assert np.array_equal(check_stage(grey, [[(pr.CONTRAST, 0.0)]]), grey)       # CONTRAST with f = 0 returns a flat grey sample


def test_a_mean_of_exactly_one_half_rounds_up():
    src = np.array([[[[10, 10, 10], [11, 11, 11]]]], np.uint8)                   # 1 x 2, greys 10 and 11: mean 10.5, m = 11
    got = check_stage(src, [[(pr.CONTRAST, 0.0)]])
    assert (got == 11).all()


def test_equalize_with_step_one_and_step_zero():
    rng = np.random.default_rng(16)
    one = rng.integers(0, 200, (16, 16, 3), dtype=np.uint8)
    one[5, 9] = 200                                                              # exactly one pixel at its maximum: w * h - H[last] = 255, step 1
    two = one.copy()
    two[11, 2] = 200                                                             # two: 254, step 0 - the identity
    got = check_stage(np.stack([one, two]), [[(pr.EQUALIZE, 0)]] * 2)
    assert not np.array_equal(got[0], one) and np.array_equal(got[1], two)


def test_a_non_trivial_equalize():
    src = samples(2, (33, 17), 21)
    got = check_stage(src, [[(pr.EQUALIZE, 0)]] * 2, "float32", "NCHW")
    assert got.shape == (2, 3, 17, 33)
    assert not np.array_equal(pr.apply_op(src[0], pr.EQUALIZE), src[0])


def test_autocontrast_over_512_random_ranges_per_channel():
    """every sample holds every value of its range [lo, hi] of each channel (16 x 16 = 256 pixels)"""
    rng = np.random.default_rng(512)
    src = np.empty((512, 16, 16, 3), np.uint8)
    for e in range(512):
        for c in range(3):
            lo = int(rng.integers(0, 255))
            hi = int(rng.integers(lo + 1, 256))
            vals = np.concatenate([np.arange(lo, hi + 1), rng.integers(lo, hi + 1, 256 - (hi - lo + 1))])
            src[e, :, :, c] = rng.permutation(vals).reshape(16, 16)
    check_stage(src, [[(pr.AUTOCONTRAST, 0)]] * 512)


def test_the_same_call_twice_gives_the_same_bytes():
    chains = [[(pr.EQUALIZE, 0), (pr.SHARPNESS, 1.3), (pr.CONTRAST, 1.2)], [(pr.AUTOCONTRAST, 0)], [(pr.COLOR, 0.3), (pr.CONTRAST, 0.7)]]
    src = samples(3, (65, 17), 9)
    first = run_stage(src, chains, "bfloat16", "NCHW")
    assert np.array_equal(run_stage(src, chains, "bfloat16", "NCHW"), first)
    assert np.array_equal(first, expected(src, chains, "bfloat16", "NCHW"))


def test_no_entries_and_the_counters():
    L = _lib()
    out = DeviceBuffer.from_numpy(np.full(64, POISON, np.uint8))
    sbuf = DeviceBuffer.from_numpy(samples(2, (3, 3), 1))
    desc = decoder.tensor_desc((3, 3), "uint8", "NCHW", 0, SCALE, BIAS)
    pd = decoder.photo_desc((3, 3))
    s0 = decoder.photo_stats()
    assert L.hipdec_tensor_photo(sbuf.ptr, sbuf.nbytes, C.byref(pd), None, C.byref(desc), 0, out.ptr, 64, None) == 0
    assert L.hipdec_tensor_photo(None, 0, C.byref(pd), None, C.byref(desc), 0, None, 0, None) == 0
    decoder.check(L.hipdec_stream_synchronize(None))
    assert decoder.photo_stats() == s0 and (out.to_numpy((64,), np.uint8) == POISON).all()
    assert decoder.tensor_photo(sbuf, [], src_size=(3, 3), dtype="uint8", to_host=True).shape == (0, 3, 3, 3)
    # steps without statistics launch no histogram kernel: one launch per step
    src = samples(4, (65, 17), 2)
    check_stage(src, [[(pr.BRIGHTNESS, 1.2), (pr.SHARPNESS, 0.5), (pr.POSTERIZE, 4), (pr.COLOR, 0.2)], [(pr.INVERT, 0)], [], [(pr.SOLARIZE, 64), (pr.SOLARIZE, 200)]])
    s1 = decoder.photo_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, 4, 4)
    # ... and never more than two per step of the longest chain
    check_stage(src, [[(pr.CONTRAST, 1.2)] * 4, [(pr.EQUALIZE, 0)] * 3, [(pr.AUTOCONTRAST, 0)], []])
    s2 = decoder.photo_stats()
    assert (s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2]) == (1, 4, 8)
    check_stage(src[:1], [[]])                                                    # an empty chain alone: one launch, the float stage
    assert decoder.photo_stats()[2] - s2[2] == 1


# ---- the decode-side forms
def run_photo(h, size, chains, entries, codes, dtype, layout, filt):
    n = len(chains)
    nbytes = n * 3 * size[0] * size[1] * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    assert h.to_tensor_photo(size, chains, entries, filter=filt, orientations=codes, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out) is out
    got = as_bits(h.tensor_to_host())
    assert got.shape == ((n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    return got


FORM_ENTRIES = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0), (0, 36, 20, 31, 19, 1)]
FORM_CODES = (1, 6, 0, 3)
FORM_CHAINS = [[(pr.CONTRAST, 1.4), (pr.SHARPNESS, 1.6)], [], [(pr.EQUALIZE, 0)], [(pr.COLOR, 0.0), (pr.AUTOCONTRAST, 0), (pr.POSTERIZE, 5)]]


@pytest.mark.parametrize("dtype,layout,filt", [("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_BILINEAR), ("float32", "NHWC", SCALE_BICUBIC), ("bfloat16", "NCHW", SCALE_NEAREST)])
def test_batch_form_over_an_8_bit_still(dtype, layout, filt):
    b = _b(SMALL)
    for size in ((33, 17), (65, 17)):
        mid = run_oriented(b, size, FORM_ENTRIES, FORM_CODES, "uint8", "NHWC", filt)
        got = run_photo(b, size, FORM_CHAINS, FORM_ENTRIES, FORM_CODES, dtype, layout, filt)
        assert np.array_equal(got, expected(mid, FORM_CHAINS, dtype, layout)), (size, dtype, layout, filt)
        want = run_oriented(b, size, FORM_ENTRIES, FORM_CODES, dtype, layout, filt)          # empty chains: the oriented call's bytes
        assert np.array_equal(run_photo(b, size, [[]] * 4, FORM_ENTRIES, FORM_CODES, dtype, layout, filt), want)


def test_a_ten_bit_still_goes_through_as_uint8_and_is_refused_as_float():
    L = _lib()
    b = _b(TEN_BIT)
    size = (33, 17)
    entries, codes = [(0,) + WHOLE, (0, 2, 2, 31, 21, 1)], (0, 5)
    chains = [[(pr.CONTRAST, 1.3), (pr.EQUALIZE, 0)], [(pr.SHARPNESS, 0.4)]]
    mid = run_oriented(b, size, entries, codes, "uint8", "NHWC", SCALE_BILINEAR)
    for layout in LAYOUTS:
        assert np.array_equal(run_photo(b, size, chains, entries, codes, "uint8", layout, SCALE_BILINEAR), expected(mid, chains, "uint8", layout))
    out = DeviceBuffer.from_numpy(np.full(16384, POISON, np.uint8))
    for dtype in ("float32", "float16", "bfloat16"):
        with pytest.raises(decoder.HipDecError) as ei:
            b.to_tensor_photo(size, [[(pr.INVERT, 0)]], dtype=dtype, out=out)
        assert ei.value.code == -4 and "10-bit" in ei.value.message, ei.value
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((16384,), np.uint8) == POISON).all()


@pytest.mark.parametrize("kind", ["444", "mixed10"])
def test_album_form(kind):
    """two 8-bit 4:4:4 photos, and 10-bit photos (U8 only)"""
    from test_album_gpu import _photos
    a = Album(_photos(kind))
    try:
        a.run()
        a.status()
        size = (33, 17)
        entries, codes = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 1), (0, 33, 11, 71, 57, 0), (1, 1, 1, 63, 61, 0)], (3, 0, 6, 5)
        wide = a.info(0)["bit_depth_luma"] > 8
        for dtype, layout, filt in (("uint8", "NHWC", SCALE_BOX), ("uint8", "NCHW", SCALE_BILINEAR)) + (() if wide else (("float16", "NCHW", SCALE_BICUBIC),)):
            out = DeviceBuffer(4 * 3 * size[0] * size[1])
            a.to_tensor(size, entries, dtype="uint8", layout="NHWC", filter=filt, out=out, orientations=codes)
            mid = a.tensor_to_host()
            assert np.array_equal(run_photo(a, size, FORM_CHAINS, entries, codes, dtype, layout, filt), expected(mid, FORM_CHAINS, dtype, layout)), (dtype, layout, filt)
            a.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=DeviceBuffer(4 * 3 * size[0] * size[1] * ES[dtype]), orientations=codes)
            want = as_bits(a.tensor_to_host())
            assert np.array_equal(run_photo(a, size, [[]] * 4, entries, codes, dtype, layout, filt), want)
        if wide:
            with pytest.raises(decoder.HipDecError) as ei:
                a.to_tensor_photo(size, [[]] * 4, entries, dtype="float16")
            assert ei.value.code == -4
    finally:
        a.free()


def _chain(*ops, n_ops=None, reserved=0):
    ch = decoder.PhotoChain()
    ch.n_ops = len(ops) if n_ops is None else n_ops
    ch.reserved = reserved
    for k, o in enumerate(ops):
        ch.ops[k].op, ch.ops[k].value = o[0], o[1]
        ch.ops[k].reserved = o[2] if len(o) > 2 else 0
    return ch


def test_refusals_have_a_status_a_message_and_leave_the_output_untouched():
    L = _lib()
    b = _b(SMALL)
    size = (16, 8)
    nbytes = 2 * 16 * 8 * 3 * 4
    out = DeviceBuffer.from_numpy(np.full(nbytes, POISON, np.uint8))
    entries = decoder.tensor_entries([(0,) + WHOLE] * 2)
    good = _chain((pr.CONTRAST, 1.2))

    def call(dtype="uint8", chains=(good, good), codes=(0, 1), handle=b._h, room=nbytes, filt=SCALE_BOX, desc=None, photo=None, fn=L.hipdec_batch_to_tensor_photo, no_chains=False):
        desc = desc or decoder.tensor_desc(size, dtype, "NCHW", filt, SCALE, BIAS)
        photo = photo or decoder.photo_desc(size)
        return fn(handle, C.byref(desc), entries, (C.c_int * 2)(*codes), C.byref(photo), None if no_chains else decoder.photo_chains(chains), 2, out.ptr, room, None)

    def names(*texts):
        for text in texts:
            assert text in L.hipdec_last_error(), L.hipdec_last_error()

    nan, inf = float("nan"), float("inf")
    for n_ops in (-1, 5):
        _refused(L, call(chains=(good, _chain(n_ops=n_ops))), -1)
        names(b"entry 1", b"n_ops")
    for op in (0, 10, -3):
        _refused(L, call(chains=(_chain((pr.INVERT, 0), (op, 1.0)), good)), -1)
        names(b"entry 0", b"operation 1", b"unknown op")
    _refused(L, call(chains=(good, _chain((pr.COLOR, 1.0, 7)))), -1)
    names(b"entry 1", b"operation 0", b"COLOR", b"reserved")
    _refused(L, call(chains=(good, _chain(reserved=1))), -1)
    names(b"entry 1", b"reserved")
    for v in (nan, inf, -inf):
        _refused(L, call(chains=(good, _chain((pr.BRIGHTNESS, 1.0), (pr.SHARPNESS, v)))), -1)
        names(b"entry 1", b"operation 1", b"SHARPNESS", b"not finite")
    for v in (65536.5, -1e9):
        _refused(L, call(chains=(_chain((pr.SOLARIZE, v)), good)), -1)
        names(b"entry 0", b"operation 0", b"SOLARIZE", b"65536")
    for v in (2.5, -1.0, 9.0):
        _refused(L, call(chains=(good, _chain((pr.POSTERIZE, v)))), -1)
        names(b"entry 1", b"POSTERIZE")
    for ssz in ((32768, 8), (16, 32768), (0, 8), (16, -1)):
        _refused(L, call(photo=decoder.photo_desc(ssz)), -1)
        names(b"source size")
    _refused(L, call(photo=decoder.photo_desc((16, 9))), -1)                                       # the tensor's size is not the source size
    names(b"not the source size")
    _refused(L, call(photo=decoder.PhotoDesc(16, 8, (C.c_int * 2)(0, 1))), -1)
    _refused(L, call(no_chains=True), -1)
    _refused(L, call(room=2 * 16 * 8 * 3 - 1), -1)                                                 # out_bytes below hipdec_tensor_bytes
    for bad in (-1, 8):
        _refused(L, call(codes=(0, bad)), -1)
        names(b"entry 1")
    _refused(L, call(handle=None), -1)
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_photo), -1)
    _refused(L, call(filt=2), -1)                                                                  # what the sibling calls refuse: an unknown resize filter
    _refused(L, call("float32", handle=_b(TEN_BIT)._h), -4)                                        # ... and a float dtype from a 10-bit source
    # the stage alone: buffers too small, no source, a negative count, scale that is not finite
    sbuf = DeviceBuffer.from_numpy(samples(2, size, 3))
    pd, chains = decoder.photo_desc(size), decoder.photo_chains((good, good))

    def stage(src=sbuf.ptr, sbytes=sbuf.nbytes, n=2, room=nbytes, desc=None, dst=out.ptr):
        desc = desc or decoder.tensor_desc(size, "float32", "NCHW", 0, SCALE, BIAS)
        return L.hipdec_tensor_photo(src, sbytes, C.byref(pd), chains, C.byref(desc), n, dst, room, None)

    _refused(L, stage(sbytes=sbuf.nbytes - 1), -1)
    names(b"src_bytes")
    _refused(L, stage(room=nbytes - 1), -1)
    names(b"out_bytes")
    _refused(L, stage(src=None), -1)
    _refused(L, stage(dst=None), -1)
    _refused(L, stage(n=-1), -1)
    _refused(L, stage(desc=decoder.tensor_desc(size, "float32", "NCHW", 0, np.array([1, nan, 1], np.float32), BIAS)), -1)
    bad_desc = decoder.tensor_desc(size, "float32", "NCHW", 0, SCALE, BIAS)
    bad_desc.dtype = 4
    _refused(L, stage(desc=bad_desc), -1)
    bad_desc.dtype, bad_desc.layout = 1, 2
    _refused(L, stage(desc=bad_desc), -1)
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((nbytes,), np.uint8) == POISON).all()
    s0 = decoder.photo_stats()
    assert call() == 0 and stage() == 0                                                            # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    s1 = decoder.photo_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (2, 4, 4)
    with pytest.raises(ValueError):
        b.to_tensor_photo(size, [[], []], dtype="uint8")                                           # two chains for one entry
    with pytest.raises(ValueError):
        decoder.photo_chain(*[("invert",)] * 5)
    with pytest.raises(ValueError):
        decoder.photo_chain(("hue", 0.1))


def test_photo_chain_builds_the_structure():
    ch = decoder.photo_chain(("contrast", 1.3), ("posterize", 4), "equalize", (decoder.PHOTO_INVERT,))
    assert ch.n_ops == 4 and ch.reserved == 0
    assert [(o.op, o.value, o.reserved) for o in ch.ops] == [(pr.CONTRAST, 1.3, 0), (pr.POSTERIZE, 4.0, 0), (pr.EQUALIZE, 0.0, 0), (pr.INVERT, 0.0, 0)]
    assert decoder.PHOTO_OPS == pr.NAMES and decoder.PHOTO_MAX_OPS == pr.MAX_OPS
