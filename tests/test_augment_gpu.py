"""Augmented tensor output on the device: hipdec_tensor_augment, hipdec_batch_to_tensor_augmented, hipdec_album_to_tensor_augmented (the photo stage's
operations plus Pillow-exact hue and Gaussian blur, chains of up to eight, normalised; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code:
  stage         tests/augment_ref.py applied to synthetic uint8 samples: the NumPy restatement that tests/test_augment_ref.py pins to Pillow's
                convert("HSV") / convert("RGB") and ImageFilter.GaussianBlur (operations 1 .. 9: tests/photo_ref.py).
  photo stage   chains of at most four photo operations: the bytes of the EXISTING hipdec_tensor_photo.
  intermediate  (decode-side forms) what the EXISTING hipdec_batch_to_tensor_oriented returns for the same entries and codes with dtype U8, layout NHWC
                (Batch.to_tensor(..., orientations=)).
  float stage   as tests/test_photo_gpu.py.
The output buffer is 256 bytes longer than the tensor and pre-filled with 0xA5: the tail must come back untouched, and the source must not be written.

The kernels' constants (augment_kernels.h): k_augment_hue has k_photo_apply's tile of 64 x 16 pixels, four pixels per lane; k_augment_blur's tile is
64 x 32 pixels (kBlurTC x kBlurTR) with a halo of 3 (r + 1) pixels, staged as dwords when the sample's address and its width are multiples of four and
as bytes otherwise; the LDS is sized for whole radii up to 1, 3 or 7.  Sizes (width x height): 1 x 1, 1 x 7, 7 x 1, 2 x 2, 3 x 3; 65 x 33 - one column
and one row beyond a blur tile; 5 x 70 - narrower than any halo and taller than two tiles; 130 x 3 - three tiles across; 72 x 34 - a width that is a
multiple of four, the dword staging, beyond a tile both ways.

Runs on the MI355X (`-m gpu`) and, through tests/test_augment_emu.py, against the library compiled for the host."""
import ctypes as C

import numpy as np
import pytest

import augment_ref as ar
import photo_ref as pr
from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album
from test_oriented_gpu import FORMATS, SMALL, _b, _free_batches, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_scale_gpu import _refused
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits, elements

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (65, 33), (5, 70), (130, 3), (72, 34)]      # (width, height)
POISON = 0xA5
ES = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
WHOLE = (0, 0, 0, 0, 0)
TEN_BIT = FORMATS[3]
ALONE = [[(ar.HUE, d)] for d in (0, 1, 128, 255)] + [[(ar.GAUSSIAN_BLUR, rho)] for rho in (0, 0.1, 1.0, 2.0, 4.0, 8.0)]
STATS = (pr.CONTRAST, pr.AUTOCONTRAST, pr.EQUALIZE)


def samples(n, size, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, size[1], size[0], 3), dtype=np.uint8)


def expected(src, chains, dtype, layout):
    n = len(chains)
    exp = np.stack([elements(ar.apply_chain(src[e], chains[e]), dtype, SCALE, BIAS) for e in range(n)])
    return exp.transpose(0, 3, 1, 2) if layout == "NCHW" else exp


def run_stage(src, chains, dtype="uint8", layout="NHWC", call=None):
    """the stage alone into a poisoned buffer 256 bytes longer than the tensor; returns the tensor's bit patterns"""
    n, h, w, _ = src.shape
    nbytes = src.size * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    sbuf = DeviceBuffer.from_numpy(src)
    got = as_bits((call or decoder.tensor_augment)(sbuf, chains, src_size=(w, h), dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out, to_host=True))
    assert got.shape == ((n, 3, h, w) if layout == "NCHW" else (n, h, w, 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    assert np.array_equal(sbuf.to_numpy(src.shape, np.uint8), src), "the source was written"
    return got


def check_stage(src, chains, dtype="uint8", layout="NHWC"):
    got, exp = run_stage(src, chains, dtype, layout), expected(src, chains, dtype, layout)
    bad = [(e, chains[e], int((got[e] != exp[e]).sum())) for e in range(len(chains)) if not np.array_equal(got[e], exp[e])]
    assert not bad, (src.shape, dtype, layout, bad)
    return got


def launches(chains):
    """the launch rule: per chain step at most one launch each of k_photo_hist, k_photo_apply, k_augment_hue and k_augment_blur, each only if an entry's
    operation at that step is of its kind (an empty chain's identity step is k_photo_apply's)"""
    total = 0
    for t in range(max(1, max(len(c) for c in chains))):
        ops = [c[t][0] if c else 0 for c in chains if t < max(len(c), 1)]
        total += any(o in STATS for o in ops) + any(o <= 9 for o in ops) + any(o == ar.HUE for o in ops) + any(o == ar.GAUSSIAN_BLUR for o in ops)
    return total


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hue_and_blur_alone_at_every_size(dtype, layout):
    for k, size in enumerate(SIZES):
        check_stage(samples(len(ALONE), size, 10 + k), ALONE, dtype, layout)


def _radii_for_every_r():
    radii = {}
    for rho in np.arange(0.0, 8.0001, 0.05):
        radii.setdefault(ar.gaussian_box(float(rho))[0], float(rho))
    assert sorted(radii) == list(range(8))
    return [radii[r] for r in range(8)]


@pytest.mark.parametrize("size", [(130, 70), (132, 40)], ids=["bytes_130x70", "dwords_132x40"])
def test_entries_of_one_call_with_different_radii_and_a_flat_sample(size):
    """whole radii 0 .. 7 in one launch, over three tiles across and two or three down: every halo crosses tile cuts and is clipped at the picture's edges"""
    radii = _radii_for_every_r()
    src = samples(len(radii) + 1, size, 40)
    src[-1] = np.array([31, 200, 117], np.uint8)
    chains = [[(ar.GAUSSIAN_BLUR, rho)] for rho in radii] + [[(ar.GAUSSIAN_BLUR, 3.3)]]
    s0 = decoder.augment_stats()
    got = check_stage(src, chains)
    s1 = decoder.augment_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, len(chains), 1)
    assert np.array_equal(got[-1], src[-1])                                   # blur of a flat sample is the identity
    assert np.array_equal(got[0], src[0])                                     # ... and so is radius 0
    check_stage(src, chains, "float16", "NCHW")


MIXED = [[],
         [(ar.GAUSSIAN_BLUR, 2.0)],
         [(ar.HUE, 43), (pr.CONTRAST, 1.4)],
         [(pr.EQUALIZE, 0), (ar.GAUSSIAN_BLUR, 0.7), (ar.HUE, 200)],
         [(pr.BRIGHTNESS, 0.8), (ar.HUE, 17), (pr.SOLARIZE, 90.0), (ar.GAUSSIAN_BLUR, 1.0)],
         [(pr.SHARPNESS, 1.8), (pr.AUTOCONTRAST, 0), (ar.GAUSSIAN_BLUR, 1.5), (pr.COLOR, 0.3), (ar.HUE, 128)],
         [(ar.HUE, 5), (pr.POSTERIZE, 3), (pr.INVERT, 0), (pr.CONTRAST, 0.5), (ar.GAUSSIAN_BLUR, 0.1), (pr.EQUALIZE, 0)],
         [(pr.BRIGHTNESS, 1.2), (pr.CONTRAST, 0.9), (pr.COLOR, 1.3), (ar.HUE, 250), (pr.COLOR, 0.0), (ar.GAUSSIAN_BLUR, 1.2), (pr.SOLARIZE, 128)],
         [(ar.GAUSSIAN_BLUR, 3.0), (ar.GAUSSIAN_BLUR, 0.5), (ar.HUE, 1), (ar.HUE, 255), (pr.SHARPNESS, 0.2), (pr.EQUALIZE, 0), (pr.INVERT, 0), (ar.GAUSSIAN_BLUR, 8.0)]]


def test_chains_of_lengths_0_to_8_share_the_launches():
    assert [len(c) for c in MIXED] == list(range(9))
    step0 = [c[0][0] if c else 0 for c in MIXED]
    assert any(o in STATS for o in step0) and any(o <= 9 for o in step0) and ar.HUE in step0 and ar.GAUSSIAN_BLUR in step0      # all four kinds in one step
    assert launches(MIXED) == 4 + 4 + 3 + 4 + 3 + 3 + 1 + 1 and launches([[]]) == 1 and launches([[(pr.INVERT, 0)] * 8, [(ar.HUE, 1)] * 8]) == 16
    for size in ((65, 33), (5, 70), (3, 3)):
        src = samples(len(MIXED), size, 77)
        s0, p0 = decoder.augment_stats(), decoder.photo_stats()
        for dtype, layout in (("uint8", "NHWC"), ("float16", "NCHW")):
            check_stage(src, MIXED, dtype, layout)
        s1 = decoder.augment_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (2, 2 * len(MIXED), 2 * launches(MIXED))
        assert decoder.photo_stats() == p0                                    # the photo stage's counters do not move


def test_later_statistics_are_those_of_the_blurred_picture():
    src = samples(2, (65, 33), 5)
    src[0] = 0
    src[0, :, :3] = 255                                                       # a bright left edge: the blur's clamp repeats it, and the mean rises
    chain = [(ar.GAUSSIAN_BLUR, 4.0), (pr.CONTRAST, 0.0)]
    got = check_stage(src, [chain] * 2)
    for e in range(2):
        blurred = ar.gaussian_blur(src[e], 4.0)
        m_blur = pr.contrast_mean(int(pr.lum(blurred).sum()), 65 * 33)
        m_src = pr.contrast_mean(int(pr.lum(src[e]).sum()), 65 * 33)
        assert (got[e] == m_blur).all()
        if e == 0:
            assert m_blur != m_src, "the sample does not tell the blurred picture's mean from the source's"
    chain = [(ar.HUE, 90), (pr.EQUALIZE, 0)]
    got = check_stage(src, [chain] * 2)
    assert not np.array_equal(got[1], pr.apply_op(src[1], pr.EQUALIZE))       # (the random sample: hue moves values between the channels' histograms)


def test_an_empty_chain_and_photo_chains_are_the_existing_calls_bytes():
    photo = [[], [(pr.SHARPNESS, 1.5)], [(pr.BRIGHTNESS, 0.6), (pr.CONTRAST, 1.4)], [(pr.POSTERIZE, 3), (pr.EQUALIZE, 0), (pr.COLOR, 0.5)],
             [(pr.SHARPNESS, 1.8), (pr.AUTOCONTRAST, 0), (pr.SOLARIZE, 90.0), (pr.SHARPNESS, 0.2)]]
    for size in ((65, 33), (3, 3)):
        src = samples(len(photo), size, 12)
        for dtype, layout in (("uint8", "NHWC"), ("float32", "NCHW"), ("bfloat16", "NHWC")):
            want = run_stage(src, photo, dtype, layout, call=decoder.tensor_photo)
            assert np.array_equal(run_stage(src, photo, dtype, layout), want), (size, dtype, layout)


def test_the_same_call_twice_gives_the_same_bytes():
    src = samples(len(MIXED), (72, 34), 9)
    first = run_stage(src, MIXED, "bfloat16", "NCHW")
    assert np.array_equal(run_stage(src, MIXED, "bfloat16", "NCHW"), first)
    assert np.array_equal(first, expected(src, MIXED, "bfloat16", "NCHW"))


def test_no_entries_and_the_counters():
    L = _lib()
    out = DeviceBuffer.from_numpy(np.full(64, POISON, np.uint8))
    sbuf = DeviceBuffer.from_numpy(samples(2, (3, 3), 1))
    desc = decoder.tensor_desc((3, 3), "uint8", "NCHW", 0, SCALE, BIAS)
    pd = decoder.photo_desc((3, 3))
    s0 = decoder.augment_stats()
    assert L.hipdec_tensor_augment(sbuf.ptr, sbuf.nbytes, C.byref(pd), None, C.byref(desc), 0, out.ptr, 64, None) == 0
    assert L.hipdec_tensor_augment(None, 0, C.byref(pd), None, C.byref(desc), 0, None, 0, None) == 0
    decoder.check(L.hipdec_stream_synchronize(None))
    assert decoder.augment_stats() == s0 and (out.to_numpy((64,), np.uint8) == POISON).all()
    assert decoder.tensor_augment(sbuf, [], src_size=(3, 3), dtype="uint8", to_host=True).shape == (0, 3, 3, 3)
    check_stage(samples(1, (7, 1), 3), [[]])                                  # an empty chain alone: one launch, the float stage
    s1 = decoder.augment_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, 1, 1)
    check_stage(samples(2, (7, 1), 3), [[(ar.HUE, 9)] * 8, [(ar.GAUSSIAN_BLUR, 1.0)] * 8])
    assert decoder.augment_stats()[2] - s1[2] == 16


# ---- the decode-side forms
def run_augmented(h, size, chains, entries, codes, dtype, layout, filt):
    n = len(chains)
    nbytes = n * 3 * size[0] * size[1] * ES[dtype]
    out = DeviceBuffer.from_numpy(np.full(nbytes + 256, POISON, np.uint8))
    assert h.to_tensor_augmented(size, chains, entries, filter=filt, orientations=codes, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, out=out) is out
    got = as_bits(h.tensor_to_host())
    assert got.shape == ((n, 3, size[1], size[0]) if layout == "NCHW" else (n, size[1], size[0], 3))
    assert (out.to_numpy((nbytes + 256,), np.uint8)[nbytes:] == POISON).all(), "bytes behind the tensor were written"
    return got


FORM_ENTRIES = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0), (0, 36, 20, 31, 19, 1)]
FORM_CODES = (1, 6, 0, 3)
FORM_CHAINS = [[(pr.CONTRAST, 1.4), (ar.HUE, 30), (pr.SHARPNESS, 1.6), (ar.GAUSSIAN_BLUR, 1.5), (pr.SOLARIZE, 128)], [], [(ar.GAUSSIAN_BLUR, 2.0)],
               [(pr.BRIGHTNESS, 1.1), (pr.CONTRAST, 0.8), (pr.COLOR, 1.2), (ar.HUE, 240), (pr.COLOR, 0.0), (ar.GAUSSIAN_BLUR, 0.6), (pr.SOLARIZE, 100)]]


@pytest.mark.parametrize("dtype,layout,filt", [("uint8", "NHWC", SCALE_BOX), ("float16", "NCHW", SCALE_BILINEAR), ("float32", "NHWC", SCALE_BICUBIC), ("bfloat16", "NCHW", SCALE_NEAREST)])
def test_batch_form_over_an_8_bit_still(dtype, layout, filt):
    b = _b(SMALL)
    for size in ((33, 17), (65, 33)):
        mid = run_oriented(b, size, FORM_ENTRIES, FORM_CODES, "uint8", "NHWC", filt)
        got = run_augmented(b, size, FORM_CHAINS, FORM_ENTRIES, FORM_CODES, dtype, layout, filt)
        assert np.array_equal(got, expected(mid, FORM_CHAINS, dtype, layout)), (size, dtype, layout, filt)
        want = run_oriented(b, size, FORM_ENTRIES, FORM_CODES, dtype, layout, filt)          # empty chains: the oriented call's bytes
        assert np.array_equal(run_augmented(b, size, [[]] * 4, FORM_ENTRIES, FORM_CODES, dtype, layout, filt), want)


def test_a_ten_bit_still_goes_through_as_uint8_and_is_refused_as_float():
    L = _lib()
    b = _b(TEN_BIT)
    size = (33, 17)
    entries, codes = [(0,) + WHOLE, (0, 2, 2, 31, 21, 1)], (0, 5)
    chains = [[(ar.HUE, 100), (pr.EQUALIZE, 0)], [(ar.GAUSSIAN_BLUR, 1.0)]]
    mid = run_oriented(b, size, entries, codes, "uint8", "NHWC", SCALE_BILINEAR)
    for layout in LAYOUTS:
        assert np.array_equal(run_augmented(b, size, chains, entries, codes, "uint8", layout, SCALE_BILINEAR), expected(mid, chains, "uint8", layout))
    out = DeviceBuffer.from_numpy(np.full(16384, POISON, np.uint8))
    for dtype in ("float32", "float16", "bfloat16"):
        with pytest.raises(decoder.HipDecError) as ei:
            b.to_tensor_augmented(size, [[(ar.HUE, 1)]], dtype=dtype, out=out)
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
            assert np.array_equal(run_augmented(a, size, FORM_CHAINS, entries, codes, dtype, layout, filt), expected(mid, FORM_CHAINS, dtype, layout)), (dtype, layout, filt)
            a.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=DeviceBuffer(4 * 3 * size[0] * size[1] * ES[dtype]), orientations=codes)
            want = as_bits(a.tensor_to_host())
            assert np.array_equal(run_augmented(a, size, [[]] * 4, entries, codes, dtype, layout, filt), want)
        if wide:
            with pytest.raises(decoder.HipDecError) as ei:
                a.to_tensor_augmented(size, [[]] * 4, entries, dtype="float16")
            assert ei.value.code == -4
    finally:
        a.free()


def _chain(*ops, n_ops=None, reserved=0):
    ch = decoder.AugmentChain()
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
    good = _chain((pr.CONTRAST, 1.2), (ar.HUE, 3), (ar.GAUSSIAN_BLUR, 1.0), (pr.INVERT, 0), (pr.INVERT, 0))

    def call(dtype="uint8", chains=(good, good), codes=(0, 1), handle=b._h, room=nbytes, filt=SCALE_BOX, desc=None, photo=None, fn=L.hipdec_batch_to_tensor_augmented, no_chains=False, no_photo=False):
        desc = desc or decoder.tensor_desc(size, dtype, "NCHW", filt, SCALE, BIAS)
        photo = photo or decoder.photo_desc(size)
        return fn(handle, C.byref(desc), entries, (C.c_int * 2)(*codes), None if no_photo else C.byref(photo), None if no_chains else decoder.augment_chains(chains), 2, out.ptr, room, None)

    def names(*texts):
        for text in texts:
            assert text in L.hipdec_last_error(), L.hipdec_last_error()

    nan, inf = float("nan"), float("inf")
    for n_ops in (-1, 9):
        _refused(L, call(chains=(good, _chain(n_ops=n_ops))), -1)
        names(b"entry 1", b"n_ops")
    for op in (0, 10, 15, 18, -3):
        _refused(L, call(chains=(_chain((pr.INVERT, 0), (op, 1.0)), good)), -1)
        names(b"entry 0", b"operation 1", b"unknown op")
    _refused(L, call(chains=(good, _chain((ar.HUE, 1.0, 7)))), -1)
    names(b"entry 1", b"operation 0", b"HUE", b"reserved")
    _refused(L, call(chains=(good, _chain(reserved=1))), -1)
    names(b"entry 1", b"reserved")
    for v in (0.5, -1.0, 256.0, 1e9):
        _refused(L, call(chains=(good, _chain((pr.BRIGHTNESS, 1.0), (ar.HUE, v)))), -1)
        names(b"entry 1", b"operation 1", b"HUE", b"0 .. 255")
    for v in (nan, inf, -inf):
        _refused(L, call(chains=(good, _chain((ar.HUE, v)))), -1)
        names(b"entry 1", b"operation 0", b"HUE", b"not finite")
        _refused(L, call(chains=(_chain((pr.INVERT, 0), (pr.INVERT, 0), (pr.INVERT, 0), (pr.INVERT, 0), (pr.INVERT, 0), (ar.GAUSSIAN_BLUR, v)), good)), -1)
        names(b"entry 0", b"operation 5", b"GAUSSIAN_BLUR", b"not finite")
    for v in (-0.1, 8.01, 1e9):
        _refused(L, call(chains=(_chain((ar.GAUSSIAN_BLUR, v)), good)), -1)
        names(b"entry 0", b"operation 0", b"GAUSSIAN_BLUR", b"radius")
    # the photo stage's refusals hold for operations 1 .. 9
    for v in (65536.5, -1e9):
        _refused(L, call(chains=(_chain((pr.SOLARIZE, v)), good)), -1)
        names(b"entry 0", b"operation 0", b"SOLARIZE", b"65536")
    for v in (2.5, -1.0, 9.0):
        _refused(L, call(chains=(good, _chain((pr.POSTERIZE, v)))), -1)
        names(b"entry 1", b"POSTERIZE")
    _refused(L, call(chains=(good, _chain((pr.SHARPNESS, nan)))), -1)
    names(b"SHARPNESS", b"not finite")
    for ssz in ((32768, 8), (16, 32768), (0, 8), (16, -1)):
        _refused(L, call(photo=decoder.photo_desc(ssz)), -1)
        names(b"source size")
    _refused(L, call(photo=decoder.photo_desc((16, 9))), -1)                                       # the tensor's size is not the source size
    names(b"not the source size")
    _refused(L, call(photo=decoder.PhotoDesc(16, 8, (C.c_int * 2)(0, 1))), -1)
    _refused(L, call(no_chains=True), -1)
    _refused(L, call(no_photo=True), -1)
    _refused(L, call(room=2 * 16 * 8 * 3 - 1), -1)                                                 # out_bytes below hipdec_tensor_bytes
    for bad in (-1, 8):
        _refused(L, call(codes=(0, bad)), -1)
        names(b"entry 1")
    _refused(L, call(handle=None), -1)
    _refused(L, call(handle=None, fn=L.hipdec_album_to_tensor_augmented), -1)
    _refused(L, call(filt=2), -1)                                                                  # what the sibling calls refuse: an unknown resize filter
    _refused(L, call("float32", handle=_b(TEN_BIT)._h), -4)                                        # ... and a float dtype from a 10-bit source
    # the stage alone: buffers too small, no source, a negative count, scale that is not finite
    sbuf = DeviceBuffer.from_numpy(samples(2, size, 3))
    pd, chains = decoder.photo_desc(size), decoder.augment_chains((good, good))

    def stage(src=sbuf.ptr, sbytes=sbuf.nbytes, n=2, room=nbytes, desc=None, dst=out.ptr, photo=pd):
        desc = desc or decoder.tensor_desc(size, "float32", "NCHW", 0, SCALE, BIAS)
        return L.hipdec_tensor_augment(src, sbytes, C.byref(photo) if photo is not None else None, chains, C.byref(desc), n, dst, room, None)

    _refused(L, stage(sbytes=sbuf.nbytes - 1), -1)
    names(b"tensor_augment", b"src_bytes")
    _refused(L, stage(room=nbytes - 1), -1)
    names(b"out_bytes")
    _refused(L, stage(src=None), -1)
    _refused(L, stage(dst=None), -1)
    _refused(L, stage(n=-1), -1)
    _refused(L, stage(photo=None), -1)
    _refused(L, stage(desc=decoder.tensor_desc(size, "float32", "NCHW", 0, np.array([1, nan, 1], np.float32), BIAS)), -1)
    bad_desc = decoder.tensor_desc(size, "float32", "NCHW", 0, SCALE, BIAS)
    bad_desc.dtype = 4
    _refused(L, stage(desc=bad_desc), -1)
    bad_desc.dtype, bad_desc.layout = 1, 2
    _refused(L, stage(desc=bad_desc), -1)
    r, ww, fw = C.c_int(), C.c_uint32(), C.c_uint32()
    for v in (nan, inf, -0.5, 8.5):
        assert L.hipdec_gaussian_box(C.c_double(v), C.byref(r), C.byref(ww), C.byref(fw)) == -1
    assert L.hipdec_gaussian_box(C.c_double(1.0), None, C.byref(ww), C.byref(fw)) == -1
    decoder.check(L.hipdec_stream_synchronize(None))
    assert (out.to_numpy((nbytes,), np.uint8) == POISON).all()
    s0 = decoder.augment_stats()
    assert call() == 0 and stage() == 0                                                            # and the same arguments without the fault are taken
    decoder.check(L.hipdec_stream_synchronize(None))
    s1 = decoder.augment_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (2, 4, 2 * 6)                          # hist + apply, hue, blur, apply, apply
    with pytest.raises(ValueError):
        b.to_tensor_augmented(size, [[], []], dtype="uint8")                                       # two chains for one entry


def test_the_python_builders():
    ch = decoder.augment_chain(("contrast", 1.3), ("hue", 43), "equalize", ("gaussian_blur", 1.5), (decoder.PHOTO_INVERT,), (decoder.AUGMENT_HUE, 7),
                               ("GAUSSIAN_BLUR", 0.25), ("solarize", 128))
    assert ch.n_ops == 8 and ch.reserved == 0 and C.sizeof(ch) == 8 + 8 * 16
    assert [(o.op, o.value, o.reserved) for o in ch.ops] == [(pr.CONTRAST, 1.3, 0), (ar.HUE, 43.0, 0), (pr.EQUALIZE, 0.0, 0), (ar.GAUSSIAN_BLUR, 1.5, 0),
                                                             (pr.INVERT, 0.0, 0), (ar.HUE, 7.0, 0), (ar.GAUSSIAN_BLUR, 0.25, 0), (pr.SOLARIZE, 128.0, 0)]
    assert decoder.AUGMENT_OPS == ar.NAMES and decoder.AUGMENT_MAX_OPS == ar.MAX_OPS and decoder.AUGMENT_BLUR_MAX_RADIUS == ar.BLUR_MAX_RADIUS
    assert decoder.PHOTO_OPS == pr.NAMES and decoder.PHOTO_MAX_OPS == pr.MAX_OPS               # the photo stage's names stay
    with pytest.raises(ValueError):
        decoder.augment_chain(*[("invert",)] * 9)
    with pytest.raises(ValueError):
        decoder.augment_chain(("gamma", 2.2))
    with pytest.raises(ValueError):
        decoder.augment_chain(("hue", 1, 2))
    arr = decoder.augment_chains([ch, [("hue", 1)], []])
    assert [c.n_ops for c in arr] == [8, 1, 0]
    with pytest.raises(ValueError):
        decoder.augment_chains([[]], 2)
    assert [decoder.hue_shift(f) for f in (0.0, 0.5, -0.5, 0.1, -0.1)] == [ar.hue_shift(f) for f in (0.0, 0.5, -0.5, 0.1, -0.1)] == [0, 127, 129, 25, 231]
    with pytest.raises(ValueError):
        decoder.hue_shift(0.6)
    for rho in (0, 0.1, 1.0, 1.41, 1.42, 2.0, 4.0, 8.0):
        assert decoder.gaussian_box(rho) == ar.gaussian_box(rho)
    with pytest.raises(decoder.HipDecError):
        decoder.gaussian_box(8.5)
