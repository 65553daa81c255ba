"""Packed tensor output on the device: hipdec_batch_to_tensor_packed / hipdec_album_to_tensor_packed (a size and an offset per entry, dense samples or
patch sequences, all entries in one launch; include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code: the header defines sample e as what the EXISTING
hipdec_batch_to_tensor_oriented writes for the same entry, code, filter, dtype, scale and bias at the sample's own size.  That call
(Batch.to_tensor(..., orientations=), run_oriented of tests/test_oriented_gpu.py) is run once per distinct size and its elements are put where the header
says: densely, or - patches - at offset + t * 3 * P * P + k with t and k computed by the header's index formulas, element by element on index arrays
(place_sample below; no reshape chain that could share a mistake with the kernel).  The reshape / transpose chains the header quotes for m = 1 NHWC and
m = 2 NCHW are held against the formulas once.  References are computed once per (entries, dtype, filter) and shared by all patch sizes.

Every call writes into a buffer pre-filled with 0xA5 that is longer than the tensor and has gaps between the samples: the whole buffer is compared, so gaps
and tail must come back untouched and no poison may survive inside a sample (no expected float element is the poison pattern: asserted).

Runs on the MI355X (`-m gpu`) and, through tests/test_packed_emu.py, against the library compiled for the host."""
import ctypes as C
import numpy as np
import pytest

from libheif_amd import decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Album, TensorPatches, TensorSample
from test_oriented_gpu import CODES, FORMATS, SMALL, _b, _free_batches, run_oriented   # noqa: F401  (_free_batches: the module fixture)
from test_scale_gpu import _batch, _refused, _still
from test_tensor_gpu import BIAS, DTYPES, LAYOUTS, SCALE, _lib, as_bits

pytestmark = pytest.mark.gpu

FILTERS = (SCALE_NEAREST, SCALE_BOX, SCALE_BILINEAR, SCALE_BICUBIC)
POISON = 0xA5
ES = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
BITS = {"uint8": np.uint8, "float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}
WHOLE = (0, 0, 0, 0, 0)
TEN_BIT = FORMATS[3]
TAIL = 64                                                  # elements behind the last sample


def poison(dtype):
    return int.from_bytes(bytes([POISON]) * ES[dtype], "little")


def place_sample(flat, offset, S, P, m, layout):
    """S: (3, h, w), the dense sample.  Writes it into flat from `offset` on as the header defines it - the index formulas, element by element."""
    _, h, w = S.shape
    c, Y, X = np.indices(S.shape, dtype=np.int64)
    if P == 0:
        idx = (c * h + Y) * w + X if layout == "NCHW" else (Y * w + X) * 3 + c
    else:
        assert w % (P * m) == 0 and h % (P * m) == 0
        gw, gy, gx, py, px = w // P, Y // P, X // P, Y % P, X % P
        t = ((gy // m) * (gw // m) + gx // m) * m * m + (gy % m) * m + gx % m
        k = (c * P + py) * P + px if layout == "NCHW" else (py * P + px) * 3 + c
        idx = t * 3 * P * P + k
    assert np.array_equal(np.sort(idx.ravel()), np.arange(3 * h * w)), "the formulas do not fill the sample's range exactly once"
    flat[offset + idx.ravel()] = S.ravel()


def test_the_index_formulas_are_the_reshape_chains_of_the_header():
    rng = np.random.default_rng(5)
    for (w, h, P) in ((24, 16, 4), (12, 36, 6), (8, 8, 1)):
        S = rng.integers(0, 1 << 16, (3, h, w)).astype(np.uint16)
        gh, gw = h // P, w // P
        flat = np.zeros(3 * h * w, np.uint16)
        place_sample(flat, 0, S, P, 1, "NHWC")
        chain = S.transpose(1, 2, 0).reshape(gh, P, gw, P, 3).transpose(0, 2, 1, 3, 4).reshape(gh * gw, P * P * 3)
        assert np.array_equal(flat.reshape(gh * gw, -1), chain), ("m = 1 NHWC", w, h, P)
        place_sample(flat, 0, S, P, 2, "NCHW")
        chain = S.reshape(3, gh // 2, 2, P, gw // 2, 2, P).transpose(1, 4, 2, 5, 0, 3, 6).reshape(gh * gw, 3 * P * P)
        assert np.array_equal(flat.reshape(gh * gw, -1), chain), ("m = 2 NCHW", w, h, P)


_REFERENCES = {}


def references(b, key, sizes, entries, codes, dtype, filt, existing=run_oriented):
    """the dense samples, (3, h, w) bit patterns each, from the EXISTING oriented call - one call per distinct size, computed once per key and left alone"""
    key = (key, tuple(sizes), tuple(entries), tuple(codes), dtype, filt)
    if key not in _REFERENCES:
        out = [None] * len(sizes)
        for size in sorted(set(sizes)):
            idx = [e for e in range(len(sizes)) if sizes[e] == size]
            S = existing(b, size, [entries[e] for e in idx], [codes[e] for e in idx], dtype, "NCHW", filt)
            assert S.shape == (len(idx), 3, size[1], size[0])
            if dtype != "uint8":
                assert not (S == poison(dtype)).any(), "an expected element is the poison pattern"
            for k, e in enumerate(idx):
                out[e] = S[k].copy()
                out[e].setflags(write=False)
        _REFERENCES[key] = out
    return _REFERENCES[key]


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    _REFERENCES.clear()


def gapped_offsets(sizes, gaps):
    """offsets in entry order with gaps[e % len(gaps)] elements in front of sample e"""
    offs, at = [], 0
    for e, (w, h) in enumerate(sizes):
        at += gaps[e % len(gaps)]
        offs.append(at)
        at += 3 * w * h
    return offs


def run_packed(b, sizes, entries, codes, P, m, dtype, layout, filt, offsets):
    """the packed call into a poisoned buffer with TAIL elements behind the last sample; returns the whole buffer as bit patterns"""
    elems = max(o + 3 * w * h for o, (w, h) in zip(offsets, sizes)) + TAIL
    out = DeviceBuffer.from_numpy(np.full(elems * ES[dtype], POISON, np.uint8))
    got = b.to_tensor_packed(sizes, entries, patch=P, merge=m, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, orientations=codes,
                             offsets=offsets, out=out)
    assert got[0] is out and list(got[1]) == list(offsets)
    assert got[2] == ([(h // P, w // P) for w, h in sizes] if P else None)
    host = b.tensor_packed_to_host()                     # (waits for the stream)
    raw = out.to_numpy((elems,), BITS[dtype])
    if P:                                                # the Python read-back: the samples' tokens in entry order
        assert host.shape == (sum((w // P) * (h // P) for w, h in sizes), 3 * P * P)
        assert np.array_equal(as_bits(host).ravel(), np.concatenate([raw[o:o + 3 * w * h] for o, (w, h) in zip(offsets, sizes)]))
    else:
        flat, view = host
        assert np.array_equal(as_bits(flat), raw)
        w, h = sizes[0]
        assert view(0).shape == ((3, h, w) if layout == "NCHW" else (h, w, 3))
    return raw


def check(b, key, sizes, entries, codes, P, m, dtype, layout, filt, gaps=(16,), order=None, existing=run_oriented):
    """order: the entries' places in the buffer (default: entry order)"""
    n = len(sizes)
    order = list(range(n)) if order is None else list(order)
    by_place = gapped_offsets([sizes[e] for e in order], gaps)
    offsets = [0] * n
    for place, e in enumerate(order):
        offsets[e] = by_place[place]
    got = run_packed(b, sizes, entries, codes, P, m, dtype, layout, filt, offsets)
    exp = np.full(got.shape, poison(dtype), BITS[dtype])
    for e, S in enumerate(references(b, key, sizes, entries, codes, dtype, filt, existing)):
        place_sample(exp, offsets[e], S, P, m, layout)
    if not np.array_equal(got, exp):
        bad = [(e, int((got[o:o + 3 * w * h] != exp[o:o + 3 * w * h]).sum())) for e, (o, (w, h)) in enumerate(zip(offsets, sizes))]
        outside = int((got != exp).sum()) - sum(k for _, k in bad)
        assert False, (P, m, dtype, layout, filt, [x for x in bad if x[1]], "outside the samples: %d" % outside)


# ---- the ragged set: three 8-bit items (4:2:0 and 4:2:2 of 72 x 40, 4:4:4 of 41 x 23), eleven entries, all eight codes, windows at odd offsets, a flipped
# entry, entries that share an item; 120 x 72 and 72 x 120 have more than one column tile (96) and row block (64 / 16) of the box stage and more than one
# 65 x 16 tile of the resampler, each with a row-preserving and a quarter-turn code
RAGGED_ITEMS = (SMALL, FORMATS[0], FORMATS[1])
RAGGED = [  # (entry, code, displayed size)
    ((0,) + WHOLE, 0, (24, 48)), ((1, 3, 5, 41, 27, 0), 1, (48, 24)), ((2,) + WHOLE, 2, (120, 72)), ((0, 1, 3, 35, 21, 1), 3, (72, 120)),
    ((1,) + WHOLE, 4, (24, 24)), ((2, 5, 7, 33, 15, 0), 5, (120, 72)), ((0,) + WHOLE, 6, (72, 120)), ((0, 37, 11, 31, 29, 0), 7, (48, 24)),
    ((1,) + WHOLE, 1, (72, 120)), ((2,) + WHOLE, 0, (24, 48)), ((0,) + WHOLE, 3, (120, 72))]
R_ENTRIES, R_CODES, R_SIZES = [r[0] for r in RAGGED], [r[1] for r in RAGGED], [r[2] for r in RAGGED]

_ragged = []


def ragged_batch():
    if not _ragged:
        _ragged.append(_batch([_still(cf, bits, dict(vui), size) for cf, bits, vui, size in RAGGED_ITEMS]))
    return _ragged[0]


@pytest.fixture(scope="module", autouse=True)
def _free_ragged():
    yield
    while _ragged:
        _ragged.pop().free()


def check_ragged(P, m, dtype, layout, filt, **kw):
    check(ragged_batch(), "ragged", R_SIZES, R_ENTRIES, R_CODES, P, m, dtype, layout, filt, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", FILTERS)
def test_ragged_set_in_patches_of_4_merged_2_by_2(filt, dtype, layout):
    """P % 4 == 0: the vector-store path of the blocked store"""
    check_ragged(4, 2, dtype, layout, filt)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", ("float16", "uint8"))
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("P,m", [(6, 1), (6, 2), (12, 1), (12, 2), (0, 1)])
def test_ragged_set_with_patches_that_groups_straddle_with_large_patches_and_dense(P, m, filt, dtype, layout):
    """P = 6: 4-pixel groups and runs straddle patches (the element path); P = 12: 24 x 24 is one token (m = 1) or one merge group; P = 0: dense samples"""
    check_ragged(P, m, dtype, layout, filt)


SMALL_SET = ([(0,) + WHOLE, (0, 1, 3, 35, 21, 1), (0,) + WHOLE, (0, 5, 7, 33, 17, 0)], (0, 1, 6, 7), [(24, 48), (24, 48), (48, 24), (24, 48)])


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("P,m", [(1, 1), (1, 2), (24, 1)])
def test_every_pixel_a_token_and_one_patch_across_a_whole_side(P, m, filt):
    entries, codes, sizes = SMALL_SET
    check(_b(SMALL), "small", sizes, entries, codes, P, m, "float16", "NCHW", filt)
    check(_b(SMALL), "small", sizes, entries, codes, P, m, "uint8", "NHWC", filt)


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_BICUBIC))
@pytest.mark.parametrize("P,m", [(4, 2), (0, 1)])
def test_offsets_in_reverse_order_and_with_odd_gaps(P, m, filt, dtype):
    """odd element gaps: the destinations of the vector stores are not aligned, the runtime test has to fall back to element stores"""
    n = len(R_SIZES)
    for layout in LAYOUTS:
        check_ragged(P, m, dtype, layout, filt, order=range(n - 1, -1, -1))
        check_ragged(P, m, dtype, layout, filt, gaps=(1, 3, 5, 2, 7))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("still", FORMATS[:3], ids=lambda s: "cf%d" % s[0])
def test_chroma_formats(still, filt):
    """4:2:2, 4:4:4 and monochrome with odd width and height"""
    sizes = [(8, 12) if c & 1 else (12, 8) for c in CODES]
    for dtype, layout, P, m in (("float16", "NHWC", 4, 1), ("uint8", "NCHW", 2, 2)):
        check(_b(still), ("format",) + tuple(still[:2]) + (still[3],), sizes, [(0,) + WHOLE] * 8, CODES, P, m, dtype, layout, filt)


@pytest.mark.parametrize("filt", (SCALE_NEAREST, SCALE_BOX))
def test_ten_bit_source_native_depth_floats_and_sdr_bytes(filt):
    """float dtypes carry the native-depth value (the 64-bit stage of the box kernel, RB = 32), uint8 the to-SDR value"""
    sizes = [(40, 72) if c & 1 else (72, 40) for c in CODES]
    for dtype, layout in (("float32", "NCHW"), ("bfloat16", "NHWC"), ("uint8", "NHWC")):
        check(_b(TEN_BIT), "tenbit", sizes, [(0,) + WHOLE] * 8, CODES, 4, 2, dtype, layout, filt)
        check(_b(TEN_BIT), "tenbit", sizes, [(0,) + WHOLE] * 8, CODES, 0, 1, dtype, layout, filt)


def test_ten_bit_source_resampled_takes_uint8_and_refuses_floats():
    L = _lib()
    b = _b(TEN_BIT)
    check(b, "tenbit-resampled", [(24, 16), (16, 24)], [(0,) + WHOLE] * 2, (0, 1), 4, 2, "uint8", "NCHW", SCALE_BILINEAR)
    desc = decoder.tensor_desc((0, 0), "float16", "NCHW", SCALE_BILINEAR, SCALE, BIAS)
    out = DeviceBuffer(3 * 24 * 16 * 2)
    samples = (TensorSample * 1)(TensorSample(24, 16, 0))
    _refused(L, L.hipdec_batch_to_tensor_packed(b._h, C.byref(desc), None, None, samples, C.byref(TensorPatches(4, 2)), 1, out.ptr, out.nbytes, None), -4)


def _album_oriented(a, size, entries, codes, dtype, layout, filt):
    out = DeviceBuffer(len(entries) * 3 * size[0] * size[1] * ES[dtype])
    a.to_tensor(size, entries, dtype=dtype, layout=layout, scale=SCALE, bias=BIAS, filter=filt, out=out, orientations=codes)
    return as_bits(a.tensor_to_host())


def test_album_form():
    """two photos of different grid geometry; one filter per dtype"""
    from test_album_gpu import _photos
    a = Album(_photos("mixed8")[:2])                      # 2 x 3 tiles of 72 x 48 clipped to 200 x 90, and 1 x 1 of 64 x 64
    try:
        a.run()
        a.status()
        entries = [(0,) + WHOLE, (1, 0, 0, 0, 0, 1), (0, 33, 11, 101, 57, 0), (1, 1, 1, 63, 63, 0), (0,) + WHOLE]
        codes, sizes = (3, 5, 6, 1, 0), [(24, 48), (48, 24), (72, 120), (24, 24), (120, 72)]
        for dtype, filt, layout in zip(DTYPES, FILTERS, ("NCHW", "NHWC", "NCHW", "NHWC")):
            for P, m in ((4, 2), (6, 1), (0, 1)):
                check(a, "album", sizes, entries, codes, P, m, dtype, layout, filt, existing=_album_oriented)
    finally:
        a.free()


@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_BILINEAR))
@pytest.mark.parametrize("dtype,layout", [("uint8", "NHWC"), ("bfloat16", "NCHW")])
def test_without_patches_and_back_to_back_it_is_the_oriented_call_byte_for_byte(dtype, layout, filt):
    L = _lib()
    b = _b(SMALL)
    size, codes = (30, 17), (0, 5, 3)
    entries = [(0,) + WHOLE, (0, 3, 5, 41, 27, 1), (0, 1, 1, 9, 9, 0)]
    want = run_oriented(b, size, entries, codes, dtype, layout, filt)
    desc = decoder.tensor_desc((0, 0), dtype, layout, filt, SCALE, BIAS)
    per = 3 * size[0] * size[1]
    samples = (TensorSample * 3)(*(TensorSample(size[0], size[1], e * per) for e in range(3)))
    out = DeviceBuffer.from_numpy(np.full(want.nbytes + 256, POISON, np.uint8))
    decoder.check(L.hipdec_batch_to_tensor_packed(b._h, C.byref(desc), decoder.tensor_entries(entries), (C.c_int * 3)(*codes), samples, None, 3, out.ptr,
                                                  out.nbytes, None))                   # patches = NULL through the C ABI
    decoder.check(L.hipdec_stream_synchronize(None))
    raw = out.to_numpy((want.nbytes + 256,), np.uint8)
    assert np.array_equal(raw[:want.nbytes], want.view(np.uint8).ravel())
    assert (raw[want.nbytes:] == POISON).all()


@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_BICUBIC))
def test_the_same_call_twice_gives_the_same_bytes(filt):
    """(the parameter blocks of the second call equal the first's and are not uploaded again; the sibling tests have no way to observe the upload either)"""
    offsets = gapped_offsets(R_SIZES, (16,))
    first = run_packed(ragged_batch(), R_SIZES, R_ENTRIES, R_CODES, 4, 2, "float16", "NCHW", filt, offsets)
    again = run_packed(ragged_batch(), R_SIZES, R_ENTRIES, R_CODES, 4, 2, "float16", "NCHW", filt, offsets)
    assert np.array_equal(first, again)


def test_statistics_count_calls_entries_and_patch_entries():
    entries, codes, sizes = SMALL_SET
    offsets = gapped_offsets(sizes, (0,))
    before = decoder.packed_stats()
    run_packed(_b(SMALL), sizes, entries, codes, 4, 1, "uint8", "NCHW", SCALE_BOX, offsets)
    middle = decoder.packed_stats()
    run_packed(_b(SMALL), sizes, entries, codes, 0, 1, "uint8", "NCHW", SCALE_NEAREST, offsets)
    after = decoder.packed_stats()
    assert tuple(x - y for x, y in zip(middle, before)) == (1, 4, 4)
    assert tuple(x - y for x, y in zip(after, middle)) == (1, 4, 0)


def test_mixed_sizes_and_codes_share_one_launch():
    before = decoder.oriented_stats()
    run_packed(ragged_batch(), R_SIZES, R_ENTRIES, R_CODES, 6, 2, "float32", "NHWC", SCALE_BOX, gapped_offsets(R_SIZES, (16,)))
    after = decoder.oriented_stats()
    assert tuple(x - y for x, y in zip(after, before)) == (1, len(R_SIZES), sum(c & 1 for c in R_CODES))


def test_refusals_on_a_live_batch():
    """(the refusals the arguments alone decide are listed in tests/test_packed_emu.py, where no device exists)"""
    L = _lib()
    b = _b(SMALL)
    desc = decoder.tensor_desc((0, 0), "uint8", "NCHW", SCALE_BOX, SCALE, BIAS)
    out = DeviceBuffer(3 * 16 * 8 * 2 + 64)
    one = (TensorSample * 1)(TensorSample(16, 8, 0))
    call = L.hipdec_batch_to_tensor_packed
    _refused(L, call(b._h, C.byref(desc), decoder.tensor_entries([(0, 70, 0, 5, 5, 0)]), None, one, None, 1, out.ptr, out.nbytes, None), -1)   # window leaves the picture
    _refused(L, call(b._h, C.byref(desc), None, None, (TensorSample * 2)(TensorSample(16, 8, 0), TensorSample(16, 8, 384)), None, 2, out.ptr, out.nbytes, None), -1)  # two entries, one item
    assert call(b._h, C.byref(desc), None, None, one, C.byref(TensorPatches(8, 1)), 1, out.ptr, out.nbytes, None) == 0
    decoder.check(L.hipdec_stream_synchronize(None))
    with pytest.raises(ValueError):
        b.to_tensor_packed([(16, 8), (16, 8)], None, out=out)                          # two sizes for one entry
    with pytest.raises(ValueError):
        decoder.packed_layout([(16, 8)], 6, 1)
    assert decoder.packed_layout([(16, 8), (8, 24)], 4, 2) == ([0, 384], [8, 12], 960)


def test_example_host_writes_the_packed_sequence(tmp_path):
    """examples/decode_batch.c --thumb N --patches P[:M] end to end: the preview size rounded down to a multiple of P * M, uint8 tokens in Conv2d weight
    order; a bad P[:M] prints the usage"""
    import os
    import subprocess
    import libheif_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.abspath(libheif_amd.library_path())
    exe = str(tmp_path / "decode_batch")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "decode_batch.c"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    for bad in (["--patches", "0"], ["--patches", "257"], ["--patches", "4:0"], ["--patches", "4:2:1"], ["--patches"]):
        r = subprocess.run([exe, "--thumb", "32"] + bad + ["x.hevc"][:len(bad) - 1], capture_output=True, text=True)
        assert r.returncode == 2 and ("usage: %s " % exe) in r.stderr, r.stderr
    f = tmp_path / "item.hevc"
    f.write_bytes(_still(*SMALL))
    r = subprocess.run([exe, "--thumb", "32", "--orient", "5", "--patches", "4:2", str(f)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    dw, dh = decoder.fit_within(40, 72, 32)                     # the displayed picture of the 72 x 40 still is 40 x 72
    dw, dh = dw - dw % 8, dh - dh % 8
    b = _b(SMALL)
    b.to_tensor_packed([(dw, dh)], None, patch=4, merge=2, dtype="uint8", layout="NCHW", filter=SCALE_BOX, orientations=(5,), out=DeviceBuffer(3 * dw * dh))
    seq = b.tensor_packed_to_host()
    assert seq.shape == ((dw // 4) * (dh // 4), 48)
    want = int(seq.astype(np.uint64).sum())
    assert "%s: %d tokens of 4x4 at %dx%d, byte sum %d\n" % (f, seq.shape[0], dw, dh, want) in r.stdout, r.stdout
    assert "packed sequence: %d tokens x 48 elements, byte sum %d\n" % (seq.shape[0], want) in r.stdout, r.stdout
