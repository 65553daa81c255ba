"""Clips on the device: hipdec_clips_* (the samples of several sequence tracks as ONE launch set, frames resident in device memory) and the video tensors
hipdec_clips_to_tensor / hipdec_clips_to_tensor_packed write from them (include/heif_hipdec.h).

Everything is bit-exact, there are no tolerances, and no expected value comes from the new code.
  Frames:  every frame's planes are the oracle's picture (orc.decode_sequence) of that picture order count.
  Tensors: the header defines frame k of clip e as what the EXISTING hipdec_batch_to_tensor_oriented writes on the borrowed batch for the frame's item with
           the entry's window, flip and code.  That call (run_oriented of tests/test_oriented_gpu.py on clips.batch, one entry per frame) gives the dense
           frames; their elements are put where the header's index formulas say, element by element on index arrays (place_clip / place_tokens below; no
           reshape chain that could share a mistake with the kernel).  The reshape chain the header quotes is held against the formulas once.
Every call writes into a buffer pre-filled with 0xA5 that is longer than the tensor; the whole buffer is compared.

Runs on the MI355X (`-m gpu`) and, through tests/test_clips_emu.py, against the library compiled for the host."""
import functools
import numpy as np
import pytest

from libheif_amd import HipDecError, decoder
from libheif_amd._capi import DeviceBuffer
from libheif_amd.color import SCALE_BOX, SCALE_NEAREST
from libheif_amd.decoder import SCALE_BICUBIC, SCALE_BILINEAR, Clips
from oracle import pyoracle as orc
from test_oriented_gpu import run_oriented
from test_packed_gpu import BITS, ES, POISON, gapped_offsets, poison
from test_sequence_gpu import B_CASES, _p_sequence
from test_tensor_gpu import BIAS, DTYPES, SCALE, _lib, as_bits, run_tensor

pytestmark = pytest.mark.gpu

FILTERS = (SCALE_NEAREST, SCALE_BOX, SCALE_BILINEAR, SCALE_BICUBIC)
ORDERS = ("TCHW", "CTHW", "THWC")
LAYOUT_OF = {"TCHW": "NCHW", "CTHW": "NCHW", "THWC": "NHWC"}
TAIL = 64                                                  # elements behind the tensor
N = 8                                                      # samples per track


def _b(name, **over):
    cfg = dict(B_CASES[name])
    cfg.update(over)
    return _p_sequence(N, w=cfg.pop("w", 200), h=cfg.pop("h", 136), bit_depth=cfg.pop("bit_depth", 8), **cfg)


def _chroma(cf):
    from test_inter_oracle import make_frames
    aus = orc.encode_sequence(make_frames(136, 104, N, mono=cf == 0, chroma_format_idc=cf or 1, seed=9), qp=26, global_mv_x=-6, global_mv_y=3, inter_num_refs=2)
    return aus, orc.decode_sequence(aus)


def _cra():
    from test_inter_emu import parameter_sets
    from test_inter_oracle import make_frames
    aus = orc.encode_sequence(make_frames(136, 104, 10), qp=27, b_frames=2, b_ref=1, temporal_mvp=1, inter_num_refs=2, open_gop=2, seed=3)
    full = orc.decode_sequence(aus)
    entered = [parameter_sets(aus[0]) + aus[4]] + list(aus[5:])      # CRA, RASL, RASL, P (POC 9), B (7), B (8)
    by_poc = {p["poc"]: p for p in full}
    return entered, [by_poc[6], None, None, by_poc[9], by_poc[7], by_poc[8]]     # per sample; None: a RASL picture 8.3.3 drops


def _two_sequences():
    a_aus, a_refs = _p_sequence(6, w=136, h=104, b_frames=2, temporal_mvp=1, seed=3)
    b_aus, b_refs = _p_sequence(5, w=136, h=104, b_frames=1, b_ref=0, temporal_mvp=1, weighted_pred=1, seed=8)
    return a_aus + b_aus, [dict(r, sequence=0) for r in a_refs] + [dict(r, sequence=1) for r in b_refs]


TRACKS = {
    "ippp": lambda: _p_sequence(N),
    "ippp_small": lambda: _p_sequence(N, w=136, h=104, seed=9, inter_num_refs=2),
    "ippp_cropped": lambda: _p_sequence(N, w=70, h=42, amp=1, inter_num_refs=2, global_mv_y=17),
    "b2_ref_multiref_weighted": lambda: _b("b2_ref_multiref_weighted"),
    "b2_small": lambda: _b("b2_ref_multiref_weighted", w=136, h=104),
    "b_main10_tiles": lambda: _b("b_main10_tiles"),
    "p444": lambda: _chroma(3),
    "p400": lambda: _chroma(0),
    "cra_entry": _cra,
    "pic_output_flag_0": lambda: _p_sequence(N, b_frames=2, b_ref=1, temporal_mvp=1, inter_num_refs=2, hidden_poc=3, seed=5),
    "two_sequences": _two_sequences,
}


@functools.lru_cache(maxsize=None)
def track(name):
    """(samples, the oracle's pictures per sample - None for a dropped one)"""
    aus, refs = TRACKS[name]()
    return list(aus), list(refs)


def expected_frames(name):
    """[(sample, poc, sequence, planes)] in output order"""
    _, refs = track(name)
    hidden = 3 if name == "pic_output_flag_0" else None
    out = [(i, r["poc"], r.get("sequence", 0), r["planes"]) for i, r in enumerate(refs) if r is not None and r["poc"] != hidden]
    return sorted(out, key=lambda f: (f[2], f[1]))


_CLIPS = {}


def clips_of(*names):
    if names not in _CLIPS:
        c = Clips([track(n)[0] for n in names])
        c.run()
        c.status()
        _CLIPS[names] = c
    return _CLIPS[names]


@pytest.fixture(scope="module", autouse=True)
def _free_clips():
    yield
    for c in _CLIPS.values():
        c.free()
    _CLIPS.clear()
    _REFERENCES.clear()


# ---- frames ----------------------------------------------------------------------------------------------------------------------------------
def _check_frames(c, t, name):
    exp = expected_frames(name)
    assert c.frame_count(t) == len(exp), (name, c.frame_count(t))
    for f, (sample, poc, sequence, planes) in enumerate(exp):
        d = c.frame(t, f)
        assert (d["sample"], d["poc"], d["sequence"]) == (sample, poc, sequence), (name, f, d)
        got = c.planes(t, f)
        assert len(got) == (3 if d["chroma_format_idc"] else 1)
        for k, g in enumerate(got):
            np.testing.assert_array_equal(g, planes[k], err_msg="%s frame %d (POC %d) plane %d" % (name, f, poc, k))
        # the borrowed batch serves the same picture under the frame's item
        np.testing.assert_array_equal(c.batch.planes(d["item"])[0], planes[0])


@pytest.mark.parametrize("name", ["ippp_cropped", "b2_ref_multiref_weighted", "b_main10_tiles", "p444", "p400", "cra_entry", "pic_output_flag_0", "two_sequences"])
def test_frames_are_the_oracles_pictures_in_output_order(name):
    if name == "b2_ref_multiref_weighted":
        assert [r["poc"] for r in track(name)[1]] != list(range(N)), "output order is to differ from decoding order"
    c = Clips([track(name)[0]])
    try:
        c.run()
        c.status()
        assert c.n_tracks == 1
        _check_frames(c, 0, name)
    finally:
        c.free()


def test_two_tracks_of_different_sizes_are_one_launch_set():
    before = decoder.clips_stats()
    c = Clips([track("ippp")[0], track("b2_small")[0]])
    try:
        after = decoder.clips_stats()
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, 2, 2 * N)
        c.run()
        c.status()
        assert c.batch.n == 2 * N
        _check_frames(c, 0, "ippp")
        _check_frames(c, 1, "b2_small")
        assert sorted(c.frame(t, f)["item"] for t in (0, 1) for f in range(N)) == list(range(2 * N))
    finally:
        c.free()


# ---- dense clips -----------------------------------------------------------------------------------------------------------------------------
def place_clip(flat, base, F, order):
    """F: T dense frames (3, H, W).  Writes clip from element `base` on as the header defines the three orders - the index formulas, element by element."""
    T = len(F)
    _, H, W = F[0].shape
    c, y, x = np.indices(F[0].shape, dtype=np.int64)
    seen = []
    for k in range(T):
        if order == "TCHW":
            idx = ((k * 3 + c) * H + y) * W + x
        elif order == "THWC":
            idx = ((k * H + y) * W + x) * 3 + c
        else:
            idx = ((c * T + k) * H + y) * W + x
        flat[base + idx.ravel()] = F[k].ravel()
        seen.append(idx.ravel())
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(3 * T * H * W)), "the formulas do not fill the clip's range exactly once"


_REFERENCES = {}


def frame_references(c, key, sizes, T, entries, frames, codes, dtype, filt):
    """F[e][k]: (3, h, w) bit patterns from the EXISTING oriented call on the borrowed batch, one entry per frame; computed once per key and left alone"""
    key = (key, tuple(sizes), T, tuple(entries), tuple(map(tuple, frames)), tuple(codes), dtype, filt)
    if key not in _REFERENCES:
        out = [[None] * T for _ in entries]
        for size in sorted(set(sizes)):
            idx = [(e, k) for e in range(len(entries)) if sizes[e] == size for k in range(T)]
            per_frame = [(c.frame(entries[e][0], frames[e][k])["item"],) + tuple(entries[e][1:]) for e, k in idx]
            S = run_oriented(c.batch, size, per_frame, [codes[e] for e, _ in idx], dtype, "NCHW", filt)
            assert S.shape == (len(idx), 3, size[1], size[0])
            if dtype != "uint8":
                assert not (S == poison(dtype)).any(), "an expected element is the poison pattern"
            for j, (e, k) in enumerate(idx):
                out[e][k] = S[j].copy()
                out[e][k].setflags(write=False)
        _REFERENCES[key] = out
    return _REFERENCES[key]


def run_clip(c, size, T, entries, frames, codes, order, dtype, filt):
    elems = len(entries) * T * 3 * size[0] * size[1] + TAIL
    out = DeviceBuffer.from_numpy(np.full(elems * ES[dtype], POISON, np.uint8))
    got = c.to_tensor(size, T, entries, frames, order=order, dtype=dtype, scale=SCALE, bias=BIAS, filter=filt, orientations=codes, out=out)
    assert got is out
    host = c.tensor_to_host()                              # (waits for the stream)
    n, (W, H) = len(entries), size
    assert host.shape == {"TCHW": (n, T, 3, H, W), "CTHW": (n, 3, T, H, W), "THWC": (n, T, H, W, 3)}[order]
    raw = out.to_numpy((elems,), BITS[dtype])
    assert np.array_equal(as_bits(host).ravel(), raw[:elems - TAIL])
    out.free()
    return raw


def check_clip(c, key, size, T, entries, frames, codes, order, dtype, filt):
    got = run_clip(c, size, T, entries, frames, codes, order, dtype, filt)
    exp = np.full(got.shape, poison(dtype), BITS[dtype])
    F = frame_references(c, key, [size] * len(entries), T, entries, frames, codes or [0] * len(entries), dtype, filt)
    per = 3 * T * size[0] * size[1]
    for e in range(len(entries)):
        place_clip(exp, e * per, F[e], order)
    if not np.array_equal(got, exp):
        bad = [(e, k, int((got[e * per:(e + 1) * per] != exp[e * per:(e + 1) * per]).sum())) for e in range(len(entries)) for k in (0,)]
        assert False, (size, T, order, dtype, filt, [x for x in bad if x[2]], "in the tail: %d" % int((got[len(entries) * per:] != exp[len(entries) * per:]).sum()))


MAIN = ("ippp", "b2_small")                                # 200 x 136 IPPP and 136 x 104 with B pictures (output order differs from decoding order)
# clips of both tracks in one call, two clips of track 0, a window at odd offsets with a flip, repeated and descending frame indices on the B track
MAIN_ENTRIES = [(0, 0, 0, 0, 0, 0), (1, 3, 5, 101, 77, 1), (0, 37, 21, 64, 40, 0), (1, 0, 0, 0, 0, 0)]
MAIN_FRAMES4 = [[0, 2, 4, 6], [7, 5, 5, 2], [1, 1, 0, 7], [3, 2, 1, 0]]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
def test_orders_dtypes_and_filters(order, dtype, filt):
    """16 x 12 with T = 4: every group of four is whole and aligned (vector stores)"""
    check_clip(clips_of(*MAIN), "main4", (16, 12), 4, MAIN_ENTRIES, MAIN_FRAMES4, None, order, dtype, filt)


@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_NEAREST, SCALE_BILINEAR))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("size,T", [((15, 11), 3), ((22, 13), 1), ((18, 7), 3)], ids=["15x11xT3", "22x13xT1", "18x7xT3"])
def test_shapes_where_the_store_can_go_wrong(size, T, order, filt):
    """15 x 11 with T = 3, channel-major: an odd plane stride - unaligned channel planes, element stores; widths that are no multiple of 4, with a flip"""
    frames = [f[:T] for f in MAIN_FRAMES4]
    for dtype in ("uint8", "float16"):
        check_clip(clips_of(*MAIN), "shapes", size, T, MAIN_ENTRIES, frames, None, order, dtype, filt)


@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_NEAREST))
@pytest.mark.parametrize("size", [(261, 67), (67, 261)], ids=lambda s: "%dx%d" % s)
def test_up_scaled_output_wider_than_a_tile(size, filt):
    """261 columns: more than one 256-pixel tile of the strided box kernel, three of the oriented one"""
    c = clips_of(*MAIN)
    entries, frames = [(0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0)], [[1, 6], [5, 0]]
    check_clip(c, "wide", size, 2, entries, frames, None, "CTHW", "float16", filt)
    check_clip(c, "wide", size, 2, entries, frames, [0, 3], "THWC", "uint8", filt)


def folded(code, flip):
    return code ^ 4 if flip else code                      # (a horizontal mirror of the displayed sample toggles m)


@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_NEAREST))
@pytest.mark.parametrize("order", ORDERS)
def test_all_eight_codes_share_a_call_and_the_strided_kernel_takes_codes_0_and_4(order, filt):
    c = clips_of(*MAIN)
    T = 3
    entries = [(e & 1, 2, 1, 90, 60, 1 if e in (2, 4, 9) else 0) for e in range(10)]
    codes = list(range(8)) + [0, 0]
    frames = [[(e + k) % N for k in range(T)] for e in range(10)]
    before = decoder.clips_stats()
    check_clip(c, "codes", (22, 13), T, entries, frames, codes, order, "float16", filt)
    after = decoder.clips_stats()
    # (check_clip's reference goes through the batch call, which never takes the strided kernel)
    want = T * sum(1 for e, code in zip(entries, codes) if folded(code, e[5]) in (0, 4)) if filt == SCALE_BOX else 0
    assert after[4] - before[4] == want, (after, before, want)
    assert after[3] - before[3] == 1


def test_frame_major_nchw_is_the_existing_batch_call_in_frame_order():
    c = clips_of(*MAIN)
    T, size = 4, (32, 20)
    got = run_clip(c, size, T, MAIN_ENTRIES, MAIN_FRAMES4, None, "TCHW", "float16", SCALE_BOX)
    per_frame = [(c.frame(e[0], f)["item"],) + tuple(e[1:]) for e, fr in zip(MAIN_ENTRIES, MAIN_FRAMES4) for f in fr]
    exp = run_tensor(c.batch, size, per_frame, "float16", "NCHW", SCALE_BOX)
    assert got[:exp.size].tobytes() == exp.tobytes()
    # and the same call twice gives the same bytes
    assert run_clip(c, size, T, MAIN_ENTRIES, MAIN_FRAMES4, None, "TCHW", "float16", SCALE_BOX).tobytes() == got.tobytes()


# ---- tokens ----------------------------------------------------------------------------------------------------------------------------------
def place_tokens(flat, offset, F, P, m, Tp, layout):
    """F: T dense frames (3, h, w).  The header's formulas of hipdec_clips_to_tensor_packed, element by element."""
    T = len(F)
    _, h, w = F[0].shape
    assert T % Tp == 0 and w % (P * m) == 0 and h % (P * m) == 0
    c, Y, X = np.indices(F[0].shape, dtype=np.int64)
    gw, gh, gy, gx, py, px = w // P, h // P, Y // P, X // P, Y % P, X % P
    ts = ((gy // m) * (gw // m) + gx // m) * m * m + (gy % m) * m + gx % m
    seen = []
    for k in range(T):
        t = (k // Tp) * gh * gw + ts
        j = ((c * Tp + k % Tp) * P + py) * P + px if layout == "NCHW" else (((k % Tp) * P + py) * P + px) * 3 + c
        idx = t * 3 * Tp * P * P + j
        flat[offset + idx.ravel()] = F[k].ravel()
        seen.append(idx.ravel())
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(3 * T * h * w)), "the formulas do not fill the clip's range exactly once"


def test_the_token_formulas_are_the_reshape_chain_of_the_header():
    rng = np.random.default_rng(5)
    for (w, h, P, T) in ((24, 16, 4, 4), (12, 36, 6, 2), (8, 8, 2, 6)):
        S = rng.integers(0, 1 << 16, (T, 3, h, w)).astype(np.uint16)
        gh, gw = h // P, w // P
        flat = np.zeros(3 * T * h * w, np.uint16)
        place_tokens(flat, 0, list(S), P, 2, 2, "NCHW")
        chain = S.reshape(T // 2, 2, 3, gh // 2, 2, P, gw // 2, 2, P).transpose(0, 3, 6, 4, 7, 2, 1, 5, 8).reshape(T // 2 * gh * gw, 3 * 2 * P * P)
        assert np.array_equal(flat.reshape(T // 2 * gh * gw, -1), chain), (w, h, P, T)


def run_tokens(c, sizes, T, entries, frames, codes, P, m, Tp, layout, dtype, filt, offsets, order="TCHW"):
    elems = max(o + 3 * T * w * h for o, (w, h) in zip(offsets, sizes)) + TAIL
    out = DeviceBuffer.from_numpy(np.full(elems * ES[dtype], POISON, np.uint8))
    got = c.to_tokens(sizes, T, entries, frames, P, merge=m, temporal_patch=Tp, layout=layout, order=order, dtype=dtype, scale=SCALE, bias=BIAS, filter=filt,
                      orientations=codes, offsets=offsets, out=out)
    assert got[0] is out and list(got[1]) == list(offsets)
    assert got[2] == ([(T // Tp, h // P, w // P) for w, h in sizes] if P else None)
    c.tensor_to_host()
    raw = out.to_numpy((elems,), BITS[dtype])
    out.free()
    return raw


def check_tokens(c, key, sizes, T, entries, frames, codes, P, m, Tp, layout, dtype, filt, gaps=(16,), reverse=False):
    n = len(sizes)
    order = list(reversed(range(n))) if reverse else list(range(n))
    by_place = gapped_offsets([(w * T, h) for w, h in (sizes[e] for e in order)], gaps)     # (3 * T * w * h elements per clip)
    offsets = [0] * n
    for place, e in enumerate(order):
        offsets[e] = by_place[place]
    got = run_tokens(c, sizes, T, entries, frames, codes, P, m, Tp, layout, dtype, filt, offsets)
    exp = np.full(got.shape, poison(dtype), BITS[dtype])
    F = frame_references(c, key, sizes, T, entries, frames, codes or [0] * n, dtype, filt)
    for e in range(n):
        place_tokens(exp, offsets[e], F[e], P, m, Tp, layout)
    if not np.array_equal(got, exp):
        bad = [(e, int((got[o:o + 3 * T * w * h] != exp[o:o + 3 * T * w * h]).sum())) for e, (o, (w, h)) in enumerate(zip(offsets, sizes))]
        assert False, (P, m, Tp, layout, dtype, filt, [x for x in bad if x[1]], "outside the clips: %d" % (int((got != exp).sum()) - sum(k for _, k in bad)))


TOKEN_ENTRIES = [(0, 0, 0, 0, 0, 0), (1, 3, 5, 101, 77, 1), (0, 37, 21, 64, 40, 0)]
TOKEN_CODES = [0, 4, 3]                                    # a row-preserving code, the mirror (with a flip: code 0 again), a quarter turn
# (P, m, Tp) -> (T, sizes): multiples of P * m; 8 x 8 with P = 8 is one patch across a whole side
TOKEN_CASES = {(4, 2, 2): (4, [(24, 16), (16, 8), (8, 24)]), (6, 1, 2): (2, [(12, 18), (6, 6), (18, 6)]), (1, 1, 1): (3, [(5, 3), (1, 7), (4, 4)]),
               (4, 1, 3): (3, [(12, 8), (4, 4), (8, 20)]), (8, 1, 2): (2, [(8, 8), (8, 8), (8, 8)])}


@pytest.mark.parametrize("filt", (SCALE_BOX, SCALE_NEAREST, SCALE_BICUBIC))
@pytest.mark.parametrize("layout", ("NCHW", "NHWC"))
@pytest.mark.parametrize("case", sorted(TOKEN_CASES), ids=lambda k: "P%d-m%d-Tp%d" % k)
def test_token_sequences_with_a_temporal_patch(case, layout, filt):
    P, m, Tp = case
    T, sizes = TOKEN_CASES[case]
    frames = [[(3 * e + 2 * k) % N for k in range(T)] for e in range(3)]
    frames[1] = list(reversed(frames[1]))
    c = clips_of(*MAIN)
    check_tokens(c, "tokens", sizes, T, TOKEN_ENTRIES, frames, TOKEN_CODES, P, m, Tp, layout, "float16", filt)
    check_tokens(c, "tokens", sizes, T, TOKEN_ENTRIES, frames, TOKEN_CODES, P, m, Tp, layout, "uint8", filt, gaps=(7, 1, 13), reverse=True)


def test_a_still_becomes_image_tokens_with_frames_0_0():
    aus, _ = track("ippp_small")
    c = Clips([aus[:1]])
    try:
        c.run()
        c.status()
        assert c.frame_count(0) == 1
        for layout in ("NCHW", "NHWC"):
            check_tokens(c, "still", [(24, 16)], 2, [(0, 0, 0, 0, 0, 0)], [[0, 0]], None, 4, 2, 2, layout, "float32", SCALE_BOX)
    finally:
        c.free()


@pytest.mark.parametrize("order", ORDERS)
def test_dense_clips_back_to_back_are_the_dense_call(order):
    c = clips_of(*MAIN)
    size, T = (16, 12), 4
    dense = run_clip(c, size, T, MAIN_ENTRIES, MAIN_FRAMES4, None, order, "bfloat16", SCALE_BOX)
    offs = decoder.clip_packed_layout([size] * 4, T)[0]
    assert offs == [e * 3 * T * size[0] * size[1] for e in range(4)]
    packed = run_tokens(c, [size] * 4, T, MAIN_ENTRIES, MAIN_FRAMES4, None, 0, 1, 1, LAYOUT_OF[order], "bfloat16", SCALE_BOX, offs, order=order)
    assert packed.tobytes() == dense.tobytes()


# ---- 10-bit ----------------------------------------------------------------------------------------------------------------------------------
def test_ten_bit_sources_native_depth_for_floats_to_sdr_for_uint8():
    c = clips_of("b_main10_tiles")
    entries, frames = [(0, 0, 0, 0, 0, 0), (0, 11, 7, 150, 99, 1)], [[0, 7, 3], [6, 6, 1]]
    for order in ("CTHW", "THWC"):
        for filt in (SCALE_BOX, SCALE_NEAREST):
            check_clip(c, "ten", (20, 14), 3, entries, frames, None, order, "float32", filt)
            check_clip(c, "ten", (20, 14), 3, entries, frames, None, order, "uint8", filt)
        check_clip(c, "ten", (20, 14), 3, entries, frames, None, order, "uint8", SCALE_BILINEAR)
    raw = c.to_tensor((20, 14), 3, entries, frames, order="CTHW", dtype="float32", filter=SCALE_BOX, out=DeviceBuffer(2 * 3 * 3 * 20 * 14 * 4))
    v = c.tensor_to_host()
    raw.free()
    assert 255 < v.max() <= 1023 and v.min() >= 0, (v.min(), v.max())          # the native-depth value
    with pytest.raises(HipDecError) as ei:
        c.to_tensor((20, 14), 3, entries, frames, order="CTHW", dtype="float16", filter=SCALE_BILINEAR, out=DeviceBuffer(2 * 3 * 3 * 20 * 14 * 2))
    assert ei.value.code == -4 and "entry 0" in ei.value.message, ei.value.message


# ---- refusals on a live object ---------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_object_carry_status_and_message():
    c = clips_of(*MAIN)
    L = _lib()
    out = DeviceBuffer(1 << 16)

    def refused(call, code, *words):
        with pytest.raises(HipDecError) as ei:
            call()
        assert ei.value.code == code, ei.value
        for w in words:
            assert w in ei.value.message, ei.value.message

    e2 = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0)]
    refused(lambda: c.to_tensor((8, 8), 2, e2, [[0, 1], [1, N]], out=out), -1, "entry 1", "frame index %d" % N)
    refused(lambda: c.to_tensor((8, 8), 2, e2, [[0, -1], [1, 2]], out=out), -1, "entry 0", "frame index -1")
    refused(lambda: c.to_tensor((8, 8), 2, [(0, 0, 0, 0, 0, 0), (2, 0, 0, 0, 0, 0)], [[0, 1], [1, 2]], out=out), -1, "entry 1", "track 2")
    cd = decoder.ClipDesc(2, 1, 0, 0)                       # channel-major + NHWC (the Python orders cannot spell it)
    desc = decoder.tensor_desc((8, 8), "uint8", "NHWC")
    fr = (decoder.C.c_int * 4)(0, 1, 1, 2)
    rc = L.hipdec_clips_to_tensor(c._h, desc, cd, decoder.tensor_entries(e2), fr, None, 2, out.ptr, out.nbytes, None)
    assert rc == -1 and b"channel-major" in L.hipdec_last_error(), L.hipdec_last_error()
    refused(lambda: c.to_tokens([(8, 8)] * 2, 3, e2, [[0, 1, 2]] * 2, 4, temporal_patch=2, offsets=[0, 4096], out=out), -1, "temporal_patch 2")
    refused(lambda: c.to_tokens([(8, 8)] * 2, 2, e2, [[0, 1]] * 2, 4, temporal_patch=17, offsets=[0, 4096], out=out), -1, "temporal_patch")
    refused(lambda: c.to_tokens([(8, 8)] * 2, 2, e2, [[0, 1]] * 2, 0, temporal_patch=2, offsets=[0, 4096], out=out), -1, "temporal_patch")
    refused(lambda: c.to_tokens([(8, 8)] * 2, 2, e2, [[0, 1]] * 2, 4, temporal_patch=2, offsets=[0, 3 * 2 * 64 - 1], out=out), -1, "overlap", "entry")
    refused(lambda: c.to_tokens([(8, 8)] * 2, 2, e2, [[0, 1]] * 2, 4, temporal_patch=2, offsets=[0, (1 << 16) - 100], out=out), -1, "entry 1")
    cd = decoder.ClipDesc(2, 1, 2, 0)                       # channel-major order with patches
    desc = decoder.tensor_desc((0, 0), "uint8", "NCHW")
    sm = (decoder.TensorSample * 2)(decoder.TensorSample(8, 8, 0), decoder.TensorSample(8, 8, 384))
    pt = decoder.TensorPatches(4, 1)
    rc = L.hipdec_clips_to_tensor_packed(c._h, desc, cd, decoder.tensor_entries(e2), fr, None, sm, pt, 2, out.ptr, out.nbytes, None)
    assert rc == -1 and b"channel-major" in L.hipdec_last_error(), L.hipdec_last_error()
    # the borrowed batch: run is refused, free is a no-op
    refused(c.batch.run, -1, "borrowed")
    L.hipdec_batch_free(c.batch._h)
    c.batch.free()
    check_clip(c, "after_free", (16, 12), 2, e2, [[0, 1], [3, 2]], None, "CTHW", "uint8", SCALE_BOX)
    out.free()


def test_create_refuses_what_the_plan_refuses_naming_track_and_sample():
    aus, _ = track("ippp_small")
    ten, _ = track("b_main10_tiles")

    def refused(tracks, code, *words):
        with pytest.raises(HipDecError) as ei:
            Clips(tracks)
        assert ei.value.code == code, ei.value
        for w in words:
            assert w in ei.value.message, ei.value.message

    def front_end_status(first, then=None):
        """the status the decoder object gives for the same samples"""
        d = decoder.HipDecoder()
        try:
            d.push_data(first)
            with pytest.raises(HipDecError) as ei:
                d.decode_next_image()
                d.push_data(then)
                d.decode_next_image()
            return ei.value.code
        finally:
            d.free()

    refused([aus, [aus[0], aus[2]]], front_end_status(aus[0], aus[2]), "track 1", "sample 1")        # its RPS names POC 1, which is not among the samples
    refused([aus, aus[1:]], front_end_status(aus[1]), "track 1", "sample 0")                          # a first sample without parameter sets
    refused([aus, [aus[0], aus[1][:-3]]], -2, "track 1", "sample 1")                                  # broken framing
    refused([aus, [aus[0], aus[1] + aus[2]]], -3, "track 1", "sample 1")                              # two pictures in one sample
    refused([aus, ten], -4, "track 1")                                                                # 8-bit beside 10-bit
    refused([aus] * 129, -5, "track 128")                                                             # 1032 samples: above the chain limit
