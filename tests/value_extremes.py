"""Shared by tests/test_value_extremes_emu.py and tests/test_value_extremes_gpu.py: the stream sets that carry extreme VALUES (transform levels
over the whole int16 range from the generator's level_torture knobs, sample planes made of 0 and (1 << bitDepth) - 1 only) and an int64 NumPy
restatement of ITU-T H.265 8.6.1 - 8.6.4.2 (scaling, transformation, residual) that knows nothing of oracle/hevc_oracle.c."""
import numpy as np

from oracle import pyoracle as orc

ALIGNED, UNIFORM, LADDER, OVER_32768, OVER_32769, EDGE = 1, 2, 3, 4, 5, 6      # hevc_testenc_params::level_torture_kind

# ------------------------------------------------------------------------------------------------
# 8.6.4.2 in int64
# ------------------------------------------------------------------------------------------------
# transMatrix column 0 (rows 0 .. 31) as printed in (8-xxx); every other coefficient is +- one of these: row j, column i holds the cosine of
# (2 i + 1) j * pi / 64, i.e. entry ((2 i + 1) j mod 128) of the sequence continued by its symmetries c[64 - k] = -c[k], c[128 - k] = c[k]
_COL0 = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4]
_DST = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)
LEVEL_SCALE = [40, 45, 51, 57, 64, 72]


def trans_matrix(n):
    """E[j][i], n x n: rows 0, 32 / n, 2 * 32 / n, ... of the 32 x 32 transMatrix, first n columns (8.6.4.2)"""
    def c(k):
        k %= 128
        if k > 64:
            k = 128 - k
        return _COL0[k] if k < 32 else (0 if k == 32 else -_COL0[64 - k])
    m = np.zeros((n, n), np.int64)
    for j in range(n):
        for i in range(n):
            m[j, i] = c((2 * i + 1) * j * (32 // n))
    return m


def residual_int64(levels, bit_depth, qP, m=None, transform_skip=False, bypass=False, dst=False):
    """TransCoeffLevel (n x n, raster [y][x]) -> residual samples r (8.6.2 .. 8.6.4.2 of version 1 / 2 without range extension tools), all in int64"""
    lev = np.asarray(levels, np.int64)
    n = lev.shape[0]
    log2n = n.bit_length() - 1
    if bypass:
        return lev.copy()
    mm = np.full((n, n), 16, np.int64) if m is None else np.asarray(m, np.int64)
    bd_shift = bit_depth + log2n - 5
    d = (((lev * mm * LEVEL_SCALE[qP % 6]) << (qP // 6)) + (1 << (bd_shift - 1))) >> bd_shift
    d = np.clip(d, -32768, 32767)
    bd_shift2 = 20 - bit_depth
    if transform_skip:
        r = d << 7
    else:
        E = _DST if dst else trans_matrix(n)
        e = E.T @ d                                  # first stage, columns: e[i][x] = sum_j E[j][i] d[j][x]
        g = np.clip((e + 64) >> 7, -32768, 32767)
        r = g @ E                                    # second stage, rows: r[y][i] = sum_j E[j][i] g[y][j]
    return (r + (1 << (bd_shift2 - 1))) >> bd_shift2


_QPC_420 = {30: 29, 31: 30, 32: 31, 33: 32, 34: 33, 35: 33, 36: 34, 37: 34, 38: 35, 39: 35, 40: 36, 41: 36, 42: 37, 43: 37}


def chroma_qp(qp_y, offset, bit_depth, chroma_format_idc):
    """8.6.1: qP of a chroma block (Qp'Cb / Qp'Cr)"""
    off = 6 * (bit_depth - 8)
    qpi = min(max(qp_y + offset, -off), 57)
    if chroma_format_idc == 1:
        qpc = qpi if qpi < 30 else (qpi - 6 if qpi >= 44 else _QPC_420[qpi])
    else:
        qpc = min(qpi, 51)
    return qpc + off


# Table 7-6: the default 8x8 lists (sizeId 1 .. 3) at their matrix positions; Table 7-5: 4x4 is flat 16.  16x16 / 32x32: upsampled, DC 16 (7.4.5)
_DEFAULT_INTRA8 = np.array([[16, 16, 16, 16, 17, 18, 21, 24], [16, 16, 16, 16, 17, 19, 22, 25], [16, 16, 17, 18, 20, 22, 25, 29], [16, 16, 18, 21, 24, 27, 31, 36],
                            [17, 17, 20, 24, 30, 35, 41, 47], [18, 19, 22, 27, 35, 44, 54, 65], [21, 22, 25, 31, 41, 54, 70, 88], [24, 25, 29, 36, 47, 65, 88, 115]], np.int64)
_DEFAULT_INTER8 = np.array([[16, 16, 16, 16, 17, 18, 20, 24], [16, 16, 16, 17, 18, 20, 24, 25], [16, 16, 17, 18, 20, 24, 25, 28], [16, 17, 18, 20, 24, 25, 28, 33],
                            [17, 18, 20, 24, 25, 28, 33, 41], [18, 20, 24, 25, 28, 33, 41, 54], [20, 24, 25, 28, 33, 41, 54, 71], [24, 25, 28, 33, 41, 54, 71, 91]], np.int64)


def default_scaling_factor(n, inter):
    if n == 4:
        return np.full((4, 4), 16, np.int64)
    return np.kron(_DEFAULT_INTER8 if inter else _DEFAULT_INTRA8, np.ones((n // 8, n // 8), np.int64))


def transform_blocks(ref, cfg):
    """every transform block of a picture from the ORACLE'S taps (map_log2_tb, map_qp_y, map_flags, map_pred, coeff): dicts with the component, the
    position in component samples, the levels and everything 8.6.2 needs.  `cfg` = the encoder parameters of the stream: transform skip only as
    transform_skip = 2 (every 4x4 block), scaling lists only as scaling_list = 1 (default lists), no PCM."""
    cf, bd = ref["chroma_format_idc"], ref["bit_depth_luma"]
    assert cfg.get("transform_skip", 0) in (0, 2) and cfg.get("scaling_list", 0) in (0, 1) and not cfg.get("pcm_pct")
    cw, ch = ref["coded_size"]
    tb, flags, qpy = ref["map_log2_tb"], ref["map_flags"], ref["map_qp_y"]
    pred = ref.get("map_pred")
    out = []

    def add(c, x, y, n, ux, uy):
        lev = ref["coeff"][c][y:y + n, x:x + n]
        if not lev.any():
            return
        inter = bool(pred is not None and pred[uy, ux] != 0)
        bypass = bool(flags[uy, ux] & 8)
        qp = int(qpy[uy, ux])
        qP = qp + 6 * (bd - 8) if c == 0 else chroma_qp(qp, cfg.get("cb_qp_offset" if c == 1 else "cr_qp_offset", 0), bd, cf)
        out.append(dict(c=c, x=x, y=y, n=n, levels=lev.astype(np.int64), qP=qP, bypass=bypass, inter=inter, bit_depth=bd,
                        ts=bool(n == 4 and cfg.get("transform_skip", 0) == 2 and not bypass), dst=bool(c == 0 and n == 4 and not inter),
                        m=default_scaling_factor(n, inter) if cfg.get("scaling_list", 0) else None))

    for uy in range(ch // 4):
        for ux in range(cw // 4):
            t = int(tb[uy, ux])
            n = 1 << t
            if (ux * 4) % n or (uy * 4) % n:
                continue
            x, y = ux * 4, uy * 4
            add(0, x, y, n, ux, uy)
            if cf == 0:
                continue
            if cf == 3:
                add(1, x, y, n, ux, uy); add(2, x, y, n, ux, uy)
            elif n > 4 or (x % 8 == 0 and y % 8 == 0):      # 4:2:0 / 4:2:2: half the size; the four 4x4 luma blocks of an 8x8 node share 4x4 chroma blocks
                nc = max(n // 2, 4)
                for c in (1, 2):
                    if cf == 1:
                        add(c, x // 2, y // 2, nc, ux, uy)
                    else:
                        add(c, x // 2, y, nc, ux, uy); add(c, x // 2, y + nc, nc, ux, uy)
    return out


# ------------------------------------------------------------------------------------------------
# stream sets
# ------------------------------------------------------------------------------------------------
def tortured_still(w, h, bit_depth=8, cf=1, kind=0, pct=35, seed=1, flat=False, **cfg):
    """flat: a mid-grey source, which the generator codes in the largest units it may use (32x32 transform blocks)"""
    planes = orc.synth_image(w, h, bit_depth, cf, seed=seed)
    if flat:
        planes = [np.full_like(p, 1 << (bit_depth - 1)) for p in planes]
    return orc.encode(planes, bit_depth=bit_depth, level_torture_pct=pct, level_torture_kind=kind, seed=seed, **cfg)


def tortured_sequence(w, h, n, bit_depth=8, cf=1, kind=0, pct=30, seed=1, **cfg):
    from test_inter_oracle import make_frames
    cfg = dict(cfg)
    cfg.setdefault("qp", 26)
    return orc.encode_sequence(make_frames(w, h, n, bit_depth, chroma_format_idc=cf, seed=seed), bit_depth=bit_depth, level_torture_pct=pct,
                               level_torture_kind=kind, seed=seed, **cfg)


def extreme_planes(pattern, w, h, bit_depth, cf=1, shift=(0, 0)):
    """planes of 0 and max only: 'black', 'white', 'checker' (1-pixel checkerboard), 'vstripes' / 'hstripes' (8 pixels wide), 'box' (a max-valued
    rectangle on zero, moved by `shift`: frames of a sequence)"""
    hi = (1 << bit_depth) - 1

    def plane(pw, ph, phase):
        yy, xx = np.mgrid[0:ph, 0:pw]
        if pattern == "black":
            on = np.zeros((ph, pw), bool)
        elif pattern == "white":
            on = np.ones((ph, pw), bool)
        elif pattern == "checker":
            on = ((xx + yy + phase) & 1) == 1
        elif pattern == "vstripes":
            on = (((xx + 3 * phase) >> 3) & 1) == 1
        elif pattern == "hstripes":
            on = (((yy + 3 * phase) >> 3) & 1) == 1
        else:
            sx, sy = shift
            on = (xx >= pw // 4 + sx) & (xx < 3 * pw // 4 + sx) & (yy >= ph // 4 + sy) & (yy < 3 * ph // 4 + sy)
        return np.where(on, hi, 0).astype(np.uint16)

    planes = [plane(w, h, 0)]
    if cf:
        pw = w if cf == 3 else (w + 1) // 2
        ph = (h + 1) // 2 if cf == 1 else h
        planes += [plane(pw, ph, 1), plane(pw, ph, 2)]
    return planes


EXTREME_PATTERNS = ["black", "white", "checker", "vstripes", "hstripes"]
# intra: exact 0 / max samples as prediction neighbours (lossless and PCM units keep them), the ends of the tc / beta tables
EXTREME_INTRA_CONFIGS = [
    dict(qp=0, lossless_pct=40, pcm_pct=20, stress=1, tc_offset_div2=6, beta_offset_div2=6),
    dict(qp=51, lossless_pct=40, pcm_pct=20, stress=1, tc_offset_div2=6, beta_offset_div2=6, strong_intra_smoothing=0),
    dict(qp=51, lossless_pct=25, pcm_pct=25, stress=1, tc_offset_div2=-6, beta_offset_div2=-6, cu_qp_delta=0),
    dict(qp=0, lossless_pct=25, pcm_pct=25, stress=1, tc_offset_div2=-6, beta_offset_div2=-6, strong_intra_smoothing=0, log2_ctb=5, log2_max_tb=5),
]
# inter: weighted and bi-predictive sums, fractional vectors at several phases
EXTREME_INTER_CONFIGS = [
    dict(weighted_pred=1, b_frames=2, b_ref=1, inter_bi_pct=80, inter_num_refs=2, global_mv_x=-7, global_mv_y=5, qp=30),
    dict(weighted_pred=1, b_frames=1, inter_bi_pct=60, global_mv_x=9, global_mv_y=-3, qp=12, amp=1, temporal_mvp=1),
    dict(weighted_pred=0, b_frames=1, inter_bi_pct=90, global_mv_x=-5, global_mv_y=-6, qp=45, inter_skip_pct=5),
]


def extreme_sequence(n, w, h, bit_depth, cf, cfg, seed=1):
    """a max-valued box moving by a few pixels per frame over zero, every third frame a 1-pixel checkerboard in the box's place"""
    frames = []
    for k in range(n):
        f = extreme_planes("box", w, h, bit_depth, cf, shift=(3 * k, 2 * k))
        if k % 3 == 2:
            ck = extreme_planes("checker", w, h, bit_depth, cf)
            f = [np.where(a > 0, b, 0).astype(np.uint16) for a, b in zip(f, ck)]
        frames.append(f)
    return orc.encode_sequence(frames, bit_depth=bit_depth, seed=seed, **cfg)
