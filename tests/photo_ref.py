"""The photometric stage of the tensor output (include/heif_hipdec.h, hipdec_tensor_photo) restated in NumPy: ImageEnhance.Brightness / Color / Contrast /
Sharpness and ImageOps.posterize / solarize / invert / autocontrast / equalize of an 8-bit RGB picture, bit for bit.  tests/test_photo_ref.py pins this
file to Pillow itself; the GPU tests and tests/test_photo_lut_host.py take their expected values from here, never from the library.

A sample is an (h, w, 3) uint8 array.  A chain is a sequence of (op, value) pairs, applied in order, each on the 8-bit result of the one before it.
Single-precision steps are written one NumPy float32 operation at a time, so each is rounded once and none is fused."""
import numpy as np

BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, INVERT, AUTOCONTRAST, EQUALIZE = range(1, 10)
NAMES = {"brightness": BRIGHTNESS, "color": COLOR, "contrast": CONTRAST, "sharpness": SHARPNESS, "posterize": POSTERIZE, "solarize": SOLARIZE,
         "invert": INVERT, "autocontrast": AUTOCONTRAST, "equalize": EQUALIZE}
MAX_OPS = 4
VALUE_LIMIT = 65536.0


def blend(D, V, f):
    """Image.blend(degenerate, image, f) per component: D and V integer arrays (or scalars) of 0 .. 255"""
    alpha = np.float32(f)
    D = np.asarray(D, np.int32)
    V = np.asarray(V, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = D.astype(np.float32) + alpha * (V - D).astype(np.float32)
    if np.float32(0) <= alpha <= np.float32(1):
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))
    return out.astype(np.uint8)


def lum(S):
    """convert("L"): one value per pixel"""
    S = S.astype(np.int64)
    return ((S[..., 0] * 19595 + S[..., 1] * 38470 + S[..., 2] * 7471 + 0x8000) >> 16).astype(np.int32)


def contrast_mean(lum_sum, pixels):
    return int(float(lum_sum) / float(pixels) + 0.5)


def smooth(S):
    """ImageFilter.SMOOTH - the kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 -: the top row first; the first and last row and column are the source's"""
    h, w, _ = S.shape
    out = S.copy()
    if w < 3 or h < 3:
        return out
    k, kc = np.float32(1.0 / 13), np.float32(5.0 / 13)
    F = S.astype(np.float32)

    def row(r, centre):
        return (F[r, :-2] * k + F[r, 1:-1] * centre) + F[r, 2:] * k

    ss = np.full((h - 2, w - 2, 3), np.float32(0.5), np.float32)
    for dy in range(3):
        ss = ss + row(slice(dy, h - 2 + dy), kc if dy == 1 else k)
    out[1:-1, 1:-1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss.astype(np.int32))).astype(np.uint8)
    return out


def posterize_lut(bits):
    return (np.arange(256) & ((0xFF << (8 - int(bits))) & 0xFF)).astype(np.uint8)


def solarize_lut(t):
    v = np.arange(256)
    return np.where(v.astype(np.float64) < float(t), v, 255 - v).astype(np.uint8)


def autocontrast_lut(lo, hi):
    """ImageOps.autocontrast with cutoff 0 for a channel whose least and greatest value present are lo and hi"""
    v = np.arange(256)
    if hi <= lo:
        return v.astype(np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip((v.astype(np.float64) * scale + offset).astype(np.int64), 0, 255).astype(np.uint8)


def equalize_lut(H):
    """ImageOps.equalize for a channel with the 256-bin histogram H"""
    H = np.asarray(H, np.int64)
    v = np.arange(256)
    nz = np.nonzero(H)[0]
    if len(nz) < 2:
        return v.astype(np.uint8)
    step = int(H.sum() - H[nz[-1]]) // 255
    if step == 0:
        return v.astype(np.uint8)
    before = np.concatenate(([0], np.cumsum(H)[:-1]))
    return np.minimum(255, (step // 2 + before) // step).astype(np.uint8)


def refused(op, value):
    """what hipdec_tensor_photo refuses of one operation"""
    if op not in NAMES.values():
        return True
    v = float(value)
    if not np.isfinite(v) or abs(v) > VALUE_LIMIT:
        return True
    return op == POSTERIZE and (v != int(v) or v < 0 or v > 8)


def apply_op(S, op, value=0.0):
    if isinstance(op, str):
        op = NAMES[op]
    assert not refused(op, value), (op, value)
    S = np.ascontiguousarray(S, np.uint8)
    if op == BRIGHTNESS:
        return blend(0, S, value)
    if op == COLOR:
        return blend(lum(S)[..., None], S, value)
    if op == CONTRAST:
        return blend(contrast_mean(int(lum(S).sum(dtype=np.int64)), S.shape[0] * S.shape[1]), S, value)
    if op == SHARPNESS:
        return blend(smooth(S), S, value)
    if op == POSTERIZE:
        return posterize_lut(value)[S]
    if op == SOLARIZE:
        return solarize_lut(value)[S]
    if op == INVERT:
        return (255 - S).astype(np.uint8)
    out = np.empty_like(S)
    for c in range(3):
        if op == AUTOCONTRAST:
            lut = autocontrast_lut(int(S[..., c].min()), int(S[..., c].max()))
        else:
            lut = equalize_lut(np.bincount(S[..., c].ravel(), minlength=256))
        out[..., c] = lut[S[..., c]]
    return out


def apply_chain(S, chain):
    assert len(chain) <= MAX_OPS
    for step in chain:
        op, value = (step, 0.0) if isinstance(step, (str, int)) else (step[0], step[1] if len(step) > 1 else 0.0)
        S = apply_op(S, op, value)
    return np.ascontiguousarray(S, np.uint8)
