"""The augment stage of the tensor output (include/heif_hipdec.h, hipdec_tensor_augment) restated in NumPy: the photo stage's nine operations
(tests/photo_ref.py, to which opcodes 1 .. 9 are delegated), Pillow's hue shift - convert("HSV"), a uint8 wrap-around add on H, convert("RGB") - and
ImageFilter.GaussianBlur, bit for bit.  tests/test_augment_ref.py pins this file to Pillow itself; the GPU tests and tests/test_augment_lut_host.py take
their expected values from here, never from the library.

A sample is an (h, w, 3) uint8 array.  A chain is a sequence of (op, value) pairs, applied in order, each on the 8-bit result of the one before it.
Single-precision steps are written one NumPy float32 operation at a time, so each is rounded once and none is fused; where the definition says double,
the operands are converted first."""
import numpy as np

import photo_ref

HUE, GAUSSIAN_BLUR = 16, 17
NAMES = dict(photo_ref.NAMES, hue=HUE, gaussian_blur=GAUSSIAN_BLUR)
MAX_OPS = 8
BLUR_MAX_RADIUS = 8.0
f32, f64 = np.float32, np.float64


def rgb2hsv(rgb):
    """convert("HSV"): rgb an (..., 3) uint8 array"""
    rgb = np.asarray(rgb, np.uint8).astype(np.int32)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(axis=-1), rgb.min(axis=-1)
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(f32)
        s = cr / mx.astype(f32)
        rc, gc, bc = (mx - R).astype(f32) / cr, (mx - G).astype(f32) / cr, (mx - B).astype(f32) / cr
        h_r = bc - gc                                                   # float
        h_g = ((f64(2.0) + rc.astype(f64)) - bc.astype(f64)).astype(f32)
        h_b = ((f64(4.0) + gc.astype(f64)) - rc.astype(f64)).astype(f32)
        h = np.where(R == mx, h_r, np.where(G == mx, h_g, h_b)).astype(f32)
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip((h.astype(f64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((s.astype(f64) * 255.0).astype(np.int64), 0, 255)
    H = np.where(grey, 0, H)
    S = np.where(grey, 0, S)
    return np.stack([H, S, mx], axis=-1).astype(np.uint8)


def _round8(v):
    """round half away from zero (v is not negative), clipped to 0 .. 255"""
    fl = np.floor(v)
    return np.clip(np.where(v - fl >= 0.5, fl + 1, fl).astype(np.int64), 0, 255)   # (v - floor(v) is exact)


def hsv2rgb(hsv):
    """convert("RGB") of an (..., 3) uint8 HSV array"""
    hsv = np.asarray(hsv, np.uint8)
    H, S, V = hsv[..., 0], hsv[..., 1], hsv[..., 2].astype(np.int64)
    hf = H.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int64)
    f = (hf - i.astype(f32).astype(f64)).astype(f32)
    fs = (S.astype(f64) / 255.0).astype(f32)
    v = V.astype(f64)
    p = _round8(v * (1.0 - fs.astype(f64)))
    q = _round8(v * (1.0 - (fs * f).astype(f64)))                       # the product in float
    t = _round8(v * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))     # all in double
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    k = i % 6
    out = np.empty(hsv.shape, np.int64)
    for c in range(3):
        out[..., c] = np.choose(k, [table[j][c] for j in range(6)])
    grey = S == 0
    for c in range(3):
        out[..., c] = np.where(grey, V, out[..., c])
    return out.astype(np.uint8)


def hue(S, d):
    """HUE with the integer shift d, 0 .. 255"""
    hsv = rgb2hsv(S)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(d)) & 255).astype(np.uint8)
    return hsv2rgb(hsv)


def hue_shift(hue_factor):
    """the d of torchvision's PIL adjust_hue: np.uint8(hue_factor * 255) - truncated toward zero, then mod 256"""
    return int(float(hue_factor) * 255) % 256


def gaussian_box(radius):
    """(r, ww, fw) of the extended box ImageFilter.GaussianBlur(radius) runs three times along each axis: single precision, one rounding per operation"""
    rho = f32(radius)
    sigma2 = rho * rho / f32(3)
    L = f32(np.sqrt(f64(12.0) * f64(sigma2) + f64(1.0)))
    l = f32(np.floor((f64(L) - 1.0) / 2.0))
    a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * sigma2)
    a = a / (f32(6) * (sigma2 - (l + f32(1)) * (l + f32(1))))
    fr = l + a
    r = int(fr)
    ww = int(f32(1 << 24) / (fr * f32(2) + f32(1)))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww & 0xFFFFFFFF, fw


def box_pass(A, axis, r, ww, fw):
    """one extended box pass along `axis` of an integer array: indices clamp, 32-bit unsigned arithmetic"""
    A = np.moveaxis(np.asarray(A, np.int64), axis, 0)
    n = A.shape[0]
    idx = np.arange(n)
    c = lambda i: np.clip(i, 0, n - 1)
    acc = np.zeros_like(A)
    for k in range(-r, r + 1):
        acc += A[c(idx + k)]
    edge = A[c(idx - r - 1)] + A[c(idx + r + 1)]
    out = (((ww * acc + fw * edge + (1 << 23)) & 0xFFFFFFFF) >> 24) & 255
    return np.moveaxis(out, 0, axis)


def gaussian_blur(S, radius):
    """ImageFilter.GaussianBlur(radius): three passes along rows, then three along columns, each on the 8-bit result of the one before"""
    r, ww, fw = gaussian_box(radius)
    A = np.asarray(S, np.uint8).astype(np.int64)
    for axis in (1, 1, 1, 0, 0, 0):
        A = box_pass(A, axis, r, ww, fw)
    return A.astype(np.uint8)


def refused(op, value):
    """what hipdec_tensor_augment refuses of one operation"""
    if op in photo_ref.NAMES.values():
        return photo_ref.refused(op, value)
    v = float(value)
    if op == HUE:
        return not np.isfinite(v) or v != int(v) or v < 0 or v > 255
    if op == GAUSSIAN_BLUR:
        return not np.isfinite(v) or v < 0 or v > BLUR_MAX_RADIUS
    return True


def apply_op(S, op, value=0.0):
    if isinstance(op, str):
        op = NAMES[op]
    assert not refused(op, value), (op, value)
    S = np.ascontiguousarray(S, np.uint8)
    if op == HUE:
        return hue(S, int(value))
    if op == GAUSSIAN_BLUR:
        return gaussian_blur(S, value)
    return photo_ref.apply_op(S, op, value)


def apply_chain(S, chain):
    assert len(chain) <= MAX_OPS
    for step in chain:
        op, value = (step, 0.0) if isinstance(step, (str, int)) else (step[0], step[1] if len(step) > 1 else 0.0)
        S = apply_op(S, op, value)
    return np.ascontiguousarray(S, np.uint8)
