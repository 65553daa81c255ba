"""The integer stage of the warped tensor output (include/heif_hipdec.h, hipdec_tensor_warp) restated in vectorised NumPy float64: what
PIL.Image.transform(size, AFFINE, data, resample, fillcolor) computes for an 8-bit RGB picture, and the two matrix helpers of libheif_amd.decoder restated.

NumPy evaluates every operation below as one IEEE double operation with one rounding; nothing here can be contracted into a fused multiply-add.
tests/test_warp_ref.py pins this file to Pillow bit for bit.  The pin holds on x86-64 builds of Pillow; an aarch64 build of Pillow may contract
a * b + c into an FMA and then differs from this restatement (and from the library) in rare last-bit cases.

Nothing in this file comes from the library under test."""
import math

import numpy as np

NEAREST, BILINEAR, BICUBIC = 0, 16, 17   # hipdec_scale_filter
LIMIT = 32000.0


def _floor_int(v):
    """FLOOR(v) = (int)floor(v) for v < 0, else (int)v"""
    return np.where(v < 0, np.floor(v), np.trunc(v)).astype(np.int64)


def _coord(v):
    """COORD(v) = -1 for v < 0, else (int)v"""
    return np.where(v < 0, -1.0, np.trunc(v)).astype(np.int64)


def refused(m, size):
    """the refusals a map alone decides for an output of size = (ow, oh)"""
    a = np.asarray(m, np.float64)
    if not np.isfinite(a).all() or (np.abs(a) >= LIMIT).any():
        return True
    for cx in (0.0, float(size[0])):
        for cy in (0.0, float(size[1])):
            if not abs(a[0] * cx + a[1] * cy + a[2]) < LIMIT or not abs(a[3] * cx + a[4] * cy + a[5]) < LIMIT:
                return True
    return False


def fix(v):
    """FIX(v) = FLOOR(v * 65536.0 + 0.5)"""
    return int(_floor_int(np.float64(v) * 65536.0 + 0.5))


def scale_table(offset, step, n):
    """t[i] = COORD(o), o starting at offset + step * 0.5, o += step after each i (a running sum)"""
    o = np.float64(offset) + np.float64(step) * 0.5
    step = np.float64(step)
    t = np.empty(n, np.int64)
    for i in range(n):
        t[i] = -1 if o < 0 else int(o)
        o = o + step
    return t


def _lerp(p, q, d):
    return p + (q - p) * d


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2.0 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def warp(src, m, size, filt, fill=(0, 0, 0)):
    """src: (sh, sw, 3) uint8; m: six numbers; size = (ow, oh).  Returns ((oh, ow, 3) uint8 with `fill` outside, (oh, ow) bool inside-mask)."""
    S = np.asarray(src)
    assert S.dtype == np.uint8 and S.ndim == 3 and S.shape[2] == 3
    sh, sw = S.shape[:2]
    ow, oh = size
    a = [np.float64(v) for v in m]
    out = np.empty((oh, ow, 3), np.uint8)
    out[...] = np.asarray(fill, np.uint8)
    x = np.arange(ow, dtype=np.int64)[None, :]
    y = np.arange(oh, dtype=np.int64)[:, None]
    if filt == NEAREST:
        if a[1] == 0 and a[3] == 0:
            sx = np.broadcast_to(scale_table(a[2], a[0], ow)[None, :], (oh, ow))
            sy = np.broadcast_to(scale_table(a[5], a[4], oh)[:, None], (oh, ow))
        else:
            A0, A1, A3, A4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
            A2 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5)
            A5 = fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
            sx = (A2 + y * A1 + x * A0) >> 16
            sy = (A5 + y * A4 + x * A3) >> 16
        inside = (sx >= 0) & (sx < sw) & (sy >= 0) & (sy < sh)
        out[inside] = S[sy[inside], sx[inside]]
        return out, inside
    xc = x.astype(np.float64) + 0.5
    yc = y.astype(np.float64) + 0.5
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    inside = ~((xin < 0) | (xin >= sw) | (yin < 0) | (yin >= sh))
    xin = xin - 0.5
    yin = yin - 0.5
    ix, iy = _floor_int(xin), _floor_int(yin)
    dx = (xin - ix)[..., None]
    dy = (yin - iy)[..., None]
    F = S.astype(np.float64)
    cx = lambda v: np.clip(v, 0, sw - 1)
    cy = lambda v: np.clip(v, 0, sh - 1)
    if filt == BILINEAR:
        r0 = cy(iy)
        v1 = _lerp(F[r0, cx(ix)], F[r0, cx(ix + 1)], dx)
        has2 = ((iy + 1 >= 0) & (iy + 1 < sh))[..., None]
        r1 = cy(iy + 1)
        v2 = np.where(has2, _lerp(F[r1, cx(ix)], F[r1, cx(ix + 1)], dx), v1)
        V = np.trunc(_lerp(v1, v2, dy))
    elif filt == BICUBIC:
        row = lambda r: _cubic(F[r, cx(ix - 1)], F[r, cx(ix)], F[r, cx(ix + 1)], F[r, cx(ix + 2)], dx)
        v = [row(cy(iy - 1))]
        for j in (0, 1, 2):
            ok = ((iy + j >= 0) & (iy + j < sh))[..., None]
            v.append(np.where(ok, row(cy(iy + j)), v[-1]))
        r = _cubic(v[0], v[1], v[2], v[3], dy)
        V = np.where(r <= 0, 0.0, np.where(r >= 255.0, 255.0, np.trunc(r)))
    else:
        raise ValueError("no warp with filter %r" % (filt,))
    out[inside] = V[inside].astype(np.uint8)
    return out, inside


def rotate_matrix(angle, size):
    """Pillow's Image.rotate matrix without expand: the angle mod 360, cos / sin of -radians(angle) rounded to 15 places, centre (w / 2, h / 2)"""
    w, h = size
    angle = angle % 360.0
    rad = -math.radians(angle)
    c, s = round(math.cos(rad), 15), round(math.sin(rad), 15)
    cx, cy = w / 2.0, h / 2.0
    return (c, s, (c * -cx + s * -cy + 0.0) + cx, -s, c, (-s * -cx + c * -cy + 0.0) + cy)


def affine_matrix(center, angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0)):
    """the inverse, by numpy.linalg.inv, of T(center + translate) . R(angle) . scale . Shear(shear) . T(-center) in homogeneous coordinates"""
    r, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    T = lambda tx, ty: np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
    R = np.array([[math.cos(r), math.sin(r), 0.0], [-math.sin(r), math.cos(r), 0.0], [0.0, 0.0, 1.0]])
    Sh = np.array([[1.0, -math.tan(sx), 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [-math.tan(sy), 1.0, 0.0], [0.0, 0.0, 1.0]])
    K = np.diag([scale, scale, 1.0])
    M = T(center[0] + translate[0], center[1] + translate[1]) @ R @ K @ Sh @ T(-center[0], -center[1])
    inv = np.linalg.inv(M)
    return tuple(inv[0]) + tuple(inv[1])


def centred(m0, m1, m3, m4, src_size, size):
    """the map with the given 2 x 2 part that sends the centre of the output to the centre of the source: m2 = sw / 2 - (m0 * ow / 2 + m1 * oh / 2)"""
    sw, sh = src_size
    ow, oh = size
    return (m0, m1, sw / 2.0 - (m0 * ow / 2.0 + m1 * oh / 2.0), m3, m4, sh / 2.0 - (m3 * ow / 2.0 + m4 * oh / 2.0))


def rotation(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return (c, s, -s, c)


def map_classes(src_size, size):
    """(name, map, centred) for every class of map the tests use, for a source of src_size read into an output of `size`"""
    sw, sh = src_size
    ow, oh = size
    out = [("identity", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), False),
           ("translate_int", (1.0, 0.0, 2.0, 0.0, 1.0, -1.0), False),
           ("translate_half", (1.0, 0.0, 0.5, 0.0, 1.0, -0.5), False),
           ("scale_half", centred(0.5, 0.0, 0.0, 0.5, src_size, size), True),
           ("scale_two", centred(2.0, 0.0, 0.0, 2.0, src_size, size), False),
           ("scale_negative", centred(-1.0, 0.0, 0.0, -0.75, src_size, size), True),
           ("shear", centred(1.0, 0.3, 0.0, 1.0, src_size, size), False),
           ("all_outside", (1.0, 0.0, float(sw) + 3.0, 0.0, 1.0, float(sh) + 5.0), False)]
    for deg in (30.0, -17.5, 123.4):
        c, s, ms, c2 = rotation(deg)
        k = 0.95 * min(sw / (abs(c) * ow + abs(s) * oh), sh / (abs(s) * ow + abs(c) * oh))   # shrunk until the turned output rectangle fits the source
        out.append(("rotate_%g" % deg, centred(k * c, k * s, k * ms, k * c2, src_size, size), True))
    return out
