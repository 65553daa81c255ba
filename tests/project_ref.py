"""The integer stage of the projective tensor output (include/heif_hipdec.h, hipdec_tensor_project) restated in vectorised NumPy float64: what
PIL.Image.transform(size, PERSPECTIVE | QUAD, data, resample, fillcolor) computes for an 8-bit RGB picture, the refusals a map decides, and the two map
helpers (hipdec_quad_map, hipdec_perspective_map) restated.

NumPy evaluates every operation below as one IEEE double operation with one rounding; nothing here can be contracted into a fused multiply-add.
tests/test_project_ref.py pins this file to Pillow bit for bit (x86-64 builds of Pillow: see tests/warp_ref.py on aarch64).  The sampling from (xin, yin)
on is written out again here, not imported from tests/warp_ref.py, so that the file states the whole definition.

Nothing in this file comes from the library under test."""
from fractions import Fraction

import numpy as np

NEAREST, BILINEAR, BICUBIC = 0, 16, 17   # hipdec_scale_filter
PERSPECTIVE, QUAD = 0, 1                 # hipdec_tensor_projection.kind
LIMIT = 32000.0
MIN_DENOMINATOR = 1.0 / 1048576


def _floor_int(v):
    """FLOOR(v) = (int)floor(v) for v < 0, else (int)v"""
    return np.where(v < 0, np.floor(v), np.trunc(v)).astype(np.int64)


def _coord(v):
    """COORD(v) = -1 for v < 0, else (int)v"""
    return np.where(v < 0, -1.0, np.trunc(v)).astype(np.int64)


def point(a, kind, xc, yc):
    """(xin, yin) of the point (xc, yc), operator for operator; a: eight float64"""
    if kind == QUAD:
        return a[0] + a[1] * xc + a[2] * yc + a[3] * xc * yc, a[4] + a[5] * xc + a[6] * yc + a[7] * xc * yc
    return (a[0] * xc + a[1] * yc + a[2]) / (a[6] * xc + a[7] * yc + 1.0), (a[3] * xc + a[4] * yc + a[5]) / (a[6] * xc + a[7] * yc + 1.0)


def refused(m, kind, size, reserved=0):
    """the refusals a map alone decides for an output of size = (ow, oh)"""
    if kind not in (PERSPECTIVE, QUAD) or reserved != 0:
        return True
    a = np.asarray(m, np.float64)
    if a.shape != (8,) or not np.isfinite(a).all() or (np.abs(a) >= LIMIT).any():
        return True
    with np.errstate(all="ignore"):
        for cx in (np.float64(0.0), np.float64(size[0])):
            for cy in (np.float64(0.0), np.float64(size[1])):
                if kind == PERSPECTIVE and not (a[6] * cx + a[7] * cy + 1.0 >= MIN_DENOMINATOR):
                    return True
                xin, yin = point(a, kind, cx, cy)
                if not abs(xin) < LIMIT or not abs(yin) < LIMIT:
                    return True
    return False


def _lerp(p, q, d):
    return p + (q - p) * d


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2.0 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def project(src, m, kind, size, filt, fill=(0, 0, 0)):
    """src: (sh, sw, 3) uint8; m: eight numbers; size = (ow, oh).  Returns ((oh, ow, 3) uint8 with `fill` outside, (oh, ow) bool inside-mask)."""
    S = np.asarray(src)
    assert S.dtype == np.uint8 and S.ndim == 3 and S.shape[2] == 3
    assert not refused(m, kind, size), "the definition covers the maps the library takes"
    sh, sw = S.shape[:2]
    ow, oh = size
    a = [np.float64(v) for v in m]
    out = np.empty((oh, ow, 3), np.uint8)
    out[...] = np.asarray(fill, np.uint8)
    xc = np.broadcast_to(np.arange(ow, dtype=np.float64)[None, :] + 0.5, (oh, ow))
    yc = np.broadcast_to(np.arange(oh, dtype=np.float64)[:, None] + 0.5, (oh, ow))
    xin, yin = point(a, kind, xc, yc)
    if filt == NEAREST:
        sx, sy = _coord(xin), _coord(yin)
        inside = (sx >= 0) & (sx < sw) & (sy >= 0) & (sy < sh)
        out[inside] = S[sy[inside], sx[inside]]
        return out, inside
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
        raise ValueError("no projection with filter %r" % (filt,))
    out[inside] = V[inside].astype(np.uint8)
    return out, inside


def quad_map(corners, size):
    """Pillow's Python arithmetic for Image.transform(size, QUAD, corners): corners = (nw, sw, se, ne) as eight numbers, size the OUTPUT size"""
    w, h = size
    nwx, nwy, swx, swy, sex, sey, nex, ney = (float(v) for v in corners)
    As = 1.0 / w
    At = 1.0 / h
    return (nwx, (nex - nwx) * As, (swx - nwx) * At, (sex - swx - nex + nwx) * As * At,
            nwy, (ney - nwy) * As, (swy - nwy) * At, (sey - swy - ney + nwy) * As * At)


def perspective_system(startpoints, endpoints, num=float):
    """the 8 x 8 system of torchvision's _get_perspective_coeffs: (rows, right-hand side) with entries of type `num`"""
    A, b = [], []
    for (sx, sy), (ex, ey) in zip(startpoints, endpoints):
        sx, sy, ex, ey = num(sx), num(sy), num(ex), num(ey)
        z, one = num(0), num(1)
        A.append([ex, ey, one, z, z, z, -sx * ex, -sx * ey])
        b.append(sx)
        A.append([z, z, z, ex, ey, one, -sy * ex, -sy * ey])
        b.append(sy)
    return A, b


def perspective_map(startpoints, endpoints):
    """the system solved by numpy.linalg.solve in float64 (LAPACK's LU with partial pivoting)"""
    A, b = perspective_system(startpoints, endpoints)
    return tuple(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)))


def perspective_map_exact(startpoints, endpoints):
    """the system solved exactly over the rationals (the points are doubles, hence rationals), each coefficient rounded once to double"""
    A, b = perspective_system(startpoints, endpoints, Fraction)
    n = 8
    M = [row + [rhs] for row, rhs in zip(A, b)]
    for col in range(n):
        piv = next(r for r in range(col, n) if M[r][col] != 0)
        M[col], M[piv] = M[piv], M[col]
        for r in range(n):
            if r != col and M[r][col] != 0:
                f = M[r][col] / M[col][col]
                M[r] = [x - f * y for x, y in zip(M[r], M[col])]
    return tuple(float(M[i][n] / M[i][i]) for i in range(n))


def keystone(src_size, size, kx, ky, shrink=1.0):
    """a PERSPECTIVE map whose denominator runs from 1 to 1 + kx across the output's width and to 1 + ky down its height, and which sends the output's
    centre to the source's centre at `shrink` source pixels per unit of the normalised output"""
    sw, sh = src_size
    ow, oh = size
    a6, a7 = kx / ow, ky / oh
    dc = a6 * ow / 2.0 + a7 * oh / 2.0 + 1.0
    a0, a4 = shrink * sw / ow, shrink * sh / oh
    # numerators at the centre: (a0 * ow / 2 + a2) / dc = sw / 2
    return (a0, 0.0, sw / 2.0 * dc - a0 * ow / 2.0, 0.0, a4, sh / 2.0 * dc - a4 * oh / 2.0, a6, a7)


def perspective_classes(src_size, size):
    """(name, eight coefficients) of every class of PERSPECTIVE map the tests use, for a source of src_size read into an output of `size`"""
    sw, sh = src_size
    ow, oh = size
    fx, fy = sw / ow, sh / oh
    return [("identity", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)),
            ("affine_only", (0.9 * fx, 0.2 * fx, 0.25, -0.15 * fy, 0.8 * fy, 0.5, 0.0, 0.0)),
            ("keystone_x", keystone(src_size, size, 0.6, 0.0)),
            ("keystone_y", keystone(src_size, size, 0.0, -0.4)),
            ("keystone_both", keystone(src_size, size, 0.5, 0.7, 1.2)),
            ("denominator_quarter_to_four", (0.25 * fx, 0.0, 0.0, 0.0, 0.25 * fy, 0.0, 3.75 / ow, 0.0) if ow > 1 else
             (0.25 * fx, 0.0, 0.0, 0.0, 0.25 * fy, 0.0, 0.0, 3.75 / oh)),
            ("partly_outside", keystone(src_size, size, 0.8, 0.3, 1.9)),
            ("all_outside", (1.0, 0.0, float(sw) + 3.0, 0.0, 1.0, float(sh) + 5.0, 0.01 / ow, 0.02 / oh))]


def quad_classes(src_size, size):
    """(name, corners nw sw se ne as eight numbers) of every class of QUAD the tests use; quad_map(corners, size) gives the coefficients"""
    sw, sh = float(src_size[0]), float(src_size[1])
    return [("own_corners", (0.0, 0.0, 0.0, sh, sw, sh, sw, 0.0)),
            ("jittered", (0.11 * sw, 0.07 * sh, -0.05 * sw, 0.93 * sh, 0.96 * sw, 1.04 * sh, 0.88 * sw, 0.13 * sh)),
            ("non_convex", (0.0, 0.0, 0.1 * sw, sh, 0.35 * sw, 0.4 * sh, sw, 0.05 * sh)),
            ("outside", (sw + 2.0, sh + 1.0, sw + 2.5, 2.0 * sh + 3.0, 2.0 * sw + 4.0, 2.0 * sh + 2.0, 2.0 * sw + 5.0, sh + 1.5))]


def map_classes(src_size, size):
    """(name, kind, eight coefficients) of all of the above"""
    return [("perspective_" + n, PERSPECTIVE, m) for n, m in perspective_classes(src_size, size)] + \
           [("quad_" + n, QUAD, quad_map(c, size)) for n, c in quad_classes(src_size, size)]
