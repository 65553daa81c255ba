"""Pillow's 8-bit bilinear / bicubic resampler restated in NumPy, as include/heif_hipdec.h defines HIPDEC_SCALE_BILINEAR / HIPDEC_SCALE_BICUBIC: per-axis
coefficient tables in IEEE double (Python floats: one rounding per operation, nothing contracted), 22 fractional bits, the horizontal pass first, the
intermediate rounded and clipped to 8 bits between the passes.  int64 sums, so an accumulator that would not fit 32 bits shows as a difference, not as a wrap.
tests/test_resample_ref.py pins it to PIL.Image.resize; the GPU tests read only this file (Pillow may be absent where they run)."""
import functools

import numpy as np

BILINEAR, BICUBIC = 16, 17
PRECISION_BITS = 22


def _f(filt, x):
    x = abs(x)
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=256)
def table(n_in, n_out, filt):
    """((xmin, (k0, k1, ...)), ...) for every output sample of an axis of n_in -> n_out samples"""
    scale = float(n_in) / n_out
    fs = max(scale, 1.0)
    support = (1.0 if filt == BILINEAR else 2.0) * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)      # int(): truncation toward zero, as the C conversion
        xmax = min(int(center + support + 0.5), n_in)
        w = [_f(filt, (x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = tuple(int(v * 4194304.0 + (-0.5 if v < 0 else 0.5)) for v in w)
        out.append((xmin, k))
    return tuple(out)


def _pass(a, n_out, filt, stats):
    """resamples axis 1 of a (rows, n_in, channels) uint8 array"""
    t = table(a.shape[1], n_out, filt)
    src = a.astype(np.int64)
    out = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
    for xx, (xmin, k) in enumerate(t):
        kk = np.asarray(k, np.int64)
        s = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + len(k), :], kk, axes=([1], [0]))
        if stats is not None:
            stats["min"] = min(stats.get("min", 0), int(s.min()))
            stats["max"] = max(stats.get("max", 0), int(s.max()))
        out[:, xx, :] = np.clip(s >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resample(img, out_w, out_h, filt, stats=None):
    """img: (h, w, c) or (h, w) uint8 -> (out_h, out_w, c) / (out_h, out_w).  stats (a dict): receives the smallest and largest pre-clip sum seen."""
    a = np.asarray(img)
    assert a.dtype == np.uint8
    flat = a.ndim == 2
    if flat:
        a = a[:, :, None]
    hpass = _pass(a, out_w, filt, stats)                                   # horizontal first
    v = _pass(np.ascontiguousarray(hpass.transpose(1, 0, 2)), out_h, filt, stats).transpose(1, 0, 2)
    v = np.ascontiguousarray(v)
    return v[:, :, 0] if flat else v
