"""NumPy restatement of pyramid viewports: the taps, the level, the support window and the resampled
picture.  CPU only; it calls nothing of the package.  The rule is evaluated in Python integers, the values in float32, one
operation at a time: vam_picture_resample and vampic.pyramid's ``viewport`` must match it bit for bit.

A viewport is ``rect = (y0, x0, h, w)`` in level-0 pixels divided by ``unit`` and ``out_hw = (oh, ow)``.  From level k, output row
Y has its centre at ``n / D`` with ``D = 2^(k+1) oh unit``, ``n = 2 oh y0 + (2 Y + 1) h - 2^k oh unit``; the tent reaches ``T = max(D,
2 h)``; the taps are the integers i with ``|D i - n| < T`` of weight ``u_i = T - |D i - n|``, read at ``clamp(i, 0, H_k - 1)``."""
from fractions import Fraction

import numpy as np


def level_shape(H, W, k):
    return -(-H // 2 ** k), -(-W // 2 ** k)


def axis_taps(origin, extent, out, k, unit):
    """[(first tap, [u_first, ...])] for the output coordinates 0 .. out - 1 of one axis, by walking outwards from the centre
    while ``|D i - n| < T`` holds."""
    D = 2 ** (k + 1) * out * unit
    T = max(D, 2 * extent)
    taps = []
    for P in range(out):
        n = 2 * out * origin + (2 * P + 1) * extent - 2 ** k * out * unit
        lo = hi = n // D                                    # |D floor(n / D) - n| < D <= T: always a tap
        while abs(D * (lo - 1) - n) < T:
            lo -= 1
        while abs(D * (hi + 1) - n) < T:
            hi += 1
        taps.append((lo, [T - abs(D * i - n) for i in range(lo, hi + 1)]))
    return taps


def scales(rect, out_hw, k, unit=1):
    """(the row scale, the column scale) at level k, exact."""
    return Fraction(rect[2], out_hw[0] * unit * 2 ** k), Fraction(rect[3], out_hw[1] * unit * 2 ** k)


def level(rect, out_hw, n_levels, unit=1):
    """k*: the largest k below n_levels with both scales at least 1; 0 when there is none."""
    ks = [k for k in range(n_levels) if min(scales(rect, out_hw, k, unit)) >= 1]
    return max(ks) if ks else 0


def support_window(rect, out_hw, k, H, W, unit=1):
    """(y0, x0, h, w) of level k: the smallest and the largest clamped tap over ALL output coordinates, per axis."""
    out = []
    for origin, extent, o_n, N in ((rect[0], rect[2], out_hw[0], level_shape(H, W, k)[0]), (rect[1], rect[3], out_hw[1], level_shape(H, W, k)[1])):
        idx = [min(max(i, 0), N - 1) for first, u in axis_taps(origin, extent, o_n, k, unit) for i in (first, first + len(u) - 1)]
        out.append((min(idx), max(idx)))
    return out[0][0], out[1][0], out[0][1] - out[0][0] + 1, out[1][1] - out[1][0] + 1


def _weights32(u):
    S = np.float32(sum(u))                                  # below 2^53: the conversion rounds once
    return [np.float32(np.float32(v) / S) for v in u]


def resample(src, src_window, level_hw, k, rect, unit, out_hw):
    """float32 [C, oh, ow]: ``sum_r wy_r * (sum_c wx_c * s[r][c])``, taps ascending, each sum from its first term, every multiply
    and add one float32 operation.  ``src`` float32 [C, hs, ws] is the window ``src_window`` of the level's picture of
    ``level_hw``; it must hold every tap.  The inner sums are taken for whole source rows at once and the outer ones for whole
    output rows: the same operations on the same operands as pixel by pixel."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    sy0, sx0, hs, ws = src_window
    assert src.shape[1:] == (hs, ws)
    (Hk, Wk), (oh, ow) = level_hw, out_hw
    C = src.shape[0]
    inner = np.empty((C, hs, ow), dtype=np.float32)
    for X, (first, u) in enumerate(axis_taps(rect[1], rect[3], ow, k, unit)):
        acc = None
        for j, wx in enumerate(_weights32(u)):
            c = min(max(first + j, 0), Wk - 1) - sx0
            assert 0 <= c < ws, "src does not hold the column taps"
            t = wx * src[:, :, c]
            acc = t if acc is None else acc + t
        inner[:, :, X] = acc
    out = np.empty((C, oh, ow), dtype=np.float32)
    for Y, (first, u) in enumerate(axis_taps(rect[0], rect[2], oh, k, unit)):
        acc = None
        for j, wy in enumerate(_weights32(u)):
            r = min(max(first + j, 0), Hk - 1) - sy0
            assert 0 <= r < hs, "src does not hold the row taps"
            t = wy * inner[:, r, :]
            acc = t if acc is None else acc + t
        out[:, Y, :] = acc
    assert out.dtype == np.float32
    return out


def resample_exact(src, src_window, level_hw, k, rect, unit, out_hw):
    """(float64 [C, oh, ow], the largest row tap count, the largest column tap count): the same sums with the exact rational
    weights u / S, rounded once to float64, and float64 arithmetic."""
    src = np.asarray(src, dtype=np.float64)
    sy0, sx0, hs, ws = src_window
    (Hk, Wk), (oh, ow) = level_hw, out_hw
    ty, tx = axis_taps(rect[0], rect[2], oh, k, unit), axis_taps(rect[1], rect[3], ow, k, unit)
    inner = np.zeros((src.shape[0], hs, ow))
    for X, (first, u) in enumerate(tx):
        for j, v in enumerate(u):
            inner[:, :, X] += float(Fraction(v, sum(u))) * src[:, :, min(max(first + j, 0), Wk - 1) - sx0]
    out = np.zeros((src.shape[0], oh, ow))
    for Y, (first, u) in enumerate(ty):
        for j, v in enumerate(u):
            out[:, Y, :] += float(Fraction(v, sum(u))) * inner[:, min(max(first + j, 0), Hk - 1) - sy0, :]
    return out, max(len(u) for _, u in ty), max(len(u) for _, u in tx)


def to_u8(x):
    """uint8 [h, w, 3] of float32 [3, h, w]: rint(clip(v, 0, 1) * 255), half to even."""
    return np.rint(np.clip(x, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
