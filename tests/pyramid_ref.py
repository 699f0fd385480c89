"""The NumPy restatement of resolution pyramids: the halving of a picture or a schedule, the shapes of
the levels and the mapping of a level-0 window onto a level.  CPU only; the device kernel (vam_picture_halve) must match
:func:`halve` bit for bit, the package's host arithmetic the rest value for value.

Nothing here calls the package: the clamped coordinates, the order of the float32 operations and the integer arithmetic are
written out again, so that a mistake in the package cannot hide in its own test."""
import numpy as np

QNAN = np.uint32(0x7FC00000)                # the NaN every NaN result is stored as


def halve(x, mode="mean"):
    """float32 [C, ceil(H / 2), ceil(W / 2)] of ``x`` float32 [C, H, W].  With y1 = min(2y + 1, H - 1), x1 = min(2x + 1, W - 1):

        mean:  ((x[c][2y][2x] + x[c][2y][x1]) + (x[c][y1][2x] + x[c][y1][x1])) * float32(0.25)
        max:   max(max(x[c][2y][2x], x[c][2y][x1]), max(x[c][y1][2x], x[c][y1][x1])),  max(p, q) = p when p >= q, else q

    every operation one float32 operation in this order (NumPy rounds every float32 add and multiply once).  inf and NaN
    propagate as the arithmetic gives them; in max mode a NaN among the four gives NaN; a NaN result has the bits ``QNAN``
    (which NaN inf - inf makes differs between processors)."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 3 and mode in ("mean", "max")
    _, H, W = x.shape
    ya, xa = 2 * np.arange((H + 1) // 2), 2 * np.arange((W + 1) // 2)
    yb, xb = np.minimum(ya + 1, H - 1), np.minimum(xa + 1, W - 1)
    a, b = x[:, ya[:, None], xa[None, :]], x[:, ya[:, None], xb[None, :]]
    c, d = x[:, yb[:, None], xa[None, :]], x[:, yb[:, None], xb[None, :]]
    with np.errstate(all="ignore"):
        if mode == "mean":
            out = ((a + b) + (c + d)) * np.float32(0.25)
        else:
            m0, m1 = np.where(a >= b, a, b), np.where(c >= d, c, d)
            out = np.where(m0 >= m1, m0, m1)
            out = np.where(np.isnan(a) | np.isnan(b) | np.isnan(c) | np.isnan(d), np.float32(np.nan), out)
    out = np.ascontiguousarray(out, dtype=np.float32)
    out.view(np.uint32)[np.isnan(out)] = QNAN
    return out


def level_shapes(H, W, n_levels):
    """[(H_k, W_k)]: level 0 is (H, W), every further level halves the one before, rounding up."""
    shapes = [(H, W)]
    for _ in range(1, n_levels):
        h, w = shapes[-1]
        shapes.append(((h + 1) // 2, (w + 1) // 2))
    return shapes


def window_at(window, k, H, W):
    """The smallest window (y0, x0, h, w) of level k whose pixels, each standing for a 2^k x 2^k block of level 0 clipped
    to the picture, cover the level-0 window ``window``."""
    y0, x0, h, w = window
    assert 0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W
    s = 2 ** k
    ya, xa = y0 // s, x0 // s
    yb, xb = (y0 + h + s - 1) // s, (x0 + w + s - 1) // s
    Hk, Wk = level_shapes(H, W, k + 1)[k]
    return ya, xa, min(yb, Hk) - ya, min(xb, Wk) - xa


def best_level(window, out_hw, H, W, n_levels):
    """The coarsest level whose window covering ``window`` has at least ``out_hw`` rows and columns; 0 when none has."""
    best = 0
    for k in range(n_levels):
        _, _, h, w = window_at(window, k, H, W)
        if h >= out_hw[0] and w >= out_hw[1]:
            best = k
    return best
