"""The NumPy float32 restatement of the tiled-picture geometry: extraction with a replicated edge, the
blend ramps and the blend.  CPU only; the device kernels (vam_tile_extract, vam_tile_blend) must match it bit for bit.

The geometry ``g`` is vampic.tiled.grid's dict, but nothing here calls the package: the ramps and the tile arithmetic are
written out again, so that a mistake in the package cannot hide in its own test."""
import numpy as np

F1 = np.float32(1)


def ramps(V):
    """(w_lo, w_hi) float32 [V]: w_hi[t] = float32((t + 0.5) / V) computed in float64 and rounded once, w_lo = 1 - w_hi in
    float32."""
    w_hi = np.array([(t + 0.5) / V for t in range(V)], dtype=np.float64).astype(np.float32)
    return (F1 - w_hi).astype(np.float32), w_hi


def extract(image, g, coords):
    """float32 [n, 3, th, tw]: tile (r, c) of ``image`` [3, H, W] for every (r, c) of ``coords``, the edge replicated."""
    out = np.empty((len(coords), 3, g["th"], g["tw"]), dtype=np.float32)
    for i, (r, c) in enumerate(coords):
        ys = np.clip(r * g["Sy"] + np.arange(g["th"]), 0, g["H"] - 1)
        xs = np.clip(c * g["Sx"] + np.arange(g["tw"]), 0, g["W"] - 1)
        out[i] = image[:, ys[:, None], xs[None, :]]
    return out


def _axis(P, S, V, n, w_lo, w_hi):
    """Per pixel coordinate P along an axis of n tiles with stride S, two candidates in ascending tile order: (tile, local
    coordinate, weight, used).  The upper tile t1 = min(n - 1, P // S) is always used; in the band (t1 > 0 and P - t1 S < V)
    it takes w_hi and tile t1 - 1, at local coordinate + S, takes w_lo."""
    t1 = np.minimum(n - 1, P // S)
    l1 = P - t1 * S
    two = (t1 > 0) & (l1 < V)
    lb = np.where(two, l1, 0)
    hi_w = np.where(two, w_hi[lb] if V else F1, F1).astype(np.float32)
    lo_w = np.where(two, w_lo[lb] if V else F1, F1).astype(np.float32)
    return [(np.where(two, t1 - 1, 0), np.where(two, l1 + S, 0), lo_w, two), (t1, l1, hi_w, np.ones_like(two))]


def blend(tiles, slot, g, window=None):
    """(float32 [3, h, w], missing): the window (y0, x0, h, w) of the picture blended from ``tiles`` [n, 3, th, tw] through
    the slot map int [R, C] (-1: absent).  Per pixel the sum, over its tiles in ascending r and within that ascending c, of
    (wy * wx) * v, each product and each add one float32 operation, starting from the first term.  ``missing``: whether a
    pixel needed an absent tile (its term is skipped; a pixel without any term is 0)."""
    y0, x0, h, w = (0, 0, g["H"], g["W"]) if window is None else window
    w_lo, w_hi = ramps(g["V"]) if g["V"] else (None, None)
    rows = _axis(y0 + np.arange(h), g["Sy"], g["V"], g["R"], w_lo, w_hi)
    cols = _axis(x0 + np.arange(w), g["Sx"], g["V"], g["C"], w_lo, w_hi)
    tiles = np.asarray(tiles, dtype=np.float32)
    slot = np.asarray(slot)
    acc = np.zeros((3, h, w), dtype=np.float32)
    started = np.zeros((h, w), dtype=bool)
    missing = False
    for r, ly, wy, uy in rows:
        for c, lx, wx, ux in cols:
            s = slot[r[:, None], c[None, :]]
            used = uy[:, None] & ux[None, :]
            missing = missing or bool((used & (s < 0)).any())
            used = used & (s >= 0)
            wgt = (wy[:, None] * wx[None, :]).astype(np.float32)
            v = tiles[np.where(used, s, 0)[None], np.arange(3)[:, None, None], ly[None, :, None], lx[None, None, :]]
            term = (wgt[None] * v).astype(np.float32)
            acc = np.where(used[None], np.where(started[None], (acc + term).astype(np.float32), term), acc)
            started = started | used
    return acc, missing


def to_u8(x):
    """uint8 [h, w, 3] of float32 [3, h, w]: rint(clip(v, 0, 1) * 255), which rounds half to even (evaluate.write_image)."""
    return np.rint(np.clip(x, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
