"""The NumPy restatement of vam_tile_refresh: the blend of tests/tiled_ref.py restricted to the pixels
that a dirty tile contributes to.  CPU only; the device kernel must match it bit for bit."""
import numpy as np

import tiled_ref as TR


def _axes(g, y0, x0, h, w):
    w_lo, w_hi = TR.ramps(g["V"]) if g["V"] else (None, None)
    return (TR._axis(y0 + np.arange(h), g["Sy"], g["V"], g["R"], w_lo, w_hi),
            TR._axis(x0 + np.arange(w), g["Sx"], g["V"], g["C"], w_lo, w_hi))


def touched(dirty, g, window):
    """bool [h, w] over ``window`` = (y0, x0, h, w): whether one of a pixel's 1, 2 or 4 tiles is marked in ``dirty`` [R, C]."""
    y0, x0, h, w = window
    d = np.asarray(dirty) != 0
    rows, cols = _axes(g, y0, x0, h, w)
    out = np.zeros((h, w), dtype=bool)
    for r, _, _, uy in rows:
        for c, _, _, ux in cols:
            out |= uy[:, None] & ux[None, :] & d[r[:, None], c[None, :]]
    return out


def refresh(canvas, tiles, slot, dirty, g, canvas_window, box):
    """(the canvas afterwards, missing): ``canvas`` float32 [3, ch, cw] holds the window ``canvas_window`` = (cy0, cx0, ch, cw)
    of the picture; inside ``box`` = (y0, x0, h, w), in picture coordinates, every pixel with a dirty tile is taken from
    ``tiled_ref.blend`` of the box; every other pixel, inside the box or outside, is left as it was.  ``missing``: whether a
    pixel that was taken needed an absent tile (a slot < 0); the slots of pixels that are left are not looked at."""
    cy0, cx0, ch, cw = canvas_window
    y0, x0, h, w = box
    assert cy0 <= y0 and cx0 <= x0 and y0 + h <= cy0 + ch and x0 + w <= cx0 + cw
    take = touched(dirty, g, box)
    # a pixel that is left may lie in an absent tile: blend it through slot 0 of a copy, its value is thrown away
    slot = np.asarray(slot)
    used = np.where(_needed(take, g, box), slot, np.where(slot < 0, 0, slot))
    new, missing = TR.blend(tiles, used, g, box)
    if np.asarray(canvas).dtype == np.uint8:                # a uint8 canvas [ch, cw, 3] takes tiled_ref.to_u8 of the blend
        out = np.array(canvas, copy=True)
        part = out[y0 - cy0:y0 - cy0 + h, x0 - cx0:x0 - cx0 + w]
        part[:] = np.where(take[:, :, None], TR.to_u8(new), part)
        return out, missing
    out = np.array(canvas, dtype=np.float32, copy=True)
    part = out[:, y0 - cy0:y0 - cy0 + h, x0 - cx0:x0 - cx0 + w]
    part[:] = np.where(take[None], new, part)
    return out, missing


def _needed(take, g, box):
    """bool [R, C]: the tiles that a taken pixel of ``box`` lies in."""
    y0, x0, h, w = box
    rows, cols = _axes(g, y0, x0, h, w)
    need = np.zeros((g["R"], g["C"]), dtype=bool)
    for r, _, _, uy in rows:
        for c, _, _, ux in cols:
            m = uy[:, None] & ux[None, :] & take
            rr, cc = np.broadcast_to(r[:, None], m.shape)[m], np.broadcast_to(c[None, :], m.shape)[m]
            need[rr, cc] = True
    return need
