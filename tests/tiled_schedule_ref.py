"""The NumPy restatement of a tile's schedule: a picture-wide schedule at pixel resolution brought down
onto the latent grid of every tile.  CPU only; the device kernel (vam_tile_schedule) must match it value for value.

The geometry ``g`` is vampic.tiled.grid's dict, but nothing here calls the package: the clamped pixel coordinates and the
block maximum are written out again, so that a mistake in the package cannot hide in its own test."""
import numpy as np


def tile_schedule(maps, g, coords):
    """float32 [n, L, th / 16, tw / 16] of ``maps`` float32 [L, H, W] for every (r, c) of ``coords``:

        out[i, k, a, b] = max over y, x in [0, 16) of maps[k, min(r Sy + 16 a + y, H - 1), min(c Sx + 16 b + x, W - 1)]

    the block maximum of a latent cell over the tile's pixels, the picture's edge replicated.  A NaN anywhere in a block
    gives NaN (np.max propagates it)."""
    maps = np.asarray(maps, dtype=np.float32)
    L = maps.shape[0]
    h, w = g["th"] // 16, g["tw"] // 16
    out = np.empty((len(coords), L, h, w), dtype=np.float32)
    for i, (r, c) in enumerate(coords):
        ys = np.minimum(r * g["Sy"] + np.arange(g["th"]), g["H"] - 1)
        xs = np.minimum(c * g["Sx"] + np.arange(g["tw"]), g["W"] - 1)
        tile = maps[:, ys[:, None], xs[None, :]]                                # [L, th, tw], what vam_tile_extract would cut
        with np.errstate(invalid="ignore"):
            out[i] = tile.reshape(L, h, 16, w, 16).max(axis=(2, 4))
    return out


def same(a, b):
    """Equal as values: -0 equals +0, NaNs at equal positions."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return bool(np.array_equal(np.where(np.isnan(a), 0, a), np.where(np.isnan(b), 0, b)))
