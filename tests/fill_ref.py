"""The NumPy float32 restatement of filled pyramid views: upsampling by 2^d with half-pixel centres, the
compose of a level's available tiles over an upsampled coarser picture (on tests/tiled_ref.py's blend), and the chain down the
levels.  CPU only; vam_tile_compose and vampic.pyramid's ``fill=True`` must match it bit for bit.

Nothing here calls the package: the index arithmetic is written out again, with Python integers and floor division in place
of the kernel's shifts, so that a mistake in the package cannot hide in its own test."""
import numpy as np

import tiled_ref as TR


def axis(P, d, N):
    """(r0, r1, f) for the coordinates ``P`` (an int array) of level k along an axis of N pixels at level j = k + d:
    n = 2 P + 1 - 2^d, a = floor(n / 2^(d+1)), f = float32(n - a 2^(d+1)) / float32(2^(d+1)), the sources clamped to 0 .. N - 1."""
    P = np.asarray(P, dtype=np.int64)
    D = 2 ** (d + 1)
    n = 2 * P + 1 - 2 ** d
    a = np.floor_divide(n, D)
    f = (n - a * D).astype(np.float32) / np.float32(D)
    return np.clip(a, 0, N - 1), np.clip(a + 1, 0, N - 1), f


def source_window(window, d, Hj, Wj):
    """The smallest window of level j that :func:`upsample` of ``window`` reads, by looking at every row and column."""
    y0, x0, h, w = window
    r0, r1, _ = axis(y0 + np.arange(h), d, Hj)
    c0, c1, _ = axis(x0 + np.arange(w), d, Wj)
    ya, yb, xa, xb = int(min(r0.min(), r1.min())), int(max(r0.max(), r1.max())), int(min(c0.min(), c1.min())), int(max(c0.max(), c1.max()))
    return ya, xa, yb - ya + 1, xb - xa + 1


def lerp(p, q, f):
    """p + f * (q - p): a subtract, a multiply and an add, each rounded to float32."""
    diff = (q - p).astype(np.float32)
    return (p + (f * diff).astype(np.float32)).astype(np.float32)


def upsample(below, below_window, window, d, Hj, Wj):
    """float32 [3, h, w]: the window (y0, x0, h, w) of level k upsampled from ``below`` float32 [3, hb, wb], the window
    ``below_window`` = (by0, bx0, hb, wb) of the level-j picture of Hj x Wj."""
    y0, x0, h, w = window
    by0, bx0, hb, wb = below_window
    below = np.asarray(below, dtype=np.float32)
    assert below.shape == (3, hb, wb) and 0 <= by0 and by0 + hb <= Hj and 0 <= bx0 and bx0 + wb <= Wj
    r0, r1, fy = axis(y0 + np.arange(h), d, Hj)
    c0, c1, fx = axis(x0 + np.arange(w), d, Wj)
    r0, r1, c0, c1 = r0 - by0, r1 - by0, c0 - bx0, c1 - bx0
    assert min(r0.min(), r1.min(), c0.min(), c1.min()) >= 0 and max(r0.max(), r1.max()) < hb and max(c0.max(), c1.max()) < wb
    fx, fy = fx[None, None, :], fy[None, :, None]
    top = lerp(below[:, r0][:, :, c0], below[:, r0][:, :, c1], fx)
    bottom = lerp(below[:, r1][:, :, c0], below[:, r1][:, :, c1], fx)
    return lerp(top, bottom, fy)


def sharp(slot, g, window):
    """bool [h, w]: the pixels all of whose tiles (1, 2 or 4: those the blend sums) have a slot >= 0."""
    y0, x0, h, w = window
    slot = np.asarray(slot)

    def tiles(P, S, n):
        t1 = np.minimum(n - 1, P // S)
        two = (t1 > 0) & (P - t1 * S < g["V"])
        return t1, np.where(two, t1 - 1, t1)
    ra, rb = tiles(y0 + np.arange(h), g["Sy"], g["R"])
    ca, cb = tiles(x0 + np.arange(w), g["Sx"], g["C"])
    ok = slot >= 0
    return ok[ra[:, None], ca[None, :]] & ok[ra[:, None], cb[None, :]] & ok[rb[:, None], ca[None, :]] & ok[rb[:, None], cb[None, :]]


def compose(tiles, slot, g, window, below, below_window, d, Hj, Wj):
    """float32 [3, h, w]: tiled_ref.blend where :func:`sharp`, :func:`upsample` of ``below`` elsewhere.  ``slot`` None: no
    tiles."""
    up = upsample(below, below_window, window, d, Hj, Wj)
    if slot is None:
        return up
    mask = sharp(slot, g, window)
    blend = TR.blend(tiles, slot, g, window)[0]
    return np.where(mask[None], blend, up).astype(np.float32)


def chain(levels, shapes, window, k):
    """float32 [3, h, w]: F_k(window).  ``levels[j]``: None for a level that is not usable, else (tiles, slot, g) with slot
    -1 where a tile is not available; ``shapes[j]`` = (H_j, W_j).  The coarsest usable level must be sharp all over the
    window it is asked for."""
    above = [j for j in range(k + 1, len(levels)) if levels[j] is not None]
    if not above:
        tiles, slot, g = levels[k]
        assert sharp(slot, g, window).all()
        return TR.blend(tiles, slot, g, window)[0]
    j = above[0]
    src = source_window(window, j - k, *shapes[j])
    below = chain(levels, shapes, src, j)
    if levels[k] is None:
        return compose(None, None, None, window, below, src, j - k, *shapes[j])
    tiles, slot, g = levels[k]
    return compose(tiles, slot, g, window, below, src, j - k, *shapes[j])
