"""Shared by the tests of the interleaved base: NHWC windows with guard channels, the host jobs they
stand for, and hand-made "embedded-4" containers.  No GPU is needed to import this."""
import numpy as np

# (B, h, w, ld, c0, C, n_slices): n = C h w = 12, 512 and 1000 — fewer elements than 64 lanes, a multiple of every K, neither
GEOMETRIES = [(3, 2, 3, 11, 2, 2, 2), (2, 4, 4, 40, 4, 32, 1), (1, 10, 20, 7, 1, 5, 1)]
FILL = -12345


def window_case(t, geom, seed, channel_index=False):
    """(sym, idx) int32 [B, h, w, ld]: random in-range symbols with some escapes inside the window [c0, c0 + n_slices C),
    FILL in every guard channel.  ``channel_index``: the table index is the channel inside the slice (what idx = NULL
    means), which needs C <= the number of tables."""
    B, h, w, ld, c0, C, ns = geom
    rng = np.random.default_rng(seed)
    n_tab = t.cdf.shape[0]
    sym = np.full((B, h, w, ld), FILL, dtype=np.int32)
    idx = np.full((B, h, w, ld), FILL, dtype=np.int32)
    shape = (B, h, w, ns * C)
    if channel_index:
        assert C <= n_tab
        ci = np.broadcast_to(np.tile(np.arange(C), ns), shape).astype(np.int32)
    else:
        ci = rng.integers(0, n_tab, shape).astype(np.int32)
    mx = t.sizes[ci].astype(np.int64) - 2
    v = rng.integers(0, 1 << 30, shape) % np.maximum(mx, 1) + t.offsets[ci]
    esc = rng.random(shape) < 0.08                           # beyond the table on either side: the bypass nibbles
    v = np.where(esc, t.offsets[ci] + np.where(rng.random(shape) < 0.5, -rng.integers(1, 3000, shape), mx + rng.integers(0, 3000, shape)), v)
    sym[..., c0:c0 + ns * C] = v.astype(np.int32)
    idx[..., c0:c0 + ns * C] = ci
    return sym, idx


def window_jobs(sym, idx, geom):
    """The host jobs of a window in stream order (stream id = slice * B + image): (symbols, indexes), each [C, h, w]."""
    B, h, w, ld, c0, C, ns = geom
    cut = lambda a, b, s: np.ascontiguousarray(a[b, :, :, c0 + s * C:c0 + (s + 1) * C].transpose(2, 0, 1))
    return [(cut(sym, b, s), cut(idx, b, s)) for s in range(ns) for b in range(B)]


def container(scheduled=False, base_lanes=8, lanes=2):
    """A hand-made "embedded-4" container of two slices: z 10 bytes, base 4 + 6, embedded 40 + 60."""
    c = {"format": "embedded-4", "lanes": lanes, "base_lanes": base_lanes, "shape": (1, 2), "z": [b"z" * 10],
         "base": [[b"a" * 4], [b"b" * 6]], "embedded": [bytes(range(40)), bytes(range(100, 160))],
         "marks": {"q": [0.5, 2.5, 10.0], "count": [[3, 5], [9, 11], [20, 30]], "bytes": [[8, 12], [16, 24], [40, 60]]}}
    if scheduled:
        index = np.zeros((3, 4, 8), dtype=np.uint8)
        index[1:, :2] = 1
        index[2] = 2
        c["schedule"] = {"levels": [0.0, 2.5, 10.0], "index": index}
        c["side_bytes"] = 8 * 3 + 3 * 4 * 8
        c["marks"]["stage"] = [0, 1, 2]
        del c["marks"]["q"]
    return c
