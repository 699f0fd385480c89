"""Resolution pyramids of tiled pictures: the picture at halved resolutions as well, coarsest first, so
that the first bytes are a thumbnail and a zoomed-out view decodes a small picture instead of every tile of the large one.

The definition, one rule for ``csrc/tiles.hip`` (vam_picture_halve), this module and ``tests/pyramid_ref.py``: level 0 is the
picture, fp32 [3, H, W]; level k >= 1 has ``H_k = ceil(H_{k-1} / 2)`` rows and ``W_k = ceil(W_{k-1} / 2)`` columns
(``H_k = ceil(H / 2^k)``), and with ``y1 = min(2y + 1, H_{k-1} - 1)``, ``x1 = min(2x + 1, W_{k-1} - 1)``

    P_k[c][y][x] = ((P_{k-1}[c][2y][2x] + P_{k-1}[c][2y][x1]) + (P_{k-1}[c][y1][2x] + P_{k-1}[c][y1][x1])) * 0.25f

every add and the multiply one fp32 operation in this order, the edge replicated at every level.  A schedule (section 9x) is
reduced alongside with the maximum of the four.  Pixel (y, x) of level k stands for the level-0 rows ``[y 2^k, (y + 1) 2^k)``
and the columns likewise, clipped to the picture; :func:`window_at` gives the smallest level-k window that covers a level-0
window.

The codestream: ``framing.PREAMBLE`` with magic ``b"VAMy"`` (version 1, reserved 0, bytes of the header, CRC-32 of the
header), a little-endian header (u32 H, W; u16 n_levels; u16 reserved (0); n_levels x u64 ``bytes_k`` for k = 0 .. n - 1, 0: the
level is absent; u64 total), then the body: the level codestreams, COARSEST FIRST (k = n - 1 down to 0), each exactly the bytes
``tiled.encode`` gives for that level's picture; nothing is re-framed.  From :func:`need_bytes` on every prefix decodes a
whole picture at some resolution.  Everything but :func:`encode`, :class:`PyramidDecoder`, and the views of
:class:`PyramidStream` is host arithmetic and needs neither a model nor a GPU.

Filled views: ``PyramidDecoder.decode(..., fill=True)`` and ``PyramidStream.view(..., fill=True)`` always
give a whole picture at the level asked for: sharp where that level's tiles have arrived, filled from the next coarser level,
upsampled, where they have not.  One rule for ``csrc/tiles.hip`` (vam_tile_compose), this module and ``tests/fill_ref.py``:
upsampling by 2^d from level j = k + d has half-pixel centres; for row Y of level k, ``n = 2 Y + 1 - 2^d``, ``a = floor(n /
2^(d+1))``, ``f_y = float(n - a 2^(d+1)) / 2^(d+1)`` (exact in fp32, never 0 or 1), the source rows ``r0 = clamp(a, 0, H_j - 1)``
and ``r1 = clamp(a + 1, 0, H_j - 1)``, the columns likewise, and with ``lerp(p, q, f) = p + f * (q - p)`` (three fp32 operations)
the value is ``lerp(lerp(s[r0][c0], s[r0][c1], f_x), lerp(s[r1][c0], s[r1][c1], f_x), f_y)``.  A level is USABLE when it is present
and the bytes hold its own picture header whole; a tile is AVAILABLE when its head is whole (at ``mark`` / ``stage`` m: and its
rounds 0 .. m).  ``F_k(window)`` composes level k's available tiles over the upsample of ``F_j(source_window(window))``, j the
smallest usable level above k; a level that is not usable contributes no tiles; the coarsest usable level has nothing below
it, and there a tile that is not available is a ValueError.  A pixel is sharp exactly when every tile the blend sums there is
available, and the switch is hard.

Viewports: ``PyramidDecoder.viewport`` and ``PyramidStream.viewport`` show a rectangle of the picture in
an output of any size, at any zoom and pan; :func:`extract_viewport` is the server's side.  One rule for ``csrc/tiles.hip``
(vam_picture_resample), this module and ``tests/resample_ref.py``, all indices and weights exact integer arithmetic: a viewport
is ``rect = (y0, x0, h, w)`` in level-0 pixels divided by an integer ``unit`` (1 .. 256; above 1 for sub-pixel pans) and
``out_hw = (oh, ow)``, 1 .. 65536 each, with ``rect / unit`` inside the picture.  Resampled from level k, output row Y has its
centre at ``n / D`` of level k, pixel i being centred at i + 1/2 on both sides (columns likewise):

    D = 2^(k+1) oh unit      n = 2 oh y0 + (2 Y + 1) h - 2^k oh unit      T = max(D, 2 h)

``T`` is the tent's half-width, max(1, scale) level-k pixels, the scale being ``h / (oh unit 2^k)``.  The taps are the integers i
with ``|D i - n| < T``, of integer weight ``u_i = T - |D i - n|`` and fp32 weight ``float(u_i) / float(S)``, ``S`` their sum, read
at ``clamp(i, 0, H_k - 1)``; the value is ``sum_r wy_r * (sum_c wx_c * s[r][c])``, taps ascending, every sum from its first term,
every multiply and add one fp32 operation.  The level ``k*`` (:func:`viewport_level`) is the largest k below n_levels with
``2^k oh unit <= h`` and ``2^k ow unit <= w``, 0 when there is none (magnification): the scales are then at least 1 on both axes
and below 2 on at least one.  A scale above 16 on either axis is refused.  The support window (:func:`viewport_window`) is what
the taps read of level k.

Viewing sessions: :func:`extract_viewport` cuts a self-contained stream per viewport and repeats what the
receiver holds; ``vampic.session`` keeps, on both sides, a ledger of the segments held per tile, and its ``Server.viewport`` /
``Server.window`` send for the same request (:func:`_viewport_cuts`, :func:`_kept`: one arithmetic) only what the ledger lacks,
to a ``Client`` that takes bytes by tile and keeps its cache of decoded tiles from viewport to viewport.

Out of scope: filters other than the tent and rotation; a persistent resampled ``Canvas``; fusing the resample into the
blend; feathering the seam between sharp and filled pixels; ``q=`` with ``fill``; a filled ``Canvas``; interleaving rounds
across levels; coding a level as a residual of the coarser one; entropy-coded headers.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence, Tuple

from . import embedded as EB
from . import tiled as TL
from .framing import PREAMBLE_BYTES, Frame, as_int, check_total, chunk_view, same, view

MAGIC = b"VAMy"
VERSION = 1
MAX_LEVELS = 16
_FIXED = struct.Struct("<IIHH")            # H, W, n_levels, reserved (0); then u64 bytes_k [n_levels] and the u64 total
FRAME = Frame(MAGIC, "a pyramid codestream", "pyramid codestream", (VERSION,), range(_FIXED.size + 16, _FIXED.size + 8 * MAX_LEVELS + 9, 8),
              f"the header of n = 1 .. {MAX_LEVELS} levels takes {_FIXED.size + 8} + 8 n")
_ALIKE = ("V", "allocation", "stages", "marks", "lanes", "base_lanes", "ns")


# ------------------------------------------------------------------------------------------------------------- geometry
def level_shapes(H: int, W: int, n_levels: int) -> List[Tuple[int, int]]:
    """[(H_k, W_k)] for k = 0 .. n_levels - 1: ``H_k = ceil(H / 2^k)``."""
    return [(-(-H // (1 << k)), -(-W // (1 << k))) for k in range(n_levels)]


def _check_levels(H: int, W: int, n: int, what: str) -> List[Tuple[int, int]]:
    if not (1 <= H <= TL.MAX_SIDE and 1 <= W <= TL.MAX_SIDE):
        raise ValueError(f"{what}: a picture of {H} x {W}: sides are 1 .. {TL.MAX_SIDE}")
    if not 1 <= n <= MAX_LEVELS:
        raise ValueError(f"{what}: levels is 1 .. {MAX_LEVELS}, got {n}")
    shapes = level_shapes(H, W, n)
    if n >= 2 and shapes[n - 2] == (1, 1):
        k = shapes.index((1, 1))
        raise ValueError(f"{what}: {n} levels of a {H} x {W} picture: level {k} is 1 x 1 already and level {k + 1} would repeat it; "
                         f"at most {k + 1} levels")
    return shapes


def default_levels(H: int, W: int, tile: int = 256) -> int:
    """Levels until a level fits one tile (``H_k <= tile and W_k <= tile``): at least 1, at most 16."""
    n = 1
    while n < MAX_LEVELS and not (-(-H // (1 << (n - 1))) <= tile and -(-W // (1 << (n - 1))) <= tile):
        n += 1
    return n


def window_at(window, k: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """The smallest window (y0, x0, h, w) of level k that covers the level-0 window ``window`` of an H x W picture (None:
    the picture): rows ``y0 >> k`` .. ``min(H_k, ceil((y0 + h) / 2^k))``, columns likewise."""
    k = as_int(k, "window_at: k")
    if not 0 <= k < 32:
        raise ValueError(f"window_at: k is a level, 0 .. 31, got {k}")
    y0, x0, h, w = TL._window({"H": H, "W": W}, window, "window_at")
    Hk, Wk = level_shapes(H, W, k + 1)[k]
    ya, xa = y0 >> k, x0 >> k
    return ya, xa, min(Hk, -(-(y0 + h) // (1 << k))) - ya, min(Wk, -(-(x0 + w) // (1 << k))) - xa


def best_level(window, out_hw, H: int, W: int, n_levels: int) -> int:
    """The coarsest level of ``n_levels`` whose window covering ``window`` (level-0 coordinates; None: the picture) has at
    least ``out_hw`` = (rows, columns) in both directions: the level to decode for a viewport of that size.  0 when not
    even level 0 has."""
    oh, ow = (as_int(v, "best_level: out_hw") for v in out_hw)
    n = as_int(n_levels, "best_level: n_levels")
    if oh < 1 or ow < 1 or n < 1:
        raise ValueError(f"best_level: out_hw is (rows, columns) >= 1 and n_levels >= 1, got {tuple(out_hw)} and {n}")
    best = 0
    for k in range(n):                                                          # the covering window never grows with k
        _, _, h, w = window_at(window, k, H, W)
        if h >= oh and w >= ow:
            best = k
    return best


def source_window(window, d: int, Hj: int, Wj: int) -> Tuple[int, int, int, int]:
    """The window (y0, x0, h, w) of level j = k + d, a picture of Hj x Wj, that upsampling by 2^d reads for the level-k
    window ``window``: rows ``clamp(a(y0))`` .. ``clamp(a(y0 + h - 1) + 1)`` with ``a(Y) = floor((2 Y + 1 - 2^d) / 2^(d+1))`` and the
    clamp to 0 .. Hj - 1, columns likewise (module docstring).  Host arithmetic only."""
    d, Hj, Wj = as_int(d, "source_window: d"), as_int(Hj, "source_window: Hj"), as_int(Wj, "source_window: Wj")
    if not 1 <= d <= 15:
        raise ValueError(f"source_window: d is 1 .. 15 (the levels between the two pictures), got {d}")
    if Hj < 1 or Wj < 1:
        raise ValueError(f"source_window: the coarser level is a picture of at least 1 x 1, got {Hj} x {Wj}")
    try:
        entries = list(window)
    except TypeError:
        entries = []
    if len(entries) != 4:
        raise ValueError(f"source_window: a window is (y0, x0, h, w), got {window!r}")
    y0, x0, h, w = (as_int(v, "source_window: a window entry") for v in entries)
    if y0 < 0 or x0 < 0 or h < 1 or w < 1:
        raise ValueError(f"source_window: a window is (y0, x0, h, w) with y0, x0 >= 0 and h, w >= 1, got {(y0, x0, h, w)}")
    a = lambda P: (2 * P + 1 - (1 << d)) >> (d + 1)         # Python's shift floors negative numbers too
    cl = lambda v, n: min(max(v, 0), n - 1)
    ya, yb, xa, xb = cl(a(y0), Hj), cl(a(y0 + h - 1) + 1, Hj), cl(a(x0), Wj), cl(a(x0 + w - 1) + 1, Wj)
    return ya, xa, yb - ya + 1, xb - xa + 1


MAX_UNIT, MAX_OUT, MAX_SCALE = 256, 65536, 16


def _viewport(what: str, rect, out_hw, H: int, W: int, unit) -> Tuple[int, int, int, int, int, int, int]:
    """The checked integers (y0, x0, h, w, oh, ow, unit) of a viewport of an H x W picture (``rect`` None: the picture)."""
    H, W, unit = as_int(H, f"{what}: H"), as_int(W, f"{what}: W"), as_int(unit, f"{what}: unit")
    if not (1 <= H <= TL.MAX_SIDE and 1 <= W <= TL.MAX_SIDE):
        raise ValueError(f"{what}: a picture of {H} x {W}: sides are 1 .. {TL.MAX_SIDE}")
    if not 1 <= unit <= MAX_UNIT:
        raise ValueError(f"{what}: unit is 1 .. {MAX_UNIT} (rect is in level-0 pixels divided by it), got {unit}")
    try:
        entries = list(out_hw)
    except TypeError:
        entries = []
    if len(entries) != 2:
        raise ValueError(f"{what}: out_hw is (rows, columns), got {out_hw!r}")
    oh, ow = (as_int(v, f"{what}: out_hw") for v in entries)
    if not (1 <= oh <= MAX_OUT and 1 <= ow <= MAX_OUT):
        raise ValueError(f"{what}: out_hw is (rows, columns) of 1 .. {MAX_OUT} each, got {(oh, ow)}")
    if rect is None:
        return 0, 0, H * unit, W * unit, oh, ow, unit
    try:
        entries = list(rect)
    except TypeError:
        entries = []
    if len(entries) != 4:
        raise ValueError(f"{what}: a rect is (y0, x0, h, w), got {rect!r}")
    y0, x0, h, w = (as_int(v, f"{what}: a rect entry") for v in entries)
    if not (y0 >= 0 and x0 >= 0 and h >= 1 and w >= 1 and y0 + h <= H * unit and x0 + w <= W * unit):
        raise ValueError(f"{what}: the rect (y0 {y0}, x0 {x0}, h {h}, w {w}) / {unit} does not lie inside the {H} x {W} picture")
    return y0, x0, h, w, oh, ow, unit


def _viewport_k(what: str, k, v) -> int:
    """Level k for the viewport ``v`` (:func:`_viewport`'s), refused where it is no level or the scale there is above 16."""
    k = as_int(k, f"{what}: level")
    if not 0 <= k < MAX_LEVELS:
        raise ValueError(f"{what}: level is 0 .. {MAX_LEVELS - 1}, got {k}")
    _, _, h, w, oh, ow, unit = v
    if h > MAX_SCALE * (oh * unit << k) or w > MAX_SCALE * (ow * unit << k):
        need = k
        while h > MAX_SCALE * (oh * unit << need) or w > MAX_SCALE * (ow * unit << need):
            need += 1
        raise ValueError(f"{what}: the rect (h {h}, w {w}) / {unit} into {oh} x {ow} at level {k} has a scale of "
                         f"{h / (oh * unit << k):.4g} x {w / (ow * unit << k):.4g}: above {MAX_SCALE}; level {need}, of a pyramid of "
                         f"{need + 1} levels, brings it to {MAX_SCALE} or below")
    return k


def _axis(origin: int, extent: int, out: int, k: int, unit: int) -> Tuple[int, int, int, int]:
    """(D, n of output coordinate 0, the step of n, T) along one axis (module docstring)."""
    half = out * unit << k
    return 2 * half, 2 * out * origin + extent - half, 2 * extent, max(2 * half, 2 * extent)


def _level_star(v, n_levels: int) -> int:
    _, _, h, w, oh, ow, unit = v
    best = 0
    for k in range(n_levels):
        if (oh * unit << k) <= h and (ow * unit << k) <= w:
            best = k
    return best


def viewport_level(rect, out_hw, H: int, W: int, n_levels: int, unit: int = 1) -> int:
    """``k*``: the level of an ``n_levels`` pyramid of an H x W picture to resample the viewport ``rect`` / ``unit`` into
    ``out_hw`` from (module docstring): the largest k with ``2^k oh unit <= h`` and ``2^k ow unit <= w``, 0 when there is none.
    ValueError when the scale at ``k*`` is above 16: the viewport is strongly anisotropic or the pyramid has too few levels."""
    what = "viewport_level"
    v = _viewport(what, rect, out_hw, H, W, unit)
    n = as_int(n_levels, f"{what}: n_levels")
    _check_levels(H, W, n, what)
    return _viewport_k(what, _level_star(v, n), v)


def viewport_window(rect, out_hw, k: int, H: int, W: int, unit: int = 1) -> Tuple[int, int, int, int]:
    """The support window (y0, x0, h, w) of level k: what resampling the viewport from level k reads, rows ``clamp(first tap
    of Y = 0)`` .. ``clamp(last tap of Y = oh - 1)`` with the clamp to 0 .. H_k - 1, columns likewise.  Host arithmetic only."""
    what = "viewport_window"
    v = _viewport(what, rect, out_hw, H, W, unit)
    k = _viewport_k(what, k, v)
    y0, x0, h, w, oh, ow, unit = v
    out = []
    for origin, extent, o_n, N in ((y0, h, oh, -(-H // (1 << k))), (x0, w, ow, -(-W // (1 << k)))):
        D, n0, dn, T = _axis(origin, extent, o_n, k, unit)
        cl = lambda i: min(max(i, 0), N - 1)
        out.append((cl((n0 - T) // D + 1), cl((n0 + (o_n - 1) * dn + T - 1) // D)))
    (ya, yb), (xa, xb) = out
    return ya, xa, yb - ya + 1, xb - xa + 1


def viewport_taps(rect, out_hw, k: int, H: int, W: int, unit: int = 1, axis: int = 0) -> List[Tuple[int, Tuple[int, ...]]]:
    """The taps of one axis (0: rows, 1: columns) of the viewport resampled from level k: per output coordinate
    ``(first, weights)``, the taps being ``first``, ``first + 1``, .. with the integer weights ``u_i`` (module docstring); the
    fp32 weight is ``float(u_i) / float(sum(weights))`` and the source index ``clamp(i, 0, N_k - 1)``.  For tests and
    references to compare against; the kernel derives the same numbers itself."""
    what = "viewport_taps"
    v = _viewport(what, rect, out_hw, H, W, unit)
    k = _viewport_k(what, k, v)
    if axis not in (0, 1):
        raise ValueError(f"{what}: axis is 0 (rows) or 1 (columns), got {axis!r}")
    D, n0, dn, T = _axis(v[axis], v[2 + axis], v[4 + axis], k, v[6])
    taps = []
    for P in range(v[4 + axis]):
        n = n0 + P * dn
        first, last = (n - T) // D + 1, (n + T - 1) // D
        taps.append((first, tuple(T - abs(D * i - n) for i in range(first, last + 1))))
    return taps


# ----------------------------------------------------------------------------------------------------------- codestream
class _Pyramid:
    """A parsed pyramid header and the byte arithmetic of the body that follows from it."""

    def __init__(self, d, what: str):
        d, _, hlen, end = FRAME.open(d, what)
        H, W, n, zero = _FIXED.unpack_from(d, PREAMBLE_BYTES)
        if zero:
            raise ValueError(f"{what}: the header's reserved field is {zero}, this reader knows 0")
        if hlen != _FIXED.size + 8 * n + 8:
            raise ValueError(f"{what}: the header contradicts itself: {n} levels take {_FIXED.size + 8 * n + 8} bytes, it states {hlen}")
        self.shapes = _check_levels(H, W, n, what)
        self.H, self.W, self.n, self.header_end = H, W, n, end
        sizes = struct.unpack_from(f"<{n + 1}Q", d, PREAMBLE_BYTES + _FIXED.size)
        self.size, self.total = [int(v) for v in sizes[:n]], int(sizes[n])
        if not any(self.size):
            raise ValueError(f"{what}: the header holds no level: every level has 0 bytes")
        if end + sum(self.size) != self.total:
            raise ValueError(f"{what}: the header contradicts itself: its levels add up to {end + sum(self.size)} bytes, it states a "
                             f"total of {self.total}")
        self.off, at = [0] * n, end
        for k in reversed(range(n)):                                            # the body: coarsest first
            self.off[k] = at
            at += self.size[k]
        self.order = [k for k in reversed(range(n)) if self.size[k]]            # the present levels in the order of the body

    def held(self, n: int, k: int) -> int:
        """The bytes of level k that the first ``n`` bytes of the codestream hold."""
        return min(max(n - self.off[k], 0), self.size[k])

    def level(self, k, what: str) -> int:
        k = as_int(k, f"{what}: level")
        if not 0 <= k < self.n:
            raise ValueError(f"{what}: level is 0 .. {self.n - 1}, got {k}")
        return k


def _parse(data, what: str):
    """(view, parsed header) of a pyramid codestream, or a prefix of one, that holds its whole header."""
    d = view(data, what)
    p = _Pyramid(d, what)
    check_total(len(d), p.total, what)
    return d, p


def _facts(g: dict, meta: Optional[dict]) -> dict:
    """What the levels of one pyramid are checked on: a level's geometry, total, allocation and stages (``g``:
    ``tiled.layout``'s dict or ``tiled.PictureFeed.facts``), and, once a tile head is held, what its tiles carry."""
    f = {key: g[key] for key in ("H", "W", "th", "tw", "V", "total", "allocation", "stages")}
    for key in ("marks", "lanes", "base_lanes", "ns"):
        f[key] = None if meta is None else meta[key]
    return f


def _check_facts(p: _Pyramid, facts: dict, what: str):
    """``facts``: level -> :func:`_facts` of every level whose own header is held.  Each level against the pyramid's header,
    then the levels against each other: one overlap, one tile size, one allocation and stage count, and tiles that carry
    the same marks, lanes and base_lanes."""
    for k, f in facts.items():
        if (f["H"], f["W"]) != p.shapes[k]:
            raise ValueError(f"{what}: level {k} holds a picture of {f['H']} x {f['W']}; level {k} of a {p.H} x {p.W} picture is "
                             f"{p.shapes[k][0]} x {p.shapes[k][1]}")
        if f["total"] != p.size[k]:
            raise ValueError(f"{what}: the header contradicts level {k}: it states {p.size[k]} bytes, the level's own header a total "
                             f"of {f['total']}")
    ks = sorted(facts)
    if len(ks) < 2:
        return
    for k in ks[1:]:
        a, b = facts[ks[0]], facts[k]
        for key in _ALIKE:
            if a[key] is not None and b[key] is not None and not same(a[key], b[key]):
                name = {"V": "overlap", "stages": "stages (scheduled or not)"}.get(key, key)
                raise ValueError(f"{what}: level {k} and level {ks[0]} differ in their {name} ({b[key]!r} against {a[key]!r}): all "
                                 "levels of a pyramid are coded with the same tile geometry, marks and lanes")
    c64 = lambda v: -(-v // 64) * 64
    for axis, side in (("th", "H"), ("tw", "W")):                               # th = min(tile, ceil64(H_k)) for ONE tile
        cut = {k: f[axis] for k, f in facts.items() if f[axis] < c64(f[side])}  # levels that state the tile exactly
        least = max(f[axis] for f in facts.values())
        if len(set(cut.values())) > 1 or (cut and least > min(cut.values())):
            raise ValueError(f"{what}: the levels differ in their tile size: tiles of {[facts[k][axis] for k in ks]} along "
                             f"{side} at the levels {ks} are not min(tile, the level's side rounded up to 64) for one tile")


def _level_layout(d, p: _Pyramid, k: int, what: str) -> Optional[dict]:
    """``tiled.layout`` of what ``d`` holds of level k; None while it does not hold that level's own header."""
    held = p.held(len(d), k)
    part = d[p.off[k]:p.off[k] + held]
    try:
        return TL.layout(part) if TL.FRAME.whole(part, what) else None
    except ValueError as e:
        raise ValueError(f"{what}: level {k}: {e}") from e


def _layouts(d, p: _Pyramid, what: str) -> List[Optional[dict]]:
    """Every level's :func:`_level_layout`, checked against the header and against each other."""
    lays = [_level_layout(d, p, k, what) if p.size[k] else None for k in range(p.n)]
    _check_facts(p, {k: _facts(lay, lay if lay["marks"] is not None else None) for k, lay in enumerate(lays) if lay is not None}, what)
    return lays


def _assemble(H: int, W: int, streams: Sequence[Optional[bytes]]) -> bytes:
    """The pyramid codestream of the level codestreams ``streams[k]`` (None or empty: level k is absent)."""
    n = len(streams)
    size = [len(s) if s else 0 for s in streams]
    hlen = _FIXED.size + 8 * n + 8
    header = _FIXED.pack(H, W, n, 0) + struct.pack(f"<{n + 1}Q", *size, PREAMBLE_BYTES + hlen + sum(size))
    out = [FRAME.seal(header)]
    out += [bytes(streams[k]) for k in reversed(range(n)) if size[k]]
    return b"".join(out)


def pack(H: int, W: int, level_streams) -> bytes:
    """The pyramid codestream of an H x W picture from its whole level codestreams (``tiled.encode`` of every level's
    picture), ``level_streams[k]`` for level k, None for an absent level.  Pure framing on the host; ValueError for what
    :func:`layout` would refuse."""
    try:
        streams = [None if s is None else bytes(view(s, "pack")) for s in level_streams]
    except TypeError as e:
        raise ValueError("pack: level_streams is a sequence of picture codestreams") from e
    _check_levels(as_int(H, "pack: H"), as_int(W, "pack: W"), len(streams), "pack")
    if not any(streams):
        raise ValueError("pack: no level: every entry is None")
    data = _assemble(H, W, streams)
    d, p = _parse(data, "pack")
    for k, lay in enumerate(_layouts(d, p, "pack")):
        if streams[k] and lay is None:
            raise ValueError(f"pack: level {k}: {len(streams[k])} bytes do not hold a picture header")
    return data


def need_bytes(data) -> int:
    """The smallest length from which a whole picture decodes at some resolution, as far as ``data`` (any prefix) tells:
    the preamble's size while that is incomplete, the header's end while the header is, then the header plus
    ``tiled.need_bytes`` of the coarsest present level."""
    d = view(data, "need_bytes")
    end = FRAME.need_header(d, "need_bytes")
    if len(d) < end:
        return end
    d, p = _parse(d, "need_bytes")
    k = p.order[0]
    try:
        return end + TL.need_bytes(d[end:end + p.held(len(d), k)])
    except ValueError as e:
        raise ValueError(f"need_bytes: level {k}: {e}") from e


def layout(data) -> dict:
    """Where a pyramid codestream may be cut, from its header (``data``: any prefix that holds it): ``H``, ``W``,
    ``n_levels``, ``header_end``, ``need_bytes``, ``total``, ``ready_levels`` and ``levels``: per level k a dict of ``level``,
    ``shape`` = (H_k, W_k), ``present``, ``offset`` and ``length`` of its codestream in the whole pyramid, ``held`` (the bytes
    of it that ``data`` holds), ``ready`` (it holds the level's own ``tiled.need_bytes``: the level decodes) and ``layout``:
    ``tiled.layout`` of what is held, None while the level's own header is not.  Every held level header is checked against
    this header and against the other levels."""
    d, p = _parse(data, "layout")
    lays = _layouts(d, p, "layout")
    levels = []
    for k in range(p.n):
        held = p.held(len(d), k)
        levels.append({"level": k, "shape": p.shapes[k], "present": p.size[k] > 0, "offset": p.off[k], "length": p.size[k], "held": held,
                       "ready": lays[k] is not None and held >= lays[k]["need_bytes"], "layout": lays[k]})
    first = levels[p.order[0]]
    need = p.header_end + (TL.need_bytes(d[first["offset"]:first["offset"] + first["held"]]))
    return {"H": p.H, "W": p.W, "n_levels": p.n, "header_end": p.header_end, "need_bytes": need, "total": p.total,
            "ready_levels": [lv["level"] for lv in levels if lv["ready"]], "levels": levels}


def level_stream(data, k: int) -> bytes:
    """Level k's picture codestream as far as ``data`` (a pyramid codestream or any prefix that holds the header) holds it;
    it may end anywhere.  ValueError for an absent level."""
    d, p = _parse(data, "level_stream")
    k = p.level(k, "level_stream")
    if not p.size[k]:
        raise ValueError(f"level_stream: level {k} is absent from this codestream; it holds the levels {sorted(p.order)}")
    return bytes(d[p.off[k]:p.off[k] + p.held(len(d), k)])


def extract(data, levels: Optional[Sequence[int]] = None, window=None, rounds: Optional[int] = None) -> bytes:
    """A shorter pyramid codestream of the same picture: only the levels ``levels`` (None: those present), of each only
    the tiles that ``window``, given in LEVEL-0 coordinates, needs at that level (``tiled.extract`` with
    :func:`window_at`; None: those present) and only the first ``rounds`` rounds (None: all).  What a server does to send one
    resolution, a crop, a lower quality, without the model.  ``data`` must hold what is kept.  ``extract(data)`` is ``data``;
    an extract of an extract is an extract.  ValueError names a wanted level that ``data`` lacks."""
    d, p = _parse(data, "extract")
    _layouts(d, p, "extract")
    streams: List[Optional[bytes]] = [None] * p.n
    for k, win in _kept(p, levels, window, "extract"):
        part = d[p.off[k]:p.off[k] + p.held(len(d), k)]
        try:
            streams[k] = TL.extract(part, win, rounds)
        except ValueError as e:
            raise ValueError(f"extract: level {k}: {e}") from e
    return _assemble(p.H, p.W, streams)


def _kept(p: _Pyramid, levels, window, what: str) -> List[Tuple[int, Optional[Tuple[int, int, int, int]]]]:
    """[(level, its window or None: the level whole)], finest first, that :func:`extract` of ``levels`` and the level-0
    ``window`` keeps of the pyramid ``p``."""
    if levels is None:
        keep = sorted(p.order)
    else:
        try:
            keep = sorted({p.level(k, what) for k in levels})
        except TypeError as e:
            raise ValueError(f"{what}: levels is a sequence of levels, got {levels!r}") from e
        if not keep:
            raise ValueError(f"{what}: levels is empty: a pyramid holds at least one level")
    if window is not None:
        window = TL._window({"H": p.H, "W": p.W}, window, what)
    for k in keep:
        if not p.size[k]:
            raise ValueError(f"{what}: level {k} is absent from this codestream; it holds the levels {sorted(p.order)}")
    return [(k, None if window is None else window_at(window, k, p.H, p.W)) for k in keep]


def _viewport_cuts(p: _Pyramid, rect, out_hw, unit, thumbnail, what: str) -> List[Tuple[List[int], Optional[Tuple[int, int, int, int]]]]:
    """What :func:`extract_viewport` keeps of the pyramid ``p``: one or two (levels, level-0 window or None) for
    :func:`extract`, level ``k*`` first."""
    try:
        k = viewport_level(rect, out_hw, p.H, p.W, p.n, unit)
        ya, xa, h, w = viewport_window(rect, out_hw, k, p.H, p.W, unit)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from e
    y0, x0 = ya << k, xa << k
    window = (y0, x0, min(p.H, (ya + h) << k) - y0, min(p.W, (xa + w) << k) - x0)
    if not isinstance(thumbnail, bool):
        raise ValueError(f"{what}: thumbnail is True or False, got {thumbnail!r}")
    if not thumbnail or p.order[0] == k:                                        # k* is the coarsest level: the whole of it covers both
        return [([k], None if thumbnail else window)]
    return [([k], window), ([p.order[0]], None)]


def extract_viewport(data, rect, out_hw, unit: int = 1, rounds: Optional[int] = None, thumbnail: bool = True) -> bytes:
    """What a server sends for one viewport, without the model: of the pyramid codestream ``data``, level
    ``k*`` = :func:`viewport_level` cut to the level-0 window that covers its support window (:func:`viewport_window` times
    ``2^k*``, clipped to the picture) and, with ``thumbnail``, the coarsest present level whole, both with the first ``rounds``
    rounds (None: all), by :func:`extract`.  ``PyramidDecoder(model, it).viewport(rect, out_hw, unit, fill=thumbnail)`` equals
    the viewport of ``data`` bit for bit at the same mark.  ValueError when ``data`` lacks level ``k*``."""
    d, p = _parse(data, "extract_viewport")
    cuts = _viewport_cuts(p, rect, out_hw, unit, thumbnail, "extract_viewport")
    if len(cuts) == 1:
        return extract(d, cuts[0][0], cuts[0][1], rounds)
    streams: List[Optional[bytes]] = [None] * p.n
    for levels, window in cuts:
        streams[levels[0]] = level_stream(extract(d, levels, window, rounds), levels[0])
    return _assemble(p.H, p.W, streams)


# ---------------------------------------------------------------------------------------------------- encoder and decoder
def encode(model, image, levels: Optional[int] = None, tile: int = 256, overlap: int = 32, **tiled_kwargs) -> bytes:
    """The pyramid codestream of ``image``, fp32 [3, H, W] or [1, 3, H, W] on the device.  ``levels`` = None: levels until a
    level fits one tile (:func:`default_levels`); an explicit count is 1 .. 16 and is refused when a level would repeat a
    1 x 1 picture.  The level pictures are made on the device, one vam_picture_halve launch each (``ops.picture_halve``), and
    every level goes through ``tiled.encode`` UNCHANGED with ``tile``, ``overlap`` and ``tiled_kwargs`` (``marks``, ``coder``,
    ``lanes``, ``base_lanes``, ``group``, ``allocation``): ``level_stream(data, k)`` is ``tiled.encode`` of level k's picture byte
    for byte, level 0's is ``tiled.encode(model, image, ...)``.  ``schedule`` = S, fp32 [L, H, W], is reduced
    alongside with ``ops.picture_halve(mode="max")``, which keeps it finite, >= 0, never decreasing by stage and adds no
    value: level k is coded with its reduced schedule."""
    import torch
    from . import ops
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() not in (3, 4) \
            or tuple(image.shape[:-2]) not in ((3,), (1, 3)):
        raise ValueError("pyramid.encode: image is an fp32 tensor [3, H, W] or [1, 3, H, W], got "
                         f"{tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__}")
    H, W = (int(v) for v in image.shape[-2:])
    T = TL.grid(H, W, tile, overlap)["tile"]
    n = default_levels(H, W, T) if levels is None else as_int(levels, "pyramid.encode: levels")
    shapes = _check_levels(H, W, n, "pyramid.encode")
    schedule = tiled_kwargs.pop("schedule", None)
    pic = image.detach().reshape(3, H, W).contiguous()
    streams = []
    with torch.no_grad():
        for k in range(n):
            if k:                                                               # level 0 went through tiled.encode's own checks
                pic = ops.picture_halve(pic)
                schedule = None if schedule is None else ops.picture_halve(schedule, "max")
                assert tuple(pic.shape[1:]) == shapes[k]
            try:
                streams.append(TL.encode(model, pic, tile=tile, overlap=overlap, schedule=schedule, **tiled_kwargs))
            except ValueError as e:
                if not k:
                    raise
                raise ValueError(f"pyramid.encode: level {k} ({shapes[k][0]} x {shapes[k][1]}): {e}") from e
            if k == 0 and schedule is not None:
                schedule = schedule.detach().contiguous()
    return _assemble(H, W, streams)


def _not_ready(what: str, k: int, present: bool, ready: List[int]) -> ValueError:
    why = "its bytes end before the heads of its tiles do" if present else "it is absent from this codestream"
    return ValueError(f"{what}: level {k} does not decode: {why}; the ready levels are {ready}")


def _fill(what: str, shapes, usable: List[int], composer, window, k: int, q, mark, stage, dtype, missing: int):
    """``F_k(window)`` of the module docstring and its chain, finest to coarsest: [(level, the tiles composed sharp, those that
    ran the network)].  ``usable``: the usable levels, ascending; ``composer(j)``: level j's ``tiled.PictureDecoder`` or
    ``tiled.PictureStream``; ``missing``: the bytes still missing before the first level decodes.  A level whose window is
    all available is not filled: it is the blend, and the chain ends there.  Intermediate pictures are fp32 [3, h, w]."""
    import torch
    from . import ops
    if q is not None:
        raise ValueError(f"{what}: q does not go with fill=True: whether a tile's bytes reach a quality is only known by decoding it; "
                         "give mark, stage or neither")
    window = TL._window({"H": shapes[k][0], "W": shapes[k][1]}, window, what)
    chain: List = []

    def level(j: int, win, out_dtype):
        above = [i for i in usable if i > j]
        obj = composer(j) if j in usable else None
        if obj is None and not above:
            raise ValueError(f"{what}: nothing to fill level {j} from: no level from {j} up holds its picture header"
                             + (f"; {missing} bytes are missing before the coarsest level decodes" if missing else ""))
        at = len(chain)
        chain.append(None)
        try:
            if obj is not None and (not above or len(obj.available(win, mark, stage)) == len(TL.tiles_for(obj.grid, win))):
                out = obj.compose(win, None, None, 0, mark=mark, stage=stage, dtype=out_dtype)       # nothing to fill: the blend
            else:
                d = above[0] - j
                source = source_window(win, d, *shapes[above[0]])
                below = level(above[0], source, None)
                if obj is not None:
                    out = obj.compose(win, below, source, d, mark=mark, stage=stage, dtype=out_dtype)
                else:                                       # no tiles: the pure upsample, one launch
                    out = torch.empty((3,) + win[2:], dtype=torch.float32, device=below.device) if out_dtype in (None, torch.float32) \
                        else torch.empty(win[2:] + (3,), dtype=torch.uint8, device=below.device)
                    ops.tile_compose(None, None, None, None, shapes[j][0], shapes[j][1], 0, win, below, source, d, out, None)
        except ValueError as e:
            raise (e if str(e).startswith(f"{what}: ") else ValueError(f"{what}: level {j}: {e}")) from e
        chain[at] = (j, [], []) if obj is None else (j, list(obj.last_tiles), list(obj.last_decoded))
        return out

    if dtype not in (None, torch.float32, torch.uint8):
        raise ValueError(f"{what}: dtype is torch.float32 or torch.uint8, got {dtype}")
    return level(k, window, dtype), chain


def _viewport_plan(what: str, rect, out_hw, unit, level, dtype, H: int, W: int, n_levels: int):
    """(rect, out_hw, unit, k, the support window at k) of a viewport call, checked before anything is decoded."""
    import torch
    v = _viewport(what, rect, out_hw, H, W, unit)
    if dtype not in (None, torch.float32, torch.uint8):
        raise ValueError(f"{what}: dtype is torch.float32 or torch.uint8, got {dtype}")
    if level is None:
        k = _viewport_k(what, _level_star(v, n_levels), v)
    else:
        k = as_int(level, f"{what}: level")
        if not 0 <= k < n_levels:
            raise ValueError(f"{what}: level is 0 .. {n_levels - 1}, got {k}")
        k = _viewport_k(what, k, v)
    return v[:4], v[4:6], v[6], k, viewport_window(v[:4], v[4:6], k, H, W, v[6])


def _resample(src, window, level_hw, k: int, rect, unit: int, out_hw, dtype):
    """One vam_picture_resample launch on the fp32 support window ``src`` of level k."""
    from . import ops
    return ops.picture_resample(src.detach().contiguous(), window, level_hw, k, rect, unit, out_hw, dtype=dtype)


class PyramidDecoder:
    """Decodes a pyramid codestream by level and window.  ``data``: any prefix of at least :func:`need_bytes`, or an
    :func:`extract`.  ``shape``: the true (H, W) of level 0; ``levels``: n_levels; ``shapes``: [(H_k, W_k)]; ``ready``: per level,
    whether ``data`` holds enough of it to decode; ``usable``: whether it holds the level's own picture header, so that
    ``decode(fill=True)`` takes the level's available tiles.  A level's ``tiled.PictureDecoder`` is made when it is first
    decoded.  ``last_chain``: what the last decode composed, finest level first: [(level, the tiles composed sharp, the tiles
    that ran the network)]."""

    def __init__(self, model, data, coder: Optional[str] = None, group: Optional[int] = None):
        EB._check_model(model)
        lay = layout(data)
        self.m, self.coder, self.group, self._d = model, coder, group, bytes(view(data, "PyramidDecoder"))
        self.shape, self.levels, self.shapes = (lay["H"], lay["W"]), lay["n_levels"], [lv["shape"] for lv in lay["levels"]]
        self.ready = [lv["ready"] for lv in lay["levels"]]
        self._present = [lv["present"] for lv in lay["levels"]]
        self.usable = [lv["layout"] is not None for lv in lay["levels"]]
        if not any(self.ready):
            raise ValueError(f"PyramidDecoder: {len(self._d)} bytes end before any level decodes: {lay['need_bytes']} bytes are "
                             "needed for the coarsest level's tile heads")
        self._dec = {}
        self._partial = {}                                  # the decoders of usable levels that are not ready (fill=True)
        self.last_tiles: List[Tuple[int, int]] = []
        self.last_chain: List[Tuple[int, List[Tuple[int, int]], List[Tuple[int, int]]]] = []

    def decoder(self, level: int = 0) -> "TL.PictureDecoder":
        """The ``tiled.PictureDecoder`` of ``level`` on ``level_stream(data, level)``."""
        k = as_int(level, "PyramidDecoder.decode: level")
        if not 0 <= k < self.levels:
            raise ValueError(f"PyramidDecoder.decode: level is 0 .. {self.levels - 1}, got {k}")
        if not self.ready[k]:
            raise _not_ready("PyramidDecoder.decode", k, self._present[k], [j for j in range(self.levels) if self.ready[j]])
        if k not in self._dec:
            self._dec[k] = TL.PictureDecoder(self.m, level_stream(self._d, k), coder=self.coder, group=self.group)
        return self._dec[k]

    def _composer(self, k: int) -> "TL.PictureDecoder":
        if self.ready[k]:
            return self.decoder(k)
        if k not in self._partial:
            self._partial[k] = TL.PictureDecoder(self.m, level_stream(self._d, k), coder=self.coder, group=self.group, partial=True)
        return self._partial[k]

    def decode(self, window=None, level: int = 0, q: Optional[float] = None, mark: Optional[int] = None, stage: Optional[int] = None,
               dtype=None, fill: bool = False):
        """``tiled.PictureDecoder(model, level_stream(data, level)).decode(window, q, mark, stage, dtype)``, bit for bit and
        error for error: ``window`` is in the coordinates of ``level`` (:func:`window_at` maps a level-0 window).  A level that
        is absent or not ready is a ValueError that names it and the ready levels.

        ``fill=True`` (with ``mark``, ``stage`` or neither, never ``q``): always the whole window at
        ``level``, for any level 0 .. n - 1: sharp where the level's tiles are available, elsewhere the upsample of the same
        view of the next coarser usable level, down the chain (module docstring).  Once every tile of the window is
        available it is the call without ``fill``, bit for bit.  ``last_chain`` records what was composed."""
        if not fill:
            dec = self.decoder(level)
            out = dec.decode(window, q=q, mark=mark, stage=stage, dtype=dtype)
            self.last_tiles, self.last_chain = dec.last_tiles, [(int(level), list(dec.last_tiles), list(dec.last_tiles))]
            return out
        what = "PyramidDecoder.decode"
        k = as_int(level, f"{what}: level")
        if not 0 <= k < self.levels:
            raise ValueError(f"{what}: level is 0 .. {self.levels - 1}, got {k}")
        out, chain = _fill(what, self.shapes, [j for j in range(self.levels) if self.usable[j]], self._composer, window, k, q, mark, stage,
                           dtype, 0)
        self.last_tiles, self.last_chain = chain[0][1], chain
        return out

    def viewport(self, rect, out_hw, unit: int = 1, level: Optional[int] = None, q: Optional[float] = None, mark: Optional[int] = None,
                 stage: Optional[int] = None, dtype=None, fill: bool = False):
        """The viewport ``rect`` = (y0, x0, h, w) / ``unit`` of the picture (None: the picture) in ``out_hw`` = (oh, ow) pixels, at
        any zoom and pan: fp32 [3, oh, ow] or, with ``dtype=torch.uint8``, uint8 [oh, ow, 3].  ``level`` None
        takes :func:`viewport_level`; an explicit level is allowed while the scale there stays at most 16.  The level's support
        window (:func:`viewport_window`) is ``decode(window, level, q, mark, stage, fill=fill)`` in fp32, with its errors, and
        one vam_picture_resample launch writes the output: the result is ``tests/resample_ref.py`` on that decode, bit for bit."""
        what = "PyramidDecoder.viewport"
        rect, out_hw, unit, k, win = _viewport_plan(what, rect, out_hw, unit, level, dtype, self.shape[0], self.shape[1], self.levels)
        src = self.decode(win, k, q=q, mark=mark, stage=stage, dtype=None, fill=fill)
        return _resample(src, win, self.shapes[k], k, rect, unit, out_hw, dtype)


# --------------------------------------------------------------------------------------------------------- the receiver
class PyramidFeed:
    """The byte bookkeeping of a pyramid's receiver: a pyramid codestream, whole or an :func:`extract`, arriving in chunks
    that may end anywhere, the header included.  Once the header is complete it owns one receiver per present level
    (``receivers[k]``, None for an absent level; by default a ``tiled.PictureFeed``: host arithmetic only) and routes the
    bytes to them in the order of the body.  ``make(k)`` builds level k's receiver: a ``tiled.PictureFeed`` or anything with
    its ``feed``, ``mark`` / ``rewind``, ``ready``, ``need()``, ``data``, ``facts`` and ``meta``, as ``tiled.PictureStream``.

    ``ready``: a level decodes; ``ready_levels``; ``need()``: the bytes still missing before the first level does;
    ``shape``, ``levels``, ``shapes`` once the header is complete; ``fed_levels``: the levels that the last feed gave bytes to;
    ``data``: everything fed so far."""

    def __init__(self, what: str = "PyramidFeed", make=None):
        self._what = what
        self._make = make if make is not None else (lambda k: TL.PictureFeed(f"{what} level {k}"))
        self._head = bytearray()                            # the bytes up to the header's end
        self._p: Optional[_Pyramid] = None
        self._n = 0
        self.receivers: List = []
        self.fed_levels: List[int] = []

    def __len__(self) -> int:
        return self._n

    @property
    def data(self) -> bytes:
        return bytes(self._head) + b"".join(self.receivers[k].data for k in (self._p.order if self._p else []))

    def _header(self, name: str) -> _Pyramid:
        if self._p is None:
            raise ValueError(f"{self._what}.{name}: the header is not complete yet: {self.need()} bytes are missing")
        return self._p

    shape = property(lambda self: (self._header("shape").H, self._header("shape").W))
    levels = property(lambda self: self._header("levels").n)
    shapes = property(lambda self: list(self._header("shapes").shapes))

    @property
    def ready_levels(self) -> List[int]:
        return [k for k, r in enumerate(self.receivers) if r is not None and r.ready]

    @property
    def ready(self) -> bool:
        return bool(self.ready_levels)

    def need(self) -> int:
        if self._p is not None:
            return 0 if self.ready else self.receivers[self._p.order[0]].need()
        return FRAME.need_header(self._head, self._what) - len(self._head)

    def _facts(self) -> dict:
        out = {}
        for k, r in enumerate(self.receivers):
            g = None if r is None else r.facts
            if g is not None:
                out[k] = _facts(g, r.meta)
        return out

    def feed(self, chunk) -> List[int]:
        """``chunk``: the bytes that follow what was fed before, ``b""`` allowed.  Returns ``ready_levels``.  The feed is
        checked as a whole before anything is kept: a damaged or contradicting header, a level that contradicts the header or
        the other levels, what ``tiled.PictureFeed.feed`` refuses of a level's own bytes, bytes beyond the header's total
        and a non-bytes argument are ValueErrors that leave the receiver, and every level's, as it was."""
        what = f"{self._what}.feed"
        chunk = bytes(chunk_view(chunk, what))
        before = (len(self._head), self._p, self._n, self.receivers, self.fed_levels,
                  [None if r is None else r.mark() for r in self.receivers])
        try:
            self._route(chunk, what)
        except ValueError:
            n_head, self._p, self._n, self.receivers, self.fed_levels, marks = before
            del self._head[n_head:]
            for r, m in zip(self.receivers, marks):
                if r is not None:
                    r.rewind(m)
            raise
        return self.ready_levels

    def _route(self, chunk: bytes, what: str):
        at, fed = 0, []
        if self._p is None:
            end = FRAME.header_end(self._head + chunk[:PREAMBLE_BYTES], what)  # refuses a wrong preamble as soon as it is whole
            take = len(chunk) if end is None else min(len(chunk), end - len(self._head))
            self._head += chunk[:take]
            at = take
            if end is None or len(self._head) < end:
                self._n += take
                return
            p = _Pyramid(bytes(self._head), what)                               # a copy: a view of it would pin the buffer's size
            self._p, self.receivers = p, [self._make(k) if p.size[k] else None for k in range(p.n)]
        p = self._p
        n = self._n + len(chunk)
        check_total(n, p.total, what)
        pos = self._n + at                                                      # where chunk[at:] begins in the codestream
        for k in p.order:
            a, b = max(pos, p.off[k]), min(n, p.off[k] + p.size[k])
            if a < b:
                try:
                    self.receivers[k].feed(chunk[at + a - pos:at + b - pos])
                except ValueError as e:
                    raise ValueError(f"{what}: level {k}: {e}") from e
                fed.append(k)
        if fed:
            _check_facts(p, self._facts(), what)
        self._n, self.fed_levels = n, fed


class PyramidStream:
    """A receiver of one pyramid codestream: one ``tiled.PictureStream`` per level (``streams[k]``, None
    for an absent level), created when the header is complete, each with its own tile cache of ``cache_tiles`` tiles
    (None: ``PictureStream``'s default for that level's geometry).  :meth:`feed` takes chunks that end anywhere
    (:class:`PyramidFeed`, which it owns as ``feed_state``; ``ready``, ``ready_levels``, ``need()``, ``shape``, ``levels``,
    ``shapes``, ``fed_levels`` and ``data`` are this object's, too).  After any sequence of feeds, ``view(window, level, ...)``
    equals a fresh ``PyramidDecoder(everything fed so far).decode(window, level, ...)`` bit for bit while only the tiles that
    level has not cached run the network.  ``last_tiles`` / ``last_decoded``: those of the level viewed last."""

    def __init__(self, model, coder: Optional[str] = None, group: Optional[int] = None, cache_tiles: Optional[int] = None):
        TL.PictureStream(model, coder=coder, group=group, cache_tiles=cache_tiles)      # its checks of the arguments, now and not at the header
        self.feed_state = PyramidFeed("PyramidStream", lambda k: TL.PictureStream(model, coder=coder, group=group, cache_tiles=cache_tiles))
        self.last_tiles: List[Tuple[int, int]] = []
        self.last_decoded: List[Tuple[int, int]] = []
        self.last_chain: List[Tuple[int, List[Tuple[int, int]], List[Tuple[int, int]]]] = []

    ready = property(lambda self: self.feed_state.ready)
    ready_levels = property(lambda self: self.feed_state.ready_levels)
    shape = property(lambda self: self.feed_state.shape)
    levels = property(lambda self: self.feed_state.levels)
    shapes = property(lambda self: self.feed_state.shapes)
    fed_levels = property(lambda self: self.feed_state.fed_levels)
    data = property(lambda self: self.feed_state.data)
    streams = property(lambda self: list(self.feed_state.receivers))

    def need(self) -> int:
        return self.feed_state.need()

    def feed(self, chunk) -> List[int]:
        """:meth:`PyramidFeed.feed`: host arithmetic only; it touches no GPU and no cache entry."""
        return self.feed_state.feed(chunk)

    def _level(self, what: str, level) -> "TL.PictureStream":
        fs = self.feed_state
        if fs._p is None:
            raise ValueError(f"{what}: nothing to decode yet: the header is not complete, {fs.need()} bytes are missing")
        k = fs._p.level(level, what)
        if k not in fs.ready_levels:
            raise _not_ready(what, k, fs._p.size[k] > 0, fs.ready_levels)
        return fs.receivers[k]

    def view(self, window=None, level: int = 0, q: Optional[float] = None, mark: Optional[int] = None, stage: Optional[int] = None,
             dtype=None, fill: bool = False):
        """``streams[level].view(window, q, mark, stage, dtype)``: the window is in the coordinates of ``level``.  A level that
        is absent or not ready is a ValueError that names it and the ready levels.

        ``fill=True``: a fresh ``PyramidDecoder(everything fed so far).decode(window, level, mark=, stage=,
        dtype=, fill=True)``, bit for bit, from the moment the coarsest level decodes: tiles turn sharp one by one as their
        heads come in, and only the tiles a level has not cached run the network (``last_chain``: finest level first,
        (level, the tiles composed sharp, the tiles that ran the network); ``last_tiles`` / ``last_decoded``: those of
        ``level``).  Before that a ValueError states the bytes still missing."""
        what = "PyramidStream.view"
        if not fill:
            st = self._level(what, level)
            out = st.view(window, q=q, mark=mark, stage=stage, dtype=dtype)
            self.last_tiles, self.last_decoded = st.last_tiles, st.last_decoded
            self.last_chain = [(int(level), list(st.last_tiles), list(st.last_decoded))]
            return out
        fs = self.feed_state
        if fs._p is None:
            raise ValueError(f"{what}: nothing to decode yet: the header is not complete, {fs.need()} bytes are missing")
        k = fs._p.level(level, what)
        usable = [j for j, r in enumerate(fs.receivers) if r is not None and r.facts is not None]
        out, chain = _fill(what, fs._p.shapes, usable, lambda j: fs.receivers[j], window, k, q, mark, stage, dtype, fs.need())
        self.last_tiles, self.last_decoded, self.last_chain = chain[0][1], chain[0][2], chain
        return out

    def viewport(self, rect, out_hw, unit: int = 1, level: Optional[int] = None, q: Optional[float] = None, mark: Optional[int] = None,
                 stage: Optional[int] = None, dtype=None, fill: bool = False):
        """A fresh ``PyramidDecoder(everything fed so far).viewport(rect, out_hw, unit, level, ...)``, bit for bit: the level's
        support window is :meth:`view`'s, through that level's ``tiled.PictureStream`` and its tile cache (``last_tiles``,
        ``last_decoded`` and ``last_chain`` are the view's), then one vam_picture_resample launch.  Over cached tiles a pan step
        is one blend and one resample and runs no network."""
        what = "PyramidStream.viewport"
        fs = self.feed_state
        if fs._p is None:
            raise ValueError(f"{what}: nothing to decode yet: the header is not complete, {fs.need()} bytes are missing")
        rect, out_hw, unit, k, win = _viewport_plan(what, rect, out_hw, unit, level, dtype, fs._p.H, fs._p.W, fs._p.n)
        src = self.view(win, k, q=q, mark=mark, stage=stage, dtype=None, fill=fill)
        return _resample(src, win, fs._p.shapes[k], k, rect, unit, out_hw, dtype)

    def canvas(self, window=None, level: int = 0, dtype=None) -> "TL.Canvas":
        """``streams[level].canvas(window, dtype)``: a persistent output of that level that ``refresh()`` keeps equal to
        :meth:`view` (vam_tile_refresh)."""
        fs = self.feed_state
        if fs._p is None:
            raise ValueError(f"PyramidStream.canvas: the header is not complete yet: {fs.need()} bytes are missing")
        k = fs._p.level(level, "PyramidStream.canvas")
        if fs.receivers[k] is None:
            raise _not_ready("PyramidStream.canvas", k, False, fs.ready_levels)
        return fs.receivers[k].canvas(window, dtype)
