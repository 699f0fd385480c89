"""Tiled picture codestreams: a picture of ANY size as overlapping tiles, each tile an embedded
codestream of its own (embedded.to_bytes, section 9u), all of them in one byte string that is decodable by window.

Geometry, one definition for the host, the kernels of ``csrc/tiles.hip`` and ``tests/tiled_ref.py`` (:func:`grid`): tiles of
``th x tw`` with ``th = min(tile, ceil64(H))``, ``tw = min(tile, ceil64(W))``, an overlap ``V <= min(th, tw) / 2``, strides
``Sy = th - V`` and ``Sx = tw - V``, a grid of ``R = max(1, ceil((H - V) / Sy))`` by ``C`` likewise; tile (r, c) covers rows
``[r Sy, r Sy + th)`` and columns ``[c Sx, c Sx + tw)``, the picture's edge replicated beyond it (vam_tile_extract).  At most
two tiles overlap along an axis.  In the band that tiles r and r + 1 share, row ``(r + 1) Sy + t`` takes
``w_hi[t] = float32((t + 0.5) / V)`` of tile r + 1 and ``w_lo[t] = float32(1) - w_hi[t]`` of tile r (:func:`ramps`); an output
pixel is the sum over its tiles, ascending r and within that ascending c, of ``(wy * wx) * v`` in fp32 (vam_tile_blend):
outside the bands the picture IS the tile's decode, bit for bit.

The codestream: ``framing.PREAMBLE`` with magic ``b"VAMp"``, a little-endian header (u32 H, W; u16 th / 64, tw / 64, V, R, C,
n_rounds; a u32 table [R C][1 + n_rounds]; u64 total) under a CRC-32, then the body: the **heads** of all tiles in raster
order, then round 0 of all tiles, round 1, ...  A tile's head is its own embedded codestream up to its ``base_end``, its round
pieces are the differences of its ``round_end`` and a last piece up to its ``total``: head and pieces concatenated are exactly
``embedded.to_bytes`` of the tile, nothing is re-framed.  A head of 0 bytes marks an absent tile.  From :func:`need_bytes` on
every prefix decodes the whole picture; ``data[:round_end[k]]`` holds every tile exactly at mark k; :func:`extract` cuts a
stream down to a window and a number of rounds on the host alone, and what it returns is again a picture codestream.

:func:`encode` and :class:`PictureDecoder` run the tiles, a group at a time, through ``embedded.encode_batch`` and
``embedded.EmbeddedDecoder`` unchanged: an image codes and decodes bit for bit the same alone or in a batch, so neither the
bytes nor the pixels depend on the grouping.  By default (``allocation="tile"``) quality q keeps a quantile PER TILE: a
tiled picture at q is not the untiled forward at q.

Picture-wide marks: ``encode(..., allocation="picture")`` takes, per mark and slice, ONE sigma threshold
over the pool of all tiles' sigmas (``torch.quantile`` of the pool, bit for bit; ``csrc/pooled_select.hip``) and marks every
tile with the count of its elements at or above it.  Such a stream has a version-2 header: the version-1 fields and table,
then u16 allocation (1), n_marks, ns, reserved (0) and the thresholds float32 [n_marks][ns], then the u64 total, under the same
CRC.  Tile heads stay ordinary embedded headers.  ``PictureDecoder.decode(mark=k)`` decodes every tile at its header's counts
of mark k and, on a version-2 stream, checks them against the thresholds on its own sigma.

Rounds at byte budgets: ``encode(..., allocation="picture", max_bytes=[N_1 < ... < N_L])`` solves the
picture-wide quality of every mark so that ``round_end[k] <= N_k`` (:func:`solve_budgets`, on a cut table of every stream's
bytes for every count); the stream is the version-2 stream of those marks, and :func:`budget_marks` reads them back.

Scheduled pictures: ``encode(..., schedule=S)`` with ``S`` fp32 [L, H, W], L quality maps at PIXEL
resolution that never decrease from stage to stage, codes a region of interest first in every prefix.  A tile's schedule is
``S_tile[k][a][b] = max over y, x in [0, 16) of S[k][min(r Sy + 16 a + y, H - 1)][min(c Sx + 16 b + x, W - 1)]``
(vam_tile_schedule): ``evaluate.latent_quality_map``'s block maximum over vam_tile_extract's replicated edge.  Every tile is a
scheduled embedded codestream of L stages (``embedded.encode_batch(schedule=)``) that carries its own schedule in its head.
Such a stream has a version-3 header: the version-1 fields and table, then u16 kind (1: scheduled), u16 n_stages, u32
reserved (0), then the u64 total, under the same CRC; its rounds are stages: ``data[:round_end[k]]`` and
``extract(data, rounds=k + 1)`` hold every tile exactly at stage k, and ``PictureDecoder.decode(stage=k)`` is the blend of
``forward_quality_map(tile, S_tile[k])``.  Out of scope: a schedule together with ``allocation="picture"`` and reassembling
the picture-level schedule at the receiver.

The receiver: :class:`PictureStream` is fed the bytes as they arrive, in chunks that end anywhere
(:class:`PictureFeed`, the byte bookkeeping, needs neither a model nor a GPU), and keeps decoded tiles in a device pool across
calls: ``view(window, q | mark | stage)`` equals a fresh ``PictureDecoder(everything fed so far).decode(...)`` bit for bit
and runs through the network only the tiles of the window whose own bytes grew since they were decoded, or that were never
decoded at that level.  A :class:`Canvas` is a persistent output that ``refresh()`` re-blends only where such tiles
contribute (vam_tile_refresh).  Out of scope: per-tile entropy resumption (a resumable ``EmbeddedDecoder`` kept per tile
group) and a priority order for stale tiles.

Tiles before all heads have arrived: a tile is AVAILABLE when it is present and the bytes held hold its
head whole (``PictureFeed.tile_ready`` / ``tile_rounds``, ``PictureDecoder(partial=True)``); at ``mark=m`` or ``stage=m`` it
must hold the rounds 0 .. m whole as well.  ``compose(window, below, below_window, shift)`` of :class:`PictureDecoder` and
:class:`PictureStream` decodes the available tiles of the window only and, with one vam_tile_compose launch, gives the
blend where all tiles of a pixel are available and elsewhere the upsample of ``below``, a window of the same picture 2^shift
times coarser (``vampic.pyramid`` chains the levels).
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import embedded as EB
from .framing import MAX_HEADER, PREAMBLE as _PREAMBLE, PREAMBLE_BYTES, Frame, as_int as _int, check_total, chunk_view, same, view

MAGIC = b"VAMp"
VERSION = 1                                # allocation="tile": every tile marks its own quantiles
VERSION_POOLED = 2                         # allocation="picture" (DESIGN section 9w): the header also carries the picture's thresholds
VERSION_SCHEDULED = 3                      # schedule=S: every tile is scheduled, the rounds are stages
ALLOCATIONS = ("tile", "picture")
_ALLOC_PICTURE = 1                         # the one allocation value a version-2 header may state
_FIXED = struct.Struct("<IIHHHHHH")        # H, W, th / 64, tw / 64, V, R, C, n_rounds
_POOLED = struct.Struct("<HHHH")           # version 2, after the table: allocation, n_marks, ns, reserved (0); then f32 [n_marks][ns]
_SCHED = struct.Struct("<HHI")             # version 3, after the table: kind (1: scheduled), n_stages, reserved (0)
_KIND_SCHEDULED = 1                        # the one kind a version-3 header may state
FRAME = Frame(MAGIC, "a picture codestream", "picture codestream", (VERSION, VERSION_POOLED, VERSION_SCHEDULED),
              range(_FIXED.size + 12, MAX_HEADER + 1), f"a header takes {_FIXED.size + 12} .. {MAX_HEADER}")
_header_end = FRAME.header_end             # None while the preamble is incomplete, else where the header ends (tests read it and _PREAMBLE)
MAX_SIDE = 1 << 24                         # csrc/tiles.hip: the largest picture side
MAX_GROUP = 32
MAX_POOL = 16000000                        # csrc/pooled_select.hip: torch.quantile's largest input


# ------------------------------------------------------------------------------------------------------------- geometry
def _geometry(H: int, W: int, th: int, tw: int, V: int, what: str) -> dict:
    """The grid of th x tw tiles with overlap V over a picture of H x W."""
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: a picture of {H} x {W}: sides are 1 .. {MAX_SIDE}")
    if not 0 <= V <= min(th, tw) // 2:
        raise ValueError(f"{what}: overlap {V}: tiles of {th} x {tw} take 0 <= overlap <= {min(th, tw) // 2} (half a tile: at most two "
                         "tiles overlap along an axis)")
    Sy, Sx = th - V, tw - V
    R, C = max(1, -(-(H - V) // Sy)), max(1, -(-(W - V) // Sx))
    if R > 0xFFFF or C > 0xFFFF:
        raise ValueError(f"{what}: a grid of {R} x {C} tiles; the format carries up to 65535 along an axis, use larger tiles")
    return {"H": H, "W": W, "th": th, "tw": tw, "V": V, "Sy": Sy, "Sx": Sx, "R": R, "C": C}


def grid(H: int, W: int, tile: int = 256, overlap: int = 32) -> dict:
    """The geometry of a picture of H x W at ``tile`` (a multiple of 64 in 64 .. 1024) and ``overlap``: a dict of H, W, th,
    tw, V, Sy, Sx, R, C (module docstring) and ``tile``.  ValueError names what is out of range."""
    H, W, T, V = _int(H, "grid: H"), _int(W, "grid: W"), _int(tile, "grid: tile"), _int(overlap, "grid: overlap")
    if T % 64 or not 64 <= T <= 1024:
        raise ValueError(f"grid: tile is a multiple of 64 in 64 .. 1024, got {T}")
    c64 = lambda n: -(-n // 64) * 64
    g = _geometry(H, W, min(T, c64(max(H, 1))), min(T, c64(max(W, 1))), V, "grid")
    g["tile"] = T
    return g


def ramps(V: int) -> Tuple[np.ndarray, np.ndarray]:
    """(w_lo, w_hi) float32 [V]: ``w_hi[t] = float32((t + 0.5) / V)`` from float64, rounded once, ``w_lo = float32(1) - w_hi``
    in float32.  The kernel reads these tables and divides nothing."""
    w_hi = ((np.arange(V, dtype=np.float64) + 0.5) / max(V, 1)).astype(np.float32)
    return np.float32(1) - w_hi, w_hi


def _window(g: dict, window, what: str) -> Tuple[int, int, int, int]:
    if window is None:
        return 0, 0, g["H"], g["W"]
    try:
        y0, x0, h, w = (_int(v, f"{what}: a window entry") for v in window)
    except TypeError as e:
        raise ValueError(f"{what}: a window is (y0, x0, h, w), got {window!r}") from e
    if not (y0 >= 0 and x0 >= 0 and h >= 1 and w >= 1 and y0 + h <= g["H"] and x0 + w <= g["W"]):
        raise ValueError(f"{what}: the window (y0 {y0}, x0 {x0}, h {h}, w {w}) does not lie inside the {g['H']} x {g['W']} picture")
    return y0, x0, h, w


def tiles_for(layout: dict, window=None) -> List[Tuple[int, int]]:
    """The (r, c), in raster order, of the tiles whose extent meets ``window`` = (y0, x0, h, w) (None: the picture): exactly
    the tiles a blend of that window reads, band neighbours included.  ``layout``: :func:`layout`'s or :func:`grid`'s dict."""
    g = layout
    y0, x0, h, w = _window(g, window, "tiles_for")
    rows = [r for r in range(g["R"]) if r * g["Sy"] < y0 + h and r * g["Sy"] + g["th"] > y0]
    cols = [c for c in range(g["C"]) if c * g["Sx"] < x0 + w and c * g["Sx"] + g["tw"] > x0]
    return [(r, c) for r in rows for c in cols]


# ----------------------------------------------------------------------------------------------------------- codestream
class _Picture:
    """A parsed picture header and the byte arithmetic of the body that follows from it."""

    def __init__(self, d, what: str):
        d, version, hlen, end = FRAME.open(d, what)
        H, W, th, tw, V, R, C, nr = _FIXED.unpack_from(d, PREAMBLE_BYTES)
        if not (1 <= th <= 16 and 1 <= tw <= 16):
            raise ValueError(f"{what}: the header contradicts itself: tiles of {64 * th} x {64 * tw}, sides are 64 .. 1024")
        g = _geometry(H, W, 64 * th, 64 * tw, V, what)
        if (g["R"], g["C"]) != (R, C) or any(grid(H, W, 64 * max(th, tw), V)[k] != g[k] for k in ("th", "tw")):
            raise ValueError(f"{what}: the header contradicts itself: {H} x {W} in tiles of {64 * th} x {64 * tw} with overlap {V} "
                             f"is no grid of {R} x {C}")
        table_end = _FIXED.size + 4 * R * C * (1 + nr)
        self.version, self.thresholds, self.stages = version, None, 0
        if version == VERSION_SCHEDULED:
            v3 = f"{what}: picture codestream version {VERSION_SCHEDULED}: the header contradicts itself"
            if hlen != table_end + _SCHED.size + 8:
                raise ValueError(f"{v3}: {R} x {C} tiles of {nr} rounds and the schedule fields take "
                                 f"{table_end + _SCHED.size + 8} bytes, it states {hlen}")
            kind, n_st, zero = _SCHED.unpack_from(d, PREAMBLE_BYTES + table_end)
            if kind != _KIND_SCHEDULED or zero:
                raise ValueError(f"{v3}: kind {kind} (reserved field {zero}); this reader knows kind {_KIND_SCHEDULED}, scheduled "
                                 "tiles whose rounds are stages")
            if n_st < 1 or nr > n_st + 1:               # a whole stream has one round more than stages: what follows the last stage
                raise ValueError(f"{v3}: {n_st} stages and {nr} rounds: a picture of L >= 1 stages holds at most L + 1 rounds")
            self.stages = n_st
        elif version == VERSION_POOLED:
            # every refusal of the extension names the version: a version-1 header read as version 2 says so
            v2 = f"{what}: picture codestream version {VERSION_POOLED}: the header contradicts itself"
            if hlen < table_end + _POOLED.size + 8:
                raise ValueError(f"{v2}: {R} x {C} tiles of {nr} rounds and the allocation fields take at least "
                                 f"{table_end + _POOLED.size + 8} bytes, it states {hlen}")
            alloc, nm, ns, zero = _POOLED.unpack_from(d, PREAMBLE_BYTES + table_end)
            if hlen != table_end + _POOLED.size + 4 * nm * ns + 8:
                raise ValueError(f"{v2}: {R} x {C} tiles of {nr} rounds and thresholds of {nm} marks x {ns} slices take "
                                 f"{table_end + _POOLED.size + 4 * nm * ns + 8} bytes, it states {hlen}")
            if alloc != _ALLOC_PICTURE or zero:
                raise ValueError(f"{v2}: allocation {alloc} (reserved field {zero}); this reader knows allocation {_ALLOC_PICTURE}, "
                                 "picture-wide marks")
            if nm < 1 or ns < 1:
                raise ValueError(f"{v2}: thresholds of {nm} marks x {ns} slices")
            thr = np.frombuffer(d, dtype="<f4", count=nm * ns, offset=PREAMBLE_BYTES + table_end + _POOLED.size) \
                .astype(np.float32).reshape(nm, ns)
            with np.errstate(invalid="ignore"):
                up = np.argwhere(thr[1:] > thr[:-1])
            if len(up):
                k, j = (int(v) for v in up[0])
                raise ValueError(f"{v2}: the threshold of slice {j} rises from mark {k} ({thr[k, j]}) to mark {k + 1} ({thr[k + 1, j]}): "
                                 "a higher quality never keeps less")
            self.thresholds = thr
        elif hlen != table_end + 8:
            raise ValueError(f"{what}: the header contradicts itself: {R} x {C} tiles of {nr} rounds take "
                             f"{table_end + 8} bytes, it states {hlen}")
        self.g, self.nr, self.header_end = g, nr, end
        self.table = np.frombuffer(d, dtype="<u4", count=R * C * (1 + nr), offset=PREAMBLE_BYTES + _FIXED.size) \
            .astype(np.int64).reshape(R * C, 1 + nr)
        self.total = int(np.frombuffer(d, dtype="<u8", count=1, offset=end - 8)[0])
        self.present = self.table[:, 0] > 0
        bad = np.flatnonzero(~self.present & (self.table[:, 1:].sum(1) > 0))
        if bad.size:
            raise ValueError(f"{what}: the header contradicts itself: tile {self.rc(int(bad[0]))} is absent (a head of 0 bytes) and "
                             "has round pieces")
        if not self.present.any():
            raise ValueError(f"{what}: the header holds no tile: every head has 0 bytes")
        if end + int(self.table.sum()) != self.total:
            raise ValueError(f"{what}: the header contradicts itself: its table adds up to {end + int(self.table.sum())} bytes, it "
                             f"states a total of {self.total}")
        # the body: segment (k, i) = column k of tile i (k = 0: the head, k >= 1: round k - 1), column-major from header_end on
        self.size = np.ascontiguousarray(self.table.T)                           # [1 + nr, R C]
        ends = np.cumsum(self.size.reshape(-1)).reshape(1 + nr, R * C)
        self.off = end + ends - self.size
        self.need = end + int(self.size[0].sum())
        self.round_end = [end + int(v) for v in ends[1:, -1]]

    def rc(self, i: int) -> Tuple[int, int]:
        return i // self.g["C"], i % self.g["C"]

    def index(self, r, c, what: str) -> int:
        r, c = _int(r, f"{what}: r"), _int(c, f"{what}: c")
        if not (0 <= r < self.g["R"] and 0 <= c < self.g["C"]):
            raise ValueError(f"{what}: tile ({r}, {c}) is outside the grid of {self.g['R']} x {self.g['C']}")
        return r * self.g["C"] + c

    def held(self, n: int) -> np.ndarray:
        """int64 [1 + nr, R C]: the bytes of every segment that the first ``n`` bytes of the codestream hold."""
        return np.clip(n - self.off, 0, self.size)

    def facts(self) -> dict:
        """The geometry with ``total``, ``allocation`` and ``stages`` as :func:`layout` names them."""
        return dict(self.g, total=self.total, allocation=ALLOCATIONS[self.version == VERSION_POOLED], stages=self.stages)

    def stream(self, d, i: int) -> bytes:
        """Tile i's embedded codestream as far as ``d`` holds it."""
        n = len(d)
        return b"".join(bytes(d[int(o):min(int(o + s), n)]) for o, s in zip(self.off[:, i], self.size[:, i]) if s and o < n)


def _parse(data, what: str):
    """(view, parsed header) of a picture codestream, or a prefix of one, that holds its whole header."""
    d = view(data, what)
    s = _Picture(d, what)
    check_total(len(d), s.total, what)
    return d, s


def _tile_layout(stream, g: dict, rc, what: str, stages: int = 0) -> dict:
    """embedded.layout of one tile's head or codestream, with this format's refusals.  ``stages`` = L > 0: the tiles of a
    scheduled picture (version 3), scheduled codestreams marked by the stages 0 .. L - 1; 0: plain tiles."""
    try:
        lay = EB.layout(stream)
    except ValueError as e:
        raise ValueError(f"{what}: tile {rc}: {e}") from e
    if not stages:
        if lay["scheduled"]:
            raise ValueError(f"{what}: tile {rc} is scheduled ({lay['format']!r}); a picture codestream carries no schedules")
    elif not lay["scheduled"]:
        raise ValueError(f"{what}: tile {rc} is plain ({lay['format']!r}); a scheduled picture codestream (version "
                         f"{VERSION_SCHEDULED}) of {stages} stages carries scheduled tiles only")
    elif [int(v) for v in lay["marks"]["stage"]] != list(range(stages)):
        raise ValueError(f"{what}: tile {rc} is marked at the stages {[int(v) for v in lay['marks']['stage']]}; the tiles of this "
                         f"picture have {stages} stages and are marked at {list(range(stages))}")
    if tuple(lay["shape"]) != (g["th"] // 64, g["tw"] // 64):
        raise ValueError(f"{what}: tile {rc} is an image of {64 * lay['shape'][0]} x {64 * lay['shape'][1]}, the tiles of this picture "
                         f"are {g['th']} x {g['tw']}")
    # the marked qualities, or the stages of a scheduled tile; counts and bytes are a tile's own
    lay["marks"] = [int(v) for v in lay["marks"]["stage"]] if stages else [float(q) for q in lay["marks"]["q"]]
    return lay


_ALIKE = ("marks", "lanes", "base_lanes", "ns")


def _unlike(lay: dict, first: dict, rc, rc0, what: str):
    for key in _ALIKE:
        if not same(lay[key], first[key]):
            raise ValueError(f"{what}: tile {rc} and tile {rc0} differ in their {key}: all tiles of a picture carry the same "
                             "marks, lanes and base_lanes")


def _pieces(lay: dict) -> List[int]:
    """[bytes of the head, of round 0, ..., of the last piece] of a tile with embedded.layout ``lay``."""
    edges = [0, lay["base_end"]] + list(lay["round_end"]) + [lay["total"]]
    return [b - a for a, b in zip(edges, edges[1:])]


def _check_head(head, s: _Picture, i: int, first: Optional[dict], rc0, what: str) -> dict:
    """The embedded.layout of tile i's whole head, checked against the table: the head ends at the tile's base_end, the
    round pieces are those of its marks, plain or scheduled as the picture is, the picture's tile shape; and against
    ``first``, the layout of tile ``rc0`` (None: this is the first head, and it is checked against the header's thresholds):
    all tiles alike."""
    lay = _tile_layout(head, s.g, s.rc(i), what, s.stages)
    want = _pieces(lay)
    if s.nr > len(want) - 1 or [int(v) for v in s.table[i]] != want[:1 + s.nr]:
        raise ValueError(f"{what}: the header contradicts tile {s.rc(i)}: its table row {[int(v) for v in s.table[i]]} is not the "
                         f"head and the first {s.nr} round pieces of the tile's own codestream, {want}")
    if first is None:
        if s.thresholds is not None and tuple(s.thresholds.shape) != (len(lay["marks"]), lay["ns"]):
            raise ValueError(f"{what}: the header contradicts tile {s.rc(i)}: thresholds of {s.thresholds.shape[0]} marks x "
                             f"{s.thresholds.shape[1]} slices, the tile carries {len(lay['marks'])} marks of {lay['ns']} slices")
    else:
        _unlike(lay, first, s.rc(i), rc0, what)
    return lay


def _tile_meta(d, s: _Picture, what: str) -> Optional[dict]:
    """Reads the head of every present tile that ``d`` holds whole and checks it (:func:`_check_head`).  Returns the first
    one's embedded.layout, None when ``d`` holds no head yet."""
    first, rc0 = None, None
    for i in (int(v) for v in np.flatnonzero(s.present)):
        off, size = int(s.off[0, i]), int(s.size[0, i])
        if off + size > len(d):
            break
        lay = _check_head(d[off:off + size], s, i, first, rc0, what)
        if first is None:
            first, rc0 = lay, s.rc(i)
    return first


def _assemble(g: dict, table: np.ndarray, get, thresholds: Optional[np.ndarray] = None, stages: int = 0) -> bytes:
    """The picture codestream of ``table`` int64 [R C, 1 + nr]; ``get(i, k)`` gives the bytes of column k of tile i.
    ``thresholds`` fp32 [n_marks][ns]: a version-2 header that carries them (picture-wide marks).  ``stages`` = L > 0: a
    version-3 header that states them (scheduled tiles)."""
    nr = table.shape[1] - 1
    ext, version = b"", VERSION
    if stages:
        if not 1 <= stages <= 0xFFFF or nr > stages + 1:
            raise ValueError(f"{stages} stages and {nr} rounds: a picture of L stages, 1 .. 65535, holds at most L + 1 rounds")
        ext, version = _SCHED.pack(_KIND_SCHEDULED, stages, 0), VERSION_SCHEDULED
    elif thresholds is not None:
        version = VERSION_POOLED
        thr = np.ascontiguousarray(thresholds, dtype="<f4")
        if thr.ndim != 2 or not (1 <= thr.shape[0] <= 0xFFFF and 1 <= thr.shape[1] <= 0xFFFF):
            raise ValueError(f"thresholds are float32 [n_marks][ns], got {list(thr.shape)}")
        ext = _POOLED.pack(_ALLOC_PICTURE, thr.shape[0], thr.shape[1], 0) + thr.tobytes()
    if (table >= 1 << 32).any():
        raise ValueError("a head or round piece of 2^32 bytes or more does not fit the header's table")
    hlen = _FIXED.size + 4 * table.size + len(ext) + 8
    if hlen > MAX_HEADER:
        raise ValueError(f"the header would take {hlen} bytes, the limit is {MAX_HEADER}; use larger tiles")
    if nr > 0xFFFF:
        raise ValueError(f"{nr} rounds; the format carries up to 65535")
    header = _FIXED.pack(g["H"], g["W"], g["th"] // 64, g["tw"] // 64, g["V"], g["R"], g["C"], nr) + table.astype("<u4").tobytes() \
        + ext + struct.pack("<Q", PREAMBLE_BYTES + hlen + int(table.sum()))
    out = [FRAME.seal(header, version)]
    out += [get(i, k) for k in range(1 + nr) for i in range(table.shape[0]) if table[i, k]]
    return b"".join(out)


def pack(H: int, W: int, tile: int, overlap: int, tile_streams, thresholds=None, stages: Optional[int] = None) -> bytes:
    """The picture codestream of R C whole tile codestreams (``embedded.to_bytes``), given in raster order as one flat
    sequence or as [R][C]; None marks an absent tile.  Pure framing on the host.  ValueError for a wrong count, a cut or
    scheduled tile, a tile of another shape and tiles that differ in marks, lanes or base_lanes.  ``thresholds`` fp32
    [n_marks][ns]: the picture-wide thresholds behind the tiles' marks, one row per mark, never rising
    with the mark; the header is then version 2 and carries them.  None: version 1, byte for byte as ever.

    ``stages`` = L (exclusive with ``thresholds``): every present tile is a SCHEDULED embedded codestream
    of exactly L stages, marked at the stages 0 .. L - 1; a plain tile and another stage count are ValueErrors naming the
    tile.  The header is then version 3 and states L; the heads are the tiles' own and carry their schedules.  None:
    nothing changes, and a scheduled tile is refused."""
    if stages is not None:
        stages = _int(stages, "pack: stages")
        if not 1 <= stages <= 0xFFFF:
            raise ValueError(f"pack: stages is 1 .. 65535, got {stages}")
        if thresholds is not None:
            raise ValueError("pack: give thresholds or stages, not both: picture-wide marks (version 2) are marks of plain tiles, a "
                             "scheduled picture (version 3) is marked by stage")
    g = grid(H, W, tile, overlap)
    try:
        streams = list(tile_streams)
    except TypeError as e:
        raise ValueError(f"pack: tile_streams is a sequence of {g['R'] * g['C']} codestreams") from e
    if len(streams) == g["R"] and all(isinstance(row, (list, tuple)) for row in streams):
        streams = [s for row in streams for s in row]
    if len(streams) != g["R"] * g["C"]:
        raise ValueError(f"pack: a {H} x {W} picture at tile {tile}, overlap {overlap} has {g['R']} x {g['C']} = {g['R'] * g['C']} tiles, "
                         f"got {len(streams)} codestreams")
    rows, views, first, rc0 = [], [], None, None
    for i, s in enumerate(streams):
        rc = (i // g["C"], i % g["C"])
        if s is None:
            rows.append(None)
            views.append(None)
            continue
        v = view(s, f"pack: tile {rc}")
        lay = _tile_layout(v, g, rc, "pack", stages or 0)
        if len(v) != lay["total"]:
            raise ValueError(f"pack: tile {rc}: {len(v)} bytes, its header states a total of {lay['total']}: a picture is packed from "
                             "whole tile codestreams and cut as bytes")
        if first is None:
            first, rc0 = lay, rc
        else:
            _unlike(lay, first, rc, rc0, "pack")
        rows.append(_pieces(lay))
        views.append(v)
    if first is None:
        raise ValueError("pack: no tile: every entry is None")
    width = 2 + len(first["round_end"])
    table = np.asarray([row if row is not None else [0] * width for row in rows], dtype=np.int64)
    edges = np.concatenate([np.zeros((len(rows), 1), dtype=np.int64), np.cumsum(table, axis=1)], axis=1)
    if thresholds is not None:
        thresholds = np.asarray(thresholds, dtype=np.float32)
        if tuple(thresholds.shape) != (len(first["marks"]), first["ns"]):
            raise ValueError(f"pack: thresholds are float32 [{len(first['marks'])} marks][{first['ns']} slices], got "
                             f"{list(thresholds.shape)}")
        with np.errstate(invalid="ignore"):
            if (thresholds[1:] > thresholds[:-1]).any():
                raise ValueError("pack: a threshold rises with the mark: a higher quality never keeps less")
    try:
        return _assemble(g, table, lambda i, k: bytes(views[i][int(edges[i, k]):int(edges[i, k + 1])]), thresholds, stages or 0)
    except ValueError as e:
        raise ValueError(f"pack: {e}") from e


def need_bytes(data) -> int:
    """The smallest length from which the whole picture decodes, as far as ``data`` (any prefix) tells: the preamble's size
    while that is incomplete, the header's end while the header is, then the end of the last head."""
    d = view(data, "need_bytes")
    end = FRAME.need_header(d, "need_bytes")
    return end if len(d) < end else _parse(d, "need_bytes")[1].need


def layout(data) -> dict:
    """Where a picture codestream may be cut, from its header (``data``: any prefix that holds it): the geometry of
    :func:`grid` (H, W, th, tw, V, Sy, Sx, R, C), ``header_end``, ``need_bytes``, ``n_rounds``, ``total``,
    ``present[r][c]``, ``head[r][c]`` = (offset, length), ``piece[k][r][c]`` = (offset, length) and ``round_end[k]`` for
    k < n_rounds: ``data[:round_end[k]]`` holds every present tile exactly at its mark k (a whole stream has one round more
    than marks, and its last ``round_end`` is ``total``).  ``marks``, ``lanes``, ``base_lanes``, ``ns`` and ``format`` are
    those of the tiles, read from the heads that ``data`` holds whole (all checked against the table and each other); None
    while it holds none.  ``allocation``: "tile" (version 1) or "picture" (version 2), and then
    ``thresholds`` float32 [marks][ns], the picture-wide sigma thresholds behind the tiles' marks (None for "tile").
    ``scheduled`` and ``stages``: True and L for a version-3 stream, whose tiles are scheduled, whose
    rounds are stages and whose ``marks`` is the stage list [0 .. L - 1]; False and 0 otherwise."""
    d, s = _parse(data, "layout")
    g, meta = s.g, _tile_meta(d, s, "layout")
    R, C = g["R"], g["C"]
    seg = lambda k: [[(int(s.off[k, r * C + c]), int(s.size[k, r * C + c])) for c in range(C)] for r in range(R)]
    out = dict(g)
    out.update({"header_end": s.header_end, "need_bytes": s.need, "n_rounds": s.nr, "total": s.total,
                "present": [[bool(s.present[r * C + c]) for c in range(C)] for r in range(R)],
                "head": seg(0), "piece": [seg(1 + k) for k in range(s.nr)], "round_end": list(s.round_end)})
    for key in _ALIKE + ("format",):
        out[key] = meta[key] if meta is not None else None
    out["allocation"] = ALLOCATIONS[s.version == VERSION_POOLED]
    out["thresholds"] = None if s.thresholds is None else s.thresholds.copy()
    out["scheduled"], out["stages"] = s.stages > 0, s.stages
    return out


def tile_stream(data, r: int, c: int) -> bytes:
    """Tile (r, c)'s embedded codestream as far as ``data`` (a picture codestream or any prefix that holds the header) holds
    it: its head and round pieces, concatenated.  The result may end anywhere, also inside a piece; from the tile's head on
    ``embedded.from_bytes`` accepts it.  ValueError for an absent tile."""
    d, s = _parse(data, "tile_stream")
    i = s.index(r, c, "tile_stream")
    if not s.present[i]:
        raise ValueError(f"tile_stream: tile ({r}, {c}) is absent from this codestream")
    return s.stream(d, i)


def _kept(s: _Picture, window, rounds, what: str) -> Tuple[int, np.ndarray]:
    """(the rounds, bool [R C]: the tiles) that :func:`extract` of ``window`` and ``rounds`` keeps of the picture ``s``."""
    nr = s.nr if rounds is None else _int(rounds, f"{what}: rounds")
    if not 0 <= nr <= s.nr:
        raise ValueError(f"{what}: rounds is 0 .. {s.nr} (the rounds this codestream holds), got {nr}")
    keep = np.zeros_like(s.present)
    if window is None:
        keep[:] = s.present
    else:
        for r, c in tiles_for(s.g, _window(s.g, window, what)):
            i = r * s.g["C"] + c
            if not s.present[i]:
                raise ValueError(f"{what}: the window {tuple(window)} needs tile ({r}, {c}), which is absent from this codestream")
            keep[i] = True
    return nr, keep


def extract(data, window=None, rounds: Optional[int] = None) -> bytes:
    """A shorter picture codestream of the same picture: only the tiles ``tiles_for(window)`` (None: those present) and only
    the first ``rounds`` rounds (None: all it has).  What a server does to crop and to cut the quality, without the model.
    ``data`` must hold what is kept.  ``extract(data)`` is ``data``; an extract of an extract is an extract.  ValueError
    names a wanted tile that ``data`` lacks.  An extract keeps the version, and a version-2 stream its thresholds: the pool
    is the picture's, not the window's; a version-3 stream keeps its n_stages, and ``rounds=k + 1`` holds every kept tile
    exactly at stage k."""
    d, s = _parse(data, "extract")
    _tile_meta(d, s, "extract")
    nr, keep = _kept(s, window, rounds, "extract")
    table = np.where(keep[:, None], s.table[:, :1 + nr], 0)
    short = np.argwhere((s.held(len(d))[:1 + nr].T < table))
    if len(short):
        i, k = (int(v) for v in short[0])
        raise ValueError(f"extract: {len(d)} bytes end before {'the head' if k == 0 else f'round {k - 1}'} of tile {s.rc(i)} does; "
                         "a codestream is extracted from bytes that hold what is kept")
    return _assemble(s.g, table, lambda i, k: bytes(d[int(s.off[k, i]):int(s.off[k, i] + s.size[k, i])]), s.thresholds, s.stages)


# ---------------------------------------------------------------------------------------------------- encoder and decoder
def _default_group(th: int, tw: int) -> int:
    """The most tiles of th x tw that control.sweep_groups keeps in one plan, at most MAX_GROUP."""
    from .control import sweep_groups
    n = 1
    while n < MAX_GROUP and len(sweep_groups(1, n + 1, th, tw)) == 1:
        n += 1
    return n


def _check_group(group, th: int, tw: int, what: str) -> int:
    if group is None:
        return _default_group(th, tw)
    group = _int(group, f"{what}: group")
    if group < 1:
        raise ValueError(f"{what}: group is the tiles per batch, >= 1, got {group}")
    return group


def _check_picture_schedule(schedule, H: int, W: int, device):
    """A picture-wide schedule for a picture of H x W on ``device``: an fp32 tensor [L, H, W] there,
    1 <= L <= VAM_MAX_LAYER_LEVELS, every entry finite and >= 0, never decreasing from stage to stage at any pixel.  Shape,
    dtype, device and L are checked on the host; the values with a few reductions on the device and ONE read.  Returns the
    contiguous tensor; ValueError names the stage and the pixel of the first violation."""
    import torch
    from . import _lib as L
    G = L.VAM_MAX_LAYER_LEVELS
    if not isinstance(schedule, torch.Tensor) or schedule.dtype != torch.float32 or schedule.dim() != 3 \
            or tuple(schedule.shape[1:]) != (H, W):
        got = f"{schedule.dtype} {list(schedule.shape)}" if isinstance(schedule, torch.Tensor) else type(schedule).__name__
        raise ValueError(f"tiled.encode: schedule is an fp32 tensor [L, H, W] = [1..{G}, {H}, {W}], L quality maps at pixel "
                         f"resolution, got {got}")
    if schedule.device != device:
        raise ValueError(f"tiled.encode: schedule lies on {schedule.device}, the image on {device}: a picture-wide schedule is "
                         "read on the image's device")
    n_st = int(schedule.shape[0])
    if not 1 <= n_st <= G:
        raise ValueError(f"tiled.encode: schedule: 1..{G} stages, got {n_st}")
    S = schedule.detach().contiguous()
    with torch.no_grad():
        flat = S.reshape(-1)
        bad = (~torch.isfinite(flat)) | (flat < 0)
        down = (S[1:] < S[:-1]).reshape(-1) if n_st > 1 else torch.zeros((1,), dtype=torch.bool, device=device)
        at_bad, at_down = bad.to(torch.uint8).argmax(), down.to(torch.uint8).argmax()      # the first violation of each kind
        lo = flat[at_down] if n_st > 1 else flat[0]
        hi = flat[at_down + H * W] if n_st > 1 else flat[0]
        got = torch.stack([bad[at_bad].double(), at_bad.double(), flat[at_bad].double(), down[at_down].double(), at_down.double(),
                           lo.double(), hi.double()]).cpu().numpy()
    where = lambda i: (int(i) // (H * W), (int(i) % (H * W)) // W, int(i) % W)
    if got[0]:
        k, y, x = where(got[1])
        raise ValueError(f"tiled.encode: schedule: stage {k}, pixel ({y}, {x}): qualities are finite and >= 0, got {float(got[2])}")
    if got[3]:
        k, y, x = where(got[4])
        raise ValueError(f"tiled.encode: schedule: pixel ({y}, {x}): stage {k + 1} lowers the quality from {float(got[5])} to "
                         f"{float(got[6])}; a schedule never decreases from one stage to the next")
    return S


MAX_BUDGETS = 32                           # the marks of one container (progressive.check_q_list)


def check_budgets(max_bytes, what: str = "tiled.encode") -> List[int]:
    """``max_bytes`` as the budget list of :func:`encode`: one integer or 1 .. MAX_BUDGETS strictly increasing integers."""
    if isinstance(max_bytes, (int, np.integer)) and not isinstance(max_bytes, bool):
        max_bytes = [max_bytes]
    try:
        budgets = [_int(v, f"{what}: max_bytes") for v in max_bytes]
    except TypeError as e:
        raise ValueError(f"{what}: max_bytes is a byte budget or a list of them, got {type(max_bytes).__name__}") from e
    if not 1 <= len(budgets) <= MAX_BUDGETS:
        raise ValueError(f"{what}: max_bytes: 1 .. {MAX_BUDGETS} budgets, got {len(budgets)}")
    for k in range(1, len(budgets)):
        if budgets[k] <= budgets[k - 1]:
            raise ValueError(f"{what}: max_bytes: budget {k}, {budgets[k]} bytes, does not exceed budget {k - 1}, {budgets[k - 1]} "
                             "bytes: budgets are strictly increasing")
    return budgets


def solve_budgets(sizes, heads_end: int, budgets: Sequence[int], q_tol: float = 1e-3, what: str = "tiled.encode") -> List[float]:
    """The qualities of a budgeted picture, on the host alone: per budget N_k the largest quality that
    ``control.rate_search`` reaches at ``q_tol`` whose round ends within N_k; raising it by q_tol (capped at 10) would not
    fit unless it is 10.  ``sizes(rows)``: ``rows`` is a list of ascending quality lists in (0, 10], each at most
    ``control.RATE_GRID`` long, and the result holds, row by row, the byte position at which a round marked at each of those
    qualities ends, heads included; it never decreases with the quality.  ``heads_end``: where the heads end, what a round
    of nothing costs.  Every budget is solved on its own: the heads do not depend on the qualities.  ValueError names a
    budget below ``heads_end``, one that holds the heads but not the smallest quality tried (with the bytes that one needs)
    and two budgets that solve to one quality."""
    from .control import rate_search
    budgets = check_budgets(list(budgets), what)
    if not q_tol > 0:
        raise ValueError(f"{what}: q_tol must be > 0, got {q_tol}")
    for k, N in enumerate(budgets):
        if N < heads_end:
            raise ValueError(f"{what}: max_bytes: budget {k}, {N} bytes, is below heads_end = {heads_end} bytes: the header, z, the "
                             "base and the tile heads, which every prefix needs")
    least = {}                                                   # per budget: the smallest quality tried and the bytes it needs

    def curve(q, need):
        rows = [k for k in range(len(budgets)) if need[k, 0].any()]
        got = sizes([[float(v) for v in q[k, 0][need[k, 0]]] for k in rows])
        out = np.zeros(q.shape)
        for k, r in zip(rows, got):
            out[k, 0][need[k, 0]] = np.asarray(r, dtype=np.float64)
            q0 = float(q[k, 0][need[k, 0]][0])
            if k not in least or q0 < least[k][0]:
                least[k] = (q0, int(r[0]))
        return out
    quality, _, _ = rate_search(curve, np.asarray([float(heads_end)]), np.asarray(budgets, dtype=np.float64)[:, None], q_tol)
    qs = [float(v) for v in quality[:, 0]]
    for k, q in enumerate(qs):
        if q <= 0:
            raise ValueError(f"{what}: max_bytes: budget {k}, {budgets[k]} bytes, holds the heads ({heads_end} bytes) but no round: "
                             f"the smallest quality tried, {least[k][0]:.6g}, needs {least[k][1]} bytes")
        if k and q <= qs[k - 1]:
            raise ValueError(f"{what}: max_bytes: budgets {k - 1} and {k}, {budgets[k - 1]} and {budgets[k]} bytes, solve to the same "
                             f"quality {q:.6g}: the second round would be empty; drop one of them")
    return qs


def budget_marks(data) -> List[Tuple[float, int]]:
    """What a picture-wide encode marked, and :func:`encode` with ``max_bytes`` solved: ``[(q_k, round_end[k])]`` per mark,
    the qualities from the tile heads, the round ends from the header's table.  ``data``: any prefix that holds the header
    and one tile's head.  ValueError for a stream that is not picture-wide (version 2)."""
    lay = layout(data)
    if lay["allocation"] != "picture" or lay["marks"] is None:
        raise ValueError("budget_marks: " + ("these bytes hold no tile's head yet" if lay["allocation"] == "picture" else
                                             "the marks of this codestream are not picture-wide (allocation='picture')"))
    return [(float(q), int(e)) for q, e in zip(lay["marks"], lay["round_end"])]


def _round_ends(keys, cuts, qs):
    """int64 [len(qs)] on the device: the bytes of all tiles' embedded streams up to a picture-wide mark at each of the
    ascending qualities ``qs`` (at most 32), from the pooled keys and the cut table ``cuts`` int32 [T, ns, n + 1]: one
    vam_pooled_select, one vam_threshold_counts, a gather and a sum.  No synchronisation."""
    import torch
    from . import ops
    T, ns, _ = keys.shape
    thr = torch.empty((len(qs), ns), dtype=torch.float32, device=keys.device)
    count = torch.empty((len(qs), T, ns), dtype=torch.int32, device=keys.device)
    ops.pooled_select(keys, qs, thr)
    ops.threshold_counts(keys, thr, count)
    return torch.gather(cuts, 2, count.permute(1, 2, 0).long()).sum(dim=(0, 1), dtype=torch.int64)


def _heads_end(H: int, W: int, tile: int, overlap: int, passes, n_marks: int) -> int:
    """Where the heads of a picture-wide stream of ``n_marks`` marks end, measured on a packed stream: the picture of the
    front passes' z and base strings with EMPTY embedded strings is nothing but header and heads.  Neither the picture
    header nor a tile head depends on the values of marks, counts, bytes or thresholds, only on how many there are."""
    streams = []
    for _, st in passes:
        K, Kb, ns = st["K"], st["Kb"], st["m"].ns0
        zero = [[0] * ns for _ in range(n_marks)]
        for b in range(st["B"]):                      # the container embedded._encode_finish builds, with nothing embedded
            c = {"format": EB._format_of(K, Kb, False), "shape": (st["H"] // 64, st["W"] // 64), "z": [st["z_str"][b]],
                 "base": [[st["base"][i][b]] for i in range(ns)], "embedded": [b""] * ns,
                 "marks": {"q": [float(k + 1) for k in range(n_marks)], "count": zero, "bytes": zero}}
            if c["format"] != EB.FORMAT:
                c["lanes"] = K
            if Kb > 1:
                c["base_lanes"] = Kb
            streams.append(EB.to_bytes(c))
    return len(pack(H, W, tile, overlap, streams, thresholds=np.zeros((n_marks, passes[0][1]["m"].ns0), dtype=np.float32)))


def encode(model, image, tile: int = 256, overlap: int = 32, marks: Optional[Sequence[float]] = None, coder: Optional[str] = None,
           lanes: int = 1, base_lanes: int = 1, group: Optional[int] = None, allocation: str = "tile", schedule=None,
           max_bytes=None, q_tol: float = 1e-3) -> bytes:
    """The picture codestream of ``image``, fp32 [3, H, W] or [1, 3, H, W] on the device, any H, W >= 1: the tiles are cut
    ``group`` at a time (vam_tile_extract, one launch per group), each group goes through ``embedded.encode_batch`` (``marks``,
    ``coder``, ``lanes`` and ``base_lanes`` are its) and ``embedded.to_bytes``, and :func:`pack` frames them.  ``group``: the
    tiles per batch, by default the most that one plan holds, at most 32; the bytes do not depend on it.

    ``allocation`` = "tile" (the default, version-1 bytes as ever): every tile marks its own quantiles.  "picture" (DESIGN
    section 9w): the marks are picture-wide.  Pass 1 runs every group's network, rank order and gather once
    (``embedded._encode_front``) and writes its sigmas, in rank order, as keys into one buffer [T, ns, n] (vam_pool_keys); one
    vam_pooled_select gives, per mark and slice, ``torch.quantile`` of the pool of ALL tiles' sigmas, one vam_threshold_counts
    every tile's counts; pass 2 (``embedded._encode_finish``) marks the tiles with them.  The tile heads stay ordinary
    embedded headers; the picture header is version 2 and carries the thresholds.  Marks are qualities > 0.

    ``max_bytes`` = N or [N_1 < ... < N_L], 1 <= L <= 32 (with ``allocation="picture"`` only, exclusive
    with ``marks`` and ``schedule``): rounds that end at byte budgets.  The result is an ordinary version-2 stream of L
    marks whose ``layout(data)["round_end"][k] <= N_k``; mark k's quality is the largest that ``control.rate_search``
    reaches at ``q_tol`` (:func:`solve_budgets`), and :func:`budget_marks` reads it back.  Pass 1 also fills a cut table int32
    [T, ns, n + 1] on the device, the bytes of every stream for EVERY count: one vam_rans_interleaved_cut_table_device
    launch per group on the device coder, ``bitstream.cut_table`` of the coded strings on the host coder.  A candidate
    quality then costs one vam_pooled_select and one vam_threshold_counts per 32 of them, a gather and a sum; the coder runs
    once, in pass 2, with the solved counts, and the bytes it marks must equal the table's (checked, not tolerated).
    ValueError names a budget that is out of order, below the heads, too small for the smallest quality tried, or that
    solves to its neighbour's quality.

    ``schedule`` (exclusive with ``marks`` and with ``allocation="picture"``): a picture-wide schedule,
    fp32 [L, H, W] on the image's device, 1 <= L <= 32 quality maps at PIXEL resolution, every entry finite and >= 0 and
    never decreasing from stage to stage (checked on the device up front; a violation names stage and pixel).  Per group one
    vam_tile_extract, one vam_tile_schedule (the block maximum of every latent cell over the tile's replicated pixels), one
    copy of that small result to the host and ``embedded.encode_batch(schedule=)`` unchanged; the picture header is
    version 3 and its rounds are stages.  A tile whose schedule holds more than 32 distinct qualities is
    ``embedded.check_schedule``'s error, naming the tile (r, c)."""
    import torch
    from . import ops
    if allocation not in ALLOCATIONS:
        raise ValueError(f"tiled.encode: allocation is one of {ALLOCATIONS}, got {allocation!r}")
    budgets = None
    if max_bytes is not None:
        if marks is not None or schedule is not None:
            raise ValueError("tiled.encode: give max_bytes or " + ("marks" if marks is not None else "schedule") + ", not both: "
                             "byte budgets solve the marks' qualities themselves")
        if allocation != "picture":
            raise ValueError(f"tiled.encode: max_bytes goes with allocation='picture', not with {allocation!r}: one threshold per "
                             "slice over all tiles is what spends a budget where the picture is busy")
        budgets = check_budgets(max_bytes)
        if not q_tol > 0:
            raise ValueError(f"tiled.encode: q_tol must be > 0, got {q_tol}")
    if schedule is not None and marks is not None:
        raise ValueError("tiled.encode: give marks or schedule, not both (a scheduled picture is marked per stage)")
    if schedule is not None and allocation != "tile":
        raise ValueError(f"tiled.encode: a schedule goes with allocation='tile', not with {allocation!r}: picture-wide marks are "
                         "marks of plain tiles")
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() not in (3, 4) \
            or tuple(image.shape[:-2]) not in ((3,), (1, 3)):
        raise ValueError("tiled.encode: image is an fp32 tensor [3, H, W] or [1, 3, H, W], got "
                         f"{tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__}")
    H, W = (int(v) for v in image.shape[-2:])
    g = grid(H, W, tile, overlap)
    group = _check_group(group, g["th"], g["tw"], "tiled.encode")
    EB._check_model(model)
    img = image.detach().reshape(3, H, W).contiguous()
    coords = [(r, c) for r in range(g["R"]) for c in range(g["C"])]
    streams: List[bytes] = []

    def cut(i0, with_coords=False):
        part = coords[i0:i0 + group]
        cd = torch.tensor(part, dtype=torch.int32).to(img.device)
        x = torch.empty((len(part), 3, g["th"], g["tw"]), dtype=torch.float32, device=img.device)
        ops.tile_extract(img, cd, x, g["V"])
        return (x, cd) if with_coords else x
    if schedule is not None:
        S = _check_picture_schedule(schedule, H, W, img.device)
        n_st, h, w = int(S.shape[0]), g["th"] // 16, g["tw"] // 16
        with torch.no_grad():
            for i0 in range(0, len(coords), group):
                x, cd = cut(i0, True)
                st = torch.empty((x.shape[0], n_st, h, w), dtype=torch.float32, device=img.device)
                ops.tile_schedule(S, cd, st, g["th"], g["tw"], g["V"])
                st = st.cpu().numpy()
                stage_maps = [st[:, k] for k in range(n_st)]
                try:
                    cs = EB.encode_batch(model, x, schedule=stage_maps, coder=coder, lanes=lanes, base_lanes=base_lanes)
                except ValueError:
                    for b, rc in enumerate(coords[i0:i0 + group]):     # a tile's schedule is checked alone as in its group
                        try:
                            EB.check_schedule([m[b:b + 1] for m in stage_maps], 1, h, w)
                        except ValueError as e:
                            raise ValueError(f"tiled.encode: tile {rc}: {e}") from e
                    raise
                streams += [EB.to_bytes(c) for c in cs]
        return pack(H, W, tile, overlap, streams, stages=n_st)
    if allocation == "tile":
        with torch.no_grad():
            for i0 in range(0, len(coords), group):
                cs = EB.encode_batch(model, cut(i0), marks=marks, coder=coder, lanes=lanes, base_lanes=base_lanes)
                streams += [EB.to_bytes(c) for c in cs]
        return pack(H, W, tile, overlap, streams)
    from . import bitstream as bs
    from . import progressive as P
    if budgets is not None:                # placeholders until the search has run: the front pass needs only their number
        marks = [10.0 * (k + 1) / len(budgets) for k in range(len(budgets))]
    qs = P.check_q_list(EB.Q_LIST if marks is None else marks)
    if qs[0] <= 0:
        raise ValueError(f"tiled.encode: a picture-wide mark is a quality > 0, got {qs}")
    coder, K, Kb = P._check_coder(model, coder), bs.check_lanes(lanes), bs.check_lanes(base_lanes)
    T, ns, n = len(coords), model.ns0, model.dim_chunk * (g["th"] // 16) * (g["tw"] // 16)
    if T * n > MAX_POOL:
        raise ValueError(f"tiled.encode: the pool of a slice holds {T} tiles x {n} = {T * n} sigmas, torch.quantile and "
                         f"vam_pooled_select take up to {MAX_POOL}; use allocation='tile'")
    with torch.no_grad():
        keys = torch.empty((T, ns, n), dtype=torch.int32, device=img.device)      # the bits of uint32 keys
        passes = []
        cuts = cut_status = None
        if budgets is not None:                                                   # the cut table: bytes for EVERY count of every stream
            cuts = torch.empty((T, ns, n + 1), dtype=torch.int32, device=img.device)
            cut_status = torch.zeros(T * ns, dtype=torch.int32, device=img.device)
            tg = bs.DeviceCoderTables.of(model.gaussian_conditional, img.device) if coder == "device" \
                else bs.Tables.of(model.gaussian_conditional)
        for i0 in range(0, T, group):                                             # pass 1: the network runs once per tile
            st = EB._encode_front(model, cut(i0), qs, coder, K, Kb)
            ops.pool_keys(st.pop("std_p"), st.pop("perm"), keys, t0=i0, n_slice=ns)
            passes.append((i0, st))
            if budgets is None:
                continue
            B = st["B"]
            if coder == "device":                                                 # one dry walk of the encoder, no read-back
                bs.cut_table_launch(st["r_sym"], st["r_idx"], tg, K, cuts[i0:i0 + B], cut_status[i0 * ns:(i0 + B) * ns])
            else:                                                                 # one decoding pass per coded string, on the host's threads
                rows = EB._map_threads(lambda bj, st=st: bs.cut_table(st["emb_str"][bj[0] * ns + bj[1]], st["r_idx"][bj[0], bj[1]], tg, K),
                                       [(b, j) for b in range(B) for j in range(ns)])
                cuts[i0:i0 + B].copy_(torch.from_numpy(np.stack(rows).reshape(B, ns, n + 1)))
        if budgets is not None:
            bs.raise_cut_status(cut_status)
            heads_end = _heads_end(H, W, tile, overlap, passes, len(budgets))

            def round_ends(rows):                                                 # per row: 2 launches, a gather, a sum; ONE read-back
                ends = torch.stack([_round_ends(keys, cuts, row) for row in rows]).cpu().numpy()      # a pass asks rows of one length
                return [heads_end + e for e in ends]
            qs = solve_budgets(round_ends, heads_end, budgets, q_tol)
            for _, st in passes:
                st["qs"] = list(qs)
        thr = torch.empty((len(qs), ns), dtype=torch.float32, device=img.device)
        count = torch.empty((len(qs), T, ns), dtype=torch.int32, device=img.device)
        ops.pooled_select(keys, qs, thr)
        ops.threshold_counts(keys, thr, count)
        if budgets is not None:                                                   # what the table says the marks' bytes are
            want = torch.gather(cuts, 2, count.permute(1, 2, 0).long()).cpu().numpy().astype(np.int64)      # [T, ns, L]
        for i0, st in passes:                                                     # pass 2: the marks' bytes from the picture's counts
            cs = EB._encode_finish(st, count[:, i0:i0 + st["B"]].contiguous())
            if budgets is not None:
                for b, c in enumerate(cs):                                        # the coder's own positions: equal, or a bug
                    got = np.asarray(c["marks"]["bytes"], dtype=np.int64).T
                    if not np.array_equal(got, want[i0 + b]):
                        raise AssertionError(f"tiled.encode: tile {coords[i0 + b]}: the coder marks its slices at {got.tolist()} bytes, "
                                             f"the cut table says {want[i0 + b].tolist()} (slice by mark)")
            streams += [EB.to_bytes(c) for c in cs]
        thr = thr.cpu().numpy()
    data = pack(H, W, tile, overlap, streams, thresholds=thr)
    if budgets is not None:
        ends = [int(want[:, :, k].sum()) + heads_end for k in range(len(budgets))]
        got = layout(data)["round_end"][:len(budgets)]
        if got != ends or any(e > N for e, N in zip(ends, budgets)):
            raise AssertionError(f"tiled.encode: the rounds end at {got}, the search placed them at {ends} within the budgets {budgets}")
    return data


def _ramps_on(have, V: int, device):
    """The blend ramps of overlap V as tensors on ``device``; ``have``: what an earlier call returned, or None."""
    import torch
    if have is None or have[0].device != device:
        have = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in ramps(V))
    return have


def _check_dtype(what: str, dtype):
    """The dtype of an output, torch.float32 when None."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{what}: dtype is torch.float32 or torch.uint8, got {dtype}")
    return dtype


def _slot_table(g: dict, tiles) -> np.ndarray:
    """int32 [R, C] for a buffer that holds just ``tiles``, in their order: i at the i-th of them, -1 elsewhere."""
    slot = np.full((g["R"], g["C"]), -1, dtype=np.int32)
    for i, (r, c) in enumerate(tiles):
        slot[r, c] = i
    return slot


def _check_pooled(model, thresholds, dec, containers, part):
    """A version-2 header's thresholds against the tiles' marks: the decoder's OWN sigma, in its own rank order
    (vam_pool_keys), counted against the header's thresholds (vam_threshold_counts), must give the counts the tiles'
    marks state, for every mark."""
    import torch
    from . import ops
    dp, ns = dec.dp, model.ns0
    thr = np.ascontiguousarray(thresholds, dtype=np.float32)
    with torch.no_grad():
        dec._own()
        with dp.runner.on_stream():
            keys = torch.empty((dp.B, ns, dp.perm.shape[2]), dtype=torch.int32, device=dp.device)
            count = torch.empty((thr.shape[0], dp.B, ns), dtype=torch.int32, device=dp.device)
            ops.pool_keys(dp.sc.std_p, dp.perm, keys, t0=0, n_slice=ns)
            ops.threshold_counts(keys, torch.from_numpy(thr).to(dp.device), count)
            got = count.cpu().numpy()
    want = np.stack([np.asarray(c["marks"]["count"], dtype=np.int64).reshape(-1, ns) for c in containers], axis=1)
    bad = np.argwhere(got != want) if got.shape == want.shape else np.zeros((1, 3), dtype=np.int64)
    if len(bad):
        k, b, j = (int(v) for v in bad[0])
        raise ValueError(f"tile {part[b] if part is not None else b}, mark {k}, slice {j}: the header's picture-wide threshold "
                         f"{thr[k, j]} keeps {int(got[k, b, j])} elements of this tile's sigma, the tile's mark states "
                         f"{int(want[k, b, j])}: thresholds and tiles are not of one picture")


def _decode_tiles(model, coder, thresholds, containers, q, mark=None, part=None, stage=None):
    """x_hat of one group of tile containers through a fresh ``embedded.EmbeddedDecoder``: from everything they hold, at a
    quality, at a mark (checked against ``thresholds`` when the picture carries them) or at a stage."""
    dec = EB.EmbeddedDecoder(model, containers, coder=coder)
    if stage is not None:
        return dec.decode_stages([stage])[0]["x_hat"]
    if mark is None:
        return (dec.decode() if q is None else dec.decode_qualities([q])[0])["x_hat"]
    x_hat = dec.decode_marks([mark])[0]["x_hat"]
    if thresholds is not None:
        _check_pooled(model, thresholds, dec, containers, part)
    return x_hat


def _mark_of(what: str, marks, thresholds, q, mark) -> Optional[int]:
    """The mark a decode call means: ``mark`` itself, or, on a version-2 stream, the mark whose quality ``q`` is."""
    if mark is not None:
        if q is not None:
            raise ValueError(f"{what}: give q or mark, not both")
        mark = _int(mark, f"{what}: mark")
        if not 0 <= mark < len(marks):
            raise ValueError(f"{what}: mark is 0 .. {len(marks) - 1} (the marks {marks}), got {mark}")
        return mark
    if q is None or thresholds is None:
        return None
    if float(q) not in marks:
        raise ValueError(f"{what}: quality {q} is not marked; this picture's marks are picture-wide (allocation "
                         f"'picture') and a picture-wide quality exists only where the encoder pooled: the marks are {marks}")
    return marks.index(float(q))


def _stage_of(what: str, scheduled: bool, stages: int, q, mark, stage) -> Optional[int]:
    """The stage a decode call means, checked against what the picture is."""
    if stage is None:
        if q is not None and scheduled:
            raise ValueError(f"{what}: this picture is scheduled ({stages} stages): a uniform quality is no "
                             f"prefix of a scheduled rank order, decode a stage with stage=0 .. {stages - 1}")
        return None
    if q is not None or mark is not None:
        raise ValueError(f"{what}: give stage alone, not with q or mark")
    if not scheduled:
        raise ValueError(f"{what}: stage= decodes a scheduled picture (tiled.encode(schedule=)); this picture "
                         "carries no schedule, decode a quality with q or a mark with mark")
    stage = _int(stage, f"{what}: stage")
    if not 0 <= stage < stages:
        raise ValueError(f"{what}: stage is 0 .. {stages - 1}, got {stage}")
    return stage


def _level_of(what: str, stages: int, meta: Optional[dict], thresholds, q, mark, stage) -> Tuple[Optional[int], Optional[int]]:
    """(mark, stage) that a call with (q, mark, stage) means, checked against what the picture is.  ``meta`` None: no head
    is whole yet, the marks are not known, and no tile is available anyway."""
    stage = _stage_of(what, stages > 0, stages, q, mark, stage)
    return (None if meta is None else _mark_of(what, meta["marks"], thresholds, q, mark)), stage


def _decode_window(what: str, model, coder, thresholds, tiles, stream_of, group: int, g: dict, q, mark, stage):
    """fp32 [len(tiles), 3, th, tw] on the model's device: the tiles (r, c) of ``tiles``, ``group`` at a time through
    :func:`_decode_tiles`; ``stream_of(r, c)`` gives a tile's bytes.  When a group is refused its tiles are tried alone, and
    the ValueError names the one that is."""
    import torch
    buf = None
    for i0 in range(0, len(tiles), group):
        part = tiles[i0:i0 + group]
        cs = [EB.from_bytes(stream_of(r, c)) for r, c in part]
        try:
            x_hat = _decode_tiles(model, coder, thresholds, cs, q, mark, part, stage)
        except ValueError:
            for rc, c1 in zip(part, cs):            # a tile decodes alone as in its group: find the one that is refused
                try:
                    _decode_tiles(model, coder, thresholds, [c1], q, mark, [rc], stage)
                except ValueError as e:
                    raise ValueError(f"{what}: tile {rc}: {e}") from e
            raise
        if buf is None:
            buf = torch.empty((len(tiles), 3, g["th"], g["tw"]), dtype=torch.float32, device=x_hat.device)
        buf[i0:i0 + len(part)].copy_(x_hat)
    return buf


def _tile_rounds(s: _Picture, n: int) -> np.ndarray:
    """int64 [R, C]: the complete rounds that the first ``n`` bytes of the codestream hold of every tile (a piece of 0 bytes
    is whole), -1 where the tile is absent or its head is not whole."""
    held = s.held(n)
    done = np.cumprod(held[1:] == s.size[1:], axis=0).sum(0) if s.nr else np.zeros(s.present.size, dtype=np.int64)
    return np.where(s.present & (held[0] == s.size[0]), done, -1).astype(np.int64).reshape(s.g["R"], s.g["C"])


def _available(rounds: np.ndarray, tiles, level: Optional[int]) -> List[Tuple[int, int]]:
    """Those of ``tiles`` whose head is whole and, at mark or stage ``level``, whose rounds 0 .. level are."""
    least = 0 if level is None else level + 1
    return [(r, c) for r, c in tiles if rounds[r, c] >= least]


def _not_available(what: str, s: _Picture, window, rc, missing: int, level: Optional[int], rounds: np.ndarray) -> ValueError:
    """The error of a window that needs tile ``rc`` where nothing coarser stands in for it."""
    y0, x0, h, w = window
    if not s.present[rc[0] * s.g["C"] + rc[1]]:
        why = "which is absent from this codestream"
    elif rounds[rc] < 0:
        why = f"whose head has not arrived: {missing} bytes are missing before every tile's head is whole"
    else:
        why = f"which holds {int(rounds[rc])} whole rounds, {level + 1} are needed"
    return ValueError(f"{what}: the window ({y0}, {x0}, {h}, {w}) needs tile ({rc[0]}, {rc[1]}), {why}, and there is no coarser "
                      "level to fill it from")


def _blend_out(what: str, g: dict, window, buf, slot: Optional[np.ndarray], ramps_on, dtype, below=None, below_window=None, shift=None,
               dirty: Optional[np.ndarray] = None, box=None, out=None):
    """One launch over ``window`` from ``buf`` fp32 [n, 3, th, tw] and ``slot`` int32 [R, C] (both None: no tile is
    available); ``ramps_on(dev)`` gives the blend ramps there.  ``dirty`` int32 [R, C]: vam_tile_refresh of ``box`` into
    ``out``, a canvas of the window, whose dtype holds (``dtype`` is not looked at when ``out`` is given); else ``out`` is new,
    of ``dtype``, and with ``below`` it is vam_tile_compose's, without (every tile of the window is available)
    vam_tile_blend's."""
    import torch
    from . import _lib as L
    from . import ops
    if below is not None:
        if not isinstance(below, torch.Tensor) or below.dtype != torch.float32 or below.dim() != 3 or below.shape[0] != 3 or not below.is_cuda:
            raise ValueError(f"{what}: below is an fp32 tensor [3, hb, wb] on the device, got "
                             f"{(below.dtype, tuple(below.shape)) if isinstance(below, torch.Tensor) else type(below).__name__}")
        shift = _int(shift, f"{what}: shift")
        if not 1 <= shift <= 15:
            raise ValueError(f"{what}: shift is 1 .. 15 (below is 2^shift times coarser), got {shift}")
        lower = {"H": -(-g["H"] // (1 << shift)), "W": -(-g["W"] // (1 << shift))}
        below_window = _window(lower, below_window, f"{what}: below_window")
        if tuple(below.shape[1:]) != below_window[2:]:
            raise ValueError(f"{what}: below is {tuple(below.shape)}, its window {below_window} takes [3, {below_window[2]}, {below_window[3]}]")
        if buf is not None and buf.device != below.device:
            raise ValueError(f"{what}: below lies on {below.device}, the tiles on {buf.device}")
    dev = buf.device if buf is not None else below.device
    with torch.no_grad():
        w_lo, w_hi = ramps_on(dev) if buf is not None and g["V"] else (None, None)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        if out is None:
            h, w = window[2:]
            out = torch.empty((3, h, w), dtype=torch.float32, device=dev) if dtype == torch.float32 \
                else torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        slot_dev = None if slot is None else torch.from_numpy(slot).to(dev)
        if dirty is not None:
            ops.tile_refresh(buf, slot_dev, torch.from_numpy(dirty).to(dev), w_lo, w_hi, g["H"], g["W"], g["V"], window, box, out, status)
        elif below is None:
            ops.tile_blend(buf, slot_dev, w_lo, w_hi, g["H"], g["W"], g["V"], window, out, status)
        else:
            ops.tile_compose(buf, slot_dev, w_lo, w_hi, g["H"], g["W"], g["V"], window, below.detach().contiguous(), below_window, shift,
                             out, status)
        if int(status.item()):
            raise L.VamError(f"{what}: the kernel met a slot beyond the tile buffer inside the window")
    return out


class PictureDecoder:
    """Decodes a picture codestream by window.  ``data``: any prefix of at least :func:`need_bytes`, or an :func:`extract`.
    ``shape``: the true (H, W); ``grid``: the geometry; ``rounds``: int [R, C], the complete rounds ``data`` holds of every
    tile, -1 where the tile is absent; ``scheduled`` and ``stages``: whether the picture is scheduled and
    its L, else False and 0.  Every :meth:`decode` decodes the tiles of its window afresh, ``group`` at a time
    through ``embedded.EmbeddedDecoder`` (``coder`` is its), and blends them with one vam_tile_blend launch.

    ``partial=True``: any prefix that holds the header is accepted; ``rounds`` is then -1 also for a tile
    whose head is not whole, ``meta`` is None while no head is, and :meth:`decode` names such a tile when its window needs
    it.  :meth:`compose` fills what is not available from a coarser picture."""

    def __init__(self, model, data, coder: Optional[str] = None, group: Optional[int] = None, partial: bool = False):
        from . import progressive as P
        EB._check_model(model)
        d, s = _parse(data, "PictureDecoder")
        if not partial and len(d) < s.need:
            raise ValueError(f"PictureDecoder: {len(d)} bytes end before the heads of the tiles do: {s.need} bytes are needed, every "
                             "tile's z and base are decoded whole")
        self.meta = _tile_meta(d, s, "PictureDecoder")
        self.m, self.coder, self._d, self._s = model, P._check_coder(model, coder), bytes(d), s
        self.grid, self.shape = dict(s.g), (s.g["H"], s.g["W"])
        self.scheduled, self.stages = s.stages > 0, s.stages                     # version 3: rounds are stages
        self.group = _check_group(group, s.g["th"], s.g["tw"], "PictureDecoder")
        self.rounds = _tile_rounds(s, len(d))                                    # from need_bytes on every present tile's head is whole
        self.partial = bool(partial)
        self.last_tiles: List[Tuple[int, int]] = []
        self.last_decoded: List[Tuple[int, int]] = []
        self._ramps = None

    def _ramps_at(self, dev):
        self._ramps = _ramps_on(self._ramps, self.grid["V"], dev)
        return self._ramps

    def _level(self, what: str, q, mark, stage) -> Tuple[Optional[int], Optional[int]]:
        return _level_of(what, self.stages, self.meta, self._s.thresholds, q, mark, stage)

    def available(self, window=None, mark: Optional[int] = None, stage: Optional[int] = None) -> List[Tuple[int, int]]:
        """Those of ``tiles_for(window)`` that are available: present, the head whole and, at ``mark`` or ``stage`` m, the
        rounds 0 .. m whole."""
        mark, stage = self._level("PictureDecoder.available", None, mark, stage)
        tiles = tiles_for(self.grid, _window(self.grid, window, "PictureDecoder.available"))
        return _available(self.rounds, tiles, stage if stage is not None else mark)

    def compose(self, window, below, below_window, shift, mark: Optional[int] = None, stage: Optional[int] = None, dtype=None):
        """The window like :meth:`decode` (everything held, a ``mark`` or a ``stage``; no ``q``: whether a tile's bytes reach
        a quality is only known by decoding it), from the AVAILABLE tiles alone (:meth:`available`; ``last_tiles``, which are
        also ``last_decoded``): a pixel all of whose tiles are available is :meth:`decode`'s, bit for bit; any other is the
        upsample by 2^``shift`` of ``below``, fp32 [3, hb, wb] on the device, the window ``below_window`` of the same picture
        ``shift`` levels coarser, which must cover ``pyramid.source_window(window, shift, ...)``.  One vam_tile_compose launch.
        ``below`` = None: nothing stands in, and a tile that is not available is a ValueError that names it."""
        import torch
        what = "PictureDecoder.compose"
        g, s = self.grid, self._s
        dtype = _check_dtype(what, dtype)
        mark, stage = self._level(what, None, mark, stage)
        level = stage if stage is not None else mark
        window = _window(g, window, what)
        wanted = tiles_for(g, window)
        tiles = _available(self.rounds, wanted, level)
        if below is None and len(tiles) < len(wanted):
            rc = next(rc for rc in wanted if rc not in tiles)
            raise _not_available(what, s, window, rc, max(0, s.need - len(self._d)), level, self.rounds)
        buf = slot = None
        if tiles:
            with torch.no_grad():
                buf = _decode_window(what, self.m, self.coder, s.thresholds, tiles, lambda r, c: s.stream(self._d, r * g["C"] + c),
                                     self.group, g, None, mark, stage)
            slot = _slot_table(g, tiles)
        out = _blend_out(what, g, window, buf, slot, self._ramps_at, dtype, below, below_window, shift)
        self.last_tiles = self.last_decoded = tiles
        return out

    def decode(self, window=None, q: Optional[float] = None, mark: Optional[int] = None, stage: Optional[int] = None, dtype=None):
        """The window (y0, x0, h, w) of the picture (None: all of it): fp32 [3, h, w], or uint8 [h, w, 3] for
        ``dtype=torch.uint8`` (round half to even of clamp(v, 0, 1) * 255, as evaluate.write_image).  ``q`` = None: from
        everything ``data`` holds of every tile (``EmbeddedDecoder.decode``); a quality: ``decode_qualities([q])``, every tile
        at its own quantile.  Only ``tiles_for(window)`` are decoded (``last_tiles``).  ValueError names the tile (r, c) that
        the window needs and the codestream lacks, or whose bytes end before ``q``.

        ``mark`` = k (exclusive with ``q``): every tile at the counts its own header states for mark k
        (``EmbeddedDecoder.decode_marks``), for both versions.  On a version-2 stream (picture-wide marks)
        every decoded tile is also checked: its own sigma against the header's thresholds must reproduce its marks' counts,
        else a ValueError names tile, mark and slice; and ``q`` is accepted only when it is a marked quality and then means
        that mark: any other q is a ValueError that lists the marks.

        ``stage`` = k (exclusive with ``q`` and ``mark``; scheduled pictures): every tile at stage k of its
        own schedule (``EmbeddedDecoder.decode_stages([k])``), the blend of ``forward_quality_map(tile, S_tile[k])``; a tile
        whose bytes end before stage k is named.  On a scheduled picture ``mark=k`` gives the same pixels and ``q`` is a
        ValueError that points here; on a plain picture ``stage`` is a ValueError."""
        import torch
        what = "PictureDecoder.decode"
        g, s = self.grid, self._s
        dtype = _check_dtype(what, dtype)
        if self.partial and len(self._d) < s.need:          # a prefix that ends inside the heads: the tiles the window needs must be whole
            win = _window(g, window, "PictureDecoder.decode")
            for r, c in tiles_for(g, win):
                if s.present[r * g["C"] + c] and self.rounds[r, c] < 0:
                    raise ValueError(f"PictureDecoder.decode: the window {win} needs tile ({r}, {c}), whose head has not arrived: "
                                     f"{s.need - len(self._d)} bytes are missing before every tile's head is whole")
        mark, stage = self._level(what, q, mark, stage)       # no head is whole (a partial prefix): the tiles are refused below
        y0, x0, h, w = _window(g, window, what)
        tiles = tiles_for(g, (y0, x0, h, w))
        for r, c in tiles:
            if not s.present[r * g["C"] + c]:
                raise ValueError(f"PictureDecoder.decode: the window ({y0}, {x0}, {h}, {w}) needs tile ({r}, {c}), which is absent "
                                 "from this codestream")
        with torch.no_grad():
            buf = _decode_window(what, self.m, self.coder, s.thresholds, tiles, lambda r, c: s.stream(self._d, r * g["C"] + c),
                                 self.group, g, q, mark, stage)
        out = _blend_out(what, g, (y0, x0, h, w), buf, _slot_table(g, tiles), self._ramps_at, dtype)
        self.last_tiles = tiles
        return out


# ------------------------------------------------------------------------------------- the receiver
class PictureFeed:
    """The byte bookkeeping of a receiver: a picture codestream, whole or an :func:`extract`, of any
    header version, arriving in chunks that may end anywhere.  Host arithmetic only: it needs no model and no GPU.
    :class:`PictureStream` owns one and adds the decoder.

    ``ready``: whether the bytes reach :func:`need_bytes` (every present tile's head).  ``need()``: the bytes still missing
    before that, as far as the bytes tell.  Once the header is complete (it is parsed once, by the parser of
    :func:`layout`): ``shape``, ``grid``, ``scheduled``, ``stages``; ``meta``: the tiles' own layout as far as heads are
    whole (``PictureDecoder.meta`` once ready); and once ready ``rounds`` (``PictureDecoder.rounds``) and ``held`` int [R, C],
    the bytes present of each tile's own codestream, -1 where the tile is absent.  Per tile, from the header on:
    ``tile_ready`` bool [R, C] and ``tile_rounds`` int [R, C].  ``fed_tiles``: the (r, c), in raster order, whose held bytes
    grew in the last feed.  ``data``: everything fed so far.  ``facts``, ``mark()`` and ``rewind(mark)``: what
    ``pyramid.PyramidFeed`` asks of a level's receiver besides."""

    def __init__(self, what: str = "PictureFeed"):
        self._what = what
        self._buf = bytearray()
        self._s: Optional[_Picture] = None
        self._heads = 0                                     # the whole heads that were checked against the table
        self._per_tile = None                               # int64 [R C]: bytes of every tile's stream, absent tiles 0
        self.meta: Optional[dict] = None
        self.fed_tiles: List[Tuple[int, int]] = []

    @property
    def data(self) -> bytes:
        return bytes(self._buf)

    def __len__(self) -> int:
        return len(self._buf)

    @property
    def ready(self) -> bool:
        return self._s is not None and len(self._buf) >= self._s.need

    def need(self) -> int:
        if self._s is not None:
            return max(0, self._s.need - len(self._buf))
        return FRAME.need_header(self._buf, self._what) - len(self._buf)

    def _header(self, name: str):
        if self._s is None:
            raise ValueError(f"{self._what}.{name}: the header is not complete yet: {self.need()} bytes are missing")
        return self._s

    @property
    def grid(self) -> dict:
        return dict(self._header("grid").g)

    @property
    def shape(self) -> Tuple[int, int]:
        g = self._header("shape").g
        return g["H"], g["W"]

    @property
    def stages(self) -> int:
        return self._header("stages").stages

    @property
    def scheduled(self) -> bool:
        return self._header("scheduled").stages > 0

    @property
    def held(self) -> Optional[np.ndarray]:
        if not self.ready:
            return None
        s = self._s
        return np.where(s.present, self._per_tile, -1).reshape(s.g["R"], s.g["C"])

    @property
    def rounds(self) -> Optional[np.ndarray]:
        if not self.ready:
            return None
        s = self._s
        whole = (s.held(len(self._buf))[1:] == s.size[1:])                       # as PictureDecoder: a piece of 0 bytes is whole
        done = np.cumprod(whole, axis=0).sum(0) if s.nr else np.zeros(s.present.size, dtype=np.int64)
        return np.where(s.present, done, -1).astype(np.int64).reshape(s.g["R"], s.g["C"])

    @property
    def tile_rounds(self) -> Optional[np.ndarray]:
        """int [R, C] once the header is complete (None before): the complete rounds held of every tile, -1 where the tile
        is absent or its head is not whole yet.  Once ``ready`` it is ``rounds``."""
        return None if self._s is None else _tile_rounds(self._s, len(self._buf))

    @property
    def tile_ready(self) -> Optional[np.ndarray]:
        """bool [R, C] once the header is complete (None before): the tile is present and its head is whole in the bytes
        held, so it decodes."""
        return None if self._s is None else self.tile_rounds >= 0

    def tile_bytes(self, r: int, c: int) -> bytes:
        """Tile (r, c)'s embedded codestream as far as the fed bytes hold it (:func:`tile_stream`)."""
        s = self._header("tile_bytes")
        return s.stream(self._buf, s.index(r, c, f"{self._what}.tile_bytes"))

    def feed(self, chunk) -> Optional[np.ndarray]:
        """``chunk``: the bytes that follow what was fed before, ``b""`` allowed.  Returns ``rounds`` once ready, else None.
        The feed is checked as a whole before anything is kept: a damaged or contradicting header, a tile head that
        contradicts the table or the other tiles, bytes beyond the header's total and a non-bytes argument are ValueErrors
        that leave the receiver as it was."""
        what = f"{self._what}.feed"
        chunk = bytes(chunk_view(chunk, what))
        s, heads, meta, n = self._s, self._heads, self.meta, len(self._buf) + len(chunk)
        if s is None or heads < int(s.present.sum()):                             # the header or a head may complete: look at the bytes
            d = memoryview(bytes(self._buf) + chunk)
            if s is None and FRAME.whole(d, what):
                s = _Picture(d, what)
            if s is not None:
                whole = int((s.present & (s.off[0] + s.size[0] <= n)).sum())
                if whole != heads:
                    meta, heads = _tile_meta(d, s, what), whole
        if s is not None:
            check_total(n, s.total, what)
        self._buf += chunk
        self._s, self._heads, self.meta = s, heads, meta
        self.fed_tiles = []
        if s is not None:
            per_tile = s.held(n).sum(0)
            before = self._per_tile if self._per_tile is not None else np.zeros_like(per_tile)
            self.fed_tiles = [s.rc(int(i)) for i in np.flatnonzero(per_tile > before)]
            self._per_tile = per_tile
        return self.rounds

    @property
    def facts(self) -> Optional[dict]:
        """Once the header is complete (None before): the geometry of :func:`grid` with ``total``, ``allocation`` and
        ``stages`` as :func:`layout` names them; with ``meta``, what vampic.pyramid checks its levels on."""
        return None if self._s is None else self._s.facts()

    def mark(self):
        """What :meth:`rewind` needs to undo the feeds that follow: vampic.pyramid feeds one receiver per level and refuses
        a chunk as a whole."""
        return len(self._buf), self._s, self._heads, self._per_tile, self.meta, self.fed_tiles

    def rewind(self, mark):
        n, self._s, self._heads, self._per_tile, self.meta, self.fed_tiles = mark
        del self._buf[n:]


class PictureStream:
    """A receiver of one picture codestream that is fed bytes and caches decoded tiles.

    :meth:`feed` takes the bytes that follow what was fed before (:class:`PictureFeed`, which it owns as ``feed_state``; its
    attributes ``ready``, ``need()``, ``shape``, ``grid``, ``scheduled``, ``stages``, ``meta``, ``rounds``, ``held`` and
    ``fed_tiles`` are this object's, too).  After any sequence of feeds and views, ``view(window, q, mark, stage, dtype)``
    equals, bit for bit, ``PictureDecoder(model, everything fed so far, coder, group).decode(window, q, mark, stage, dtype)``
    and raises that call's ValueErrors, but it runs through the network only the tiles it has not cached: an image decodes
    bit for bit the same alone or in a batch (DESIGN sections 9r, 9v), so a tile decoded earlier, in another group, holds
    the pixels a fresh decode would give.

    The cache is a device pool fp32 [cache_tiles, 3, th, tw], allocated at the first view on the model's device: 12 th tw
    bytes per tile.  Default ``cache_tiles``: the most tiles a 1024 x 1024 window can meet at the stream's geometry, at least
    ``group``; at 256 x 256 tiles with overlap 32 that is 36 tiles, 27 MiB.  An entry is (tile, key, generation).  With q, mark
    and stage all None the key is ("held", the bytes held of that tile): the tile is stale exactly when its own bytes grew,
    and a round piece of 0 bytes leaves it fresh.  With a level the key is ("q", q), ("mark", k) or ("stage", k): a tile's
    pixels at a level do not depend on later bytes, so such an entry never goes stale.  Keys of one tile coexist.  Eviction
    is least recently used and never takes a tile of the current call; a window of more tiles than ``cache_tiles`` is a
    ValueError before any GPU work.  A decode that raises leaves the cache as it was.  ``last_tiles``: the tiles of the last
    view's window; ``last_decoded``: those that ran the network; ``decoded_total``: the running count.  :meth:`drop` empties
    the cache."""

    def __init__(self, model, coder: Optional[str] = None, group: Optional[int] = None, cache_tiles: Optional[int] = None,
                 feed_state=None):
        """``feed_state``: the byte bookkeeping, by default a new :class:`PictureFeed`.  Anything else keeps the bytes its own
        way (``vampic.session`` holds them by tile) and gives what the cache and the views read of a ``PictureFeed``: ``_s``,
        ``meta``, ``ready``, ``need()``, ``tile_rounds``, ``_per_tile`` and ``tile_bytes``; it is then filled from outside, not
        through :meth:`feed`."""
        from . import progressive as P
        EB._check_model(model)
        self.m, self.coder = model, P._check_coder(model, coder)
        self._group_arg = None if group is None else _check_group(group, 64, 64, "PictureStream")
        if cache_tiles is not None:
            cache_tiles = _int(cache_tiles, "PictureStream: cache_tiles")
            if cache_tiles < 1:
                raise ValueError(f"PictureStream: cache_tiles is the tiles the cache holds, >= 1, got {cache_tiles}")
        self._cache_arg = cache_tiles
        self.feed_state = PictureFeed("PictureStream") if feed_state is None else feed_state
        self.group: Optional[int] = None
        self.cache_tiles: Optional[int] = None
        self.last_tiles: List[Tuple[int, int]] = []
        self.last_decoded: List[Tuple[int, int]] = []
        self.decoded_total = 0
        self._pool = None
        self._ramps = None
        self._entries = {}                                  # (tile index, key) -> [slot, generation], least recently used first
        self._free: List[int] = []
        self._held_key = {}                                 # tile index -> the ("held", n) key it is cached under
        self._generation = 0
        self._sized()

    # ------------------------------------------------------------------------------------------------------ the bytes
    ready = property(lambda self: self.feed_state.ready)
    shape = property(lambda self: self.feed_state.shape)
    grid = property(lambda self: self.feed_state.grid)
    scheduled = property(lambda self: self.feed_state.scheduled)
    stages = property(lambda self: self.feed_state.stages)
    meta = property(lambda self: self.feed_state.meta)
    rounds = property(lambda self: self.feed_state.rounds)
    held = property(lambda self: self.feed_state.held)
    tile_ready = property(lambda self: self.feed_state.tile_ready)
    tile_rounds = property(lambda self: self.feed_state.tile_rounds)
    fed_tiles = property(lambda self: self.feed_state.fed_tiles)
    data = property(lambda self: self.feed_state.data)
    facts = property(lambda self: self.feed_state.facts)

    def need(self) -> int:
        return self.feed_state.need()

    def mark(self):
        return self.feed_state.mark()

    def rewind(self, mark):
        """:meth:`PictureFeed.rewind`; when the header went with the bytes, the stream's geometry is open again."""
        self.feed_state.rewind(mark)
        if self.feed_state._s is None:
            self.group = self.cache_tiles = None

    def feed(self, chunk) -> Optional[np.ndarray]:
        """:meth:`PictureFeed.feed`: host arithmetic only, it touches no GPU and no cache entry (a stale tile is found by
        its key at the next view)."""
        out = self.feed_state.feed(chunk)
        self._sized()
        return out

    def _sized(self):
        """``group`` and ``cache_tiles`` for the stream's geometry, once the header is complete."""
        if self.group is None and self.feed_state._s is not None:
            g = self.feed_state._s.g
            self.group = self._group_arg if self._group_arg is not None else _default_group(g["th"], g["tw"])
            span = lambda n, t, S, N: min(N, (min(1024, n) + t - 2) // S + 1)     # the most tiles a span of 1024 meets along an axis
            self.cache_tiles = self._cache_arg if self._cache_arg is not None else \
                max(self.group, span(g["H"], g["th"], g["Sy"], g["R"]) * span(g["W"], g["tw"], g["Sx"], g["C"]))

    # ------------------------------------------------------------------------------------------------------ the cache
    def drop(self):
        """Empties the cache; the pool stays allocated."""
        self._entries, self._held_key = {}, {}
        self._free = list(range(self.cache_tiles)) if self._pool is not None else []

    def _update(self, what: str, window, q, mark, stage, below=False):
        """Brings the tiles of ``window`` into the cache at the level (q, mark, stage).  Returns (window, its tiles, the level
        key or None, slot int32 [R, C], generation int64 [R, C]); both tables are -1 outside the window's tiles.  ``below``
        (:meth:`compose`; None: nothing stands in): the header suffices, and its tiles are the AVAILABLE ones of the window."""
        import torch
        fs = self.feed_state
        partial = below is not False
        if partial and fs._s is None:
            raise ValueError(f"{what}: nothing to decode yet: the header is not complete, {fs.need()} bytes are missing")
        if not partial and not fs.ready:
            raise ValueError(f"{what}: nothing to decode yet: {fs.need()} bytes are missing before every tile's head is whole")
        s, g = fs._s, fs._s.g
        mark, stage = _level_of(what, s.stages, fs.meta, s.thresholds, q, mark, stage)
        y0, x0, h, w = _window(g, window, what)
        tiles = tiles_for(g, (y0, x0, h, w))
        if partial:
            rounds, wanted, m = fs.tile_rounds, tiles, stage if stage is not None else mark
            tiles = _available(rounds, wanted, m)
            if below is None and len(tiles) < len(wanted):
                raise _not_available(what, s, (y0, x0, h, w), next(rc for rc in wanted if rc not in tiles), fs.need(), m, rounds)
        for r, c in tiles:
            if not s.present[r * g["C"] + c]:
                raise ValueError(f"{what}: the window ({y0}, {x0}, {h}, {w}) needs tile ({r}, {c}), which is absent "
                                 "from this codestream")
        if len(tiles) > self.cache_tiles:
            raise ValueError(f"{what}: the window ({y0}, {x0}, {h}, {w}) needs {len(tiles)} tiles, the cache holds {self.cache_tiles}: "
                             "give PictureStream a larger cache_tiles or view a smaller window")
        level = ("stage", stage) if stage is not None else ("mark", mark) if mark is not None else ("q", float(q)) if q is not None \
            else None
        index = [r * g["C"] + c for r, c in tiles]
        keys = [(i, level if level is not None else ("held", int(fs._per_tile[i]))) for i in index]
        missing = [(rc, k) for rc, k in zip(tiles, keys) if k not in self._entries]
        if missing:
            part = [rc for rc, _ in missing]
            with torch.no_grad():                           # everything is decoded before the cache changes
                fresh = _decode_window(what, self.m, self.coder, s.thresholds, part, fs.tile_bytes, self.group, g, q, mark, stage)
                if self._pool is None:
                    self._pool = torch.empty((self.cache_tiles, 3, g["th"], g["tw"]), dtype=torch.float32, device=fresh.device)
                    self._free = list(range(self.cache_tiles))
                slots = []
                for _, k in missing:
                    if level is None and self._held_key.get(k[0]) in self._entries:       # the tile's bytes grew: its entry is stale
                        self._free.append(self._entries.pop(self._held_key[k[0]])[0])
                    if not self._free:
                        now = set(keys)
                        old = next(e for e in self._entries if e not in now)              # the least recently used, never a tile of this call
                        if self._held_key.get(old[0]) == old:
                            del self._held_key[old[0]]
                        self._free.append(self._entries.pop(old)[0])
                    self._generation += 1
                    slots.append(self._free.pop())
                    self._entries[k] = [slots[-1], self._generation]
                    if level is None:
                        self._held_key[k[0]] = k
                self._pool.index_copy_(0, torch.tensor(slots, dtype=torch.int64, device=fresh.device), fresh)
        slot = np.full((g["R"], g["C"]), -1, dtype=np.int32)
        gen = np.full((g["R"], g["C"]), -1, dtype=np.int64)
        for (r, c), k in zip(tiles, keys):
            e = self._entries.pop(k)
            self._entries[k] = e                            # the most recently used last
            slot[r, c], gen[r, c] = e
        self.last_tiles, self.last_decoded = tiles, [rc for rc, _ in missing]
        self.decoded_total += len(missing)
        return (y0, x0, h, w), tiles, level, slot, gen

    def _ramps_at(self, dev):
        self._ramps = _ramps_on(self._ramps, self.feed_state._s.g["V"], dev)
        return self._ramps

    def view(self, window=None, q: Optional[float] = None, mark: Optional[int] = None, stage: Optional[int] = None, dtype=None):
        """``PictureDecoder(model, everything fed so far).decode(window, q, mark, stage, dtype)``, bit for bit, with its
        ValueErrors under the prefix ``PictureStream.view:``; only the tiles of the window that are not cached at that level
        run the network (``last_decoded``).  Before ``ready`` a ValueError states ``need()``."""
        what = "PictureStream.view"
        dtype = _check_dtype(what, dtype)
        window, _, _, slot, _ = self._update(what, window, q, mark, stage)
        return _blend_out(what, self.feed_state._s.g, window, self._pool, slot, self._ramps_at, dtype)

    def available(self, window=None, mark: Optional[int] = None, stage: Optional[int] = None) -> List[Tuple[int, int]]:
        """``PictureDecoder(model, everything fed so far, partial=True).available(window, mark, stage)``; [] before the header
        is complete."""
        fs, what = self.feed_state, "PictureStream.available"
        if fs._s is None:
            return []
        s = fs._s
        mark, stage = _level_of(what, s.stages, fs.meta, s.thresholds, None, mark, stage)
        return _available(fs.tile_rounds, tiles_for(s.g, _window(s.g, window, what)), stage if stage is not None else mark)

    def compose(self, window, below, below_window, shift, mark: Optional[int] = None, stage: Optional[int] = None, dtype=None):
        """``PictureDecoder(model, everything fed so far, partial=True).compose(...)``, bit for bit, from
        the header on: the available tiles of the window come from the cache (``last_tiles``), only those not cached at that
        level run the network (``last_decoded``), and one vam_tile_compose launch fills the rest from ``below``.  The cache's
        keys, eviction and ``cache_tiles`` refusal are :meth:`view`'s."""
        what = "PictureStream.compose"
        dtype = _check_dtype(what, dtype)
        window, tiles, _, slot, _ = self._update(what, window, None, mark, stage, below)
        return _blend_out(what, self.feed_state._s.g, window, self._pool if tiles else None, slot if tiles else None, self._ramps_at, dtype,
                          below, below_window, shift)

    def canvas(self, window=None, dtype=None) -> "Canvas":
        """A persistent output of ``window`` (None: the picture) that :meth:`Canvas.refresh` keeps equal to :meth:`view`."""
        return Canvas(self, window, dtype)


class Canvas:
    """A persistent output tensor of one window of a :class:`PictureStream`: ``out`` is fp32 [3, h, w], or
    uint8 [h, w, 3] for ``dtype=torch.uint8``, on the model's device.  Per tile of the grid it remembers the generation of the
    cache entry it last blended from, and the level (q, mark or stage) of its last :meth:`refresh`."""

    def __init__(self, stream: PictureStream, window=None, dtype=None):
        import torch
        what = "PictureStream.canvas"
        fs = stream.feed_state
        if fs._s is None:
            raise ValueError(f"{what}: the header is not complete yet: {fs.need()} bytes are missing")
        dtype = _check_dtype(what, dtype)
        g = fs._s.g
        self.stream, self.window, self.dtype = stream, _window(g, window, what), dtype
        dev, (_, _, h, w) = next(stream.m.parameters()).device, self.window
        self.out = torch.zeros((3, h, w), dtype=torch.float32, device=dev) if dtype == torch.float32 \
            else torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
        self._gen = np.full((g["R"], g["C"]), -1, dtype=np.int64)
        self._level = None

    def refresh(self, q: Optional[float] = None, mark: Optional[int] = None, stage: Optional[int] = None):
        """Brings the window's tiles up to date through the cache, as :meth:`PictureStream.view` does, and re-blends, with one
        vam_tile_refresh launch, only the pixels that a dirty tile contributes to: a tile is dirty when its cache entry is
        not the one this canvas last blended from, and every tile of the window is when the level changed.  Returns the box
        (y0, x0, h, w), in picture coordinates, that was visited: the bounding box of the dirty tiles' extents inside the
        window; None when nothing was dirty, and then nothing is launched.  Afterwards ``out`` equals
        ``view(window, q, mark, stage, dtype)`` of the same moment, bit for bit."""
        what = "Canvas.refresh"
        st = self.stream
        (cy0, cx0, ch, cw), tiles, level, slot, gen = st._update(what, self.window, q, mark, stage)
        g = st.feed_state._s.g
        if level != self._level:
            self._gen[:] = -1
        dirty = np.zeros(gen.shape, dtype=np.int32)
        for r, c in tiles:
            dirty[r, c] = gen[r, c] != self._gen[r, c]
        if not dirty.any():
            return None
        rows, cols = np.flatnonzero(dirty.any(1)), np.flatnonzero(dirty.any(0))
        y0, y1 = max(cy0, int(rows[0]) * g["Sy"]), min(cy0 + ch, int(rows[-1]) * g["Sy"] + g["th"])
        x0, x1 = max(cx0, int(cols[0]) * g["Sx"]), min(cx0 + cw, int(cols[-1]) * g["Sx"] + g["tw"])
        box = (y0, x0, y1 - y0, x1 - x0)
        _blend_out(what, g, self.window, st._pool, slot, st._ramps_at, self.dtype, dirty=dirty, box=box, out=self.out)
        for r, c in tiles:
            self._gen[r, c] = gen[r, c]
        self._level = level
        return box
