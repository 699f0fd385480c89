"""Viewing sessions: a server that sends, request after request, only what the receiver lacks of one
pyramid codestream, and a receiver that takes bytes by TILE instead of by position and keeps its cache of decoded tiles from
viewport to viewport.  ``pyramid.extract_viewport`` cuts a self-contained stream per viewport and repeats every header and
round the receiver holds; ``Server.viewport`` of the same request sends the difference.

The ledger says what a receiver holds: a dict, level -> int16 [R_k, C_k] of SEGMENTS held: 0 nothing, 1 the head, 1 + j the
head and the rounds 0 .. j - 1, whole.  A tile's segments are a run from the head on, without gaps; a level that the
server's data lacks is no key.  ``Server.have`` (what was sent) and ``Receiver.have`` agree entry for entry after every
merged message.

An increment message: ``framing.PREAMBLE`` with magic ``b"VAMi"`` (version 1), a little-endian header (u32 tag; u16 flags, bit
0: the picture's headers are in the body, every other bit 0; u16 reserved (0); u32 n_records; n_records x (u16 level, r, c,
first, count); u64 total) under a CRC-32, then the body.  The records are canonical: the coarsest level first, raster order
within a level, at most one record per tile, ``count >= 1``.  With the flag the body begins with a u32 length and the
server's pyramid header (``data[:header_end]``) and every present level's WHOLE picture header, preamble included, coarsest
first: the full tables, not an extract's.  Then every record's segments ``first .. first + count - 1``, concatenated; their
sizes are those of the level's table row, so the body carries no lengths.  ``tag`` is the CRC-32 of the header bytes as
carried, the pyramid header and then the level headers.  Equal requests against equal ledgers give equal bytes.  A reader
trusts nothing: a damaged preamble or header, a short message (the error states the bytes missing), bytes beyond ``total``,
records out of order or doubled and a reserved bit are ValueErrors.

Whatever message a server sends first carries the headers: a request's, or that of ``Server.open()``, which carries nothing
else, so that an opened session pays for the headers once and every request's message is records and segments alone.

:class:`Server` and :class:`Receiver` are host arithmetic and need neither a model nor a GPU.  :class:`Client` is a receiver
with the views of ``pyramid.PyramidStream``: one ``tiled.PictureStream`` per level over the receiver's bytes, so the tile
cache, its keys and the kernels are that class's.  ``Receiver.snapshot(rounds)`` writes what is held as an ordinary pyramid
codestream.

Out of scope: transport and the serialisation of requests; feeding an increment in chunks; evicting bytes at the client and
re-synchronising ledgers; several pictures per session; mixing ``feed`` and ``merge`` on one receiver; a decode budget or a
priority order for stale tiles; a persistent or filled resampled canvas; per-tile entropy resumption.
"""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import pyramid as PY
from . import tiled as TL
from .framing import MAX_HEADER, PREAMBLE_BYTES, Frame, as_int, check_total, view

MAGIC = b"VAMi"
VERSION = 1
FLAG_HEADERS = 1                           # bit 0 of the flags: the body begins with the picture's headers
MAX_SEGMENTS = 0x7FFF                      # a ledger entry is an int16
_FIXED = struct.Struct("<IHHI")            # tag, flags, reserved (0), n_records; then the records and the u64 total
_RECORD = struct.Struct("<5H")             # level, r, c, first, count
FRAME = Frame(MAGIC, "an increment", "increment", (VERSION,), range(_FIXED.size + 8, MAX_HEADER + 1, _RECORD.size),
              f"the header of n records takes {_FIXED.size + 8} + {_RECORD.size} n")


def _crc(b) -> int:
    return zlib.crc32(b) & 0xFFFFFFFF


def _seal(tag: int, headers: Optional[bytes], records, parts: List[bytes]) -> bytes:
    """The increment of ``records`` [(level, r, c, first, count)] whose segments are ``parts``; ``headers``: the pyramid
    header and the level headers as the body carries them behind their u32 length, or None."""
    body = ([] if headers is None else [headers]) + parts
    hlen = _FIXED.size + _RECORD.size * len(records) + 8
    if hlen > MAX_HEADER:
        raise ValueError(f"an increment of {len(records)} records would take a header of {hlen} bytes, the limit is {MAX_HEADER}")
    header = _FIXED.pack(tag, 0 if headers is None else FLAG_HEADERS, 0, len(records)) + b"".join(_RECORD.pack(*r) for r in records) \
        + struct.pack("<Q", PREAMBLE_BYTES + hlen + sum(len(b) for b in body))
    return b"".join([FRAME.seal(header)] + body)


class _Message:
    """A parsed increment: ``tag``, ``records`` [(level, r, c, first, count)], ``header_end``, ``total``, ``at`` (where the
    segments begin) and, when the body carries the headers, ``p`` (``pyramid._Pyramid``), ``header`` (level -> its picture
    header's bytes) and ``picture`` (level -> ``tiled._Picture``)."""

    def __init__(self, message, what: str):
        d = view(message, what)
        end = FRAME.need_header(d, what)
        if len(d) < end:
            raise ValueError(f"{what}: {len(d)} bytes do not hold the header of an increment: {end - len(d)} bytes are missing")
        d, _, hlen, end = FRAME.open(d, what)
        tag, flags, zero, n = _FIXED.unpack_from(d, PREAMBLE_BYTES)
        if flags & ~FLAG_HEADERS or zero:
            raise ValueError(f"{what}: the header's flags are {flags:#06x} (reserved field {zero}); this reader knows bit 0, the "
                             "picture's headers, and a reserved field of 0")
        if hlen != _FIXED.size + _RECORD.size * n + 8:
            raise ValueError(f"{what}: the header contradicts itself: {n} records take {_FIXED.size + _RECORD.size * n + 8} bytes, "
                             f"it states {hlen}")
        rec = np.frombuffer(d, dtype="<u2", count=5 * n, offset=PREAMBLE_BYTES + _FIXED.size).astype(np.int64).reshape(n, 5)
        self.records = [tuple(int(v) for v in row) for row in rec]
        self.total = int(np.frombuffer(d, dtype="<u8", count=1, offset=end - 8)[0])
        if self.total < end:
            raise ValueError(f"{what}: the header contradicts itself: it ends at byte {end} and states a total of {self.total}")
        if len(d) < self.total:
            raise ValueError(f"{what}: {len(d)} bytes of an increment of {self.total}: {self.total - len(d)} bytes are missing; a "
                             "message is merged whole")
        check_total(len(d), self.total, what)
        last = None
        for level, r, c, first, count in self.records:
            key = (-level, r, c)
            if last is not None and key <= last:
                raise ValueError(f"{what}: the records are not canonical: level {level}, tile ({r}, {c}) follows level {-last[0]}, tile "
                                 f"({last[1]}, {last[2]}); records go the coarsest level first, in raster order, one per tile")
            if count < 1:
                raise ValueError(f"{what}: the record of level {level}, tile ({r}, {c}) holds {count} segments; a record holds at least 1")
            last = key
        self.d, self.tag, self.header_end, self.at = d, int(tag), end, end
        self.p, self.header, self.picture, self.pyramid_header = None, {}, {}, b""
        if flags & FLAG_HEADERS:
            self._headers(what)

    def _headers(self, what: str):
        d, at = self.d, self.header_end
        if self.total < at + 4:
            raise ValueError(f"{what}: the body ends before the length of the pyramid header does")
        n = struct.unpack_from("<I", d, at)[0]
        first = at = at + 4
        if self.total < at + n:
            raise ValueError(f"{what}: the body ends before the pyramid header of {n} bytes does")
        self.pyramid_header = bytes(d[at:at + n])
        self.p = PY._Pyramid(self.pyramid_header, what)
        if self.p.header_end != n:
            raise ValueError(f"{what}: the body states a pyramid header of {n} bytes, the header itself ends at {self.p.header_end}")
        at += n
        for k in self.p.order:
            rest = d[at:self.total]
            try:
                end = TL.FRAME.need_header(rest, what)
                if len(rest) < end:
                    raise ValueError(f"{what}: the body ends before the picture header does")
                self.picture[k] = TL._Picture(rest[:end], what)
            except ValueError as e:
                raise ValueError(f"{what}: level {k}: {e}") from e
            self.header[k] = bytes(rest[:end])
            at += end
        if _crc(d[first:at]) != self.tag:
            raise ValueError(f"{what}: the tag {self.tag:#010x} is not the CRC-32 of the headers the body carries, {_crc(d[first:at]):#010x}")
        self.at = at


def layout(message) -> dict:
    """What an increment states, from the message alone: ``tag``, ``headers`` (whether the body carries the picture's headers),
    ``records`` [(level, r, c, first, count)], ``header_end``, ``total``, ``header_bytes`` (of the picture's headers in the
    body, their u32 length included) and ``segment_bytes`` (of the records' segments).  Whether the segments are those of the
    records is :meth:`Receiver.merge`'s to check: it takes the tables."""
    m = _Message(message, "layout")
    return {"tag": m.tag, "headers": m.p is not None, "records": list(m.records), "header_end": m.header_end, "total": m.total,
            "header_bytes": m.at - m.header_end, "segment_bytes": m.total - m.at}


def _check_rounds(s, k: int, what: str):
    if 1 + s.nr > MAX_SEGMENTS:
        raise ValueError(f"{what}: level {k} holds {s.nr} rounds; a ledger counts up to {MAX_SEGMENTS} segments of a tile")


# ------------------------------------------------------------------------------------------------------------ the server
class Server:
    """The sending side of a session, host only.  ``data``: a pyramid codestream, whole or a prefix or an extract, that holds
    its header and the picture header of every present level (one level, ``pyramid.encode(levels=1)``, is a plain tiled
    picture).  ``have``: the ledger of what was sent, empty at first.  The first message carries the headers, be it a
    request's or :meth:`open`'s, which carries nothing else; a request that adds nothing gives a valid message of no records."""

    def __init__(self, data):
        what = "Server"
        d, p = PY._parse(data, what)
        PY._layouts(d, p, what)
        d = memoryview(bytes(d))                            # a copy: the session outlives the caller's buffer
        self._d, self._p, self._s, self._held = d, p, {}, {}
        headers = [bytes(d[:p.header_end])]
        for k in p.order:
            part = d[p.off[k]:p.off[k] + p.held(len(d), k)]
            if not TL.FRAME.whole(part, what):
                raise ValueError(f"{what}: the data ends before the picture header of level {k} does; a session opens with every "
                                 "present level's header")
            s = self._s[k] = TL._Picture(part, what)
            _check_rounds(s, k, what)
            self._held[k] = s.held(len(part)) == s.size                          # bool [1 + nr, R C]: the segment is whole in the data
            headers.append(bytes(part[:s.header_end]))
        self._headers = struct.pack("<I", len(headers[0])) + b"".join(headers)
        self.tag = _crc(self._headers[4:])
        self.have: Dict[int, np.ndarray] = {k: np.zeros((s.g["R"], s.g["C"]), dtype=np.int16) for k, s in sorted(self._s.items())}
        self.sent_headers = False

    def _want(self, want: dict, cuts, rounds, what: str):
        """Adds to ``want`` (level -> int [R C], the segments a tile should hold) what ``pyramid.extract`` of every (levels,
        level-0 window) of ``cuts`` keeps at ``rounds``."""
        for levels, window in cuts:
            for k, win in PY._kept(self._p, levels, window, what):
                nr, keep = TL._kept(self._s[k], win, rounds, f"{what}: level {k}")
                want[k] = np.maximum(want.get(k, 0), np.where(keep, 1 + nr, 0))

    def _send(self, want: dict, what: str) -> bytes:
        records, parts = [], []
        for k in self._p.order:
            if k not in want:
                continue
            s, base, have = self._s[k], self._p.off[k], self.have[k].reshape(-1)
            for i in (int(v) for v in np.flatnonzero(want[k] > have)):
                first, end = int(have[i]), int(want[k][i])
                for j in range(first, end):
                    if not self._held[k][j, i]:
                        raise ValueError(f"{what}: level {k}: the data ends before {'the head' if j == 0 else f'round {j - 1}'} (segment "
                                         f"{j}) of tile {s.rc(i)} does; a server sends from bytes that hold what is asked for")
                records.append((k,) + s.rc(i) + (first, end - first))
                parts += [bytes(self._d[base + int(s.off[j, i]):base + int(s.off[j, i] + s.size[j, i])]) for j in range(first, end)]
        message = _seal(self.tag, None if self.sent_headers else self._headers, records, parts)
        for k, r, c, first, count in records:                                    # nothing was kept before the message stood
            self.have[k][r, c] = first + count
        self.sent_headers = True
        return message

    def open(self) -> bytes:
        """The session's opening message: the picture's headers and no record (no record and no headers once they were
        sent).  A session that opens with it pays for the headers once, before the first request, and every request's
        message is then records and segments alone."""
        return self._send({}, "Server.open")

    def window(self, levels=None, window=None, rounds: Optional[int] = None) -> bytes:
        """The increment that brings the receiver what ``pyramid.extract(data, levels, window, rounds)`` holds and ``have``
        lacks; afterwards ``have`` includes it.  ValueError, with ``have`` unchanged, for what ``extract`` refuses and for a
        wanted segment that is not whole in ``data``: it names level, tile and segment."""
        what, want = "Server.window", {}
        self._want(want, [(levels, window)], rounds, what)
        return self._send(want, what)

    def viewport(self, rect, out_hw, unit: int = 1, rounds: Optional[int] = None, thumbnail: bool = True) -> bytes:
        """:meth:`window` for ``pyramid.extract_viewport(data, rect, out_hw, unit, rounds, thumbnail)``: the same level
        (``pyramid.viewport_level``), the same level-0 window and the same thumbnail rule."""
        what, want = "Server.viewport", {}
        self._want(want, PY._viewport_cuts(self._p, rect, out_hw, unit, thumbnail, what), rounds, what)
        return self._send(want, what)


# ---------------------------------------------------------------------------------------------------------- the receiver
class _Level:
    """One level of a :class:`Receiver`: the picture header and, per tile, the segments held and their bytes.  It gives what
    ``tiled.PictureStream`` reads of a ``tiled.PictureFeed`` (``_s``, ``meta``, ``ready``, ``need()``, ``tile_rounds``,
    ``_per_tile``, ``tile_bytes``) and what ``pyramid`` checks its levels on (``facts``).  A level of a session is ``ready`` from
    its header on: tiles come one by one, and a view asks for each tile it needs."""

    ready = True

    def __init__(self, what: str, header: bytes, s):
        self._what, self.header, self._s = what, header, s
        n = s.g["R"] * s.g["C"]
        self.segments = np.zeros(n, dtype=np.int16)
        self._per_tile = np.zeros(n, dtype=np.int64)
        self._tile = [bytearray() for _ in range(n)]
        self._edge = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(s.table, axis=1)], axis=1)
        self.meta: Optional[dict] = None
        self._first: Optional[int] = None                   # the tile whose layout ``meta`` is: the first in raster order
        self.fed_tiles: List[Tuple[int, int]] = []

    def need(self) -> int:
        return 0

    grid = property(lambda self: dict(self._s.g))
    shape = property(lambda self: (self._s.g["H"], self._s.g["W"]))
    stages = property(lambda self: self._s.stages)
    scheduled = property(lambda self: self._s.stages > 0)
    facts = property(lambda self: self._s.facts())
    have = property(lambda self: self.segments.reshape(self._s.g["R"], self._s.g["C"]).copy())

    @property
    def held(self) -> np.ndarray:
        """int [R, C]: the bytes held of each tile's own codestream, -1 where the tile is absent."""
        s = self._s
        return np.where(s.present, self._per_tile, -1).reshape(s.g["R"], s.g["C"])

    @property
    def tile_rounds(self) -> np.ndarray:
        """int [R, C]: the whole rounds held of every tile, -1 where its head is not held."""
        return (self.segments.astype(np.int64) - 1).reshape(self._s.g["R"], self._s.g["C"])

    @property
    def tile_ready(self) -> np.ndarray:
        return self.tile_rounds >= 0

    def tile_bytes(self, r: int, c: int) -> bytes:
        """Tile (r, c)'s embedded codestream as far as it is held: its segments, concatenated."""
        i = self._s.index(r, c, f"{self._what}.tile_bytes")
        if not self.segments[i]:
            raise ValueError(f"{self._what}.tile_bytes: tile ({r}, {c}) holds no bytes: its head has not arrived")
        return bytes(self._tile[i])

    def segment(self, i: int, j: int) -> bytes:
        return bytes(self._tile[i][int(self._edge[i, j]):int(self._edge[i, j + 1])])


class Receiver:
    """The receiving side of a session, host only: the counterpart of ``pyramid.PyramidFeed`` for bytes that arrive by tile.
    ``have``: the ledger.  ``shape``, ``levels``, ``shapes``: the picture's, once the headers have arrived.  ``level(k)``: level
    k's bookkeeping, with ``facts``, ``meta``, ``grid``, ``stages``, ``scheduled``, ``held``, ``tile_rounds``, ``tile_ready``,
    ``tile_bytes(r, c)`` and ``fed_tiles`` as ``tiled.PictureFeed`` names them."""

    def __init__(self, what: str = "Receiver"):
        self._what = what
        self._p = None
        self.tag: Optional[int] = None
        self._header = b""
        self._levels: Dict[int, _Level] = {}

    def _pyramid(self, name: str):
        if self._p is None:
            raise ValueError(f"{self._what}.{name}: the picture's headers have not arrived yet: the first message of a server carries them")
        return self._p

    shape = property(lambda self: (self._pyramid("shape").H, self._pyramid("shape").W))
    levels = property(lambda self: self._pyramid("levels").n)
    shapes = property(lambda self: list(self._pyramid("shapes").shapes))

    @property
    def have(self) -> Dict[int, np.ndarray]:
        return {k: lv.have for k, lv in sorted(self._levels.items())}

    def level(self, k: int) -> _Level:
        p = self._pyramid("level")
        k = p.level(k, f"{self._what}.level")
        if k not in self._levels:
            raise ValueError(f"{self._what}.level: level {k} is absent from this session; it holds the levels {sorted(self._levels)}")
        return self._levels[k]

    def merge(self, message) -> List[Tuple[int, int, int]]:
        """Takes one whole increment and returns the (level, r, c) whose bytes grew, in the order of the records.  The
        message is checked as a whole before anything is kept, and a refused merge leaves the receiver as it was: what
        the module docstring lists of a message alone; records before any headers; a tag that is not the one held (headers
        that come again under the held tag are ignored); a level that the pyramid header calls absent; a tile outside the
        level's grid or absent from its table; ``first`` that is not the segments held (a gap or a repeat); segments beyond
        the level's rounds; a body that is not exactly the records' segments; a head that fails ``tiled``'s checks against the
        table and the other tiles; and level facts that contradict each other (``pyramid``'s check)."""
        what = f"{self._what}.merge"
        m = _Message(message, what)
        p, levels = self._p, self._levels
        if p is None:
            if m.p is None:
                if m.records:
                    raise ValueError(f"{what}: {len(m.records)} records before any headers: the first message of a server carries the "
                                     "picture's headers")
                return []
            p, levels = m.p, {k: _Level(f"{self._what} level {k}", m.header[k], m.picture[k]) for k in m.p.order}
            for k, lv in levels.items():
                _check_rounds(lv._s, k, what)
        elif m.tag != self.tag:
            raise ValueError(f"{what}: the message's tag is {m.tag:#010x}, the headers held have {self.tag:#010x}: it is of another "
                             "picture or another coding of it")
        first = {k: (lv.meta, lv._first) for k, lv in levels.items()}
        at, plan = m.at, []
        for k, r, c, a, count in m.records:
            if k not in levels:
                p.level(k, what)
                raise ValueError(f"{what}: level {k} is absent from this picture; it holds the levels {sorted(levels)}")
            lv = levels[k]
            s = lv._s
            try:
                i = s.index(r, c, what)
            except ValueError as e:
                raise ValueError(f"{what}: level {k}: {e}") from e
            if not s.present[i]:
                raise ValueError(f"{what}: level {k}: tile ({r}, {c}) is absent from this picture (a head of 0 bytes)")
            if a != lv.segments[i]:
                raise ValueError(f"{what}: level {k}, tile ({r}, {c}): the record begins at segment {a}, the tile holds "
                                 f"{int(lv.segments[i])}: {'a gap' if a > lv.segments[i] else 'a repeat'}; a tile's segments are a run from the head on")
            if a + count > 1 + s.nr:
                raise ValueError(f"{what}: level {k}, tile ({r}, {c}): segments {a} .. {a + count - 1}; the level has a head and {s.nr} rounds")
            size = int(s.table[i, a:a + count].sum())
            if at + size > m.total:
                raise ValueError(f"{what}: the body ends before the segments of level {k}, tile ({r}, {c}) do: "
                                 f"{at + size - m.total} bytes are missing")
            piece = bytes(m.d[at:at + size])
            at += size
            if a == 0:
                meta, i0 = first[k]
                lay = TL._check_head(piece[:int(s.table[i, 0])], s, i, meta, None if meta is None else s.rc(i0), f"{what}: level {k}")
                if meta is None or i < i0:
                    first[k] = (lay, i)
            plan.append((k, i, a + count, piece))
        if at != m.total:
            raise ValueError(f"{what}: {m.total - at} bytes follow the segments of the last record")
        PY._check_facts(p, {k: PY._facts(lv.facts, first[k][0]) for k, lv in levels.items()}, what)
        if self._p is None:
            self._p, self._levels, self.tag, self._header = p, levels, m.tag, m.pyramid_header
        grew = []
        for lv in levels.values():
            lv.fed_tiles = []
        for k, i, segments, piece in plan:
            lv = levels[k]
            lv.segments[i] = segments
            lv.meta, lv._first = first[k]
            if piece:
                lv._tile[i] += piece
                lv._per_tile[i] += len(piece)
                lv.fed_tiles.append(lv._s.rc(i))
                grew.append((k,) + lv._s.rc(i))
        return grew

    def snapshot(self, rounds: int) -> bytes:
        """What is held as a pyramid codestream: per level the tiles that hold at least ``rounds`` whole rounds (0: the head),
        each cut to exactly ``rounds`` rounds; other tiles and levels without such a tile are absent.  The picture header's
        version and a version-2 header's thresholds are kept as ``extract`` keeps them.  ValueError when no tile qualifies."""
        what = f"{self._what}.snapshot"
        p = self._pyramid("snapshot")
        nr = as_int(rounds, f"{what}: rounds")
        if nr < 0:
            raise ValueError(f"{what}: rounds is >= 0 (0: the heads alone), got {nr}")
        streams: List[Optional[bytes]] = [None] * p.n
        for k, lv in self._levels.items():
            s = lv._s
            keep = lv.segments >= 1 + nr
            if nr > s.nr or not keep.any():
                continue
            streams[k] = TL._assemble(s.g, np.where(keep[:, None], s.table[:, :1 + nr], 0), lv.segment, s.thresholds, s.stages)
        if not any(streams):
            raise ValueError(f"{what}: no tile holds {nr} whole rounds: the ledger's most is "
                             f"{max([int(lv.segments.max()) - 1 for lv in self._levels.values()], default=-1)}")
        return PY._assemble(p.H, p.W, streams)


# ------------------------------------------------------------------------------------------------------------ the client
class Client(Receiver):
    """A :class:`Receiver` with the views of ``pyramid.PyramidStream``, same signatures, ``last_tiles`` / ``last_decoded`` /
    ``last_chain``: one ``tiled.PictureStream`` per level (``streams[k]``, made when first viewed) over that level's bytes
    here, each with its own cache of ``cache_tiles`` decoded tiles.  A tile is available at mark or stage m when it holds the
    rounds 0 .. m.  The cache keys are ``PictureStream``'s: a level key never goes stale across merges,
    ("held", bytes) does when the tile's bytes grew."""

    def __init__(self, model, coder: Optional[str] = None, group: Optional[int] = None, cache_tiles: Optional[int] = None):
        super().__init__("Client")
        TL.PictureStream(model, coder=coder, group=group, cache_tiles=cache_tiles)      # its checks of the arguments, now
        self._make = lambda lv: TL.PictureStream(model, coder=coder, group=group, cache_tiles=cache_tiles, feed_state=lv)
        self._streams: Dict[int, "TL.PictureStream"] = {}
        self.last_tiles: List[Tuple[int, int]] = []
        self.last_decoded: List[Tuple[int, int]] = []
        self.last_chain: List[Tuple[int, List[Tuple[int, int]], List[Tuple[int, int]]]] = []

    @property
    def streams(self) -> List[Optional["TL.PictureStream"]]:
        return [self._stream(k) if k in self._levels else None for k in range(self._pyramid("streams").n)]

    def _stream(self, k: int) -> "TL.PictureStream":
        if k not in self._streams:
            self._streams[k] = self._make(self._levels[k])
        return self._streams[k]

    def _at(self, what: str, level) -> Tuple[int, "TL.PictureStream"]:
        if self._p is None:
            raise ValueError(f"{what}: nothing to decode yet: the picture's headers have not arrived")
        k = self._p.level(level, what)
        if k not in self._levels:
            raise PY._not_ready(what, k, False, sorted(self._levels))
        return k, self._stream(k)

    def available(self, window=None, level: int = 0, mark: Optional[int] = None, stage: Optional[int] = None) -> List[Tuple[int, int]]:
        """Those of the tiles of ``window`` at ``level`` that are available: the head held and, at ``mark`` or ``stage`` m, the
        rounds 0 .. m."""
        return self._at("Client.available", level)[1].available(window, mark, stage)

    def view(self, window=None, level: int = 0, q: Optional[float] = None, mark: Optional[int] = None, stage: Optional[int] = None,
             dtype=None, fill: bool = False):
        """``PyramidDecoder(model, snapshot).decode(window, level, ...)`` of the snapshot that holds the window's tiles at the
        level asked for, bit for bit; only the tiles not cached at that level run the network.  Without ``fill`` a tile
        of the window that is not available is a ValueError naming it and the rounds it holds; with ``fill=True`` (mark,
        stage or neither) the chain of DESIGN section 9za runs over the levels that have a tile available there, which are the
        levels of ``snapshot(m + 1)``, each giving the tiles it has."""
        what = "Client.view"
        if fill:
            if self._p is None:
                raise ValueError(f"{what}: nothing to decode yet: the picture's headers have not arrived")
            k = self._p.level(level, what)
            m = stage if stage is not None else mark        # what is no mark is refused below; a level counts when a tile of it does
            least = m + 1 if isinstance(m, (int, np.integer)) and not isinstance(m, bool) else 0
            usable = [j for j, lv in sorted(self._levels.items()) if (lv.segments > least).any()]
            out, chain = PY._fill(what, self._p.shapes, usable, self._stream, window, k, q, mark, stage, dtype, 0)
            self.last_tiles, self.last_decoded, self.last_chain = chain[0][1], chain[0][2], chain
            return out
        k, st = self._at(what, level)
        lv = self._levels[k]
        window = TL._window(lv._s.g, window, what)
        have = st.available(window, None if q is not None else mark, None if q is not None else stage)
        for r, c in TL.tiles_for(lv._s.g, window):
            if (r, c) not in have:
                n = int(lv.tile_rounds[r, c])
                m = stage if stage is not None else mark
                raise ValueError(f"{what}: level {k}: the window {window} needs tile ({r}, {c}), which holds "
                                 + ("nothing: its head has not arrived" if n < 0 else f"{n} whole rounds, {m + 1} are needed"))
        out = st.view(window, q=q, mark=mark, stage=stage, dtype=dtype)
        self.last_tiles, self.last_decoded = st.last_tiles, st.last_decoded
        self.last_chain = [(k, list(st.last_tiles), list(st.last_decoded))]
        return out

    def viewport(self, rect, out_hw, unit: int = 1, level: Optional[int] = None, q: Optional[float] = None, mark: Optional[int] = None,
                 stage: Optional[int] = None, dtype=None, fill: bool = False):
        """The viewport ``rect`` / ``unit`` in ``out_hw`` pixels: :meth:`view` of the level's support window,
        then one vam_picture_resample launch."""
        what = "Client.viewport"
        p = self._p
        if p is None:
            raise ValueError(f"{what}: nothing to decode yet: the picture's headers have not arrived")
        rect, out_hw, unit, k, win = PY._viewport_plan(what, rect, out_hw, unit, level, dtype, p.H, p.W, p.n)
        src = self.view(win, k, q=q, mark=mark, stage=stage, dtype=None, fill=fill)
        return PY._resample(src, win, p.shapes[k], k, rect, unit, out_hw, dtype)

    def canvas(self, window=None, level: int = 0, dtype=None) -> "TL.Canvas":
        """``streams[level].canvas(window, dtype)``: a persistent output of that level that ``refresh()`` keeps equal to
        :meth:`view` (vam_tile_refresh)."""
        return self._at("Client.canvas", level)[1].canvas(window, dtype)
