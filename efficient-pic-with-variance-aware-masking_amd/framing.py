"""The framing that the four formats share: embedded (``VAMe``, ``embedded.py``), tiled picture
(``VAMp``, ``tiled.py``) and pyramid (``VAMy``, ``pyramid.py``) codestreams and a viewing session's increment messages (``VAMi``,
``session.py``) all open with one 16-byte preamble, magic,
version, reserved (0), bytes of the header, CRC-32 of the header, then the header and the body.  A :class:`Frame` holds what
differs between formats as data and refuses a preamble that cannot be trusted with one set of messages; the formats keep
their own header fields and body arithmetic.  Host only."""
import struct
import zlib
from typing import Optional, Sequence

import numpy as np

PREAMBLE = struct.Struct("<4sHHII")        # magic, version, reserved (0), bytes of the header, CRC-32 of the header
PREAMBLE_BYTES = PREAMBLE.size             # 16
MAX_HEADER = 1 << 24                       # far above any header: 32 marks of 65535 slices stay below it


def view(data, what: str):
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f"{what}: a codestream is a bytes-like object, got {type(data).__name__}")
    d = memoryview(data)
    return d if d.format == "B" and d.ndim == 1 and d.contiguous else memoryview(bytes(d))


def chunk_view(chunk, what: str):
    """A receiver's chunk as bytes, whatever the item size of a memoryview."""
    if not isinstance(chunk, (bytes, bytearray, memoryview)):
        raise ValueError(f"{what}: expected bytes, got {type(chunk).__name__}")
    return view(chunk, what)


def as_int(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what} is an integer, got {v!r}")
    return int(v)


def same(a, b) -> bool:
    """Equality of container entries: dicts and sequences entry by entry (a list equals a tuple), arrays by value."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def check_total(n: int, total: int, what: str, per_image: bool = False):
    """Refuses ``n`` bytes of a codestream whose header states ``total``.  ``per_image``: the wording of a receiver of several
    codestreams, whose ``what`` names the image."""
    if n > total:
        raise ValueError(f"{what}: {n} bytes, {'its' if per_image else 'the'} header states a total of {total}: "
                         f"{'' if per_image else f'{n - total} '}bytes follow the codestream")


class Frame:
    """One format's framing: its ``magic``, the ``versions`` its reader knows, its name in refusals (``noun`` with its article,
    ``kind`` before the word "version"), the header lengths it may state (``lengths``, a range: the step carries a modulus
    rule) and how a refusal words them (``takes``)."""

    def __init__(self, magic: bytes, noun: str, kind: str, versions: Sequence[int], lengths: range, takes: str):
        self.magic, self.noun, self.kind, self.versions, self.lengths, self.takes = magic, noun, kind, tuple(versions), lengths, takes
        names = [str(v) for v in self.versions]
        self.knows = f"version {names[0]}" if len(names) == 1 else f"versions {', '.join(names[:-1])} and {names[-1]}"

    def seal(self, header: bytes, version: Optional[int] = None) -> bytes:
        """The preamble of ``header`` and the header: magic, ``version`` (None: the first), its length and its CRC-32."""
        return PREAMBLE.pack(self.magic, self.versions[0] if version is None else version, 0, len(header),
                             zlib.crc32(header) & 0xFFFFFFFF) + header

    def header_end(self, d, what: str) -> Optional[int]:
        """The byte at which the header of ``d`` ends, read from its preamble; None while the preamble is incomplete.  A wrong
        magic, version or header length is a ValueError."""
        if len(d) < PREAMBLE_BYTES:
            return None
        magic, version, reserved, hlen, _ = PREAMBLE.unpack_from(d, 0)
        if magic != self.magic:
            raise ValueError(f"{what}: not {self.noun}: it begins with {bytes(magic)!r}, not with the magic {self.magic!r}")
        if version not in self.versions or reserved:
            raise ValueError(f"{what}: {self.kind} version {version}{f' (reserved field {reserved})' if reserved else ''}; this reader "
                             f"knows {self.knows}")
        if hlen not in self.lengths:
            raise ValueError(f"{what}: a header of {hlen} bytes: {self.takes}")
        return PREAMBLE_BYTES + hlen

    def need_header(self, d, what: str) -> int:
        """The bytes at which the header ends as far as ``d`` tells: the preamble's size while that is incomplete."""
        end = self.header_end(d, what)
        return PREAMBLE_BYTES if end is None else end

    def whole(self, d, what: str) -> bool:
        """Whether ``d`` holds the header whole: a receiver's question at every feed until it does."""
        return len(d) >= self.need_header(d, what)

    def open(self, data, what: str):
        """(view, version, stated header bytes, header end) of a codestream that holds its whole header under a matching
        CRC-32; too few bytes are a ValueError with the need."""
        d = view(data, what)
        end = self.need_header(d, what)
        if len(d) < end:
            raise ValueError(f"{what}: {len(d)} bytes do not hold the header: {end} bytes are needed before it can be read")
        version, _, hlen, crc = PREAMBLE.unpack_from(d, 0)[1:]
        if zlib.crc32(d[PREAMBLE_BYTES:end]) & 0xFFFFFFFF != crc:
            raise ValueError(f"{what}: the header's CRC-32 does not match: the first {end} bytes are damaged")
        return d, version, hlen, end
