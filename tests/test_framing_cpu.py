"""The framing that the embedded, picture and pyramid codestreams share (vampic.framing): on the smallest
stream of each kind, the refusals of a preamble that cannot be trusted, word for word, from the entry points and from the
receivers; every prefix up to the header's end; the seal; and receivers that are fed byte by byte or refused.  No model and
no GPU are needed."""
import struct
import zlib

import pytest

from test_embedded_stream_cpu import _Inner, _Model
from test_tiled_cpu import _tile, picture
from vampic import embedded as EB, framing as FR, pyramid as PY, tiled as TL

PRE = 16
_MADE = {}
# per format: its module, the entry point that refuses trailing bytes, and the refusals' wording, written out
KINDS = {
    "embedded": dict(mod=EB, strict=EB.from_bytes, strict_name="from_bytes", magic=b"VAMe", version=1,
                     not_a="not an embedded codestream: it begins with b'XAMe', not with the magic b'VAMe'",
                     v9="codestream version 9; this reader knows version 1",
                     reserved="codestream version 1 (reserved field 256); this reader knows version 1",
                     lengths=[(23, "a header of 23 bytes: a header takes 24 .. 16777216"),
                              (16777217, "a header of 16777217 bytes: a header takes 24 .. 16777216")]),
    "picture": dict(mod=TL, strict=TL.layout, strict_name="layout", magic=b"VAMp", version=1,
                    not_a="not a picture codestream: it begins with b'XAMp', not with the magic b'VAMp'",
                    v9="picture codestream version 9; this reader knows versions 1, 2 and 3",
                    reserved="picture codestream version 1 (reserved field 256); this reader knows versions 1, 2 and 3",
                    lengths=[(31, "a header of 31 bytes: a header takes 32 .. 16777216"),
                             (16777217, "a header of 16777217 bytes: a header takes 32 .. 16777216")]),
    "pyramid": dict(mod=PY, strict=PY.layout, strict_name="layout", magic=b"VAMy", version=1,
                    not_a="not a pyramid codestream: it begins with b'XAMy', not with the magic b'VAMy'",
                    v9="pyramid codestream version 9; this reader knows version 1",
                    reserved="pyramid codestream version 1 (reserved field 256); this reader knows version 1",
                    lengths=[(20, "a header of 20 bytes: the header of n = 1 .. 16 levels takes 20 + 8 n"),
                             (156, "a header of 156 bytes: the header of n = 1 .. 16 levels takes 20 + 8 n"),
                             (32, "a header of 32 bytes: the header of n = 1 .. 16 levels takes 20 + 8 n")]),      # 20 + 8 n for no n
}
RECEIVERS = {"embedded": ["StreamDecoder"], "picture": ["PictureFeed", "PictureStream"], "pyramid": ["PyramidFeed", "PyramidStream"]}
CASES = [(kind, name) for kind, names in RECEIVERS.items() for name in names]


def stream(kind):
    """One 64 x 64 embedded stream, a picture of 1 x 2 tiles, a pyramid of that picture and a level of one tile."""
    if not _MADE:
        pic = picture(H=60, W=100, tile=64, overlap=16)[2]
        _MADE.update(embedded=_tile(1), picture=pic, pyramid=PY.pack(60, 100, [pic, picture(H=30, W=50, tile=64, overlap=16)[2]]))
    return _MADE[kind]


def refused(text, fn, *args):
    with pytest.raises(ValueError) as e:
        fn(*args)
    assert str(e.value) == text


class Receiver:
    """One face for the five receivers: ``feed``, and the state that a refused feed must leave alone."""

    def __init__(self, name):
        self.name = name
        self.r = {"StreamDecoder": lambda: EB.StreamDecoder(_Model(), 1, coder="host"), "PictureFeed": TL.PictureFeed,
                  "PictureStream": lambda: TL.PictureStream(_Model(), coder="host", group=2), "PyramidFeed": PY.PyramidFeed,
                  "PyramidStream": lambda: PY.PyramidStream(_Model(), coder="host", group=2)}[name]()
        self.what = f"{name}.feed: image 0" if name == "StreamDecoder" else f"{name}.feed"

    def feed(self, chunk):
        return self.r.feed([chunk] if self.name == "StreamDecoder" else chunk)

    def state(self):
        r = self.r
        if self.name == "StreamDecoder":
            return r.ready, r.need()[0], bytes(r._buf[0])
        levels = getattr(r, "streams", None) or getattr(r, "receivers", [])
        return r.ready, r.need(), r.data, getattr(r, "group", None), getattr(r, "cache_tiles", None), \
            [None if lv is None else (lv.ready, lv.need(), lv.data, getattr(lv, "group", None), getattr(lv, "cache_tiles", None))
             for lv in levels]


@pytest.fixture
def receiver(monkeypatch):
    monkeypatch.setattr(EB, "_check_model", lambda m: None)
    monkeypatch.setattr(EB, "EmbeddedDecoder", _Inner)
    return Receiver


def _preamble(data, **fields):
    """``data`` with fields of its preamble replaced; the header and its CRC stay."""
    magic, version, reserved, hlen, crc = FR.PREAMBLE.unpack_from(data, 0)
    got = {**dict(magic=magic, version=version, reserved=reserved, hlen=hlen, crc=crc), **fields}
    return struct.pack("<4sHHII", *(got[k] for k in ("magic", "version", "reserved", "hlen", "crc"))) + data[PRE:]


def _damaged(kind):
    """[(a stream with a preamble or header that cannot be trusted, the refusal after ``what: ``)]."""
    k, data = KINDS[kind], stream(kind)
    end = k["mod"].layout(data)["header_end"]
    flipped = data[:end - 3] + bytes([data[end - 3] ^ 0x10]) + data[end - 2:]
    return [(_preamble(data, magic=b"X" + k["magic"][1:]), k["not_a"]), (_preamble(data, version=9), k["v9"]),
            (_preamble(data, reserved=256), k["reserved"])] + [(_preamble(data, hlen=n), text) for n, text in k["lengths"]] \
        + [(flipped, f"the header's CRC-32 does not match: the first {end} bytes are damaged")]


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_preamble_is_the_same_sixteen_bytes_and_seal_writes_it(kind):
    k, data = KINDS[kind], stream(kind)
    lay = k["mod"].layout(data)
    end = lay["header_end"]
    frame = k["mod"].FRAME
    assert FR.PREAMBLE_BYTES == PRE == k["mod"].PREAMBLE_BYTES and lay["total"] == len(data)
    assert struct.unpack_from("<4sHHII", data, 0) == (k["magic"], k["version"], 0, end - PRE, zlib.crc32(data[PRE:end]) & 0xFFFFFFFF)
    assert frame.seal(data[PRE:end], k["version"]) == data[:end] == frame.seal(data[PRE:end])      # the first version by default
    assert frame.header_end(data, "t") == frame.need_header(data[:PRE], "t") == end and frame.header_end(data[:PRE - 1], "t") is None
    d, version, hlen, header_end = frame.open(bytearray(data), "t")
    assert (bytes(d), version, hlen, header_end) == (data, k["version"], end - PRE, end)
    if kind == "embedded":
        assert EB._seal(data[PRE:end]) == data[:end]
    if kind == "picture":                                                       # a later version is sealed by its number
        assert FR.PREAMBLE.unpack_from(frame.seal(b"abc", TL.VERSION_SCHEDULED), 0)[:4] == (b"VAMp", 3, 0, 3)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_entry_points_refuse_a_preamble_that_cannot_be_trusted_word_for_word(kind):
    k = KINDS[kind]
    for bad, text in _damaged(kind):
        for name, fn in (("need_bytes", k["mod"].need_bytes), ("layout", k["mod"].layout), (k["strict_name"], k["strict"])):
            refused(f"{name}: {text}", fn, bad)
    for bad in ("text", None, 5):
        refused(f"need_bytes: a codestream is a bytes-like object, got {type(bad).__name__}", k["mod"].need_bytes, bad)


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_prefix_up_to_the_header_states_its_need_and_a_byte_beyond_the_total_is_refused(kind):
    k, data = KINDS[kind], stream(kind)
    end = k["mod"].layout(data)["header_end"]
    for n in range(end + 1):
        need = PRE if n < PRE else end
        if n < end:
            assert k["mod"].need_bytes(data[:n]) == need
            for name, fn in (("layout", k["mod"].layout), (k["strict_name"], k["strict"])):
                refused(f"{name}: {n} bytes do not hold the header: {need} bytes are needed before it can be read", fn, data[:n])
        else:
            assert k["mod"].need_bytes(data[:n]) > end and k["mod"].layout(data[:n])["header_end"] == end
    refused(f"{k['strict_name']}: {len(data) + 1} bytes, the header states a total of {len(data)}: 1 bytes follow the codestream",
            k["strict"], data + b"\0")
    refused(f"{k['strict_name']}: {len(data) + 8} bytes, the header states a total of {len(data)}: 8 bytes follow the codestream",
            k["strict"], data + b"abcdefgh")


@pytest.mark.parametrize("kind,name", CASES)
def test_a_receiver_fed_byte_by_byte_is_the_receiver_fed_whole(receiver, kind, name):
    data = stream(kind)
    need_bytes = KINDS[kind]["mod"].need_bytes
    whole, single = receiver(name), receiver(name)
    assert whole.state()[:2] == (False, PRE)
    whole.feed(data)
    for n in range(len(data)):
        single.feed(data[n:n + 1])
        assert single.state()[:2] == (n + 1 >= need_bytes(data), max(0, need_bytes(data[:n + 1]) - n - 1))
    assert single.state() == whole.state() and whole.state()[:3] == (True, 0, data)
    for r in (whole, single):                                                   # and neither takes a byte beyond the total
        was = r.state()
        tail = f"{len(data) + 1} bytes, its header states a total of {len(data)}: bytes follow the codestream" if name == "StreamDecoder" \
            else f"{len(data) + 1} bytes, the header states a total of {len(data)}: 1 bytes follow the codestream"
        refused(f"{r.what}: {tail}", r.feed, b"\0")
        assert r.state() == was


@pytest.mark.parametrize("kind,name", CASES)
def test_a_refused_feed_leaves_the_receiver_as_it_was(receiver, kind, name):
    data = stream(kind)
    for bad, text in _damaged(kind):
        at = next(i for i in range(len(data)) if bad[i] != data[i])
        for lo in sorted({0, at // 2, at}):                                     # fed before: bytes that hold nothing damaged
            r = receiver(name)
            r.feed(data[:lo])
            was = r.state()
            refused(f"{r.what}: {text}", r.feed, bad[lo:])
            assert r.state() == was
            if "CRC" not in text:                                               # a preamble is refused as soon as it is whole
                refused(f"{r.what}: {text}", r.feed, bad[lo:PRE])
            r.feed(data[lo:])
            assert r.state()[:3] == (True, 0, data)
    r = receiver(name)
    refused(f"{r.what}: expected bytes, got str", r.feed, "text")
    assert r.state()[:3] == (False, PRE, b"")


@pytest.mark.parametrize("name", RECEIVERS["pyramid"])
def test_a_refused_chunk_that_held_a_level_s_whole_header_takes_it_back(receiver, name):
    """The body holds level 1, then level 0: a chunk whose level 0 is damaged is refused after level 1's receiver took its
    bytes, its header among them, and set its geometry by it."""
    data = stream("pyramid")
    lay = PY.layout(data)
    o0, o1 = lay["levels"][0]["offset"], lay["levels"][1]["offset"]
    bad = data[:o0] + b"X" + data[o0 + 1:]
    level = "PictureStream" if name == "PyramidStream" else "PyramidFeed level 0"
    text = f"{name}.feed: level 0: {level}.feed: not a picture codestream: it begins with b'XAMp', not with the magic b'VAMp'"
    for lo in (0, o1, o1 + 5, o1 + TL.layout(PY.level_stream(data, 1))["header_end"]):    # before the header, at level 1, in and after its header
        r = receiver(name)
        r.feed(data[:lo])
        was = r.state()
        assert lo == 0 or was[5][1][3] == (2 if name == "PyramidStream" and lo > o1 + 5 else None)    # group: open until the level's header
        refused(text, r.feed, bad[lo:])
        assert r.state() == was
        r.feed(data[lo:])
        fresh = receiver(name)
        fresh.feed(data)
        assert r.state() == fresh.state() and r.state()[:3] == (True, 0, data)
        if name == "PyramidStream":
            assert [(s.group, s.cache_tiles) for s in r.r.streams] == [(2, 2), (2, 2)]
