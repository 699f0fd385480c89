"""Embedded codestreams on the host (embedded.to_bytes / need_bytes / layout / from_bytes): hand-made
containers of every format as one byte string, every prefix of it, the round ends against truncate, and the refusals.  No
model and no GPU are needed."""
import struct
import zlib

import numpy as np
import pytest

from vampic import embedded as EB

NS = 3
PRE = EB.PREAMBLE_BYTES
CASES = [(K, Kb, scheduled, L, variant) for K in (1, 8) for Kb in (1, 8) for scheduled in (False, True) for L in (1, 3)
         for variant in ("random", "zeros")]
_MADE = {}


def make(K, Kb, scheduled, L, variant):
    """(container, codestream) of three slices of random bytes with consistent marks, made once.  ``variant`` "zeros": the
    first mark row is all zeros and, with L = 3, the last two marks are one mark twice; "random": increasing rows, slice 0
    ending at its last mark, the others going on after it, slice 1 with an odd length."""
    key = (K, Kb, scheduled, L, variant)
    if key not in _MADE:
        rng = np.random.default_rng(1000 * K + 100 * Kb + 10 * L + 2 * scheduled + (variant == "zeros"))
        lens = [int(v) for v in rng.integers(40, 90, NS)]
        lens[1] |= 1
        rows = np.sort(rng.integers(4, 36, (L, NS)), axis=0) // 4 * 4
        q = [0.5, 2.5, 10.0][:L]
        if variant == "zeros":
            rows[0] = 0
            if L == 3:
                rows[2], q = rows[1], [0.5, 2.5, 2.5]
        else:
            lens[0] = int(rows[-1, 0])
        c = {"format": EB._format_of(K, Kb, scheduled), "shape": (1, 2), "z": [rng.bytes(10 + K)],
             "base": [[rng.bytes(int(n))] for n in rng.integers(5, 30, NS)], "embedded": [rng.bytes(n) for n in lens],
             "marks": {"q": q, "count": [[int(v) for v in row] for row in rows // 2], "bytes": [[int(v) for v in row] for row in rows]}}
        if c["format"] != "embedded-1":
            c["lanes"] = K
        if Kb > 1:
            c["base_lanes"] = Kb
        if scheduled:
            index = np.sort(rng.integers(0, 3, (L, 4, 8)), axis=0).astype(np.uint8)
            c["schedule"], c["side_bytes"] = {"levels": [0.0, 2.5, 10.0], "index": index}, 24 + index.size
            c["marks"]["stage"] = list(range(L))
            del c["marks"]["q"]
        _MADE[key] = (c, EB.to_bytes(c))
    return _MADE[key]


def _marks(c):
    return c["marks"]["stage" if "stage" in c["marks"] else "q"]


def test_the_cases_cover_all_four_formats():
    assert {make(*case)[0]["format"] for case in CASES} == {"embedded-1", "embedded-2", "embedded-3", "embedded-4"}
    assert any("schedule" in make(*case)[0] and make(*case)[0]["format"] == "embedded-4" for case in CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_whole_codestream_is_the_container(case):
    c, data = make(*case)
    back = EB.from_bytes(data)
    assert EB._same(back, c) and EB._same(c, back) and EB._check_container(back) == case[0]
    assert isinstance(data, bytes) and EB.from_bytes(bytearray(data)) is not None and EB._same(EB.from_bytes(memoryview(data)), c)
    lay = EB.layout(data)
    assert lay["total"] == len(data) and lay["base_end"] == lay["header_end"] + sum(EB.container_bytes(c)[:2])
    assert lay["lanes"] == case[0] and lay["base_lanes"] == case[1] and lay["scheduled"] is case[2] and lay["shape"] == (1, 2)
    assert lay["format"] == c["format"] and lay["ns"] == NS and EB._same(lay["marks"], c["marks"]) and len(lay["round_end"]) == case[3]
    assert EB._same(EB.layout(data[:lay["header_end"]]), lay)                # from the header alone
    last = c["marks"]["bytes"][-1]
    if last[1]:                                                                 # a cut below the last mark: no codestream
        cut = EB.truncate(c, slice_bytes=[last[1] - 1 if j == 1 else len(s) for j, s in enumerate(c["embedded"])])
        with pytest.raises(ValueError, match=rf"slice 1 holds {last[1] - 1} bytes, its last mark needs {last[1]}: the container was cut"):
            EB.to_bytes(cut)
    else:                                                                       # the only mark is the base: every cut holds it
        assert EB.layout(EB.to_bytes(EB.truncate(c, slice_bytes=[0] * NS)))["total"] == lay["base_end"]


@pytest.mark.parametrize("case", CASES)
def test_every_prefix(case):
    c, data = make(*case)
    lay = EB.layout(data)
    need, total = lay["base_end"], lay["total"]
    assert EB.need_bytes(data) == need
    full = [len(s) for s in c["embedded"]]
    last, held, first = None, None, None
    for n in range(total + 1):
        if n < need:
            want = PRE if n < PRE else lay["header_end"] if n < lay["header_end"] else need
            assert EB.need_bytes(data[:n]) == want, n
            with pytest.raises(ValueError, match=rf"\b{want} bytes are needed"):
                EB.from_bytes(data[:n])
            continue
        got = EB.from_bytes(data[:n])
        assert EB._check_container(got) == case[0] and EB.need_bytes(data[:n]) == need
        lens = [len(s) for s in got["embedded"]]
        assert all(bytes(s) == bytes(o[:ln]) for s, o, ln in zip(got["embedded"], c["embedded"], lens)), n
        assert sum(lens) == n - need, n
        for key in set(c) - {"embedded"}:
            assert EB._same(got[key], c[key]), (n, key)
        if last is not None:
            assert all(a <= b for a, b in zip(last, lens)) and sum(lens) == sum(last) + 1, n      # one slice gains the byte
            assert sum(len(s) for s in EB.delta(got, held)) == 1
            assert EB.delta(got, first) == got["embedded"]
        else:
            first = got
            assert lens == [0] * NS
        last, held = lens, got
    assert last == full and EB.delta(EB.from_bytes(data), held) == [b""] * NS
    for n1 in range(need, total + 1, 7):                                        # n1 <= n2 at a stride, and the whole
        a = EB.from_bytes(data[:n1])
        for n2 in list(range(n1, total + 1, 13)) + [total]:
            more = EB.delta(EB.from_bytes(data[:n2]), a)
            assert sum(len(s) for s in more) == n2 - n1


@pytest.mark.parametrize("case", CASES)
def test_a_round_end_is_truncate_at_that_mark(case):
    c, data = make(*case)
    lay = EB.layout(data)
    ends = lay["round_end"]
    assert lay["base_end"] <= ends[0] and all(a <= b for a, b in zip(ends, ends[1:])) and ends[-1] <= lay["total"]
    for k, mark in enumerate(_marks(c)):
        want = EB.truncate(c, stage=mark) if case[2] else EB.truncate(c, q=mark)
        assert EB._same(EB.from_bytes(data[:ends[k]]), want), k
        assert ends[k] == lay["base_end"] + sum(c["marks"]["bytes"][k])
    if case[4] == "zeros":
        assert ends[0] == lay["base_end"] and (case[3] == 1 or ends[1] == ends[2])


def test_need_bytes_at_the_edges():
    c, data = make(8, 8, True, 3, "random")
    lay = EB.layout(data)
    h, b = lay["header_end"], lay["base_end"]
    assert PRE == 16 and PRE < h < b < lay["total"]
    for n, want in ((0, PRE), (1, PRE), (PRE - 1, PRE), (PRE, h), (h - 1, h), (h, b), (b - 1, b), (b, b), (lay["total"], b)):
        assert EB.need_bytes(data[:n]) == want, n
    with pytest.raises(ValueError, match=f"{h} bytes are needed"):
        EB.layout(data[:h - 1])
    for bad in ("text", None, 5, [1, 2]):
        for fn in (EB.need_bytes, EB.layout, EB.from_bytes):
            with pytest.raises(ValueError, match="bytes-like"):
                fn(bad)


# ------------------------------------------------------------------------------------------------ refusals
def _reseal(data, edit):
    """``data`` with ``edit(header bytearray, fields)`` applied to its header and a preamble that fits the result: a
    header that is damaged in what it says, not in its CRC.  ``fields``: the byte offset of every field in the header."""
    end = EB.layout(data)["header_end"]
    header = bytearray(data[PRE:end])
    ns, L = struct.unpack_from("<HH", header, 8)
    scheduled = header[1] & 1
    at = {"format": 0, "flags": 1, "lanes": 2, "base_lanes": 3, "shape": 4, "ns": 8, "L": 10, "z_len": 12, "base_len": 16,
          "emb_len": 16 + 4 * ns}
    at["values"] = at["emb_len"] + 4 * ns
    at["count"] = at["values"] + (4 if scheduled else 8) * L
    at["bytes"] = at["count"] + 4 * L * ns
    at["total"] = len(header) - 8
    header = edit(header, at) or header
    return EB._seal(bytes(header)) + data[end:]


def _u32(header, off, delta=None, value=None):
    v = struct.unpack_from("<I", header, off)[0]
    struct.pack_into("<I", header, off, v + delta if value is None else value)


def test_a_header_that_contradicts_itself_is_refused_by_message():
    c, data = make(8, 1, False, 3, "random")
    assert EB._same(EB.from_bytes(_reseal(data, lambda h, at: None)), c)                      # the helper itself
    assert c["marks"]["bytes"][1][0] > 0

    def refused(edit, message, stream=data):
        bad = _reseal(stream, edit)
        for fn in (EB.from_bytes, EB.layout, EB.need_bytes):
            with pytest.raises(ValueError, match=message):
                fn(bad)
    refused(lambda h, at: _u32(h, at["bytes"] + 4 * NS, value=c["marks"]["bytes"][0][0] - 4),
            r"contradicts itself: slice 0: the bytes of mark 1, \d+, lie below those of mark 0")
    refused(lambda h, at: _u32(h, at["emb_len"] + 4, value=c["marks"]["bytes"][2][1] - 1),
            r"contradicts itself: slice 1: its last mark, \d+ bytes, lies beyond its stream's length")
    for field in ("lanes", "base_lanes"):
        for v in (0, 3, 128, 255):
            refused(lambda h, at: h.__setitem__(at[field], v), rf"the header's {field}: lanes is a power of two in 1 .. 64, got {v}")
    refused(lambda h, at: _u32(h, at["total"], delta=1), r"its lengths add up to \d+ bytes, it states a total of \d+")
    refused(lambda h, at: _u32(h, at["z_len"], delta=-1), "its lengths add up to")
    refused(lambda h, at: _u32(h, at["emb_len"] + 8, delta=4), "its lengths add up to")
    refused(lambda h, at: h + b"\0\0\0\0", r"the header's fields take \d+ of its stated \d+ bytes")
    refused(lambda h, at: h[:-8], "fields need more than its stated|fields take")
    refused(lambda h, at: struct.pack_into("<H", h, at["ns"], 4), "contradicts itself|fields")
    refused(lambda h, at: struct.pack_into("<H", h, at["L"], 0xFFFF), "fields need more than its stated")
    refused(lambda h, at: struct.pack_into("<H", h, at["ns"], 0), "none may be 0")
    refused(lambda h, at: h.__setitem__(at["format"], 1), "lanes 8, base_lanes 1 are format 'embedded-2', it says 'embedded-1'")
    refused(lambda h, at: h.__setitem__(at["format"], 5), "format digit 5")
    refused(lambda h, at: h.__setitem__(at["flags"], 1), "scheduled are format 'embedded-3', it says 'embedded-2'")
    refused(lambda h, at: h.__setitem__(at["flags"], 2), "flags 0x2")
    refused(lambda h, at: h.__setitem__(at["base_lanes"], 8), "base_lanes 8 are format 'embedded-4'")
    sched = make(1, 1, True, 3, "random")[1]
    refused(lambda h, at: h.__setitem__(at["flags"], 0), "are format 'embedded-1', it says 'embedded-3'", sched)
    refused(lambda h, at: struct.pack_into("<H", h, at["shape"], 2), "fields need more than|fields take|add up", sched)


def test_preamble_crc_trailing_bytes_and_short_data():
    c, data = make(1, 8, False, 3, "random")
    lay = EB.layout(data)
    with pytest.raises(ValueError, match="not an embedded codestream: it begins with b'XAMe'"):
        EB.from_bytes(b"X" + data[1:])
    with pytest.raises(ValueError, match="codestream version 2; this reader knows version 1"):
        EB.from_bytes(data[:4] + b"\x02\x00" + data[6:])
    with pytest.raises(ValueError, match="reserved field 256"):
        EB.need_bytes(data[:7] + b"\x01" + data[8:])
    with pytest.raises(ValueError, match="a header of 3 bytes"):
        EB.need_bytes(data[:8] + struct.pack("<I", 3) + data[12:])
    with pytest.raises(ValueError, match="a header of 4294967295 bytes"):
        EB.need_bytes(data[:8] + b"\xff" * 4 + data[12:PRE])
    with pytest.raises(ValueError, match="CRC-32 does not match"):
        EB.from_bytes(data[:12] + struct.pack("<I", (zlib.crc32(data[PRE:lay["header_end"]]) ^ 1) & 0xFFFFFFFF) + data[PRE:])
    for extra in (b"\0", b"abcdefgh"):
        with pytest.raises(ValueError, match=rf"states a total of {len(data)}: {len(extra)} bytes follow the codestream"):
            EB.from_bytes(data + extra)
    assert EB.need_bytes(data + b"\0") == lay["base_end"] and EB.layout(data + b"\0") == lay   # the header alone is read
    with pytest.raises(ValueError, match=rf"{lay['base_end']} bytes are needed"):
        EB.from_bytes(data[:lay["base_end"] - 1])


@pytest.mark.parametrize("case", [(1, 1, False, 3, "random"), (8, 8, True, 3, "zeros"), (8, 1, True, 1, "random")])
def test_every_single_byte_change_of_preamble_and_header_is_refused(case):
    c, data = make(*case)
    end = EB.layout(data)["header_end"]
    for at in range(end):
        for flip in (0x01, 0x80, 0xFF):
            bad = bytearray(data)
            bad[at] ^= flip
            with pytest.raises(ValueError):
                EB.from_bytes(bytes(bad))
            with pytest.raises(ValueError):                                     # a receiver's first look
                if EB.need_bytes(bytes(bad)) > len(bad):
                    raise ValueError("too few bytes")                           # a header length that grew
                EB.layout(bytes(bad))


def test_random_corruptions_and_prefixes_raise_nothing_but_valueerror():
    rng = np.random.default_rng(7)
    seen = {"ok": 0, "refused": 0}
    for it in range(600):
        c, data = make(*CASES[int(rng.integers(len(CASES)))])
        end = EB.layout(data)["header_end"]
        bad = bytearray(data)
        kind = it % 4
        if kind == 0:                                                           # bytes changed anywhere
            for at in rng.integers(0, len(bad), int(rng.integers(1, 4))):
                bad[at] = int(rng.integers(256))
        elif kind == 1:                                                         # a header of noise under a matching CRC
            header = bytearray(data[PRE:end])
            for at in rng.integers(0, len(header), int(rng.integers(1, 6))):
                header[at] = int(rng.integers(256))
            bad = bytearray(EB._seal(bytes(header)) + data[end:])
        elif kind == 2:                                                         # a header cut or grown under a matching CRC
            header = data[PRE:end][:int(rng.integers(0, end - PRE))] + rng.bytes(int(rng.integers(0, 9)))
            bad = bytearray(EB._seal(header) + data[end:])
        bad = bytes(bad[:int(rng.integers(0, len(bad) + 1))]) if rng.random() < 0.7 else bytes(bad) + rng.bytes(int(rng.integers(0, 3)))
        for fn in (EB.need_bytes, EB.layout, EB.from_bytes):
            try:
                got = fn(bad)
            except ValueError as e:
                assert str(e)
                seen["refused"] += 1
                continue
            seen["ok"] += 1
            if fn is EB.from_bytes:
                EB._check_container(got)
                assert sum(len(s) for s in got["embedded"]) == len(bad) - EB.layout(bad)["base_end"]
                assert len(bad) >= EB.need_bytes(bad)
    assert seen["ok"] > 100 and seen["refused"] > 100


def test_to_bytes_refuses_what_the_format_cannot_carry():
    c, _ = make(8, 8, True, 3, "random")
    with pytest.raises(ValueError, match="not an embedded container"):
        EB.to_bytes({"format": "progressive-1"})
    with pytest.raises(ValueError, match="has the keys"):
        EB.to_bytes(dict(c, extra=1))
    with pytest.raises(ValueError, match="side_bytes is 8 per level"):
        EB.to_bytes(dict(c, side_bytes=5))
    with pytest.raises(ValueError, match="marks never decrease"):
        EB.to_bytes(dict(c, marks=dict(c["marks"], bytes=c["marks"]["bytes"][::-1])))
    with pytest.raises(ValueError, match=r"integers \[3\]\[3\]"):
        EB.to_bytes(dict(c, marks=dict(c["marks"], count=c["marks"]["count"][:2])))
    with pytest.raises(ValueError, match='"base" is a list of 3 lists'):
        EB.to_bytes(dict(c, base=c["base"][:2]))
    with pytest.raises(ValueError, match="the schedule's index is uint8"):
        EB.to_bytes(dict(c, schedule=dict(c["schedule"], index=c["schedule"]["index"][:, :2])))
    plain, _ = make(1, 1, False, 1, "random")
    with pytest.raises(ValueError, match="has the keys"):
        EB.to_bytes(dict(plain, base_lanes=8))                                  # a key "embedded-1" does not carry
    with pytest.raises(ValueError, match="shape is"):
        EB.to_bytes(dict(plain, shape=(0, 2)))


# ------------------------------------------------------------------------------------------------ the receiver's arithmetic
class _Model:
    ns0 = NS


class _Inner:
    """Stands in for EmbeddedDecoder: keeps the containers as ``extend`` does, decodes nothing."""
    made = 0

    def __init__(self, model, containers, coder=None, resumable=False):
        assert resumable and coder == "host"
        _Inner.made += 1
        self.containers, self.extend_bytes = [dict(c) for c in containers], sum(len(s) for c in containers for s in c["embedded"])

    def extend(self, more):
        self.extend_bytes = sum(len(s) for row in more for s in row)
        assert self.extend_bytes                              # a feed without new body bytes makes no call
        for c, row in zip(self.containers, more):
            c["embedded"] = [a + b for a, b in zip(c["embedded"], row)]

    def available(self):
        return np.asarray([[len(s) for s in c["embedded"]] for c in self.containers])


@pytest.fixture
def receiver(monkeypatch):
    monkeypatch.setattr(EB, "_check_model", lambda m: None)
    monkeypatch.setattr(EB, "EmbeddedDecoder", _Inner)
    return lambda n: EB.StreamDecoder(_Model(), n, coder="host")


@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_feeding_chunks_hands_the_inner_decoder_from_bytes_of_the_prefix(receiver, chunk):
    """Two images of one batch, each arriving at its own pace, image 1 half as fast."""
    streams = [make(8, 8, True, 3, "random")[1], make(8, 8, True, 3, "zeros")[1]]
    need = [EB.need_bytes(s) for s in streams]
    dec = receiver(2)
    assert not dec.ready and dec.need() == [PRE, PRE] and dec.available() is None
    with pytest.raises(ValueError, match="nothing to decode yet: image 0 lacks 16 bytes"):
        dec.decode()
    sent, handed = [0, 0], 0
    for it in range(2 * sum(len(s) for s in streams)):
        if sent == [len(s) for s in streams]:
            break
        step = [min(len(s) - a, chunk // (1 + b) or it % 2) for b, (s, a) in enumerate(zip(streams, sent))]
        got = dec.feed([s[a:a + n] for s, a, n in zip(streams, sent, step)])
        sent = [a + n for a, n in zip(sent, step)]
        assert dec.ready == all(a >= n for a, n in zip(sent, need)) and (got is None) == (not dec.ready)
        assert dec.need() == [max(0, EB.need_bytes(s[:a]) - a) for s, a in zip(streams, sent)]
        if dec.ready:
            want = [EB.from_bytes(s[:a]) for s, a in zip(streams, sent)]
            assert EB._same(dec.decoder.containers, want), sent
            assert np.array_equal(got, [[len(e) for e in c["embedded"]] for c in want])
            handed += dec.extend_bytes
    assert _Inner.made >= 1 and handed == sum(len(s) - n for s, n in zip(streams, need))        # every body byte once
    assert EB._same(dec.decoder.containers, [make(8, 8, True, 3, "random")[0], make(8, 8, True, 3, "zeros")[0]])
    assert dec.feed([b"", b""]) is not None and dec.extend_bytes == 0
    with pytest.raises(ValueError, match="image 1: .* bytes follow the codestream"):
        dec.feed([b"", b"\0"])


def test_a_mixed_batch_is_refused_at_the_feed_that_completes_the_second_header(receiver):
    a = make(8, 1, False, 3, "random")[1]
    for other, why in ((make(1, 1, False, 3, "random")[1], "its lanes is 1, the others' 8"),
                       (make(8, 8, False, 3, "random")[1], "its base_lanes is 8, the others' 1"),
                       (make(8, 1, True, 3, "random")[1], "it is scheduled, the others are plain")):
        dec = receiver(2)
        end = EB.layout(other)["header_end"]
        assert dec.feed([a, other[:end - 1]]) is None                           # image 0 whole, image 1 one byte short of its header
        with pytest.raises(ValueError, match=f"image 1 does not belong to this batch: {why}; decode it separately"):
            dec.feed([b"", other[end - 1:end + 5]])
        assert dec.need()[1] == 1 and not dec.ready                             # the refused feed kept nothing
    dec = receiver(2)
    with pytest.raises(ValueError, match="image 1 does not belong to this batch: it has 3 stages, the others 1"):
        dec.feed([make(8, 1, True, 1, "random")[1], make(8, 1, True, 3, "random")[1]])     # both headers in one feed
    dec = receiver(1)
    dec.m = type("M", (), {"ns0": 10})()
    with pytest.raises(ValueError, match="holds 3 slices, a container of this model has 10"):
        dec.feed([a])


def test_feed_refuses_malformed_chunks_and_damaged_headers(receiver):
    data = make(1, 1, False, 3, "random")[1]
    dec = receiver(2)
    for bad in ([data], [data, data, data], 5, [data, "text"], [None, data]):
        with pytest.raises(ValueError, match="StreamDecoder.feed"):
            dec.feed(bad)
    with pytest.raises(ValueError, match="image 1: not an embedded codestream"):
        dec.feed([data[:20], b"X" * 16])
    with pytest.raises(ValueError, match="image 0: the header's CRC-32 does not match"):
        dec.feed([data[:30] + b"\xff" + data[31:], b""])
    assert dec.need() == [PRE, PRE]
    for n in (0, True, 1.5, "2"):
        with pytest.raises(ValueError, match="n_images is an integer >= 1"):
            EB.StreamDecoder(_Model(), n, coder="host")


def test_a_schedule_of_no_levels_or_no_stages_is_refused_in_the_header():
    data = make(8, 1, True, 3, "random")[1]
    for which, message in ((0, "a schedule of 0 levels and 3 stages, none may be 0"), (2, "a schedule of 3 levels and 0 stages, none may be 0")):
        bad = _reseal(data, lambda h, at: struct.pack_into("<H", h, at["bytes"] + 4 * 3 * NS + which, 0))
        for fn in (EB.from_bytes, EB.layout, EB.need_bytes):
            with pytest.raises(ValueError, match=message):
                fn(bad)


def test_a_chunk_counts_in_bytes_whatever_its_item_size(receiver):
    data = make(1, 1, False, 3, "random")[1]
    data = data[:len(data) // 4 * 4]
    dec, ref = receiver(1), receiver(1)
    ref.feed([data])
    for at in range(0, len(data), 8):
        dec.feed([memoryview(data[at:at + 8]).cast("I")])                      # two items of four bytes
    assert EB._same(dec.decoder.containers, ref.decoder.containers) and dec.need() == [0]
    rest = make(1, 1, False, 3, "random")[1][len(data):]
    with pytest.raises(ValueError, match=rf"image 0: {len(data) + 4} bytes, its header states a total of {len(data) + len(rest)}"):
        dec.feed([memoryview(rest + b"\0" * (4 - len(rest))).cast("I")])


def test_a_feed_whose_decoder_cannot_be_built_is_not_kept(receiver, monkeypatch):
    data = make(8, 1, False, 3, "random")[1]
    need = EB.need_bytes(data)

    class Damaged(_Inner):
        def __init__(self, *a, **k):
            raise ValueError("EmbeddedDecoder: base stream (image 0, slice 1): bitstream truncated")
    dec = receiver(1)
    assert dec.feed([data[:need - 5]]) is None
    monkeypatch.setattr(EB, "EmbeddedDecoder", Damaged)
    for _ in range(2):
        with pytest.raises(ValueError, match="base stream .image 0, slice 1.: bitstream truncated"):
            dec.feed([data[need - 5:need + 9]])
        assert not dec.ready and dec.need() == [5] and dec.available() is None
        with pytest.raises(ValueError, match="nothing to decode yet: image 0 lacks 5 bytes"):
            dec.decode()
    dec = receiver(1)                                                           # ... also when that feed brought the header
    with pytest.raises(ValueError, match="bitstream truncated"):
        dec.feed([data])
    assert dec.need() == [PRE] and not dec.ready
    monkeypatch.setattr(EB, "EmbeddedDecoder", _Inner)
    assert dec.feed([data]) is not None and EB._same(dec.decoder.containers, [make(8, 1, False, 3, "random")[0]])
