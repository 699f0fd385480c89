"""Viewing sessions on the host (vampic.session): the framing of increment messages, the ledgers of a
server and a receiver along scripted tours of fabricated pyramids with picture headers of version 1, 2 and 3, the snapshot
against ``pyramid.extract`` byte for byte, and the refusals, each of which leaves the receiver as it was.  No model and no GPU
are needed."""
import re
import struct
import zlib

import numpy as np
import pytest

import test_embedded_stream_cpu as ES
from test_pyramid_cpu import H, SHAPES, TILE, V, W, pyramid as pyramid_v1
from test_tiled_cpu import _reseal, _tile
from vampic import pyramid as PY, session as SS, tiled as TL

_MADE = {}
THR = np.float32([[3.0, 2.5, 2.0], [2.0, 1.5, 1.0], [0.5, 0.25, 0.125]])


def coded(version):
    """(H, W, pyramid codestream) of three fabricated levels whose picture headers have ``version``: 1 and 2 on 150 x 200 in
    3 x 4, 2 x 2 and 1 x 1 tiles of 64 x 64; 3 (scheduled tiles, some pieces of 0 bytes) on 60 x 500 in 1 x 5, 1 x 3 and 1 x 1
    tiles of 64 x 128."""
    if version not in _MADE:
        if version == 1:
            _MADE[1] = (H, W, pyramid_v1()[1])
        elif version == 2:
            levels = []
            for h, w in SHAPES:
                g = TL.grid(h, w, TILE, V)
                levels.append(TL.pack(h, w, TILE, V, [_tile(7 * h + i) for i in range(g["R"] * g["C"])], thresholds=THR))
            _MADE[2] = (H, W, PY.pack(H, W, levels))
        else:
            levels = []
            for h, w in [(60, 500), (30, 250), (15, 125)]:
                g = TL.grid(h, w, 128, 32)
                streams = [ES.make(1, 1, True, 3, ("random", "zeros")[i % 2])[1] for i in range(g["R"] * g["C"])]
                levels.append(TL.pack(h, w, 128, 32, streams, stages=3))
            _MADE[3] = (60, 500, PY.pack(60, 500, levels))
        assert [lv["layout"]["R"] * lv["layout"]["C"] for lv in PY.layout(_MADE[version][2])["levels"]] == ([12, 4, 1] if version < 3 else [5, 3, 1])
        assert PY.level_stream(_MADE[version][2], 0)[4] == version
    return _MADE[version]


def tour(h, w):
    """Requests that overlap each other in levels, tiles and rounds: (method, arguments)."""
    rect = (h // 4, w // 4, h // 4, w // 4)
    return [("viewport", (None, (h // 5, w // 5), 1, 1)),                      # the thumbnail level alone, one round
            ("viewport", (rect, rect[2:], 1, 2)),                               # level 0 by window, two rounds; the thumbnail's second
            ("window", ([1], (0, 0, h // 2, w // 2), 1)),                       # a corner of level 1
            ("viewport", ((rect[0] + 5, rect[1] + w // 4) + rect[2:], rect[2:], 1, 2)),              # a pan: new tiles enter
            ("viewport", (rect, rect[2:], 1, 3)),                               # more rounds of the first rect
            ("window", (None, None, 1)),                                        # every tile at one round
            ("viewport", ((3 * rect[0], 3 * rect[1]) + rect[2:], rect[2:], 3, None, False))]         # a magnification, no thumbnail, all rounds


def run(server, receiver, steps):
    out = []
    for method, args in steps:
        message = getattr(server, method)(*args)
        out.append((message, receiver.merge(message)))
    return out


def same_ledger(a, b):
    return a.keys() == b.keys() and all(x.dtype == np.int16 and np.array_equal(x, y) for x, y in zip(a.values(), b.values()))


def ledger_bytes(data, have):
    """The bytes of the segments a ledger names, from the tables of ``data``."""
    lay = PY.layout(data)
    total = 0
    for k, segments in have.items():
        tl = lay["levels"][k]["layout"]
        for (r, c), n in np.ndenumerate(segments):
            total += sum(([tl["head"]] + tl["piece"])[j][r][c][1] for j in range(int(n)))
    return total


def state(rc):
    """What a refused merge must leave alone."""
    snap = []
    for r in range(3):
        try:
            snap.append(rc.snapshot(r))
        except ValueError as e:
            snap.append(str(e))
    return ({k: v.copy() for k, v in rc.have.items()}, snap,
            {k: (None if rc.level(k).meta is None else dict(rc.level(k).meta)) for k in rc.have}, rc.tag)


def same_state(a, b):
    return same_ledger(a[0], b[0]) and a[1] == b[1] and a[2].keys() == b[2].keys() and a[3] == b[3] \
        and all((x is None) == (y is None) and (x is None or TL.same(x, y)) for x, y in zip(a[2].values(), b[2].values()))


# ------------------------------------------------------------------------------------------------------------ framing
def _messages():
    _, _, data = coded(1)
    server = SS.Server(data)
    return data, server.viewport(None, (30, 40), 1, 1), server.viewport((40, 90, 70, 70), (64, 64), 1, 2)


def test_a_message_states_its_tag_records_and_sizes():
    data, first, second = _messages()
    a, b = SS.layout(first), SS.layout(second)
    lay = PY.layout(data)
    headers = data[:lay["header_end"]] + b"".join(PY.level_stream(data, k)[:lay["levels"][k]["layout"]["header_end"]] for k in (2, 1, 0))
    assert first[:4] == b"VAMi" and first[4] == 1 and a["headers"] and not b["headers"]
    assert a["tag"] == b["tag"] == zlib.crc32(headers) & 0xFFFFFFFF and a["header_bytes"] == 4 + len(headers) and b["header_bytes"] == 0
    assert a["records"] == [(2, 0, 0, 0, 2)] and a["header_end"] == 16 + 20 + 10 and a["total"] == len(first)
    assert first[a["header_end"]:][:4] == struct.pack("<I", lay["header_end"]) and first[a["header_end"] + 4:].startswith(headers)
    assert b["records"][0] == (2, 0, 0, 2, 1) and [r[0] for r in b["records"][1:]] == [0] * 9 and b["header_end"] == 36 + 10 * 10
    assert [r[1:3] for r in b["records"][1:]] == [(r, c) for r in range(3) for c in (1, 2, 3)] and all(r[3:] == (0, 3) for r in b["records"][1:])
    tl = lay["levels"][2]["layout"]
    assert a["segment_bytes"] == tl["head"][0][0][1] + tl["piece"][0][0][0][1]
    assert first.endswith(PY.level_stream(data, 2)[tl["piece"][0][0][0][0]:][:tl["piece"][0][0][0][1]])


def test_every_single_byte_change_of_preamble_and_header_is_refused():
    for message in _messages()[1:]:
        end = SS.layout(message)["header_end"]
        for at in range(end):
            for flip in (0x01, 0x80):
                bad = message[:at] + bytes([message[at] ^ flip]) + message[at + 1:]
                with pytest.raises(ValueError):
                    SS.layout(bad)
                with pytest.raises(ValueError):
                    SS.Receiver().merge(bad)


def test_random_corruptions_raise_nothing_but_valueerror():
    _, first, second = _messages()
    rng = np.random.default_rng(11)
    held = SS.Receiver()
    held.merge(first)
    before = state(held)
    for i in range(200):
        message = (first, second)[i % 2]
        bad = bytearray(message[:int(rng.integers(0, len(message) + 1))] if i % 4 == 3 else message)
        for at in rng.integers(0, max(len(bad), 1), int(rng.integers(1, 4))):
            if len(bad):
                bad[int(at)] = int(rng.integers(0, 256))
        for fn in (SS.layout, SS.Receiver().merge):
            try:
                fn(bytes(bad))
            except ValueError:
                pass
        try:
            held.merge(bytes(bad))
        except ValueError:
            assert same_state(state(held), before)
        else:                                               # only round bytes were hit, which no check covers: start again
            held = SS.Receiver()
            held.merge(first)


def test_every_proper_prefix_is_refused_and_states_the_missing_bytes_and_one_trailing_byte_is_refused():
    for message in _messages()[1:]:
        end = SS.layout(message)["header_end"]
        for n in range(len(message)):
            want = 16 - n if n < 16 else end - n if n < end else len(message) - n
            for fn in (SS.layout, SS.Receiver().merge):
                with pytest.raises(ValueError) as e:
                    fn(message[:n])
                assert int(re.search(r"(\d+) bytes are missing", str(e.value)).group(1)) == want, n
        for fn in (SS.layout, SS.Receiver().merge):
            with pytest.raises(ValueError, match="1 bytes follow the codestream"):
                fn(message + b"\0")


def test_reserved_bits_and_records_out_of_order_or_doubled_are_refused():
    _, _, second = _messages()

    def flags(h):
        struct.pack_into("<H", h, 4, 2)

    def reserved(h):
        struct.pack_into("<H", h, 6, 1)

    def swap(h):
        h[12 + 10:12 + 30] = h[12 + 20:12 + 30] + h[12 + 10:12 + 20]

    def double(h):
        h[12 + 20:12 + 30] = h[12 + 10:12 + 20]

    def level_up(h):                                                            # a finer level before a coarser one
        h[12:12 + 20] = h[12 + 10:12 + 20] + h[12:12 + 10]

    def count(h):
        struct.pack_into("<H", h, 12 + 8, 0)
    for edit, text in [(flags, "flags are 0x0002"), (reserved, r"reserved field 1"), (swap, "not canonical: level 0, tile \\(0, 1\\) follows level 0, tile \\(0, 2\\)"),
                       (double, "not canonical"), (level_up, "not canonical: level 2, tile \\(0, 0\\) follows level 0"),
                       (count, "holds 0 segments")]:
        with pytest.raises(ValueError, match=text):
            SS.layout(_reseal(second, edit))
    assert SS.layout(_reseal(second, lambda h: None)) == SS.layout(second)


# ------------------------------------------------------------------------------------------------------------- ledger
@pytest.mark.parametrize("version", [1, 2, 3])
def test_along_a_tour_the_ledgers_agree_and_no_segment_is_sent_twice(version):
    h, w, data = coded(version)
    server, receiver = SS.Server(data), SS.Receiver()
    assert server.have.keys() == {0, 1, 2} and not any(v.any() for v in server.have.values()) and receiver.have == {}
    sent = 0
    for i, (method, args) in enumerate(tour(h, w)):
        message = getattr(server, method)(*args)
        lay = SS.layout(message)
        assert lay["headers"] == (i == 0) and lay["records"], (i, method)
        grew = receiver.merge(message)
        assert set(grew) <= {r[:3] for r in lay["records"]} and (version == 3 or grew == [r[:3] for r in lay["records"]])
        assert [(k,) + rc for k in (2, 1, 0) for rc in receiver.level(k).fed_tiles] == grew
        sent += lay["segment_bytes"]
        assert same_ledger(receiver.have, server.have) and sent == ledger_bytes(data, server.have), (i, method)
        for k, r, c, first, count in lay["records"]:
            assert receiver.have[k][r, c] == first + count
            stream = TL.tile_stream(PY.level_stream(data, k), r, c)
            assert receiver.level(k).tile_bytes(r, c) == stream[:receiver.level(k).held[r, c]]
            assert receiver.level(k).tile_rounds[r, c] == first + count - 1 and receiver.level(k).tile_ready[r, c]
    assert (receiver.shape, receiver.levels, receiver.shapes) == ((h, w), 3, PY.level_shapes(h, w, 3))
    assert any(0 < n < v.max() for v in server.have.values() for n in v.reshape(-1))       # the tour leaves an uneven state
    for k in range(3):
        lv, tl = receiver.level(k), PY.layout(data)["levels"][k]["layout"]
        assert lv.grid == {key: tl[key] for key in lv.grid} and (lv.stages, lv.scheduled) == (tl["stages"], tl["scheduled"])
        assert TL.same(lv.meta["marks"], tl["marks"]) and lv.facts["total"] == tl["total"] and lv.facts["allocation"] == tl["allocation"]


@pytest.mark.parametrize("version", [1, 3])
def test_a_repeated_request_is_a_message_of_no_records_and_two_servers_give_the_same_bytes(version):
    h, w, data = coded(version)
    a, b, receiver = SS.Server(data), SS.Server(data), SS.Receiver()
    assert receiver.merge(SS._seal(5, None, [], [])) == [] and receiver.have == {}           # nothing before the headers: nothing to refuse
    for method, args in tour(h, w):
        message = getattr(a, method)(*args)
        assert message == getattr(b, method)(*args)
        receiver.merge(message)
        before = state(receiver)
        again = getattr(a, method)(*args)
        lay = SS.layout(again)
        assert lay["records"] == [] and not lay["headers"] and lay["total"] == len(again) == 36 and again == getattr(b, method)(*args)
        assert receiver.merge(again) == [] and same_state(state(receiver), before) and same_ledger(a.have, receiver.have)
        assert all(receiver.level(k).fed_tiles == [] for k in range(3))


@pytest.mark.parametrize("version", [1, 2, 3])
def test_tours_that_reach_the_same_ledger_in_another_order_give_the_same_snapshot(version):
    h, w, data = coded(version)
    steps = tour(h, w)
    snaps = []
    for order in (steps, steps[::-1], steps[3:] + steps[:3]):
        server, receiver = SS.Server(data), SS.Receiver()
        run(server, receiver, order)
        snaps.append((receiver.have, [receiver.snapshot(r) for r in range(4)]))
    for have, snap in snaps[1:]:
        assert same_ledger(have, snaps[0][0]) and snap == snaps[0][1]
    assert len(set(snaps[0][1])) == 4


@pytest.mark.parametrize("version", [1, 2, 3])
def test_an_opened_session_sends_the_headers_once_and_then_records_alone(version):
    h, w, data = coded(version)
    plain, opened, receiver = SS.Server(data), SS.Server(data), SS.Receiver()
    opening = opened.open()
    lay, first = SS.layout(opening), SS.layout(SS.Server(data).viewport(None, (h // 5, w // 5), 1, 1))
    assert lay["headers"] and lay["records"] == [] and lay["segment_bytes"] == 0 and lay["header_end"] == 36 and lay["tag"] == first["tag"]
    assert lay["header_bytes"] == first["header_bytes"] == len(opening) - 36 and opened.sent_headers and not any(v.any() for v in opened.have.values())
    assert receiver.merge(opening) == [] and sorted(receiver.have) == [0, 1, 2] and receiver.shape == (h, w)
    assert receiver.level(0).meta is None and not receiver.level(0).tile_ready.any()
    again = opened.open()                                                       # the headers went: nothing is left to say
    assert SS.layout(again)["total"] == 36 and not SS.layout(again)["headers"] and receiver.merge(again) == []
    for method, args in tour(h, w):
        a, b = getattr(plain, method)(*args), getattr(opened, method)(*args)
        la, lb = SS.layout(a), SS.layout(b)
        assert not lb["headers"] and la["records"] == lb["records"] and a[la["header_end"] + la["header_bytes"]:] == b[lb["header_end"]:]
        receiver.merge(b)
    assert same_ledger(plain.have, opened.have) and same_ledger(receiver.have, opened.have)
    whole = SS.Receiver()
    whole.merge(SS.Server(data).window())
    assert all(receiver.snapshot(r) for r in range(2)) and whole.snapshot(3) == PY.extract(data, rounds=3)


# ------------------------------------------------------------------------------------------------- snapshot as oracle
@pytest.mark.parametrize("version", [1, 2, 3])
def test_after_everything_at_r_rounds_the_snapshot_is_the_extract_byte_for_byte(version):
    h, w, data = coded(version)
    rounds = PY.layout(data)["levels"][0]["layout"]["n_rounds"]
    assert rounds >= 3
    grown = (SS.Server(data), SS.Receiver())
    for r in range(rounds + 1):
        server, receiver = SS.Server(data), SS.Receiver()
        receiver.merge(server.window(rounds=r))
        grown[1].merge(grown[0].window(rounds=r))                               # and one receiver that grows round by round
        for rc in (receiver, grown[1]):
            assert all(rc.snapshot(j) == PY.extract(data, rounds=j) for j in range(r + 1)), r
            with pytest.raises(ValueError, match=f"Receiver.snapshot: no tile holds {r + 1} whole rounds: the ledger's most is {r}"):
                rc.snapshot(r + 1)
    assert grown[1].snapshot(rounds) == data == PY.extract(data)
    server, receiver = SS.Server(data), SS.Receiver()
    receiver.merge(server.window())                                            # rounds None: all of them
    assert receiver.snapshot(rounds) == data
    for bad, text in [(-1, "rounds is >= 0"), (1.0, "rounds is an integer")]:
        with pytest.raises(ValueError, match=text):
            receiver.snapshot(bad)
    with pytest.raises(ValueError, match="Receiver.snapshot: the picture's headers have not arrived yet"):
        SS.Receiver().snapshot(0)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_after_one_window_of_one_level_the_snapshot_is_that_extract(version):
    h, w, data = coded(version)
    for k, window, r in [(0, (h // 3, w // 3, h // 3, w // 3), 2), (1, (0, 0, h // 2, w // 2), 0), (2, None, 3), (1, (h - 1, w - 1, 1, 1), 1)]:
        server, receiver = SS.Server(data), SS.Receiver()
        receiver.merge(server.window([k], window, r))
        want = PY.extract(data, [k], window, r)
        assert receiver.snapshot(r) == want and len(want) < len(data)
        assert sorted(receiver.have) == [0, 1, 2] and not any(receiver.have[j].any() for j in range(3) if j != k)
    server, receiver = SS.Server(data), SS.Receiver()
    args = ((h // 4, w // 4, h // 2, w // 2), (h // 2, w // 2), 1, 2)
    receiver.merge(server.viewport(*args))
    assert receiver.snapshot(2) == PY.extract_viewport(data, *args)
    receiver.merge(server.viewport(*args, thumbnail=False))                    # nothing new without the thumbnail
    assert receiver.snapshot(2) == PY.extract_viewport(data, *args)
    one = PY.extract(data, [0])                                                 # one level: a plain tiled picture in a pyramid's frame
    server, receiver = SS.Server(one), SS.Receiver()
    receiver.merge(server.viewport(None, (h, w)))
    assert receiver.snapshot(3) == PY.extract(one, rounds=3) and sorted(receiver.have) == [0] == sorted(server.have)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_a_snapshot_of_an_uneven_state_parses_and_every_tile_stream_is_the_prefix_its_rounds_imply(version):
    h, w, data = coded(version)
    server, receiver = SS.Server(data), SS.Receiver()
    run(server, receiver, tour(h, w))
    full = PY.layout(data)
    for r in range(4):
        snap = receiver.snapshot(r)
        lay = PY.layout(snap)
        assert (lay["H"], lay["W"], lay["n_levels"], lay["total"]) == (h, w, 3, len(snap))
        for k in range(3):
            keep = receiver.have[k] >= 1 + r
            assert lay["levels"][k]["present"] == bool(keep.any())
            if not keep.any():
                continue
            tl, fl = lay["levels"][k]["layout"], full["levels"][k]["layout"]
            assert tl["n_rounds"] == r and np.array_equal(np.asarray(tl["present"]), keep) and PY.level_stream(snap, k)[4] == version
            assert version != 2 or np.array_equal(tl["thresholds"], THR)
            assert (tl["stages"], tl["allocation"]) == (fl["stages"], fl["allocation"])
            for rc_ in np.argwhere(keep):
                r_, c_ = (int(v) for v in rc_)
                n = fl["head"][r_][c_][1] + sum(fl["piece"][j][r_][c_][1] for j in range(r))
                assert TL.tile_stream(PY.level_stream(snap, k), r_, c_) == TL.tile_stream(PY.level_stream(data, k), r_, c_)[:n]
        dec = SS.Receiver()                                                     # a snapshot serves a session of its own
        dec.merge(SS.Server(snap).window())
        assert dec.snapshot(r) == snap


# ----------------------------------------------------------------------------------------------------------- refusals
def _refused(receiver, message, text, then=None):
    before = state(receiver)
    with pytest.raises(ValueError, match=text):
        receiver.merge(message)
    assert same_state(state(receiver), before), text
    if then is not None:
        assert receiver.merge(then) != [] and not same_state(state(receiver), before)


def _segments(data, k, r, c, first, count):
    tl = PY.layout(data)["levels"][k]["layout"]
    stream, at = PY.level_stream(data, k), [tl["head"]] + tl["piece"]
    return b"".join(stream[at[j][r][c][0]:at[j][r][c][0] + at[j][r][c][1]] for j in range(first, first + count))


@pytest.mark.parametrize("version", [1, 3])
def test_every_refused_merge_leaves_the_receiver_as_it_was_and_a_correct_merge_continues(version):
    h, w, data = coded(version)
    server = SS.Server(data)
    first, second = server.viewport(None, (h // 5, w // 5), 1, 1), server.window([0, 1], (0, 0, h // 2, w // 2), 2)
    tag, rounds = server.tag, PY.layout(data)["levels"][0]["layout"]["n_rounds"]
    receiver = SS.Receiver("Client")
    _refused(receiver, second, f"Client.merge: {len(SS.layout(second)['records'])} records before any headers", first)
    assert same_ledger(receiver.have, {0: np.zeros_like(server.have[0]), 1: np.zeros_like(server.have[1]), 2: np.int16([[2]])})
    receiver = SS.Receiver()
    receiver.merge(first)
    seg = lambda *rec: SS._seal(tag, None, [rec], [_segments(data, *rec)])
    _refused(receiver, SS._seal(tag ^ 1, None, [], []), "Receiver.merge: the message's tag is 0x.* the headers held have 0x")
    _refused(receiver, SS._seal(tag ^ 1, None, [(0, 0, 0, 0, 1)], [_segments(data, 0, 0, 0, 0, 1)]), "of another picture")
    assert receiver.merge(SS._seal(tag, server._headers, [], [])) == []        # the headers again, under the held tag: ignored
    other = SS.Server(PY.extract(data, rounds=rounds - 1))                      # another coding of the picture: other tables, another tag
    _refused(receiver, other.window(rounds=0), "the message's tag is")
    _refused(receiver, SS._seal(tag, None, [(3, 0, 0, 0, 1)], [b""]), "level is 0 .. 2, got 3")
    _refused(receiver, SS._seal(tag, None, [(2, 0, 1, 0, 1)], [b""]), r"level 2: Receiver.merge: tile \(0, 1\) is outside the grid of 1 x 1")
    _refused(receiver, SS._seal(tag, None, [(0, 7, 0, 0, 1)], [b""]), r"level 0: .*tile \(7, 0\) is outside the grid")
    _refused(receiver, first, r"level 2, tile \(0, 0\): the record begins at segment 0, the tile holds 2: a repeat")
    _refused(receiver, seg(2, 0, 0, 1, 1), r"begins at segment 1, the tile holds 2: a repeat")
    _refused(receiver, seg(0, 0, 0, 1, 1), r"level 0, tile \(0, 0\): the record begins at segment 1, the tile holds 0: a gap")
    _refused(receiver, seg(2, 0, 0, 3, 1), r"begins at segment 3, the tile holds 2: a gap")
    _refused(receiver, SS._seal(tag, None, [(2, 0, 0, 2, rounds)], [b""]), rf"segments 2 .. {rounds + 1}; the level has a head and {rounds} rounds")
    good = _segments(data, 0, 0, 1, 0, 1)
    _refused(receiver, SS._seal(tag, None, [(0, 0, 1, 0, 1)], [bytes(len(good))]), r"Receiver.merge: level 0: tile \(0, 1\): ")
    _refused(receiver, SS._seal(tag, None, [(0, 0, 1, 0, 1)], [good[:-1]]), "the body ends before the segments of level 0, tile \\(0, 1\\) do: 1 bytes are missing")
    _refused(receiver, SS._seal(tag, None, [(0, 0, 1, 0, 1)], [good + b"\0"]), "1 bytes follow the segments of the last record")
    moved = _segments(data, 0, 0, 0, 0, 1)                                      # another tile's head: its own pieces are not this table row's
    if len(moved) >= len(good):
        _refused(receiver, SS._seal(tag, None, [(0, 0, 1, 0, 1)], [moved[:len(good)]]), r"level 0: tile \(0, 1\)|contradicts tile \(0, 1\)")
    _refused(receiver, SS._seal(tag, None, [(0, 0, 1, 0, 2), (0, 0, 0, 0, 1)], [_segments(data, 0, 0, 1, 0, 2), moved]), "not canonical")
    assert receiver.merge(second) == [r[:3] for r in SS.layout(second)["records"]] and same_ledger(receiver.have, server.have)
    _refused(receiver, second, "a repeat", server.window(rounds=1))
    assert same_ledger(receiver.have, server.have)
    with pytest.raises(ValueError, match=r"Receiver level 0.tile_bytes: tile \(0, 9\) is outside the grid"):
        receiver.level(0).tile_bytes(0, 9)
    with pytest.raises(ValueError, match="level is 0 .. 2, got 3"):
        receiver.level(3)


def test_a_level_the_header_calls_absent_and_level_facts_that_contradict_each_other_are_refused():
    h, w, data = coded(1)
    two = PY.extract(data, [0, 2])
    server, receiver = SS.Server(two), SS.Receiver()
    assert sorted(server.have) == [0, 2]
    receiver.merge(server.window([2]))
    assert sorted(receiver.have) == [0, 2] and receiver.levels == 3
    _refused(receiver, SS._seal(server.tag, None, [(1, 0, 0, 0, 1)], [b""]), "level 1 is absent from this picture; it holds the levels \\[0, 2\\]",
             server.window([0], rounds=0))
    with pytest.raises(ValueError, match="Receiver.level: level 1 is absent from this session"):
        receiver.level(1)
    with pytest.raises(ValueError, match="Server.window: level 1 is absent from this codestream"):
        server.window([1])
    # headers that contradict each other: level 1 coded with another overlap, under a pyramid header that states its size
    lay = PY.layout(data)
    g = TL.grid(75, 100, TILE, 8)
    odd = TL.pack(75, 100, TILE, 8, [_tile(900 + i) for i in range(g["R"] * g["C"])])
    fake = PY._assemble(h, w, [PY.level_stream(data, 0), odd, PY.level_stream(data, 2)])
    headers = [fake[:lay["header_end"]], PY.level_stream(data, 2)[:lay["levels"][2]["layout"]["header_end"]], odd[:TL.layout(odd)["header_end"]],
               PY.level_stream(data, 0)[:lay["levels"][0]["layout"]["header_end"]]]
    body = struct.pack("<I", len(headers[0])) + b"".join(headers)
    tag = zlib.crc32(body[4:]) & 0xFFFFFFFF
    fresh = SS.Receiver()
    with pytest.raises(ValueError, match="Receiver.merge: level 1 and level 0 differ in their overlap"):
        fresh.merge(SS._seal(tag, body, [], []))
    with pytest.raises(ValueError, match="the tag 0x.* is not the CRC-32 of the headers the body carries"):
        fresh.merge(SS._seal(tag ^ 4, body, [], []))
    with pytest.raises(ValueError, match="level 1: .*the body ends before the picture header does|level 1: .*bytes do not hold the header"):
        fresh.merge(SS._seal(tag, body[:4 + len(headers[0]) + len(headers[1]) + 30], [], []))
    with pytest.raises(ValueError, match="the picture's headers have not arrived yet"):
        fresh.shape
    assert fresh.have == {} and fresh.tag is None
    with pytest.raises(ValueError, match="Server: level 1 and level 0 differ in their overlap"):
        SS.Server(fake)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_a_server_refuses_what_its_data_does_not_hold_whole_and_keeps_its_ledger(version):
    h, w, data = coded(version)
    lay = PY.layout(data)
    tl = lay["levels"][0]["layout"]
    r, c = tl["R"] - 1, tl["C"] - 2                                             # its round 1 is cut: the tiles after it lack theirs
    if tl["piece"][1][r][c][1] == 0:                                            # a piece of 0 bytes is whole wherever the data ends: take the next tile
        c += 1
    assert tl["piece"][1][r][c][1] > 0
    cut = lay["levels"][0]["offset"] + tl["piece"][1][r][c][0] + tl["piece"][1][r][c][1] - 1
    server, receiver = SS.Server(data[:cut]), SS.Receiver()
    receiver.merge(server.window(rounds=1))
    before = {k: v.copy() for k, v in server.have.items()}
    for call in (lambda: server.window(rounds=2), lambda: server.window([0], None, 2), lambda: server.viewport((0, 0, h, w), (h, w), 1, 2)):
        with pytest.raises(ValueError, match=rf"Server.(window|viewport): level 0: the data ends before round 1 \(segment 2\) of tile \({r}, {c}\) does"):
            call()
        assert same_ledger(server.have, before)
    message = server.window([1, 2])                                            # the levels that are whole are still served
    assert not SS.layout(message)["headers"] and receiver.merge(message) and same_ledger(receiver.have, server.have)
    assert receiver.snapshot(1) == PY.extract(data, rounds=1)
    for bad, text in [(lambda: server.window(rounds=9), "Server.window: level 0: rounds is 0 .. "),
                      (lambda: server.window([]), "Server.window: levels is empty"), (lambda: server.window([0], (0, 0, h + 1, 1)), "does not lie inside"),
                      (lambda: server.viewport(None, (0, 5)), "Server.viewport: viewport_level: out_hw"),
                      (lambda: server.viewport(None, (h // 5, w // 5), thumbnail=1), "Server.viewport: thumbnail is True or False")]:
        with pytest.raises(ValueError, match=text):
            bad()
        assert same_ledger(server.have, receiver.have)
    with pytest.raises(ValueError, match="Server: the data ends before the picture header of level 0 does"):
        SS.Server(data[:lay["levels"][0]["offset"] + 20])
    with pytest.raises(ValueError, match="Server: .* bytes do not hold the header"):
        SS.Server(data[:20])
    fresh = SS.Server(data)                                                     # a refused first request: the next message still carries the headers
    with pytest.raises(ValueError, match="rounds is 0 .. "):
        fresh.window(rounds=99)
    assert not fresh.sent_headers and SS.layout(fresh.window(rounds=0))["headers"] and fresh.sent_headers
