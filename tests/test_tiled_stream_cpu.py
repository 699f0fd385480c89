"""The receiver of tiled pictures on the host (vampic.tiled.PictureFeed): fabricated picture codestreams
of header versions 1, 2 and 3 fed in chunks that end anywhere, checked after every feed against the arithmetic of the whole
concatenation; refused feeds change nothing; and the properties of the NumPy restatement of vam_tile_refresh
(tests/tiled_stream_ref.py).  No model and no GPU are needed."""
import numpy as np
import pytest

import tiled_ref as TR
import tiled_stream_ref as RR
from test_tiled_cpu import _tile, picture as picture_v1
from test_tiled_schedule_cpu import picture as picture_v3
from vampic import tiled as TL

_MADE = {}


def _v2(H, W, tile, V, shape):
    key = (H, W, tile, V)
    if key not in _MADE:
        g = TL.grid(H, W, tile, V)
        streams = [_tile(7 * H + i, shape) for i in range(g["R"] * g["C"])]
        thr = np.float32([[3.0, 2.5, 2.0], [2.0, 1.5, 1.0], [0.5, 0.25, 0.125]])
        _MADE[key] = TL.pack(H, W, tile, V, streams, thresholds=thr)
    return _MADE[key]


def _stream(name):
    """A fabricated picture codestream: versions 1, 2 and 3 on a 1 x 5 grid of 64 x 128 tiles, 1 and 2 on a 3 x 4 grid."""
    if name == "v1-3x4":
        return picture_v1()[2]
    if name == "v1-1x5":
        return picture_v1(H=60, W=500, tile=128, overlap=32, shape=(1, 2))[2]
    if name == "v2-3x4":
        return _v2(150, 200, 64, 16, (1, 1))
    if name == "v2-1x5":
        return _v2(60, 500, 128, 32, (1, 2))
    return picture_v3()[2]                                   # "v3-1x5": tiles 1 and 3 have pieces of 0 bytes


STREAMS = ["v1-3x4", "v1-1x5", "v2-3x4", "v2-1x5", "v3-1x5"]


def _expect(data, n):
    """(ready, need, rounds, held, per-tile bytes) of ``data[:n]`` from need_bytes, layout and _Picture.held alone."""
    d = data[:n]
    need = TL.need_bytes(d)
    if n < TL.PREAMBLE_BYTES or n < TL._header_end(d, "test"):
        return False, need - n, None, None, None
    s = TL._parse(d, "test")[1]
    lay = TL.layout(d)
    assert need == lay["need_bytes"] == s.need
    held = s.held(n)
    per_tile = held.sum(0)
    if n < need:
        return False, need - n, None, None, per_tile
    whole = held[1:] == s.size[1:]
    rounds = np.where(s.present, np.cumprod(whole, axis=0).sum(0), -1).reshape(lay["R"], lay["C"])
    return True, 0, rounds, np.where(s.present, per_tile, -1).reshape(lay["R"], lay["C"]), per_tile


def _check(f, data, n, before):
    """The receiver ``f`` after a feed that brought it to ``n`` bytes; ``before``: the per-tile bytes before that feed."""
    ready, need, rounds, held, per_tile = _expect(data, n)
    assert f.ready == ready and f.need() == need and len(f) == n and f.data == data[:n]
    if not ready:
        assert f.rounds is None and f.held is None
    else:
        assert np.array_equal(f.rounds, rounds) and np.array_equal(f.held, held)
        lay = TL.layout(data[:n])
        assert all(f.meta[k] == lay[k] for k in ("marks", "lanes", "base_lanes", "ns", "format"))
        assert f.shape == (lay["H"], lay["W"]) and f.scheduled == lay["scheduled"] and f.stages == lay["stages"]
        assert all(f.grid[k] == lay[k] for k in ("H", "W", "th", "tw", "V", "Sy", "Sx", "R", "C"))
    if per_tile is None:
        assert f.fed_tiles == []
        return None
    C = f.grid["C"]
    grew = per_tile > (before if before is not None else 0)
    assert f.fed_tiles == [(int(i) // C, int(i) % C) for i in np.flatnonzero(grew)]
    return per_tile


def _feed_at(data, cuts):
    f, at, before = TL.PictureFeed(), 0, None
    for n in cuts:
        got = f.feed(data[at:n])
        before = _check(f, data, n, before)
        assert (got is None) == (not f.ready) and (got is None or np.array_equal(got, f.rounds))
        at = n
    return f


@pytest.mark.parametrize("name,step", [(n, s) for n in STREAMS for s in (1, 7, 4096) if s > 1 or n.endswith("1x5")])    # single bytes: the short streams
def test_chunks_of_any_size_give_the_arithmetic_of_the_concatenation(name, step):
    data = _stream(name)
    f = _feed_at(data, list(range(step, len(data), step)) + [len(data)])
    assert f.ready and int(f.rounds.min()) == TL.layout(data)["n_rounds"]
    assert f.feed(b"") is not None and f.fed_tiles == []


@pytest.mark.parametrize("name", ["v1-1x5", "v2-3x4", "v3-1x5"])
def test_single_bytes_up_to_the_first_round_and_every_boundary(name):
    data = _stream(name)
    lay = TL.layout(data)
    _feed_at(data, list(range(1, lay["round_end"][0] + 2)) + [len(data)])
    edges = {TL.PREAMBLE_BYTES, lay["header_end"], lay["need_bytes"], lay["total"]} | set(lay["round_end"])
    edges |= {o + n for row in lay["head"] for o, n in row} | {o + n for k in lay["piece"] for row in k for o, n in row}
    cuts = sorted({n + d for n in edges for d in (-1, 0, 1) if 0 < n + d <= len(data)})
    f = _feed_at(data, cuts)
    assert f.ready and [f.tile_bytes(0, c) for c in range(lay["C"])] == [TL.tile_stream(data, 0, c) for c in range(lay["C"])]


def test_a_piece_of_zero_bytes_does_not_feed_its_tile():
    data = _stream("v3-1x5")
    lay = TL.layout(data)
    empty = [(k, c) for k in range(lay["n_rounds"]) for c in range(5) if lay["piece"][k][0][c][1] == 0]
    assert {c for _, c in empty} == {1, 3} and {k for k, _ in empty} >= {0, 2}   # the "zeros" tiles: stage 0 adds nothing, nor does stage 2
    f = TL.PictureFeed()
    f.feed(data[:lay["need_bytes"]])
    assert f.fed_tiles == [(0, c) for c in range(5)] and f.rounds.tolist() == [[0, 1, 0, 1, 0]]
    at = lay["need_bytes"]
    for k, end in enumerate(lay["round_end"]):
        held = f.held.copy()
        f.feed(data[at:end])
        assert f.fed_tiles == [(0, c) for c in range(5) if lay["piece"][k][0][c][1] > 0]
        assert all((0, c) not in f.fed_tiles and f.held[0, c] == held[0, c] for kk, c in empty if kk == k)
        at = end


@pytest.mark.parametrize("name", ["v1-3x4", "v3-1x5"])
def test_an_extract_feeds_like_a_whole_stream(name):
    data = _stream(name)
    g = TL.layout(data)
    win = (10, 70, 30, 60) if name == "v1-3x4" else (10, 200, 30, 50)
    for ex, keep in ((TL.extract(data, win), TL.tiles_for(g, win)), (TL.extract(data, win, 1), TL.tiles_for(g, win)),
                     (TL.extract(data, rounds=2), TL.tiles_for(g))):
        f = _feed_at(ex, list(range(13, len(ex), 13)) + [len(ex)])
        assert sorted(zip(*np.nonzero(f.held >= 0))) == keep and (f.rounds[f.held < 0] == -1).all()


def _state(f):
    return (f.data, f.ready, f.need(), f.meta, f.fed_tiles, None if f.held is None else f.held.tolist(),
            None if f.rounds is None else f.rounds.tolist(), f._heads, f._s)


@pytest.mark.parametrize("name", ["v1-3x4", "v2-1x5", "v3-1x5"])
def test_a_refused_feed_changes_nothing_and_a_correct_one_continues(name):
    data = _stream(name)
    lay = TL.layout(data)
    hend = lay["header_end"]
    rng = np.random.default_rng(5)
    for at in sorted({0, 3, 4, 6, 8, 12, 15, 16, 20, 30, hend - 9, hend - 1} | {int(v) for v in rng.integers(0, hend, 12)}):
        f = TL.PictureFeed()
        lo = int(rng.integers(0, at + 1))                                       # fed before: a part that holds nothing damaged
        f.feed(data[:lo])
        was = _state(f)
        bad = data[lo:at] + bytes([data[at] ^ (0x01 if at % 2 else 0x80)]) + data[at + 1:]   # all of it: a longer header length still ends
        if 8 <= at < 12 and TL._PREAMBLE.unpack_from(data[:lo] + bad, 0)[3] + TL.PREAMBLE_BYTES > len(data):
            assert f.feed(bad) is None and f.need() == TL.need_bytes(data[:lo] + bad) - len(data)   # a longer header: it waits for it
            continue
        with pytest.raises(ValueError, match="PictureFeed.feed"):
            f.feed(bad)
        assert _state(f) == was
        f.feed(data[lo:lay["need_bytes"]])
        assert f.ready and f.data == data[:lay["need_bytes"]]
    f = TL.PictureFeed()
    f.feed(data[:len(data) - 5])
    was = _state(f)
    with pytest.raises(ValueError, match=rf"{len(data) + 1} bytes, the header states a total of {len(data)}: 1 bytes follow"):
        f.feed(data[-5:] + b"\0")
    for bad in ("text", 5, None, [1, 2], np.zeros(3, np.uint8)):
        with pytest.raises(ValueError, match="expected bytes, got"):
            f.feed(bad)
    assert _state(f) == was
    assert f.feed(memoryview(bytearray(data[-5:]))).min() == lay["n_rounds"] and f.data == data
    with pytest.raises(ValueError, match="1 bytes follow the codestream"):
        f.feed(b"\0")
    # a head that contradicts the table is refused at the feed that completes it
    o, n = lay["head"][0][1]
    f = TL.PictureFeed()
    f.feed(data[:o + 3])
    was = _state(f)
    with pytest.raises(ValueError, match=r"PictureFeed.feed: .*tile \(0, 1\)"):
        f.feed(data[o + 3:o + 20] + bytes([data[o + 20] ^ 0x40]) + data[o + 21:o + n])
    assert _state(f) == was
    assert f.feed(data[o + 3:]) is not None and f.data == data


def test_before_the_header_the_attributes_say_what_is_missing():
    data = _stream("v1-3x4")
    f = TL.PictureFeed()
    assert not f.ready and f.need() == TL.PREAMBLE_BYTES and f.meta is None and f.fed_tiles == []
    f.feed(data[:5])
    assert f.need() == TL.PREAMBLE_BYTES - 5
    with pytest.raises(ValueError, match="PictureFeed.grid: the header is not complete yet: 11 bytes are missing"):
        f.grid
    f.feed(data[5:20])
    assert f.need() == TL.layout(data)["header_end"] - 20 and not f.ready


def test_seeded_corruptions_raise_nothing_but_value_errors():
    rng = np.random.default_rng(11)
    raised = 0
    for t in range(300):
        data = bytearray(_stream(STREAMS[t % len(STREAMS)]))
        lay = TL.layout(bytes(data))
        span = (lay["header_end"], lay["need_bytes"], len(data))[t % 3]
        for at in rng.integers(0, span, int(rng.integers(1, 4))):
            data[int(at)] = int(rng.integers(0, 256))
        if t % 7 == 0:
            data = data[:int(rng.integers(1, len(data)))] + bytes(rng.integers(0, 256, 9, dtype=np.uint8))
        f, at = TL.PictureFeed(), 0
        step = int(rng.integers(1, 200))
        try:
            while at < len(data):
                f.feed(bytes(data[at:at + step]))
                at += step
            _ = (f.ready, f.need(), f.rounds, f.held, f.fed_tiles, f.meta)
        except ValueError:
            raised += 1
    assert raised > 100


# ---------------------------------------------------------------------------------------------------- the restatement
def _case(H=150, W=200, tile=64, V=16):
    g = TL.grid(H, W, tile, V)
    n = g["R"] * g["C"]
    tiles = (np.random.default_rng(n + H).random((n, 3, g["th"], g["tw"]), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    return g, tiles, np.arange(n).reshape(g["R"], g["C"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("geo", [(150, 200, 64, 16), (60, 200, 128, 32), (129, 70, 64, 0), (37, 53, 64, 0)])
def test_restatement_all_dirty_is_the_blend_and_none_dirty_changes_nothing(geo):
    g, tiles, slot = _case(*geo)
    H, W = g["H"], g["W"]
    for win in [(0, 0, H, W), (3, 5, H - 7, W - 9), (H // 2, 1, 1, W - 1)]:
        y0, x0, h, w = win
        canvas = np.full((3, h, w), -7, dtype=np.float32)
        got, missing = RR.refresh(canvas, tiles, slot, np.ones_like(slot), g, win, win)
        assert not missing and np.array_equal(_bits(got), _bits(TR.blend(tiles, slot, g, win)[0]))
        got, missing = RR.refresh(canvas, tiles, np.full_like(slot, -1), np.zeros_like(slot), g, win, win)
        assert not missing and np.array_equal(_bits(got), _bits(canvas))        # and no slot is looked at
        u8 = np.full((h, w, 3), 0x5A, dtype=np.uint8)
        assert np.array_equal(RR.refresh(u8, tiles, slot, np.ones_like(slot), g, win, win)[0], TR.to_u8(TR.blend(tiles, slot, g, win)[0]))


def test_restatement_one_dirty_tile_changes_exactly_its_extent_in_the_window():
    g, tiles, slot = _case()
    for win in [(0, 0, 150, 200), (40, 31, 70, 101)]:
        y0, x0, h, w = win
        full = TR.blend(tiles, slot, g, win)[0]
        for r, c in TL.tiles_for(g, win):
            dirty = np.zeros_like(slot)
            dirty[r, c] = 1
            canvas = np.full((3, h, w), -7, dtype=np.float32)
            only = np.full_like(slot, -1)                                       # the clean tiles that no dirty pixel needs may be absent
            for rr in range(max(0, r - 1), min(g["R"], r + 2)):
                only[rr, max(0, c - 1):c + 2] = slot[rr, max(0, c - 1):c + 2]
            got, missing = RR.refresh(canvas, tiles, only, dirty, g, win, win)
            ys = slice(max(y0, r * g["Sy"]) - y0, min(y0 + h, r * g["Sy"] + g["th"]) - y0)
            xs = slice(max(x0, c * g["Sx"]) - x0, min(x0 + w, c * g["Sx"] + g["tw"]) - x0)
            inside = np.zeros((h, w), dtype=bool)
            inside[ys, xs] = True
            assert not missing and np.array_equal(RR.touched(dirty, g, win), inside)
            assert np.array_equal(_bits(got), _bits(np.where(inside[None], full, canvas)))
            box = (y0 + ys.start, x0 + xs.start, ys.stop - ys.start, xs.stop - xs.start)
            assert np.array_equal(_bits(RR.refresh(canvas, tiles, only, dirty, g, win, box)[0]), _bits(got))
            only[r, c] = -1                                                     # the dirty tile itself absent: missing
            assert RR.refresh(canvas, tiles, only, dirty, g, win, win)[1]
