"""Resolution pyramids on the host (vampic.pyramid): the properties of the NumPy restatement
(tests/pyramid_ref.py), the framing of three fabricated level codestreams (pack / layout / level_stream / extract), the
refusals of a header that cannot be trusted and the byte bookkeeping of the receiver (PyramidFeed).  No model and no GPU
are needed."""
import struct

import numpy as np
import pytest

import pyramid_ref as PR
from test_tiled_cpu import _reseal, picture
from vampic import pyramid as PY, tiled as TL

H, W, TILE, V = 150, 200, 64, 16
SHAPES = [(150, 200), (75, 100), (38, 50)]
_MADE = {}


def pyramid():
    """(level codestreams, pyramid codestream) of three fabricated levels: 3 x 4 tiles, 2 x 2 tiles, one tile."""
    if not _MADE:
        levels = [picture(H=h, W=w, tile=TILE, overlap=V)[2] for h, w in SHAPES]
        _MADE["p"] = (levels, PY.pack(H, W, levels))
    return _MADE["p"]


# ---------------------------------------------------------------------------------------------------- the restatement
def test_a_constant_stays_the_constant_and_the_shapes_halve_rounding_up():
    for h, w in [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53), (64, 66)]:
        for value in (0.3, -7.25, 1e-42, 8e37):                                 # 4 v stays finite: doubling and * 0.25 are exact
            x = np.full((2, h, w), value, dtype=np.float32)
            for mode in ("mean", "max"):
                y = PR.halve(x, mode)
                assert y.shape == (2, (h + 1) // 2, (w + 1) // 2) and (y.view(np.uint32) == np.float32(value).view(np.uint32)).all()
    for h, w in [(150, 200), (1, 1), (2048, 3072), (37, 53), (1 << 24, 3)]:
        shapes = PR.level_shapes(h, w, 8)
        assert shapes == [(-(-h // 2 ** k), -(-w // 2 ** k)) for k in range(8)] == PY.level_shapes(h, w, 8)
    assert PR.level_shapes(H, W, 3) == SHAPES
    assert PY.default_levels(150, 200, 64) == 3 and PY.default_levels(2048, 3072, 256) == 5 and PY.default_levels(10, 10, 64) == 1
    assert PY.default_levels(1 << 24, 1 << 24, 64) == 16


def test_on_even_sizes_the_mean_is_the_float32_tree_and_two_max_levels_are_the_block_maximum():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, 12, 20)) * 10.0 ** rng.integers(-3, 4, (3, 12, 20))).astype(np.float32)
    y = PR.halve(x)
    for c, i, j in [(0, 0, 0), (1, 3, 7), (2, 5, 9), (1, 2, 4)]:
        a, b, p, q = x[c, 2 * i, 2 * j], x[c, 2 * i, 2 * j + 1], x[c, 2 * i + 1, 2 * j], x[c, 2 * i + 1, 2 * j + 1]
        want = np.float32(np.float32(np.float32(a + b) + np.float32(p + q)) * np.float32(0.25))
        assert y[c, i, j].view(np.uint32) == want.view(np.uint32)
    assert np.array_equal(y, ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * np.float32(0.25))
    m = PR.halve(PR.halve(x, "max"), "max")
    assert np.array_equal(m, x.reshape(3, 3, 4, 5, 4).max(axis=(2, 4)))
    odd = x[:, :11, :19]                                                        # the last row and column are replicated
    assert np.array_equal(PR.halve(odd, "max")[:, -1, -1], odd[:, -1, -1])
    assert np.array_equal(PR.halve(odd)[:, -1, -1], ((odd[:, -1, -1] + odd[:, -1, -1]) + (odd[:, -1, -1] + odd[:, -1, -1])) * np.float32(0.25))
    x[1, 4, 6] = np.nan
    for mode in ("mean", "max"):
        y = PR.halve(x, mode)
        assert np.isnan(y).sum() == 1 and y.view(np.uint32)[1, 2, 3] == PR.QNAN
    big = np.full((1, 2, 2), 3e38, dtype=np.float32)                            # the sum overflows before the multiply
    assert np.isposinf(PR.halve(big)).all() and (PR.halve(big, "max") == np.float32(3e38)).all()
    mixed = np.array([[[np.inf, -np.inf], [1.0, 2.0]]], dtype=np.float32)
    assert PR.halve(mixed).view(np.uint32)[0, 0, 0] == PR.QNAN and PR.halve(mixed, "max")[0, 0, 0] == np.inf


def test_window_at_covers_and_is_tight():
    rng = np.random.default_rng(1)
    for h_, w_ in [(150, 200), (37, 53), (1, 9), (2048, 3072)]:
        for _ in range(60):
            y0, x0 = int(rng.integers(0, h_)), int(rng.integers(0, w_))
            win = (y0, x0, int(rng.integers(1, h_ - y0 + 1)), int(rng.integers(1, w_ - x0 + 1)))
            for k in range(5):
                ya, xa, h, w = got = PR.window_at(win, k, h_, w_)
                assert got == PY.window_at(win, k, h_, w_)
                Hk, Wk = PR.level_shapes(h_, w_, k + 1)[k]
                assert 0 <= ya and 0 <= xa and h >= 1 and w >= 1 and ya + h <= Hk and xa + w <= Wk
                s = 2 ** k
                assert ya * s <= win[0] and min((ya + h) * s, h_) >= win[0] + win[2]      # covers
                assert xa * s <= win[1] and min((xa + w) * s, w_) >= win[1] + win[3]
                assert (ya + 1) * s > win[0] and (ya + h - 1) * s < win[0] + win[2]     # tight: the first and last row are needed
                assert (xa + 1) * s > win[1] and (xa + w - 1) * s < win[1] + win[3]
            for out_hw in [(1, 1), (20, 30), (win[2], win[3]), (4000, 4000)]:
                k = PR.best_level(win, out_hw, h_, w_, 5)
                assert k == PY.best_level(win, out_hw, h_, w_, 5)
                _, _, h, w = PR.window_at(win, k, h_, w_)
                assert k == 0 or (h >= out_hw[0] and w >= out_hw[1])
                if k < 4:
                    _, _, h, w = PR.window_at(win, k + 1, h_, w_)
                    assert h < out_hw[0] or w < out_hw[1]
    assert PY.window_at(None, 2, 150, 200) == (0, 0, 38, 50) and PY.best_level(None, (512, 768), 2048, 3072, 5) == 2
    with pytest.raises(ValueError, match="does not lie inside"):
        PY.window_at((0, 0, 151, 1), 1, 150, 200)
    with pytest.raises(ValueError, match="best_level: out_hw"):
        PY.best_level(None, (0, 5), 150, 200, 3)


# ------------------------------------------------------------------------------------------------------------ framing
def test_the_whole_stream_returns_every_level_stream_coarsest_first():
    levels, data = pyramid()
    lay = PY.layout(data)
    assert (lay["H"], lay["W"], lay["n_levels"], lay["total"]) == (H, W, 3, len(data)) and lay["header_end"] == 16 + 12 + 8 * 3 + 8
    assert data[:4] == b"VAMy" and data[4] == 1 and lay["ready_levels"] == [0, 1, 2]
    at = lay["header_end"]
    for k in (2, 1, 0):                                                         # the body: coarsest first
        lv = lay["levels"][k]
        assert PY.level_stream(data, k) == levels[k] == data[at:at + len(levels[k])]
        assert (lv["level"], lv["shape"], lv["offset"], lv["length"], lv["held"], lv["present"], lv["ready"]) == \
            (k, SHAPES[k], at, len(levels[k]), len(levels[k]), True, True)
        tl = TL.layout(levels[k])
        assert all(np.array_equal(lv["layout"][key], tl[key]) for key in tl)
        at += len(levels[k])
    assert [(lv["layout"]["R"], lv["layout"]["C"]) for lv in lay["levels"]] == [(3, 4), (2, 2), (1, 1)]
    assert lay["need_bytes"] == PY.need_bytes(data) == lay["header_end"] + TL.need_bytes(levels[2])
    assert PY.pack(H, W, [bytearray(s) for s in levels]) == data
    with pytest.raises(ValueError, match="level is 0 .. 2, got 3"):
        PY.level_stream(data, 3)


def test_every_prefix_from_need_bytes_on():
    levels, data = pyramid()
    lay = PY.layout(data)
    need, hend = lay["need_bytes"], lay["header_end"]
    ends = [lv["offset"] + lv["length"] for lv in lay["levels"]]
    cuts = sorted(set(range(need, len(data) + 1, 37)) | {len(data)} | {e + d for e in ends for d in (-1, 0, 1, 15, 16, 17) if need <= e + d <= len(data)})
    for n in cuts:
        got = [PY.level_stream(data[:n], k) for k in range(3)]
        assert all(s[:len(t)] == t for s, t in zip(levels, got)), n
        assert sum(len(t) for t in got) == n - hend, n                          # every byte received is some level's
        assert len(got[2]) >= TL.need_bytes(levels[2]) and TL.layout(got[2])["marks"] is not None
        part = PY.layout(data[:n])
        assert [lv["held"] for lv in part["levels"]] == [len(t) for t in got]
        assert part["ready_levels"] == [k for k in range(3) if len(got[k]) >= TL.layout(levels[k])["need_bytes"]] and 2 in part["ready_levels"]
        assert part["need_bytes"] == need == PY.need_bytes(data[:n])
        if len(got[1]) < 16:
            assert part["levels"][1]["layout"] is None
    for n in (0, 5, 16, hend - 1):
        assert PY.need_bytes(data[:n]) == (16 if n < 16 else hend)
        with pytest.raises(ValueError, match="bytes are needed"):
            PY.layout(data[:n])
    assert PY.need_bytes(data[:hend]) == hend + 16 and PY.layout(data[:hend])["ready_levels"] == []
    assert PY.need_bytes(data[:hend + 16]) == hend + TL.layout(levels[2])["header_end"]


def test_extract_by_level_window_and_rounds_is_shorter_composes_and_is_idempotent():
    levels, data = pyramid()
    assert PY.extract(data) == data and PY.extract(bytearray(data)) == data
    win = (40, 90, 30, 17)
    for keep in ([1], [0, 2], [2, 1], [0, 1, 2]):
        for window in (None, win):
            for rounds in (None, 2, 0):
                ex = PY.extract(data, keep, window, rounds)
                el = PY.layout(ex)
                assert len(ex) == el["total"] and (len(ex) < len(data) or (len(keep) == 3 and window is None and rounds is None))
                assert (el["H"], el["W"], el["n_levels"]) == (H, W, 3) and [lv["present"] for lv in el["levels"]] == [k in keep for k in range(3)]
                for k in keep:
                    want = TL.extract(levels[k], None if window is None else PR.window_at(window, k, H, W), rounds)
                    assert PY.level_stream(ex, k) == want
                assert PY.extract(ex) == ex
                assert PY.need_bytes(ex) == el["header_end"] + TL.need_bytes(PY.level_stream(ex, max(keep)))
    one = PY.extract(data, [1], win, 2)
    assert PY.layout(one)["ready_levels"] == [1] and PY.window_at(win, 1, H, W) == (20, 45, 15, 9)
    assert one == PY.extract(PY.extract(data, [0, 1]), [1], win, 2) == PY.extract(PY.extract(data, rounds=3), [1], win, 2)
    assert one == PY.extract(PY.extract(data, [1, 2], (0, 0, 100, 200)), [1], win, 2)
    with pytest.raises(ValueError, match="level_stream: level 0 is absent from this codestream; it holds the levels \\[1\\]"):
        PY.level_stream(one, 0)
    with pytest.raises(ValueError, match="extract: level 2 is absent"):
        PY.extract(one, [2])
    with pytest.raises(ValueError, match=r"extract: level 1: extract: the window .* needs tile \(1, 1\), which is absent"):
        PY.extract(one, [1], (130, 180, 10, 10))
    with pytest.raises(ValueError, match="extract: level 1: extract: rounds is 0 .. 2"):
        PY.extract(one, rounds=3)
    with pytest.raises(ValueError, match="extract: levels is empty"):
        PY.extract(data, [])
    with pytest.raises(ValueError, match="extract: level is 0 .. 2, got 5"):
        PY.extract(data, [5])
    with pytest.raises(ValueError, match="does not lie inside"):
        PY.extract(data, None, (0, 0, 151, 10))
    cut = data[:PY.layout(data)["levels"][1]["offset"] + 40]                    # level 2 whole, 40 bytes of level 1
    assert PY.extract(cut, [2]) == PY.extract(data, [2])
    with pytest.raises(ValueError, match="extract: level 0: "):
        PY.extract(cut)


# ----------------------------------------------------------------------------------------------------------- refusals
def _u64(header, off, delta):
    struct.pack_into("<Q", header, off, struct.unpack_from("<Q", header, off)[0] + delta)


def test_a_header_that_cannot_be_trusted_is_refused():
    levels, data = pyramid()
    S0 = 12                                                                     # the level sizes follow H, W, n_levels, reserved
    with pytest.raises(ValueError, match="CRC-32 does not match"):
        PY.layout(data[:20] + bytes([data[20] ^ 1]) + data[21:])
    with pytest.raises(ValueError, match="not a pyramid codestream"):
        PY.layout(b"VAMp" + data[4:])
    with pytest.raises(ValueError, match="not a pyramid codestream"):
        PY.layout(levels[0])                                                    # a level's own codestream is no pyramid
    with pytest.raises(ValueError, match="pyramid codestream version 2"):
        PY.layout(data[:4] + b"\x02" + data[5:])
    with pytest.raises(ValueError, match=r"version 1 \(reserved field 1\)"):
        PY.layout(data[:6] + b"\x01" + data[7:])
    with pytest.raises(ValueError, match="a header of 45 bytes"):
        PY.layout(data[:8] + struct.pack("<I", 45) + data[12:])
    with pytest.raises(ValueError, match="bytes follow the codestream"):
        PY.layout(data + b"\0")
    with pytest.raises(ValueError, match="a bytes-like object"):
        PY.layout("VAMy")
    with pytest.raises(ValueError, match="reserved field is 7"):
        PY.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 10, 7)))
    with pytest.raises(ValueError, match="2 levels take 36 bytes, it states 44"):        # a length not implied by n_levels
        PY.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 8, 2)))
    with pytest.raises(ValueError, match="4 levels take 52 bytes, it states 60"):
        PY.layout(_reseal(data, lambda h: (struct.pack_into("<H", h, 8, 4), h.extend(b"\0" * 16))[0]))
    with pytest.raises(ValueError, match="its levels add up to"):               # lengths that do not sum to total
        PY.layout(_reseal(data, lambda h: _u64(h, S0 + 8, 4)))
    with pytest.raises(ValueError, match="its levels add up to"):
        PY.layout(_reseal(data, lambda h: _u64(h, len(h) - 8, 1)))

    def both(h, delta=4):                                                       # sizes and total agree, level 0 (the last) does not
        _u64(h, S0, delta)
        _u64(h, len(h) - 8, delta)
    with pytest.raises(ValueError, match=r"level 0: layout: .* bytes follow the codestream"):
        PY.layout(_reseal(data, both) + b"\0" * 4)
    with pytest.raises(ValueError, match="the header contradicts level 0: it states .* bytes, the level's own header a total of"):
        PY.layout(_reseal(data, lambda h: both(h, -4))[:-4])

    def moved(h):                                                               # four bytes of level 2 counted as level 1's
        _u64(h, S0 + 16, -4)
        _u64(h, S0 + 8, 4)
    with pytest.raises(ValueError, match="level 1: layout: not a picture codestream"):
        PY.layout(_reseal(data, moved))
    with pytest.raises(ValueError, match="level 0 holds a picture of 150 x 200; level 0 of a 151 x 200 picture is 151 x 200"):
        PY.layout(_reseal(data, lambda h: struct.pack_into("<I", h, 0, 151)))
    with pytest.raises(ValueError, match="level 1 holds a picture of 75 x 100; level 1 of a 150 x 201 picture is 75 x 101"):
        PY.layout(_reseal(data, lambda h: struct.pack_into("<I", h, 4, 201))[:PY.layout(data)["levels"][0]["offset"]])
    with pytest.raises(ValueError, match="sides are 1 .. "):
        PY.layout(_reseal(data, lambda h: struct.pack_into("<I", h, 0, 0)))
    with pytest.raises(ValueError, match="holds no level"):
        PY.layout(_reseal(data, lambda h: struct.pack_into("<4Q", h, S0, 0, 0, 0, 16 + len(h)))[:16 + 44])
    assert PY.layout(_reseal(data, lambda h: None))["total"] == len(data)


def test_levels_that_contradict_each_other_and_levels_that_repeat_are_refused():
    levels, data = pyramid()
    with pytest.raises(ValueError, match=r"level 1 and level 0 differ in their marks"):
        PY.pack(H, W, [levels[0], picture(H=75, W=100, tile=TILE, overlap=V, q=(0.5, 2.0, 10.0))[2], levels[2]])
    with pytest.raises(ValueError, match=r"level 2 and level 0 differ in their lanes"):
        PY.pack(H, W, [levels[0], None, picture(H=38, W=50, tile=TILE, overlap=V, K=8)[2]])
    with pytest.raises(ValueError, match=r"level 2 and level 1 differ in their base_lanes"):
        PY.pack(H, W, [None, picture(H=75, W=100, tile=TILE, overlap=V, K=8, Kb=8)[2], picture(H=38, W=50, tile=TILE, overlap=V, K=8, Kb=4)[2]])
    with pytest.raises(ValueError, match=r"level 1 and level 0 differ in their overlap \(8 against 16\)"):
        PY.pack(H, W, [levels[0], picture(H=75, W=100, tile=TILE, overlap=8)[2], levels[2]])
    with pytest.raises(ValueError, match="the levels differ in their tile size"):
        PY.pack(H, W, [levels[0], picture(H=75, W=100, tile=128, overlap=V, shape=(2, 2))[2], levels[2]])
    with pytest.raises(ValueError, match="level 1 holds a picture of 38 x 50"):
        PY.pack(H, W, [levels[0], levels[2], levels[2]])
    with pytest.raises(ValueError, match="level 1: 10 bytes do not hold a picture header"):
        PY.pack(H, W, [levels[0], levels[1][:10], levels[2]])
    with pytest.raises(ValueError, match="pack: no level"):
        PY.pack(H, W, [None, None])
    with pytest.raises(ValueError, match="levels is 1 .. 16, got 17"):
        PY.pack(H, W, [None] * 16 + [levels[0]])
    with pytest.raises(ValueError, match="3 levels of a 2 x 1 picture: level 1 is 1 x 1 already and level 2 would repeat it; at most 2 levels"):
        PY.pack(2, 1, [None, None, levels[2]])
    absent = PY.pack(H, W, [levels[0], None, levels[2]])                         # an absent level is framed as 0 bytes
    lay = PY.layout(absent)
    assert [lv["present"] for lv in lay["levels"]] == [True, False, True] and lay["ready_levels"] == [0, 2]
    assert PY.extract(data, [0, 2]) == absent and PY.level_stream(absent, 0) == levels[0]


def test_every_single_byte_change_of_preamble_and_header_is_refused():
    levels, data = pyramid()
    hend = PY.layout(data)["header_end"]
    for at in range(hend):
        for flip in (0x01, 0x80):
            bad = data[:at] + bytes([data[at] ^ flip]) + data[at + 1:]
            for fn in (PY.layout, lambda d: PY.level_stream(d, 2), lambda d: PY.extract(d, [1], None, 1), PY.need_bytes):
                with pytest.raises(ValueError):
                    fn(bad)
            feed = PY.PyramidFeed()
            with pytest.raises(ValueError):
                feed.feed(bad)
            assert len(feed) == 0 and feed.data == b"" and feed.receivers == []


def test_random_corruptions_raise_nothing_but_valueerror():
    levels, data = pyramid()
    rng = np.random.default_rng(5)
    for _ in range(300):
        bad = bytearray(data[:int(rng.integers(0, len(data) + 1))])
        for at in rng.integers(0, max(len(bad), 1), int(rng.integers(0, 4))):
            if len(bad):
                bad[int(at)] = int(rng.integers(0, 256))
        for fn in (PY.layout, PY.need_bytes, lambda d: PY.level_stream(d, 1), lambda d: PY.extract(d, [2, 0], (10, 10, 50, 50), 1),
                   lambda d: PY.PyramidFeed().feed(d)):
            try:
                fn(bytes(bad))
            except ValueError:
                pass


# ------------------------------------------------------------------------------------------------------- the receiver
def _state(feed):
    """What a test compares of a PyramidFeed's host state."""
    out = [len(feed), feed.data, feed.ready, feed.ready_levels, feed.need(), feed.fed_levels, len(feed.receivers)]
    for r in feed.receivers:
        out.append(None if r is None else (r.data, r.ready, r.need(), None if r.held is None else r.held.tolist(),
                                           None if r.rounds is None else r.rounds.tolist(), r.meta))
    return out


def _check_against_layout(feed, data, n):
    """The host state after ``n`` bytes against ``layout`` / ``need_bytes`` of the concatenation."""
    assert len(feed) == n and feed.data == data[:n]
    need = PY.need_bytes(data[:n])
    assert feed.need() == max(0, need - n) and feed.ready == (n >= need and n >= 16 + 44)
    if n < 16 + 44:
        assert feed.receivers == [] and feed.ready_levels == []
        with pytest.raises(ValueError, match="PyramidFeed.shape: the header is not complete yet"):
            feed.shape
        return
    lay = PY.layout(data[:n])
    assert feed.shape == (H, W) and feed.levels == 3 and feed.shapes == SHAPES and feed.ready_levels == lay["ready_levels"]
    for lv, r in zip(lay["levels"], feed.receivers):
        assert len(r) == lv["held"] and r.data == PY.level_stream(data[:n], lv["level"]) and r.ready == lv["ready"]
        if lv["ready"]:
            assert np.array_equal(r.rounds, TL.PictureFeed().feed(r.data))
            assert all(np.array_equal(r.meta[key], lv["layout"][key]) for key in ("marks", "lanes", "base_lanes", "ns"))


def test_one_byte_chunks_across_the_header_then_uneven_chunks():
    levels, data = pyramid()
    lay = PY.layout(data)
    feed = PY.PyramidFeed()
    assert feed.need() == 16 and not feed.ready and feed.feed(b"") == []
    n = 0
    while n < lay["header_end"] + 40:                                           # byte by byte into level 2's own header
        feed.feed(data[n:n + 1])
        n += 1
        _check_against_layout(feed, data, n)
    assert feed.fed_levels == [2]
    rng = np.random.default_rng(3)
    while n < len(data):
        step = int(rng.choice([1, 7, 100, 1500, 4096]))
        m = min(len(data), n + step)
        was = [lv["held"] for lv in PY.layout(data[:n])["levels"]]
        assert feed.feed(data[n:m]) == PY.layout(data[:m])["ready_levels"]
        now = [lv["held"] for lv in PY.layout(data[:m])["levels"]]
        assert feed.fed_levels == [k for k in (2, 1, 0) if now[k] > was[k]]     # in the order of the body
        n = m
        _check_against_layout(feed, data, n)
    assert feed.ready_levels == [0, 1, 2]
    whole = PY.PyramidFeed()
    assert whole.feed(data) == [0, 1, 2] and whole.fed_levels == [2, 1, 0] and _state(whole) == _state(feed)[:5] + [[2, 1, 0]] + _state(feed)[6:]
    ex = PY.extract(data, [1], (40, 90, 30, 17), 2)                             # an extract feeds like a whole stream
    part = PY.PyramidFeed()
    for a in range(0, len(ex), 53):
        part.feed(ex[a:a + 53])
    assert part.ready_levels == [1] and part.receivers[0] is None and part.receivers[2] is None and part.data == ex
    assert part.receivers[1].data == PY.level_stream(ex, 1)


def test_a_refused_feed_changes_nothing_and_a_correct_feed_continues():
    levels, data = pyramid()
    lay = PY.layout(data)
    off1 = lay["levels"][1]["offset"]
    feed = PY.PyramidFeed()
    feed.feed(data[:10])
    for bad in (b"\xff" * 20, data[10:30] + bytes([data[30] ^ 1]) + data[31:70]):     # a wrong preamble; a damaged header
        before = _state(feed)
        with pytest.raises(ValueError):
            feed.feed(bad)
        assert _state(feed) == before
    with pytest.raises(ValueError, match="PyramidFeed.feed: expected bytes, got str"):
        feed.feed("x")
    feed.feed(data[10:off1 - 5])                                                # five bytes before level 2 ends
    before = _state(feed)
    other = picture(H=75, W=100, tile=TILE, overlap=V, q=(0.5, 2.0, 10.0))[2]    # a level 1 with other marks
    with pytest.raises(ValueError, match="level 2 and level 1 differ in their marks"):      # the chunk ends level 2 and brings level 1's first head
        feed.feed(data[off1 - 5:off1] + other[:TL.layout(other)["head"][0][0][0] + TL.layout(other)["head"][0][0][1]])
    assert _state(feed) == before and not feed.receivers[2].data == levels[2]
    with pytest.raises(ValueError, match="PyramidFeed.feed: level 1: PyramidFeed level 1.feed: .*CRC-32 does not match"):
        feed.feed(data[off1 - 5:off1 + 20] + bytes([data[off1 + 20] ^ 1]) + data[off1 + 21:off1 + 2000])
    assert _state(feed) == before
    with pytest.raises(ValueError, match=rf"PyramidFeed.feed: {len(data) + 1} bytes, the header states a total of {len(data)}"):
        feed.feed(data[off1 - 5:] + b"\0")
    assert _state(feed) == before
    feed.feed(data[off1 - 5:off1 + 3])                                          # the true bytes continue
    assert feed.fed_levels == [2, 1] and feed.receivers[2].data == levels[2] and len(feed.receivers[1]) == 3
    feed.feed(data[off1 + 3:])
    assert feed.data == data and feed.ready_levels == [0, 1, 2]
    with pytest.raises(ValueError, match="1 bytes follow the codestream"):
        feed.feed(b"\0")
    assert feed.data == data
