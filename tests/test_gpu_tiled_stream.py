"""The receiver of tiled pictures end to end on the GPU (vampic.tiled.PictureStream / Canvas, evaluate.tiled_stream_rd, DESIGN
section 9y): after any sequence of feeds and views, ``view`` equals a fresh ``PictureDecoder`` on everything fed so far, bit
for bit and error for error, while only the tiles that are not cached run the network; a canvas that is refreshed equals
the view.  Nothing is asserted about PSNR values: the synthetic weights are untrained."""
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_embedded_schedule import _net                         # noqa: E402
from test_gpu_tiled import MAIN, MARKS, _coded as _plain            # noqa: E402
from test_gpu_tiled_allocation import _coded as _pooled             # noqa: E402
from test_gpu_tiled_schedule import _coded as _scheduled            # noqa: E402
from test_tiled_cpu import _reseal                                  # noqa: E402
from vampic import evaluate as EV, tiled as TL                     # noqa: E402

WINDOWS = [(70, 20, 20, 24), (40, 90, 30, 17), (131, 181, 19, 19), (48, 96, 1, 1)]     # core, band, bottom-right, corner
_FRESH, _SHARED = {}, {}


def _fresh(tag, data, n, **kw):
    """A fresh PictureDecoder on ``data[:n]``, built once per prefix."""
    key = (tag, n, tuple(sorted(kw.items())))
    if key not in _FRESH:
        _FRESH[key] = TL.PictureDecoder(_net(), data[:n], **kw)
    return _FRESH[key]


def _feed_unevenly(stream, data, n):
    """Feeds ``data[len(stream.data):n]`` in three chunks: one byte, about a third, the rest."""
    at = len(stream.feed_state)
    for end in (min(n, at + 1), at + (n - at) // 3 + 1, n):
        if end > at:
            stream.feed(data[at:end])
            at = end
    assert len(stream.feed_state) == n


def _shared(tag, data, n, **kw):
    """One PictureStream per tag that only moves forward: fed up to ``n`` bytes (a new one when it is past them)."""
    if tag not in _SHARED or len(_SHARED[tag].feed_state) > n:
        _SHARED[tag] = TL.PictureStream(_net(), **kw)
    _feed_unevenly(_SHARED[tag], data, n)
    return _SHARED[tag]


def _whole_view(st, g):
    """``st.view()``, which must run exactly the tiles whose own bytes grew since this stream's last whole view."""
    seen = st.__dict__.setdefault("_seen_by_test", {})
    held = st.held
    stale = [rc for rc in TL.tiles_for(g) if seen.get(rc) != int(held[rc])]
    out = st.view()
    assert st.last_decoded == stale and st.last_tiles == TL.tiles_for(g)
    seen.update({rc: int(held[rc]) for rc in TL.tiles_for(g)})
    return out, stale


def _cuts(lay):
    inside = (lay["round_end"][1] + 2 * lay["round_end"][2]) // 3 + 1          # inside round 2, not at a word boundary
    return sorted([lay["need_bytes"], *lay["round_end"], inside])            # the last mark is 10: its round end is the total, twice


@pytest.mark.parametrize("i", range(7))
def test_after_every_feed_a_view_is_the_fresh_decode(i):
    x, g, data = _plain(**MAIN)
    lay = TL.layout(data)
    cuts = _cuts(lay)
    assert len(cuts) == 7 and cuts[0] == lay["need_bytes"] and cuts[-1] == cuts[-2] == len(data)
    n = cuts[i]
    st = _shared("plain", data, n, group=5)
    assert st.ready and st.need() == 0 and st.shape == (150, 200) and not st.scheduled and st.stages == 0
    assert all(st.grid[key] == g[key] for key in st.grid)
    dec = _fresh("plain", data, n, group=4)
    assert np.array_equal(st.rounds, dec.rounds) and all(st.meta[key] == dec.meta[key] for key in ("marks", "lanes", "base_lanes", "ns", "format"))
    assert torch.equal(_whole_view(st, g)[0], dec.decode())                     # runs exactly the tiles whose own bytes grew
    for win in WINDOWS:
        assert torch.equal(st.view(win), dec.decode(win)), win
        assert st.last_tiles == dec.last_tiles == TL.tiles_for(g, win) and st.last_decoded == []
    assert torch.equal(st.view(WINDOWS[1], dtype=torch.uint8), dec.decode(WINDOWS[1], dtype=torch.uint8)) and st.last_decoded == []
    total = st.decoded_total
    assert torch.equal(st.view(), st.view()) and st.decoded_total == total and st.last_decoded == []


def test_a_quality_and_a_mark_are_cached_under_their_own_keys():
    x, g, data = _plain(**MAIN)
    lay = TL.layout(data)
    n = lay["round_end"][2]
    st = TL.PictureStream(_net(), group=4, cache_tiles=32)
    _feed_unevenly(st, data, lay["round_end"][1])
    dec1 = _fresh("plain", data, lay["round_end"][1], group=4)
    win = WINDOWS[1]
    assert torch.equal(st.view(win, q=0.5), dec1.decode(win, q=0.5)) and len(st.last_decoded) == 4
    assert torch.equal(st.view(win), dec1.decode(win)) and len(st.last_decoded) == 4                    # another key of the same tiles
    _feed_unevenly(st, data, n)
    dec = _fresh("plain", data, n, group=4)
    assert torch.equal(st.view(win, q=0.5), dec.decode(win, q=0.5)) and st.last_decoded == []          # a level never goes stale
    assert torch.equal(st.view(win, mark=1, dtype=torch.uint8), dec.decode(win, mark=1, dtype=torch.uint8)) and len(st.last_decoded) == 4
    assert torch.equal(st.view(q=0.5), dec.decode(q=0.5)) and st.last_decoded == [t for t in TL.tiles_for(g) if t not in TL.tiles_for(g, win)]
    assert torch.equal(st.view(win), dec.decode(win)) and len(st.last_decoded) == 4                     # the bytes of all four grew
    st.drop()
    assert torch.equal(st.view(win), dec.decode(win)) and len(st.last_decoded) == 4


def test_a_moved_window_decodes_the_new_tiles_and_a_feed_makes_its_tiles_stale():
    x, g, data = _plain(**MAIN)
    lay = TL.layout(data)
    n = lay["round_end"][1]
    st = TL.PictureStream(_net(), group=4)
    st.feed(data[:n])
    dec = _fresh("plain", data, n, group=4)
    a, b = (0, 0, 64, 64), (0, 48, 64, 64)                                      # moved by one stride
    assert TL.tiles_for(g, a) == [(0, 0), (0, 1), (1, 0), (1, 1)] and TL.tiles_for(g, b) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    assert torch.equal(st.view(a), dec.decode(a)) and st.last_decoded == TL.tiles_for(g, a)
    assert torch.equal(st.view(b), dec.decode(b)) and st.last_decoded == [(0, 2), (1, 2)] and st.decoded_total == 6
    o, size = lay["piece"][2][1][0]                                             # up to the middle of tile (1, 0)'s piece of round 2
    m = o + size // 2
    st.feed(data[n:m])
    assert st.fed_tiles == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)]
    dec = _fresh("plain", data, m, group=4)
    assert torch.equal(st.view(b), dec.decode(b)) and st.last_decoded == [(0, 0), (0, 1), (0, 2), (1, 0)]
    st.feed(b"")
    assert st.fed_tiles == [] and torch.equal(st.view(b), dec.decode(b)) and st.last_decoded == []


def test_a_cache_of_one_window_evicts_and_refuses_a_larger_window():
    x, g, data = _plain(**MAIN)
    st = TL.PictureStream(_net(), group=4, cache_tiles=4)
    st.feed(data)
    dec = _fresh("plain", data, len(data), group=4)
    a, b = (0, 0, 64, 64), (100, 150, 50, 50)
    assert TL.tiles_for(g, b) == [(1, 2), (1, 3), (2, 2), (2, 3)] and not set(TL.tiles_for(g, a)) & set(TL.tiles_for(g, b))
    want = {a: dec.decode(a), b: dec.decode(b)}
    for win in (a, b, a, b, b):
        assert torch.equal(st.view(win), want[win])
    assert st.decoded_total == 16 and st.last_decoded == [] and st.cache_tiles == 4 and tuple(st._pool.shape) == (4, 3, 64, 64)
    with pytest.raises(ValueError, match=r"PictureStream.view: the window \(0, 0, 150, 200\) needs 12 tiles, the cache holds 4"):
        st.view()
    with pytest.raises(ValueError, match="needs 6 tiles, the cache holds 4"):
        st.canvas((0, 48, 64, 64)).refresh()
    assert st.decoded_total == 16 and torch.equal(st.view(b), want[b]) and st.last_decoded == []
    assert TL.PictureStream(_net(), group=5).feed(data[:40]) is None            # defaults: a 1024 x 1024 window, at least the group
    full = TL.PictureStream(_net(), group=16)
    full.feed(data)
    assert full.cache_tiles == 16 and full.group == 16


def test_picture_wide_marks_and_a_resealed_threshold():
    net = _net()
    x, g, data = _pooled()
    lay = TL.layout(data)
    assert data[4] == 2 and lay["allocation"] == "picture"
    st = TL.PictureStream(net, group=4)
    _feed_unevenly(st, data, lay["round_end"][2])
    dec = _fresh("pooled", data, lay["round_end"][2], group=4)
    assert torch.equal(st.view(mark=2), dec.decode(mark=2)) and len(st.last_decoded) == 12
    assert torch.equal(st.view(WINDOWS[1], q=MARKS[1]), dec.decode(WINDOWS[1], q=MARKS[1])) and len(st.last_decoded) == 4
    assert torch.equal(st.view(WINDOWS[3], mark=1), dec.decode(WINDOWS[3], mark=1)) and st.last_decoded == []      # q = 0.5 is mark 1
    with pytest.raises(ValueError, match="PictureStream.view: quality 1.0 is not marked; this picture's marks are picture-wide"):
        st.view(q=1.0)
    ext = 20 + 4 * 12 * 6                                                       # fixed fields, the table of 12 x (1 + 5)
    k, j = 1, 0
    assert lay["thresholds"][2, j] < lay["thresholds"][k, j]

    def edit(h):
        struct.pack_into("<f", h, ext + 8 + 4 * (k * net.ns0 + j), float(lay["thresholds"][2, j]))      # mark 1 with mark 2's threshold
    bad = _reseal(data, edit)
    with pytest.raises(ValueError) as fresh:
        TL.PictureDecoder(net, bad, group=4).decode(mark=2)
    sb = TL.PictureStream(net, group=4)
    sb.feed(bad[:1000])
    sb.feed(bad[1000:])
    with pytest.raises(ValueError) as mine:
        sb.view(mark=2)
    assert "picture-wide threshold" in str(fresh.value) and f"mark {k}, slice {j}" in str(fresh.value)
    assert str(mine.value) == str(fresh.value).replace("PictureDecoder.decode:", "PictureStream.view:")
    assert sb.decoded_total == 0 and sb._entries == {}                          # a decode that raises leaves the cache as it was


@pytest.mark.parametrize("k", range(6))
def test_a_scheduled_stream_fed_stage_by_stage(k):
    x, g, data = _scheduled(**MAIN)
    lay = TL.layout(data)
    piece = lay["piece"]
    n = lay["round_end"][k]                                                     # k = 5: what follows the last stage
    if k == 0:
        st = _SHARED["scheduled"] = TL.PictureStream(_net(), group=4, cache_tiles=48)    # from the heads on: the first picture, then stage 0
        _feed_unevenly(st, data, lay["need_bytes"])
        base = _fresh("scheduled", data, lay["need_bytes"], group=4)
        assert st.scheduled and st.stages == 5 and torch.equal(_whole_view(st, g)[0], base.decode()) and len(st.last_decoded) == 12
        was = lay["need_bytes"]
    else:
        was = len(_SHARED["scheduled"].feed_state) if "scheduled" in _SHARED else None
        was = was if was is not None and "_seen_by_test" in _SHARED["scheduled"].__dict__ else None
    st = _shared("scheduled", data, n, group=4, cache_tiles=48)             # every key this test asks for stays cached
    dec = _fresh("scheduled", data, n, group=4)
    fed_now = [(r, c) for r, c in TL.tiles_for(g) if piece[k][r][c][1] > 0]
    got, stale = _whole_view(st, g)
    assert torch.equal(got, dec.decode())
    if was == ([lay["need_bytes"]] + lay["round_end"])[k]:                      # the stage before was viewed: only this stage's tiles run
        assert stale == fed_now
    if k in (1, 2):                                                             # the region climbs: the boxes' tiles, no background-only tile
        assert {(0, 1), (0, 2), (1, 1), (1, 2), (2, 3)} <= set(fed_now) and (2, 0) not in fed_now and len(fed_now) < 12
    window = (58, 100, 20, 20)
    kk = min(k, 4)
    assert torch.equal(st.view(window, stage=kk), dec.decode(window, stage=kk)) and st.last_tiles == [(0, 1), (0, 2), (1, 1), (1, 2)]
    assert torch.equal(st.view(window, stage=kk), dec.decode(window, stage=kk)) and st.last_decoded == []
    if k == 3:
        cached = sum((i, ("stage", 1)) in st._entries for i in range(12))       # from the feed of stage 1, when that ran on this stream
        assert torch.equal(st.view(stage=1), dec.decode(stage=1)) and len(st.last_decoded) == 12 - cached and cached in (0, 4)
        with pytest.raises(ValueError, match=r"PictureStream.view: this picture is scheduled \(5 stages\).* decode a stage with stage=0 .. 4"):
            st.view(q=2.5)
        with pytest.raises(ValueError, match=r"PictureStream.view: tile \(\d, \d\): .*stage 4 needs"):
            st.view(stage=4)
        with pytest.raises(ValueError, match="PictureStream.view: stage is 0 .. 4, got 5"):
            st.view(stage=5)


def _box_of(g, tiles, window):
    cy0, cx0, ch, cw = window
    rows, cols = sorted({r for r, _ in tiles}), sorted({c for _, c in tiles})
    y0, y1 = max(cy0, rows[0] * g["Sy"]), min(cy0 + ch, rows[-1] * g["Sy"] + g["th"])
    x0, x1 = max(cx0, cols[0] * g["Sx"]), min(cx0 + cw, cols[-1] * g["Sx"] + g["tw"])
    return (y0, x0, y1 - y0, x1 - x0)


def test_a_canvas_is_refreshed_where_tiles_changed_and_equals_the_view():
    x, g, data = _plain(**MAIN)
    lay = TL.layout(data)
    st = TL.PictureStream(_net(), group=4, cache_tiles=24)
    st.feed(data[:lay["header_end"]])
    whole, part = st.canvas(), st.canvas((60, 31, 85, 101), dtype=torch.uint8)
    assert tuple(whole.out.shape) == (3, 150, 200) and part.out.dtype == torch.uint8 and tuple(part.out.shape) == (85, 101, 3)
    with pytest.raises(ValueError, match="Canvas.refresh: nothing to decode yet: .* bytes are missing"):
        whole.refresh()
    o, size = lay["piece"][2][1][1]                                             # ends inside tile (1, 1)'s piece of round 2
    cuts = [lay["need_bytes"], lay["round_end"][1], o + size // 2, len(data)]
    part_tiles = TL.tiles_for(g, part.window)
    assert len(part_tiles) == 9
    for i, n in enumerate(cuts):
        before = st.held.copy() if st.ready else None
        _feed_unevenly(st, data, n)
        grown = [rc for rc in TL.tiles_for(g) if before is None or st.held[rc] > before[rc]]
        assert len(grown) == (6 if i == 2 else 12)                              # the third step ends inside a round
        assert whole.refresh() == _box_of(g, grown, whole.window) and st.last_decoded == grown
        total = st.decoded_total
        assert torch.equal(whole.out, st.view())
        assert part.refresh() == _box_of(g, [t for t in part_tiles if t in grown], part.window)
        assert torch.equal(part.out, st.view(part.window, dtype=torch.uint8))
        assert whole.refresh() is None and part.refresh() is None and st.decoded_total == total          # nothing changed: nothing runs
        if i == 2:
            assert _box_of(g, grown, whole.window) == (0, 0, 112, 200) and _box_of(g, grown, part.window) == (60, 31, 52, 101)
            assert torch.equal(whole.out, _fresh("plain", data, n, group=4).decode())
    dec = _fresh("plain", data, len(data), group=4)
    assert torch.equal(whole.out, dec.decode()) and torch.equal(part.out, dec.decode(part.window, dtype=torch.uint8))
    assert whole.refresh(q=0.5) == (0, 0, 150, 200) and torch.equal(whole.out, dec.decode(q=0.5))        # a key change: the whole window
    assert whole.refresh(q=0.5) is None
    assert whole.refresh() == (0, 0, 150, 200) and torch.equal(whole.out, dec.decode()) and st.last_decoded == []
    assert part.refresh(mark=1) == part.window and torch.equal(part.out, dec.decode(part.window, mark=1, dtype=torch.uint8))


def test_the_device_coder_on_lanes_gives_the_host_coder_s_pixels():
    x, g, data = _plain(**MAIN, lanes=64, base_lanes=8)
    lay = TL.layout(data)
    assert (lay["lanes"], lay["base_lanes"]) == (64, 8)
    n = lay["round_end"][1]
    views = []
    for coder in ("host", "device"):
        st = TL.PictureStream(_net(), coder=coder, group=4)
        _feed_unevenly(st, data, n)
        first = st.view(WINDOWS[1])
        _feed_unevenly(st, data, len(data))
        views.append((first, st.view(WINDOWS[1]), st.view(WINDOWS[1], q=0.5)))
    assert all(torch.equal(a, b) for a, b in zip(*views))
    dec = TL.PictureDecoder(_net(), data, coder="device", group=4)
    assert torch.equal(views[1][1], dec.decode(WINDOWS[1])) and torch.equal(views[1][2], dec.decode(WINDOWS[1], q=0.5))


def test_an_unaligned_stride_end_to_end():
    x, g, data = _plain(100, 70, 64, 8, group=3)
    assert (g["R"], g["C"], g["Sy"]) == (2, 2, 56)
    lay = TL.layout(data)
    st = TL.PictureStream(_net(), group=3)
    canvas = None
    for n in (lay["need_bytes"], lay["round_end"][1] + 5, len(data)):
        _feed_unevenly(st, data, n)
        canvas = st.canvas(dtype=torch.uint8) if canvas is None else canvas
        dec = TL.PictureDecoder(_net(), data[:n], group=3)
        assert torch.equal(st.view(), dec.decode()) and torch.equal(st.view((33, 9, 60, 50)), dec.decode((33, 9, 60, 50)))
        assert canvas.refresh() is not None and torch.equal(canvas.out, dec.decode(dtype=torch.uint8))


def test_refusals_by_message():
    net = _net()
    x, g, data = _plain(**MAIN)
    lay = TL.layout(data)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="PictureStream: cache_tiles"):
            TL.PictureStream(net, cache_tiles=bad)
    with pytest.raises(ValueError, match="PictureStream: group"):
        TL.PictureStream(net, group=0)
    st = TL.PictureStream(net, group=4)
    with pytest.raises(ValueError, match=f"PictureStream.view: nothing to decode yet: {TL.PREAMBLE_BYTES} bytes are missing"):
        st.view()
    with pytest.raises(ValueError, match="PictureStream.canvas: the header is not complete yet"):
        st.canvas()
    st.feed(data[:lay["need_bytes"] - 1])
    with pytest.raises(ValueError, match="PictureStream.view: nothing to decode yet: 1 bytes are missing"):
        st.view()
    with pytest.raises(ValueError, match="PictureStream.feed: expected bytes, got str"):
        st.feed("x")
    st.feed(data[lay["need_bytes"] - 1:lay["round_end"][0]])
    with pytest.raises(ValueError, match=rf"PictureStream.feed: {len(data) + 1} bytes, the header states a total of {len(data)}"):
        st.feed(data[lay["round_end"][0]:] + b"\0")
    assert len(st.data) == lay["round_end"][0]
    assert st.view(WINDOWS[0]).shape == (3, 20, 24) and st.decoded_total == 1
    entries = dict(st._entries)
    with pytest.raises(ValueError, match=r"PictureStream.view: tile \([01], [12]\): .*quality 0.5 needs"):
        st.view(WINDOWS[1], q=0.5)                                              # the bytes end before q: as the fresh decoder says
    assert st._entries == entries and st.decoded_total == 1 and st.last_tiles == TL.tiles_for(g, WINDOWS[0])
    for kw, text in ((dict(dtype=torch.float16), "PictureStream.view: dtype is torch.float32 or torch.uint8"),
                     (dict(q=0.5, mark=1), "PictureStream.view: give q or mark, not both"),
                     (dict(mark=4), r"PictureStream.view: mark is 0 .. 3 \(the marks \[0.05, 0.5, 2.5, 10.0\]\), got 4"),
                     (dict(stage=0), "PictureStream.view: stage= decodes a scheduled picture"),
                     (dict(window=(0, 0, 151, 1)), r"PictureStream.view: the window \(y0 0, x0 0, h 151, w 1\) does not lie inside")):
        with pytest.raises(ValueError, match=text):
            st.view(**kw)
    with pytest.raises(ValueError, match="PictureStream.canvas: dtype is torch.float32 or torch.uint8"):
        st.canvas(dtype=torch.int32)
    ex = TL.PictureStream(net)
    ex.feed(TL.extract(data, WINDOWS[1], rounds=1))
    assert (ex.held[2] == -1).all() and ex.view(WINDOWS[1]).shape == (3, 30, 17)
    with pytest.raises(ValueError, match=r"PictureStream.view: the window \(40, 60, 30, 47\) needs tile \(0, 0\), which is absent"):
        ex.view((40, 60, 30, 47))


def test_tiled_stream_rd_decodes_a_tile_once_per_held_size():
    net = _net()
    x, g, data = _plain(**MAIN)
    lay = TL.layout(data)
    rows = EV.tiled_stream_rd(net, x, tile=64, overlap=16, marks=MARKS, group=4)
    cuts = sorted({lay["need_bytes"], *lay["round_end"]})
    assert [r["bytes"] for r in rows] == cuts and all(r["tiles"] == 12 and r["bpp"] == 8.0 * r["bytes"] / (150 * 200) for r in rows)
    assert all(np.isfinite(r["psnr"]) for r in rows) and rows[0]["decoded"] == 12
    f, sizes = TL.PictureFeed(), set()
    for a, b in zip([0] + cuts, cuts):
        f.feed(data[a:b])
        sizes |= {(rc, int(f.held[rc])) for rc in TL.tiles_for(g)}
    assert sum(r["decoded"] for r in rows) <= len(sizes)
    win = WINDOWS[1]
    inside = (lay["round_end"][1] + 2 * lay["round_end"][2]) // 3 + 1
    rows = EV.tiled_stream_rd(net, x, [lay["need_bytes"], inside, inside, len(data)], win, tile=64, overlap=16, marks=MARKS, group=4)
    assert [r["tiles"] for r in rows] == [4] * 4 and rows[0]["decoded"] == 4 and rows[2]["decoded"] == 0 and rows[3]["decoded"] == 4
    with pytest.raises(ValueError, match="tiled_stream_rd: cuts are ascending byte positions"):
        EV.tiled_stream_rd(net, x, [lay["need_bytes"] - 1], tile=64, overlap=16, marks=MARKS, group=4)
