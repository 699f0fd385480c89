"""Filled pyramid views end to end on the GPU (``PyramidDecoder.decode(fill=True)``, ``PyramidStream.view(fill=True)``, DESIGN
section 9za): at cuts derived from the layouts — the thumbnail alone, inside level 1's heads, inside level 0's heads, inside
level 0's round 0, the whole stream — every filled view equals the restatement's chain (tests/fill_ref.py) over per-tile
decodes made with ``embedded.EmbeddedDecoder`` on ``tiled.tile_stream`` alone, bit for bit; the receiver gives the fresh
decoder's pixels and runs the network only for tiles whose bytes grew; an extract of a window plus the thumbnail shows the
window sharp inside a filled surround."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fill_ref as FR                                              # noqa: E402
import tiled_ref as TR                                             # noqa: E402
from test_gpu_embedded_schedule import _net, _x                    # noqa: E402
from test_gpu_tiled import MAIN, MARKS                             # noqa: E402
from vampic import embedded as EB, pyramid as PY, tiled as TL    # noqa: E402

H, W = MAIN["H"], MAIN["W"]
KW = dict(tile=MAIN["tile"], overlap=MAIN["overlap"], group=4)
SHAPES = [(150, 200), (75, 100), (38, 50)]
WINDOWS = {0: [None, (40, 90, 30, 17), (56, 30, 60, 150)], 1: [None, (20, 45, 15, 9), (40, 3, 30, 90)]}
_DATA, _TILE, _DEC = [], {}, {}


def _coded():
    if not _DATA:
        _DATA.append(PY.encode(_net(), _x(1, H, W)[0], marks=MARKS, **KW))
    return _DATA[0]


def _cuts():
    """The byte counts of the five cuts, every one from the layouts."""
    data = _coded()
    lay = PY.layout(data)
    off = [lv["offset"] for lv in lay["levels"]]
    l0, l1 = lay["levels"][0]["layout"], lay["levels"][1]["layout"]
    assert [(lv["layout"]["R"], lv["layout"]["C"]) for lv in lay["levels"]] == [(3, 4), (2, 2), (1, 1)]
    head_end = lambda l, i: sum(l["head"][i // l["C"]][i % l["C"]])
    cuts = {"need": lay["need_bytes"], "level 1: 2 heads": off[1] + head_end(l1, 1), "level 0: 5 heads": off[0] + head_end(l0, 4) + 3,
            "level 0: in round 0": off[0] + (l0["need_bytes"] + l0["round_end"][0]) // 2, "whole": len(data)}
    assert list(cuts.values()) == sorted(cuts.values()) and len(set(cuts.values())) == 5
    return cuts


CUTS = ["need", "level 1: 2 heads", "level 0: 5 heads", "level 0: in round 0", "whole"]


def _tile(stream, mark):
    """One tile's pixels from its own bytes alone, float32 [3, 64, 64]; decoded once per (bytes, mark)."""
    key = (stream, mark)
    if key not in _TILE:
        dec = EB.EmbeddedDecoder(_net(), [EB.from_bytes(stream)])
        _TILE[key] = (dec.decode() if mark is None else dec.decode_marks([mark])[0])["x_hat"][0].cpu().numpy()
    return _TILE[key]


def _levels(prefix, mark=None):
    """What fill_ref.chain takes, from ``layout`` alone: per usable level (tiles, slot, grid), None for the others; a tile is
    available when the prefix holds its head and, at a mark m, its pieces 0 .. m."""
    lay = PY.layout(prefix)
    out = []
    for lv in lay["levels"]:
        l = lv["layout"]
        if l is None:
            out.append(None)
            continue
        part = PY.level_stream(prefix, lv["level"])
        tiles, slot = [], np.full((l["R"], l["C"]), -1)
        for r in range(l["R"]):
            for c in range(l["C"]):
                segs = [l["head"][r][c]] + [l["piece"][k][r][c] for k in range(0 if mark is None else mark + 1)]
                if l["present"][r][c] and all(n == 0 or o + n <= len(part) for o, n in segs):       # a piece of 0 bytes is whole
                    slot[r, c] = len(tiles)
                    tiles.append(_tile(TL.tile_stream(part, r, c), mark))
        g = {k: l[k] for k in ("H", "W", "th", "tw", "V", "Sy", "Sx", "R", "C")}
        out.append((np.stack(tiles) if tiles else np.zeros((0, 3, l["th"], l["tw"]), np.float32), slot, g))
    return out


def _fresh(n):
    if n not in _DEC:
        _DEC[n] = PY.PyramidDecoder(_net(), _coded()[:n], group=4)
    return _DEC[n]


def _same(got, want):
    got = got.cpu().numpy()
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _full(win, k):
    return win if win is not None else (0, 0) + SHAPES[k]


@pytest.mark.parametrize("cut", CUTS)
def test_a_filled_view_is_the_restatement_s_chain_at_every_cut(cut):
    n = _cuts()[cut]
    dec = _fresh(n)
    levels = _levels(_coded()[:n])
    avail = [None if lv is None else int((lv[1] >= 0).sum()) for lv in levels]
    assert avail == {"need": [None, None, 1], "level 1: 2 heads": [None, 2, 1], "level 0: 5 heads": [5, 4, 1],
                     "level 0: in round 0": [12, 4, 1], "whole": [12, 4, 1]}[cut]
    assert dec.usable == [lv is not None for lv in levels]
    for k in (0, 1):
        for win in WINDOWS[k]:
            want = FR.chain(levels, SHAPES, _full(win, k), k)
            assert _same(dec.decode(win, level=k, fill=True), want), (k, win)
            assert [e[0] for e in dec.last_chain][0] == k and all(e[1] == e[2] for e in dec.last_chain)     # a fresh decoder decodes what it composes
            assert _same(dec.decode(win, level=k, fill=True, dtype=torch.uint8), TR.to_u8(want)), (k, win)
    assert torch.equal(dec.decode(level=2, fill=True), dec.decode(level=2)) and dec.last_chain == [(2, [(0, 0)], [(0, 0)])]
    if cut == "need":                                                           # the level-0 view is the d = 2 upsample of level 2's decode
        thumb = dec.decode(level=2).cpu().numpy()
        assert _same(dec.decode(level=0, fill=True), FR.upsample(thumb, (0, 0, 38, 50), (0, 0, 150, 200), 2, 38, 50))
        assert dec.last_chain == [(0, [], []), (2, [(0, 0)], [(0, 0)])]
        win = WINDOWS[0][1]
        src = FR.source_window(win, 2, 38, 50)
        assert _same(dec.decode(win, fill=True), FR.upsample(dec.decode(src, level=2).cpu().numpy(), src, win, 2, 38, 50))
    if cut == "level 0: 5 heads":
        dec.decode(level=0, fill=True)
        five, row, four = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0)], [(0, 0), (0, 1), (0, 2), (0, 3)], [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert dec.last_chain == [(0, five, five), (1, four, four)]
        dec.decode((0, 0, 40, 200), fill=True)                                  # all of its tiles are there: the chain ends at level 0
        assert dec.last_chain == [(0, row, row)]
        part = TL.PictureDecoder(_net(), PY.level_stream(_coded()[:n], 0), group=4, partial=True)
        assert part.rounds.tolist() == [[0] * 4, [0, -1, -1, -1], [-1] * 4] and part.available() == five
        assert torch.equal(dec.decode((0, 0, 40, 200), fill=True), part.decode((0, 0, 40, 200)))
        with pytest.raises(ValueError, match=r"PictureDecoder.decode: the window \(60, 60, 10, 10\) needs tile \(1, 1\), whose head has not arrived"):
            part.decode((60, 60, 10, 10))
        with pytest.raises(ValueError, match="PictureDecoder: .* bytes end before the heads of the tiles do"):      # as ever without partial
            TL.PictureDecoder(_net(), PY.level_stream(_coded()[:n], 0), group=4)
    if cut == "whole":                                                          # every tile has arrived: fill changes nothing
        for k in (0, 1, 2):
            for win in WINDOWS.get(k, [None]):
                for dtype in (None, torch.uint8):
                    assert torch.equal(dec.decode(win, level=k, fill=True, dtype=dtype), dec.decode(win, level=k, dtype=dtype)), (k, win)
                assert dec.last_chain == [(k, dec.last_tiles, dec.last_tiles)]


def test_the_receiver_gives_the_fresh_decoder_s_pixels_and_decodes_only_what_grew():
    net, data, cuts = _net(), _coded(), _cuts()
    st = PY.PyramidStream(net, group=4)
    with pytest.raises(ValueError, match="PyramidStream.view: nothing to decode yet: the header is not complete, 16 bytes are missing"):
        st.view(fill=True)
    lay = PY.layout(data)
    st.feed(data[:lay["header_end"] + 30])                                      # inside the coarsest level's header
    assert st.need() > 0
    with pytest.raises(ValueError, match=rf"PyramidStream.view: nothing to fill level 0 from: .*; {st.need()} bytes are missing"):
        st.view(fill=True)
    st.feed(data[len(st.data):lay["need_bytes"] - 5])                           # its header is whole, its one head is not
    with pytest.raises(ValueError, match=r"PyramidStream.view: level 2: .*needs tile \(0, 0\), whose head has not arrived: 5 bytes are missing"):
        st.view(fill=True)
    seen = {}                                                                   # (level, tile) -> the bytes it held when it last ran the network
    for cut in CUTS:
        n = cuts[cut]
        st.feed(data[len(st.data):n])
        dec = _fresh(n)
        for k, win in ((0, None), (0, WINDOWS[0][2]), (1, None), (0, None)):
            got = st.view(win, level=k, fill=True)
            assert torch.equal(got, dec.decode(win, level=k, fill=True)), (cut, k, win)
            assert [(e[0], e[1]) for e in st.last_chain] == [(e[0], e[1]) for e in dec.last_chain]
            assert (st.last_tiles, st.last_decoded) == st.last_chain[0][1:]
            for j, composed, ran in st.last_chain:
                part = PY.level_stream(data[:n], j) if composed else b""
                held = {rc: len(TL.tile_stream(part, *rc)) for rc in composed}
                assert ran == [rc for rc in composed if seen.get((j, rc)) != held[rc]], (cut, k, win, j)
                seen.update({(j, rc): held[rc] for rc in ran})
        assert st.last_chain[0][2] == [] and torch.equal(st.view(level=0, fill=True, dtype=torch.uint8), dec.decode(level=0, fill=True, dtype=torch.uint8))
    assert torch.equal(st.view(fill=True), st.view()) and st.last_decoded == []


def test_a_mark_falls_back_where_a_tile_lacks_its_round():
    n = _cuts()["level 0: in round 0"]
    prefix = _coded()[:n]
    dec = _fresh(n)
    levels = _levels(prefix, mark=0)
    have = int((levels[0][1] >= 0).sum())
    assert 0 < have < 12 and dec.decoder(0).rounds.min() == 0 and int((dec.decoder(0).rounds >= 1).sum()) == have
    assert (levels[1][1] >= 0).all() and (levels[2][1] >= 0).all()
    for win in WINDOWS[0]:
        assert _same(dec.decode(win, mark=0, fill=True), FR.chain(levels, SHAPES, _full(win, 0), 0)), win
    dec.decode(mark=0, fill=True)
    sharp = [(r, c) for r in range(3) for c in range(4) if levels[0][1][r, c] >= 0]
    assert dec.last_chain[0] == (0, sharp, sharp) and dec.last_chain[1][0] == 1
    assert not torch.equal(dec.decode(mark=0, fill=True), dec.decode(fill=True))
    assert torch.equal(dec.decode(fill=True), dec.decode())                     # without a mark every head suffices
    st = PY.PyramidStream(_net(), group=4)
    st.feed(prefix)
    assert torch.equal(st.view(mark=0, fill=True), dec.decode(mark=0, fill=True)) and st.last_tiles == sharp
    with pytest.raises(ValueError, match=r"mark is 0 .. 3"):
        dec.decode(mark=4, fill=True)


def test_an_extract_of_a_window_and_the_thumbnail_shows_the_window_sharp():
    net, data = _net(), _coded()
    win = (70, 80, 20, 30)                                                      # in tiles (1, 1) and (1, 2), across their band
    ex = PY.pack(H, W, [TL.extract(PY.level_stream(data, 0), win), None, PY.level_stream(data, 2)])
    assert len(ex) < len(data) // 2
    dec = PY.PyramidDecoder(net, ex, group=4)
    assert dec.usable == [True, False, True]
    levels = _levels(ex)
    kept = TL.tiles_for(TL.grid(H, W, 64, 16), win)
    assert levels[1] is None and sorted(zip(*np.nonzero(levels[0][1] >= 0))) == kept and 1 < len(kept) < 12
    got = dec.decode(fill=True)
    assert _same(got, FR.chain(levels, SHAPES, (0, 0, H, W), 0)) and dec.last_chain == [(0, kept, kept), (2, [(0, 0)], [(0, 0)])]
    full = _fresh(len(data))
    assert torch.equal(dec.decode(win, fill=True), full.decode(win)) and dec.last_chain == [(0, kept, kept)]       # the window is sharp
    sharp = torch.from_numpy(FR.sharp(levels[0][1], levels[0][2], (0, 0, H, W))).cuda()
    thumb = full.decode(level=2).cpu().numpy()
    up = torch.from_numpy(FR.upsample(thumb, (0, 0, 38, 50), (0, 0, H, W), 2, 38, 50)).cuda()
    assert 0 < int(sharp.sum()) < H * W and torch.equal(got, torch.where(sharp[None], full.decode(), up))            # the surround at d = 2
    st = PY.PyramidStream(net, group=4)
    st.feed(ex)
    assert torch.equal(st.view(fill=True), got)
    only = PY.PyramidDecoder(net, PY.extract(data, levels=[0], window=win), group=4)          # nothing below: the absent tile is named
    assert torch.equal(only.decode(win, fill=True), full.decode(win))
    with pytest.raises(ValueError, match=r"PyramidDecoder.decode: level 0: .*needs tile \(0, 0\), which is absent from this codestream, and there is no "
                                         "coarser level"):
        only.decode(fill=True)


def test_pyramid_fill_rd_reports_bytes_quality_and_the_sharp_share():
    from vampic import evaluate as EV
    cuts = list(_cuts().values())
    rows = EV.pyramid_fill_rd(_net(), _x(1, H, W), cuts + [10 ** 9], tile=64, overlap=16, marks=MARKS, group=4)
    assert [r["bytes"] for r in rows] == cuts + [len(_coded())] and all(r["bpp"] == 8.0 * r["bytes"] / (H * W) and np.isfinite(r["psnr"]) for r in rows)
    five = np.zeros((H, W), dtype=bool)
    five[:48, :] = True                                                         # the first row of tiles and (1, 0): what no later tile touches
    five[48:64, :48] = True
    five[64:96, :48] = True
    assert [r["sharp"] for r in rows] == [0.0, 0.0, float(five.mean()), 1.0, 1.0, 1.0]
    assert [r["chain"] for r in rows][:3] == [[(0, 0, 0), (2, 1, 1)], [(0, 0, 0), (1, 2, 2), (2, 1, 1)], [(0, 5, 5), (1, 4, 4)]]
    assert [r["chain"][0][:2] for r in rows[3:]] == [(0, 12)] * 3 and rows[4]["chain"] == [(0, 12, 12)] and rows[5]["chain"] == [(0, 12, 0)]
    for bad in ([], [cuts[1], cuts[0]], [cuts[0] - 1]):
        with pytest.raises(ValueError, match="pyramid_fill_rd: "):
            EV.pyramid_fill_rd(_net(), _x(1, H, W), bad, tile=64, overlap=16, marks=MARKS, group=4)


def test_what_fill_refuses():
    dec = _fresh(len(_coded()))
    with pytest.raises(ValueError, match="PyramidDecoder.decode: q does not go with fill=True"):
        dec.decode(q=0.5, fill=True)
    with pytest.raises(ValueError, match="PyramidDecoder.decode: level is 0 .. 2, got 3"):
        dec.decode(level=3, fill=True)
    with pytest.raises(ValueError, match="PyramidDecoder.decode: .*does not lie inside the 75 x 100 picture"):
        dec.decode((0, 0, 76, 1), level=1, fill=True)
    with pytest.raises(ValueError, match="PyramidDecoder.decode: dtype is"):
        dec.decode(fill=True, dtype=torch.float16)
    st = PY.PyramidStream(_net(), group=4)
    st.feed(_coded()[:_cuts()["need"]])
    with pytest.raises(ValueError, match="PyramidStream.view: q does not go with fill=True"):
        st.view(q=0.5, fill=True)
    with pytest.raises(ValueError, match="PyramidStream.view: level is 0 .. 2, got -1"):
        st.view(level=-1, fill=True)
    with pytest.raises(ValueError, match=r"PyramidStream.view: level 0 does not decode: .*the ready levels are \[2\]"):
        st.view(level=0)                                                        # without fill nothing changed
    assert tuple(st.view(level=0, fill=True).shape) == (3, 150, 200)
