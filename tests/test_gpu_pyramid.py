"""Resolution pyramids end to end on the GPU (vampic.pyramid.encode / PyramidDecoder / PyramidStream / extract,
evaluate.pyramid_rd): a level's stream is ``tiled.encode`` of the restatement's level picture
(tests/pyramid_ref.py) byte for byte, and every decode — by level, by window, from the prefix of ``need_bytes``, from an
extract, through the receiver, on a picture-wide allocation, a schedule and the device coder — equals ``tiled.PictureDecoder``
on that level's stream bit for bit.  Nothing is asserted about PSNR values: the synthetic weights are untrained."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pyramid_ref as PR                                           # noqa: E402
from test_gpu_embedded_schedule import _net, _x                    # noqa: E402
from test_gpu_tiled import MAIN, MARKS, _coded as _plain           # noqa: E402
from vampic import evaluate as EV, pyramid as PY, tiled as TL    # noqa: E402

H, W = MAIN["H"], MAIN["W"]
KW = dict(tile=MAIN["tile"], overlap=MAIN["overlap"], group=4)
SHAPES = [(150, 200), (75, 100), (38, 50)]
WINDOWS = {0: [(40, 90, 30, 17), (131, 181, 19, 19)], 1: [(20, 45, 15, 9), (0, 40, 75, 21)], 2: [(5, 7, 20, 30), (37, 49, 1, 1)]}
BOX = (56, 104, 88, 136)                                                        # (y0, x0, y1, x1): across a blend band of level 0
_CODED, _PICTURES, _FRESH = {}, {}, {}


def _pictures():
    """The restatement's level pictures of the test picture, on the device."""
    if not _PICTURES:
        p = _x(1, H, W)[0].cpu().numpy()
        for k in range(3):
            _PICTURES[k] = torch.from_numpy(p).cuda()
            p = PR.halve(p)
    return _PICTURES


def _coded(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CODED:
        _CODED[key] = PY.encode(_net(), _x(1, H, W)[0], marks=MARKS, **KW, **kw)
    return _CODED[key]


def _fresh(data, n):
    """A fresh PyramidDecoder on ``data[:n]``, built once per prefix."""
    if (id(data), n) not in _FRESH:
        _FRESH[(id(data), n)] = PY.PyramidDecoder(_net(), data[:n], group=4)
    return _FRESH[(id(data), n)]


def _schedules():
    """A two-stage schedule (the floor of 0.5, then a box of quality 10 on it) and the restatement's max-reduced levels."""
    S = EV.picture_roi_schedule(H, W, [BOX], (0.5, 10.0), (0.5,), "cuda")
    out, s = [], S.cpu().numpy()
    for _ in range(3):
        out.append(s)
        s = PR.halve(s, "max")
    return S, out


def test_three_levels_each_the_tiled_encode_of_the_restatement_s_picture():
    net, data = _net(), _coded()
    lay = PY.layout(data)
    assert lay["n_levels"] == 3 and [lv["shape"] for lv in lay["levels"]] == SHAPES and lay["ready_levels"] == [0, 1, 2]
    assert [(lv["layout"]["R"], lv["layout"]["C"], lv["layout"]["th"], lv["layout"]["tw"]) for lv in lay["levels"]] == \
        [(3, 4, 64, 64), (2, 2, 64, 64), (1, 1, 64, 64)]
    assert PY.level_stream(data, 0) == _plain(**MAIN)[2]                        # today's tiled.encode of the picture
    for k in (1, 2):
        assert PY.level_stream(data, k) == TL.encode(net, _pictures()[k], marks=MARKS, **KW), k
    assert data == PY.pack(H, W, [PY.level_stream(data, k) for k in range(3)]) and lay["total"] == len(data)
    assert PY.encode(net, _x(1, H, W), levels=3, marks=MARKS, tile=64, overlap=16, group=5) == data       # [1, 3, H, W], another grouping
    one = PY.encode(net, _pictures()[2], marks=MARKS, **KW)
    assert PY.layout(one)["n_levels"] == 1 and PY.level_stream(one, 0) == PY.level_stream(data, 2)
    for bad, text in ((0, "levels is 1 .. 16, got 0"), (17, "levels is 1 .. 16, got 17"), (10, "level 8 is 1 x 1 already and level 9 would repeat it"),
                      (2.0, "levels is an integer")):
        with pytest.raises(ValueError, match=f"pyramid.encode: .*{text}"):
            PY.encode(net, _x(1, H, W)[0], levels=bad, **KW)
    with pytest.raises(ValueError, match=r"pyramid.encode: image is an fp32 tensor \[3, H, W\] or \[1, 3, H, W\]"):
        PY.encode(net, _x(2, H, W), **KW)
    with pytest.raises(ValueError, match=r"pyramid.encode: level 1 \(38 x 50\): grid: overlap 40"):     # level 0: one tile of 128 x 128
        PY.encode(net, _pictures()[1], levels=2, tile=128, overlap=40, marks=MARKS)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_a_level_decodes_as_the_picture_decoder_on_its_stream(k):
    net, data = _net(), _coded()
    dec = _fresh(data, len(data))
    assert dec.shape == (H, W) and dec.levels == 3 and dec.shapes == SHAPES and dec.ready == [True] * 3
    ref = TL.PictureDecoder(net, PY.level_stream(data, k), group=4)
    for win in [None] + WINDOWS[k]:
        for dtype in (None, torch.uint8):
            got = dec.decode(win, level=k, dtype=dtype)
            assert torch.equal(got, ref.decode(win, dtype=dtype)) and dec.last_tiles == ref.last_tiles, (win, dtype)
    assert tuple(dec.decode(level=k).shape) == (3,) + SHAPES[k]
    assert torch.equal(dec.decode(WINDOWS[k][0], level=k, q=0.5), ref.decode(WINDOWS[k][0], q=0.5))
    assert torch.equal(dec.decode(WINDOWS[k][0], level=k, mark=1, dtype=torch.uint8), ref.decode(WINDOWS[k][0], mark=1, dtype=torch.uint8))
    with pytest.raises(ValueError) as mine:                                     # error for error
        dec.decode((0, 0, SHAPES[k][0] + 1, 1), level=k)
    with pytest.raises(ValueError) as theirs:
        ref.decode((0, 0, SHAPES[k][0] + 1, 1))
    assert str(mine.value) == str(theirs.value) and "does not lie inside" in str(mine.value)
    with pytest.raises(ValueError, match="PyramidDecoder.decode: level is 0 .. 2, got 3"):
        dec.decode(level=3)


def test_the_prefix_of_need_bytes_is_the_thumbnail():
    net, data = _net(), _coded()
    need = PY.need_bytes(data)
    assert need == PY.layout(data)["header_end"] + TL.need_bytes(PY.level_stream(data, 2)) < PY.layout(data)["levels"][1]["offset"]
    dec = PY.PyramidDecoder(net, data[:need], group=4)
    assert dec.ready == [False, False, True]
    assert torch.equal(dec.decode(level=2), TL.PictureDecoder(net, PY.level_stream(data, 2)[:need - PY.layout(data)["header_end"]]).decode())
    for k in (1, 0):
        with pytest.raises(ValueError, match=rf"PyramidDecoder.decode: level {k} does not decode: its bytes end before the heads of its tiles do; "
                                             r"the ready levels are \[2\]"):
            dec.decode(level=k)
    with pytest.raises(ValueError, match=f"PyramidDecoder: {need - 1} bytes end before any level decodes: {need} bytes are needed"):
        PY.PyramidDecoder(net, data[:need - 1])
    part = PY.PyramidDecoder(net, data[:PY.layout(data)["levels"][0]["offset"] + 40], group=4)        # levels 2 and 1 whole
    assert part.ready == [False, True, True] and torch.equal(part.decode(level=1), _fresh(data, len(data)).decode(level=1))


def test_an_extract_of_one_level_decodes_the_mapped_window():
    net, data = _net(), _coded()
    win = WINDOWS[0][0]
    at = PY.window_at(win, 1, H, W)
    assert at == WINDOWS[1][0] == PR.window_at(win, 1, H, W)
    ex = PY.extract(data, levels=[1], window=win)
    assert len(ex) < len(PY.level_stream(data, 1)) and PY.layout(ex)["ready_levels"] == [1]
    dec = PY.PyramidDecoder(net, ex, group=4)
    assert dec.ready == [False, True, False] and torch.equal(dec.decode(at, level=1), _fresh(data, len(data)).decode(at, level=1))
    with pytest.raises(ValueError, match=r"level 0 does not decode: it is absent from this codestream; the ready levels are \[1\]"):
        dec.decode(level=0)
    with pytest.raises(ValueError, match=r"PictureDecoder.decode: the window \(60, 80, 10, 10\) needs tile \(1, 1\), which is absent"):
        dec.decode((60, 80, 10, 10), level=1)
    low = PY.extract(data, levels=[1], window=win, rounds=2)                    # and cut in quality: mark 1 is whole
    assert torch.equal(PY.PyramidDecoder(net, low, group=4).decode(at, level=1, mark=1), _fresh(data, len(data)).decode(at, level=1, mark=1))


def test_the_receiver_fed_unevenly_up_to_each_level_s_end():
    net, data = _net(), _coded()
    lay = PY.layout(data)
    st = PY.PyramidStream(net, group=5)
    with pytest.raises(ValueError, match="PyramidStream.view: nothing to decode yet: the header is not complete, 16 bytes are missing"):
        st.view()
    at = 0
    ends = [lay["need_bytes"]] + [lay["levels"][k]["offset"] + lay["levels"][k]["length"] for k in (2, 1, 0)]
    for i, n in enumerate(ends):
        for end in (min(n, at + 1), at + (n - at) // 3 + 1, n):                 # one byte, about a third, the rest
            if end > at:
                st.feed(data[at:end])
                at = end
        assert st.ready and st.need() == 0 and st.shape == (H, W) and st.levels == 3 and st.shapes == SHAPES and st.data == data[:n]
        dec = _fresh(data, n)
        ready = [k for k in range(3) if dec.ready[k]]
        assert st.ready_levels == ready == [[2], [2], [1, 2], [0, 1, 2]][i]
        for k in ready:
            grew = i == {2: 0, 1: 2, 0: 3}[k] or (k, i) == (2, 1)               # the level's first view; level 2's tile got its rest at feed 1
            assert torch.equal(st.view(level=k), dec.decode(level=k)) and st.last_decoded == (TL.tiles_for(st.streams[k].grid) if grew else []), (i, k)
            assert torch.equal(st.view(level=k), dec.decode(level=k)) and st.last_decoded == []          # a second view runs no tile
            win = WINDOWS[k][0]
            assert torch.equal(st.view(win, level=k, dtype=torch.uint8), dec.decode(win, level=k, dtype=torch.uint8)) and st.last_decoded == []
        for k in range(3):
            if k not in ready:
                with pytest.raises(ValueError, match=rf"PyramidStream.view: level {k} does not decode: its bytes end before the heads"):
                    st.view(level=k)
    canvas = st.canvas(WINDOWS[1][1], level=1)
    assert canvas.refresh() == WINDOWS[1][1] and torch.equal(canvas.out, _fresh(data, len(data)).decode(WINDOWS[1][1], level=1))
    assert canvas.refresh() is None
    assert torch.equal(st.view(WINDOWS[0][1], level=0, q=0.5), _fresh(data, len(data)).decode(WINDOWS[0][1], level=0, q=0.5))
    before = len(st.data)
    with pytest.raises(ValueError, match="PyramidStream.feed: .* bytes follow the codestream"):
        st.feed(b"\0")
    assert len(st.data) == before
    for bad in (dict(cache_tiles=0), dict(group=0)):
        with pytest.raises(ValueError, match="PictureStream: "):
            PY.PyramidStream(net, **bad)


def test_picture_wide_marks_level_by_level():
    net, data = _net(), _coded(allocation="picture")
    lay = PY.layout(data)
    assert [lv["layout"]["allocation"] for lv in lay["levels"]] == ["picture"] * 3
    for k in range(3):
        assert PY.level_stream(data, k) == TL.encode(net, _pictures()[k], marks=MARKS, allocation="picture", **KW), k
    dec = PY.PyramidDecoder(net, data, group=4)
    assert torch.equal(dec.decode(level=1, mark=2), TL.PictureDecoder(net, PY.level_stream(data, 1), group=4).decode(mark=2))


def test_a_schedule_is_reduced_alongside_with_the_maximum():
    net = _net()
    S, reduced = _schedules()
    data = PY.encode(net, _x(1, H, W)[0], schedule=S, **KW)
    lay = PY.layout(data)
    assert lay["n_levels"] == 3 and all(lv["layout"]["scheduled"] and lv["layout"]["stages"] == 2 for lv in lay["levels"])
    assert [sorted(np.unique(s).tolist()) for s in reduced] == [[0.5, 10.0]] * 3 and reduced[2].shape == (2, 38, 50)
    assert (reduced[1][1] == 10).sum() == 16 * 16 and (reduced[1][0] == 0.5).all()
    for k in range(3):
        assert PY.level_stream(data, k) == TL.encode(net, _pictures()[k], schedule=torch.from_numpy(reduced[k]).cuda(), **KW), k
    dec = PY.PyramidDecoder(net, data, group=4)
    ref = TL.PictureDecoder(net, PY.level_stream(data, 1), group=4)
    assert torch.equal(dec.decode(level=1, stage=0), ref.decode(stage=0)) and torch.equal(dec.decode(level=1, stage=1), ref.decode(stage=1))
    assert not torch.equal(dec.decode(level=1, stage=0), dec.decode(level=1, stage=1))
    with pytest.raises(ValueError, match="PictureDecoder.decode: this picture is scheduled"):
        dec.decode(level=2, q=0.5)


def test_the_device_coder_on_lanes_gives_the_host_coder_s_bytes():
    host, device = _coded(coder="host", lanes=64, base_lanes=8), _coded(coder="device", lanes=64, base_lanes=8)
    assert host == device and host != _coded()
    lay = PY.layout(host)
    assert all((lv["layout"]["lanes"], lv["layout"]["base_lanes"]) == (64, 8) for lv in lay["levels"])
    a, b = (PY.PyramidDecoder(_net(), host, coder=coder, group=4).decode(level=1) for coder in ("host", "device"))
    assert torch.equal(a, b)


def test_pyramid_rd_returns_its_fields_and_more_quality_costs_more_bytes():
    net, data = _net(), _coded()
    lay = PY.layout(data)
    rows = EV.pyramid_rd(net, _x(1, H, W), MARKS, tile=64, overlap=16, group=4)
    assert [(r["level"], r["q"]) for r in rows] == [(k, float(q)) for k in range(3) for q in MARKS]
    for r in rows:
        lv = lay["levels"][r["level"]]
        assert r["shape"] == SHAPES[r["level"]] and r["bytes"] == lay["header_end"] + lv["layout"]["round_end"][MARKS.index(r["q"])]
        assert r["bpp"] == 8.0 * r["bytes"] / (H * W) and np.isfinite(r["psnr"]) and r["enc_s"] > 0 and r["dec_s"] > 0
        assert r["total_over_level0"] == len(data) / lay["levels"][0]["length"] > 1
    for k in range(3):
        bpp = [r["bpp"] for r in rows if r["level"] == k]
        assert all(b > a for a, b in zip(bpp, bpp[1:]))
