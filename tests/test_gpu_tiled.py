"""Tiled pictures end to end on the GPU (vampic.tiled.encode / PictureDecoder / extract, evaluate.tiled_rd, DESIGN section
9v): a tile's stream is the tile's own embedded codestream, the bytes do not depend on the grouping, and every decode —
whole, per mark, from a prefix cut anywhere, by window, from an extract, on either coder — equals the NumPy blend
(tests/tiled_ref.py) of what the embedded decoder or the forward makes of each tile, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiled_ref as TR                                             # noqa: E402
from test_gpu_embedded_schedule import _net, _same, _x             # noqa: E402
from vampic import embedded as EB, evaluate as EV, tiled as TL   # noqa: E402

MARKS = [0.05, 0.5, 2.5, 10]
MAIN = dict(H=150, W=200, tile=64, overlap=16)
_CODED, _FORWARD = {}, {}


def _coded(H, W, tile, overlap, group=4, **kw):
    """(picture [3, H, W] on the device, grid, codestream), coded once per case."""
    key = (H, W, tile, overlap, group, tuple(sorted(kw.items())))
    if key not in _CODED:
        x = _x(1, H, W)[0]
        _CODED[key] = (x, TL.grid(H, W, tile, overlap), TL.encode(_net(), x, tile=tile, overlap=overlap, marks=MARKS, group=group, **kw))
    return _CODED[key]


def _tiles(x, g):
    """The tiles of ``x`` by the restatement, on the device, [R C, 3, th, tw]."""
    return torch.from_numpy(TR.extract(x.cpu().numpy(), g, TL.tiles_for(g))).cuda()


def _forward(H, W, tile, overlap, q):
    """The restatement's blend of forward_single_quality(tiles, q)["x_hat"], computed once per case and quality."""
    key = (H, W, tile, overlap, q)
    if key not in _FORWARD:
        x, g, _ = _coded(H, W, tile, overlap)
        with torch.no_grad():
            x_hat = _net().forward_single_quality(_tiles(x, g), q)["x_hat"].cpu().numpy()
        _FORWARD[key] = TR.blend(x_hat, np.arange(g["R"] * g["C"]).reshape(g["R"], g["C"]), g)[0]
    return _FORWARD[key]


def _eq(got, want):
    return tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_a_tile_s_stream_is_its_own_embedded_codestream_and_the_grouping_does_not_show():
    net = _net()
    x, g, data = _coded(**MAIN)
    assert (g["R"], g["C"], g["th"], g["tw"]) == (3, 4, 64, 64)
    tiles = _tiles(x, g)
    lay = TL.layout(data)
    assert lay["marks"] == [float(q) for q in MARKS] and lay["n_rounds"] == 5 and lay["total"] == len(data)
    for r, c in [(2, 3), (1, 1), (0, 3)]:                                       # a replicated corner, an interior tile, a right edge
        alone = EB.to_bytes(EB.encode_batch(net, tiles[r * 4 + c:r * 4 + c + 1], marks=MARKS)[0])
        assert TL.tile_stream(data, r, c) == alone, (r, c)
    assert TL.encode(net, x[None], tile=64, overlap=16, marks=MARKS, group=3) == data      # [1, 3, H, W], another grouping
    with pytest.raises(ValueError, match=r"image is an fp32 tensor \[3, H, W\] or \[1, 3, H, W\]"):
        TL.encode(net, x[None].repeat(2, 1, 1, 1))
    with pytest.raises(ValueError, match="tile is a multiple of 64"):
        TL.encode(net, x, tile=100)


def test_the_full_decode_and_every_mark_equal_the_blend_of_the_forwards():
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    dec = TL.PictureDecoder(net, data, group=5)
    assert dec.shape == (150, 200) and dec.grid["R"] == 3 and (dec.rounds == 5).all()
    full = dec.decode()
    assert full.dtype == torch.float32 and _eq(full, _forward(**MAIN, q=10))
    assert dec.last_tiles == TL.tiles_for(g)
    u8 = dec.decode(dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), TR.to_u8(full.cpu().numpy()))
    for k, q in enumerate(MARKS):
        part = TL.PictureDecoder(net, data[:lay["round_end"][k]], group=4)
        assert (part.rounds >= k + 1).all()
        assert _eq(part.decode(q=q), _forward(**MAIN, q=q)), q
        assert _eq(dec.decode(q=q), _forward(**MAIN, q=q)), q                   # and from the whole stream
    short = TL.PictureDecoder(net, data[:lay["round_end"][1]])
    with pytest.raises(ValueError, match=r"PictureDecoder.decode: tile \(\d, \d\): .*quality 2.5 needs"):
        short.decode(q=2.5)
    with pytest.raises(ValueError, match=rf"{lay['need_bytes']} bytes are needed"):
        TL.PictureDecoder(net, data[:lay["need_bytes"] - 1])
    base = TL.PictureDecoder(net, data[:lay["need_bytes"]])                     # the heads alone: every tile's base
    assert (base.rounds == 0).all() and torch.equal(base.decode(q=0), dec.decode(q=0))
    assert torch.equal(base.decode(), TL.PictureDecoder(net, TL.extract(data, rounds=0)).decode())


def test_a_prefix_cut_inside_a_round_is_the_blend_of_the_tile_prefixes():
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    n = (lay["round_end"][1] + 2 * lay["round_end"][2]) // 3 + 1                 # inside round 2, not at a word boundary
    assert lay["round_end"][1] < n < lay["round_end"][2]
    dec = TL.PictureDecoder(net, data[:n], group=4)
    assert set(np.unique(dec.rounds)) == {2, 3}                                 # the earlier tiles hold round 2, the later ones do not
    cs = [EB.from_bytes(TL.tile_stream(data[:n], r, c)) for r, c in TL.tiles_for(g)]
    x_hat = torch.cat([EB.EmbeddedDecoder(net, cs[i:i + 6]).decode()["x_hat"] for i in (0, 6)]).cpu().numpy()
    assert _eq(dec.decode(), TR.blend(x_hat, np.arange(12).reshape(3, 4), g)[0])


@pytest.mark.parametrize("window,n_tiles", [((70, 20, 20, 24), 1), ((40, 90, 30, 17), 4), ((131, 181, 19, 19), 1), ((48, 96, 1, 1), 4)],
                         ids=["core", "band", "bottom-right", "corner"])
def test_a_window_is_the_crop_of_the_full_decode(window, n_tiles):
    net = _net()
    x, g, data = _coded(**MAIN)
    y0, x0, h, w = window
    want = _forward(**MAIN, q=10)[:, y0:y0 + h, x0:x0 + w]
    dec = TL.PictureDecoder(net, data, group=4)
    got = dec.decode(window)
    assert _eq(got, want) and dec.last_tiles == TL.tiles_for(g, window) and len(dec.last_tiles) == n_tiles
    assert np.array_equal(dec.decode(window, dtype=torch.uint8).cpu().numpy(), TR.to_u8(want))
    assert _eq(dec.decode(window, q=0.5), _forward(**MAIN, q=0.5)[:, y0:y0 + h, x0:x0 + w])


def test_an_extract_decodes_its_window_and_refuses_another():
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    window = (40, 90, 30, 17)
    ex = TL.extract(data, window, rounds=1)
    assert len(ex) < lay["round_end"][0] < len(data)
    dec = TL.PictureDecoder(net, ex)
    assert dec.shape == (150, 200) and (dec.rounds[:2, 1:3] == 1).all() and (dec.rounds[2] == -1).all() and (dec.rounds[:, 0] == -1).all()
    cut = TL.PictureDecoder(net, data[:lay["round_end"][0]])
    assert torch.equal(dec.decode(window), cut.decode(window))                  # everything present: the mark's bytes may hold more
    want = cut.decode(window, q=MARKS[0])                                       # elements than the mark counts; at the mark itself:
    assert torch.equal(dec.decode(window, q=MARKS[0]), want) and _eq(want, _forward(**MAIN, q=MARKS[0])[:, 40:70, 90:107])
    with pytest.raises(ValueError, match=r"needs tile \(0, 0\), which is absent"):
        dec.decode((40, 60, 30, 47))
    with pytest.raises(ValueError, match=r"needs tile \(0, 0\), which is absent"):
        dec.decode()
    with pytest.raises(ValueError, match=r"tile \([01], [12]\): .*quality 0.5 needs"):
        dec.decode(window, q=0.5)


def test_the_device_coder_on_lanes_gives_the_host_coder_s_bytes_and_pixels():
    net = _net()
    x, g, host = _coded(**MAIN, lanes=64, base_lanes=8)
    dev = TL.encode(net, x, tile=64, overlap=16, marks=MARKS, coder="device", lanes=64, base_lanes=8, group=6)
    assert dev == host and host != _coded(**MAIN)[2]
    lay = TL.layout(host)
    assert (lay["lanes"], lay["base_lanes"], lay["format"]) == (64, 8, "embedded-4")
    window = (40, 90, 30, 17)
    a = TL.PictureDecoder(net, host, coder="host").decode(window)
    b = TL.PictureDecoder(net, host, coder="device").decode(window)
    assert torch.equal(a, b) and _eq(a, _forward(**MAIN, q=10)[:, 40:70, 90:107])     # the pixels are those of one lane, too
    cut = host[:lay["round_end"][1]]
    assert torch.equal(TL.PictureDecoder(net, cut, coder="device").decode(window, q=0.5),
                       TL.PictureDecoder(net, cut, coder="host").decode(window, q=0.5))


@pytest.mark.parametrize("H,W,tile,overlap,group", [(100, 70, 64, 16, 3), (60, 200, 128, 32, 4)], ids=["groups-3-1", "tiles-64x128"])
def test_other_shapes(H, W, tile, overlap, group):
    net = _net()
    x, g, data = _coded(H, W, tile, overlap, group=group)
    assert (g["R"], g["C"], g["th"], g["tw"]) == ((2, 2, 64, 64) if H == 100 else (1, 2, 64, 128))
    dec = TL.PictureDecoder(net, data, group=group)
    assert dec.shape == (H, W) and _eq(dec.decode(), _forward(H, W, tile, overlap, 10))
    window = (H - 30, W - 41, 30, 41)
    assert _eq(dec.decode(window, q=2.5), _forward(H, W, tile, overlap, 2.5)[:, H - 30:, W - 41:])
    assert TL.encode(net, x, tile=tile, overlap=overlap, marks=MARKS, group=1) == data


def test_tiled_rd_reports_the_round_ends():
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    rows = EV.tiled_rd(net, x, MARKS, tile=64, overlap=16, group=4)
    assert [r["q"] for r in rows] == [float(q) for q in MARKS]
    for k, r in enumerate(rows):
        assert r["bytes"] == lay["round_end"][k] and r["bpp"] == 8.0 * lay["round_end"][k] / (150 * 200)
        assert np.isfinite(r["psnr"]) and r["enc_s"] > 0 and r["dec_s"] > 0
        want = EV.compute_psnr(x[None], torch.from_numpy(_forward(**MAIN, q=MARKS[k])).cuda()[None])
        assert abs(r["psnr"] - want) <= 1e-9 * abs(want)                        # one float64 sum in two orders
    assert rows[0]["psnr"] <= rows[-1]["psnr"] + 1e-9 and rows[0]["bpp"] < rows[-1]["bpp"]
