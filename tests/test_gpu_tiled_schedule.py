"""Scheduled tiled pictures end to end on the GPU (vampic.tiled.encode(schedule=) / PictureDecoder.decode(stage=) / extract,
evaluate.tiled_roi_rd): a tile's stream is the tile's own scheduled embedded codestream on the
restatement's maps (tests/tiled_schedule_ref.py), the bytes do not depend on the grouping, the region comes first in bytes,
and every stage — from the whole stream, from a round end, from an extract, by window, on either coder — equals the NumPy
blend (tests/tiled_ref.py) of forward_quality_map of each tile, bit for bit.  Nothing is asserted about PSNR values: the
synthetic weights are untrained."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiled_ref as TR                                             # noqa: E402
import tiled_schedule_ref as SR                                    # noqa: E402
from test_gpu_embedded_schedule import _net, _x                    # noqa: E402
from vampic import embedded as EB, evaluate as EV, tiled as TL   # noqa: E402

ROI, BG = (0.5, 2.5, 5), (0.05, 0.5, 2.5)                                       # L = 5: the region climbs, then the background
MAIN = dict(H=150, W=200, tile=64, overlap=16)
BOX_A, BOX_B = (56, 104, 88, 136), (140, 190, 150, 200)                         # across a blend band; the bottom-right corner
BOXES = {(150, 200): [BOX_A, BOX_B], (100, 70): [(30, 20, 70, 50)]}
_CODED, _FORWARD, _MAPS = {}, {}, {}


def _schedule(H, W):
    return EV.picture_roi_schedule(H, W, BOXES[(H, W)], ROI, BG, "cuda")


def _coded(H, W, tile, overlap, group=4, **kw):
    """(picture [3, H, W] on the device, grid, codestream), coded once per case."""
    key = (H, W, tile, overlap, group, tuple(sorted(kw.items())))
    if key not in _CODED:
        x = _x(1, H, W)[0]
        _CODED[key] = (x, TL.grid(H, W, tile, overlap), TL.encode(_net(), x, tile=tile, overlap=overlap, schedule=_schedule(H, W), group=group, **kw))
    return _CODED[key]


def _tiles(x, g):
    return torch.from_numpy(TR.extract(x.cpu().numpy(), g, TL.tiles_for(g))).cuda()


def _tile_maps(H, W, tile, overlap):
    """The restatement's S_tile float32 [R C, L, th / 16, tw / 16] of the case's schedule."""
    key = (H, W, tile, overlap)
    if key not in _MAPS:
        g = TL.grid(H, W, tile, overlap)
        _MAPS[key] = SR.tile_schedule(_schedule(H, W).cpu().numpy(), g, TL.tiles_for(g))
    return _MAPS[key]


def _forward(H, W, tile, overlap, k):
    """The restatement's blend of forward_quality_map(tiles, S_tile[k])["x_hat"] (k = "full": forward_single_quality at 10)."""
    key = (H, W, tile, overlap, k)
    if key not in _FORWARD:
        x, g, _ = _coded(H, W, tile, overlap)
        net = _net()
        with torch.no_grad():
            out = net.forward_single_quality(_tiles(x, g), 10) if k == "full" else \
                net.forward_quality_map(_tiles(x, g), torch.from_numpy(_tile_maps(H, W, tile, overlap)[:, k]))
        _FORWARD[key] = TR.blend(out["x_hat"].cpu().numpy(), np.arange(g["R"] * g["C"]).reshape(g["R"], g["C"]), g)[0]
    return _FORWARD[key]


def _eq(got, want):
    return tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_a_tile_s_stream_is_its_own_scheduled_codestream_on_the_restatement_s_maps():
    net = _net()
    x, g, data = _coded(**MAIN)
    assert (g["R"], g["C"], g["th"], g["tw"]) == (3, 4, 64, 64)
    lay = TL.layout(data)
    assert data[4] == 3 and lay["scheduled"] and lay["stages"] == 5 and lay["marks"] == [0, 1, 2, 3, 4] and lay["n_rounds"] == 6
    assert lay["format"] == "embedded-3" and lay["total"] == len(data)
    tiles, maps = _tiles(x, g), _tile_maps(**MAIN)
    assert max(len(np.unique(m)) for m in maps) <= 7
    touched = {(r, c) for i, (r, c) in enumerate(TL.tiles_for(g)) if (maps[i, 0] == 0.5).any()}
    assert {(0, 1), (0, 2), (1, 1), (1, 2), (2, 3)} <= touched and (2, 0) not in touched
    assert maps[11, 0, 3, 3] == 0.5 and maps[11, 0, 1, 1] == np.float32(0.05)   # cell (3, 3) of tile (2, 3) holds replicated pixels of box B
    for r, c in [(0, 2), (2, 0), (2, 3)]:                                       # straddles box A, background only, the replicated corner
        i = r * 4 + c
        alone = EB.to_bytes(EB.encode_batch(net, tiles[i:i + 1], schedule=[maps[i:i + 1, k] for k in range(5)])[0])
        assert TL.tile_stream(data, r, c) == alone, (r, c)


@pytest.mark.parametrize("k", range(5))
def test_every_stage_equals_the_blend_of_the_quality_map_forwards(k):
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    want = _forward(**MAIN, k=k)
    dec = TL.PictureDecoder(net, data, group=5)
    assert dec.scheduled is True and dec.stages == 5 and dec.shape == (150, 200)
    whole = dec.decode(stage=k)
    assert _eq(whole, want) and dec.last_tiles == TL.tiles_for(g)
    assert torch.equal(dec.decode(mark=k), whole)                               # decode_marks equals decode_stages on scheduled tiles
    cut = TL.PictureDecoder(net, data[:lay["round_end"][k]], group=4)
    assert (cut.rounds >= k + 1).all() and _eq(cut.decode(stage=k), want)
    ex = TL.PictureDecoder(net, TL.extract(data, rounds=k + 1), group=4)
    assert ex.stages == 5 and (ex.rounds == k + 1).all() and _eq(ex.decode(stage=k), want)
    window = (58, 100, 20, 20)                                                  # inside box A, across the band of four tiles
    got = dec.decode(window, stage=k)
    assert _eq(got, want[:, 58:78, 100:120]) and dec.last_tiles == TL.tiles_for(g, window) == [(0, 1), (0, 2), (1, 1), (1, 2)]


def test_the_whole_stream_decodes_to_the_blend_of_the_forwards_at_10():
    net = _net()
    x, g, data = _coded(**MAIN)
    dec = TL.PictureDecoder(net, data, group=4)
    assert (dec.rounds == 6).all() and _eq(dec.decode(), _forward(**MAIN, k="full"))
    u8 = dec.decode(stage=2, dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), TR.to_u8(_forward(**MAIN, k=2)))


def test_the_region_comes_first_in_bytes():
    x, g, data = _coded(**MAIN)
    piece = TL.layout(data)["piece"]
    size = lambda k, r, c: piece[k][r][c][1]
    assert size(0, 2, 0) > 0                                                    # stage 0: the background at 0.05
    assert size(1, 2, 0) == 0 and size(2, 2, 0) == 0                            # the region climbs: nothing of a background-only tile
    assert size(1, 1, 2) > 0 and size(2, 1, 2) > 0 and size(1, 0, 1) > 0        # box A's tiles
    assert size(1, 2, 3) > 0 and size(2, 2, 3) > 0                              # box B, carried by replicated cells
    assert size(3, 2, 0) > 0 and size(4, 2, 0) > 0                              # then the background climbs


def test_the_grouping_does_not_show():
    net = _net()
    x, g, data = _coded(**MAIN)
    S = _schedule(150, 200)
    assert TL.encode(net, x[None], tile=64, overlap=16, schedule=S, group=1) == data
    assert TL.encode(net, x, tile=64, overlap=16, schedule=S, group=5) == data


def test_the_device_coder_on_lanes_gives_the_host_coder_s_bytes_and_pixels():
    net = _net()
    x, g, host = _coded(**MAIN, lanes=64, base_lanes=8)
    dev = TL.encode(net, x, tile=64, overlap=16, schedule=_schedule(150, 200), coder="device", lanes=64, base_lanes=8, group=6)
    assert dev == host and host != _coded(**MAIN)[2]
    lay = TL.layout(host)
    assert (lay["lanes"], lay["base_lanes"], lay["format"], lay["stages"]) == (64, 8, "embedded-4", 5)
    window = (58, 100, 20, 20)
    a = TL.PictureDecoder(net, host, coder="host").decode(window, stage=3)
    b = TL.PictureDecoder(net, host, coder="device").decode(window, stage=3)
    assert torch.equal(a, b) and _eq(a, _forward(**MAIN, k=3)[:, 58:78, 100:120])      # the pixels are those of one lane, too


def test_an_unaligned_stride_every_stage():
    net = _net()
    case = dict(H=100, W=70, tile=64, overlap=8)                                # stride 56: tile origins off the 16-grid
    x, g, data = _coded(**case, group=3)
    assert (g["R"], g["C"], g["Sy"]) == (2, 2, 56)
    assert _coded(**case)[2] == data                                            # groups of 3 + 1 and one group of 4
    dec = TL.PictureDecoder(net, data, group=3)
    for k in range(5):
        assert _eq(dec.decode(stage=k), _forward(**case, k=k)), k


def test_refusals_by_message():
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    S = _schedule(150, 200)
    enc = lambda **kw: TL.encode(net, x, tile=64, overlap=16, **kw)
    with pytest.raises(ValueError, match="tiled.encode: give marks or schedule, not both"):
        enc(schedule=S, marks=[0.5, 2.5])
    with pytest.raises(ValueError, match="tiled.encode: a schedule goes with allocation='tile', not with 'picture'"):
        enc(schedule=S, allocation="picture")
    down = S.clone()
    down[2, 7, 9] = 0.03125
    with pytest.raises(ValueError, match=r"schedule: pixel \(7, 9\): stage 2 lowers the quality from 0\.05\d* to 0\.03125; a schedule never"):
        enc(schedule=down)
    for value, text in ((float("nan"), "nan"), (float("inf"), "inf"), (-1.0, "-1.0")):
        bad = S.clone()
        bad[1, 3, 4] = value
        with pytest.raises(ValueError, match=rf"schedule: stage 1, pixel \(3, 4\): qualities are finite and >= 0, got {text}"):
            enc(schedule=bad)
    for bad in (S[:, :-1], S[0], S.double(), S.cpu().numpy(), [S[0], S[1]]):
        with pytest.raises(ValueError, match=r"schedule is an fp32 tensor \[L, H, W\] = \[1\.\.32, 150, 200\]"):
            enc(schedule=bad)
    with pytest.raises(ValueError, match="schedule: 1..32 stages, got 33"):
        enc(schedule=S[:1].expand(33, 150, 200))
    with pytest.raises(ValueError, match="schedule lies on cpu"):
        enc(schedule=S.cpu())
    many = torch.zeros((3, 150, 200), device="cuda")                            # tile (1, 2), rows 48 .. 111 and columns 96 .. 159:
    for k in range(3):                                                          # 16 cells x 3 stages = 48 distinct qualities
        for a in range(4):
            for b in range(4):
                many[k, 48 + 16 * a:64 + 16 * a, 96 + 16 * b:112 + 16 * b] = 0.125 * (1 + 16 * k + 4 * a + b)
    with pytest.raises(ValueError, match=r"tiled.encode: tile \(1, 2\): schedule: image 0 holds 48 distinct qualities"):
        enc(schedule=many)
    dec = TL.PictureDecoder(net, data)
    with pytest.raises(ValueError, match=r"this picture is scheduled \(5 stages\).* decode a stage with stage=0 .. 4"):
        dec.decode(q=2.5)
    with pytest.raises(ValueError, match="stage is 0 .. 4, got 5"):
        dec.decode(stage=5)
    with pytest.raises(ValueError, match="stage is 0 .. 4, got -1"):
        dec.decode(stage=-1)
    with pytest.raises(ValueError, match="give stage alone, not with q or mark"):
        dec.decode(stage=1, mark=1)
    short = TL.PictureDecoder(net, data[:lay["round_end"][1]])
    with pytest.raises(ValueError, match=r"PictureDecoder.decode: tile \(\d, \d\): .*stage 3 needs"):
        short.decode(stage=3)
    plain = TL.PictureDecoder(net, TL.encode(net, _x(1, 60, 60)[0], tile=64, overlap=0, marks=[0.5]))
    assert plain.scheduled is False and plain.stages == 0
    with pytest.raises(ValueError, match="stage= decodes a scheduled picture .*this picture carries no schedule"):
        plain.decode(stage=0)


def test_tiled_roi_rd_reports_the_round_ends():
    net = _net()
    x, g, data = _coded(**MAIN)
    lay = TL.layout(data)
    region = torch.zeros((150, 200), dtype=torch.bool)
    for y0, x0, y1, x1 in (BOX_A, BOX_B):
        region[y0:y1, x0:x1] = True
    rows = EV.tiled_roi_rd(net, x, _schedule(150, 200), region, tile=64, overlap=16, group=4)
    assert [r["stage"] for r in rows] == [0, 1, 2, 3, 4]
    assert [r["bytes"] for r in rows] == lay["round_end"][:5] and all(a <= b for a, b in zip(lay["round_end"], lay["round_end"][1:]))
    for r in rows:
        assert r["bpp"] == 8.0 * r["bytes"] / (150 * 200)
        assert all(np.isfinite(r[key]) for key in ("psnr", "psnr_in", "psnr_out")) and r["enc_s"] > 0 and r["dec_s"] > 0
    with pytest.raises(ValueError, match=r"region is a boolean \[H, W\]"):
        EV.tiled_roi_rd(net, x, _schedule(150, 200), region[None], tile=64, overlap=16)
