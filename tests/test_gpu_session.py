"""Viewing sessions end to end on the GPU (vampic.session.Server / Client, evaluate.session_rd) on the
README model and the 150 x 200 picture of test_gpu_pyramid at 64 / 16, three levels in 3 x 4, 2 x 2 and 1 x 1 tiles: along a
tour of viewports the client, which is sent only what it lacks, shows what a fresh decoder shows of the stateless extract and
of the whole stream, bit for bit, and runs the network only for the tiles a message brought.  Nothing is asserted about a
time or a PSNR value: the synthetic weights are untrained."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiled_ref as TR                                             # noqa: E402
from test_gpu_embedded_schedule import _net, _x                    # noqa: E402
from test_gpu_pyramid import H, KW, W, _coded, _fresh, _schedules  # noqa: E402
from test_gpu_pyramid_viewport import VIEWS                        # noqa: E402
from test_gpu_tiled import MARKS                                   # noqa: E402
from vampic import embedded as EB, evaluate as EV, pyramid as PY, session as SS, tiled as TL   # noqa: E402

PAN = (VIEWS[1][0][0] + 24, VIEWS[1][0][1] - 30) + VIEWS[1][0][2:]              # new tiles enter on the left
# (rect, out_hw, unit, rounds): the thumbnail; a level-0 rect; a pan; more rounds; the same again; a zoom out to level 1
TOUR = [(None, (30, 40), 1, 1), VIEWS[1][:3] + (1,), (PAN, VIEWS[1][1], 1, 1), (PAN, VIEWS[1][1], 1, 3), (PAN, VIEWS[1][1], 1, 3), VIEWS[3][:3] + (3,)]
LEVELS = [2, 0, 0, 0, 0, 1]


def _records(message, level):
    return [r[1:3] for r in SS.layout(message)["records"] if r[0] == level]


def test_along_the_tour_the_client_shows_what_fresh_decoders_show_and_decodes_only_what_a_message_brought():
    net, data = _net(), _coded()
    full = _fresh(data, len(data))
    server, client = SS.Server(data), SS.Client(net, group=5)
    with pytest.raises(ValueError, match="Client.viewport: nothing to decode yet: the picture's headers have not arrived"):
        client.viewport(None, (30, 40))
    canvases, sent = {}, 0
    for i, (rect, out_hw, unit, rounds) in enumerate(TOUR):
        m, k = rounds - 1, LEVELS[i]
        message = server.viewport(rect, out_hw, unit, rounds)
        grew = client.merge(message)
        sent += len(message)
        assert i == 0 or len(message) < len(PY.extract_viewport(data, rect, out_hw, unit, rounds))      # the first message carries every level's header
        assert PY.viewport_level(rect, out_hw, H, W, 3, unit) == k and grew == [r[:3] for r in SS.layout(message)["records"]]
        win = PY.viewport_window(rect, out_hw, k, H, W, unit)
        if i == 3:                                          # more rounds arrived: the old mark is cached, the new one runs the window's tiles once
            client.viewport(rect, out_hw, unit, mark=0)
            assert client.last_decoded == [] and client.last_tiles == TL.tiles_for(client.level(0).grid, win)
        got = client.viewport(rect, out_hw, unit, mark=m)
        if i == 2:                                          # the pan: exactly the tiles the message brought
            assert client.last_decoded == _records(message, 0) == [(r, 0) for r in range(3)] and len(client.last_tiles) == 9
        elif i == 3:
            assert client.last_decoded == client.last_tiles == _records(message, 0) and len(client.last_tiles) == 9
        elif i == 4:                                        # the repeated request: no record, no network
            assert SS.layout(message)["records"] == [] and len(message) == 36 and client.last_decoded == [] and len(client.last_tiles) == 9
        assert client.last_chain == [(k, client.last_tiles, client.last_decoded)]
        stateless = PY.PyramidDecoder(net, PY.extract_viewport(data, rect, out_hw, unit, rounds=m + 1, thumbnail=False), group=4)
        assert torch.equal(got, stateless.viewport(rect, out_hw, unit, mark=m)), i
        assert torch.equal(got, full.viewport(rect, out_hw, unit, mark=m)), i
        u8 = client.viewport(rect, out_hw, unit, mark=m, dtype=torch.uint8)
        assert client.last_decoded == [] and u8.dtype == torch.uint8
        assert torch.equal(u8, stateless.viewport(rect, out_hw, unit, mark=m, dtype=torch.uint8))
        assert torch.equal(u8, full.viewport(rect, out_hw, unit, mark=m, dtype=torch.uint8))
        snap = PY.PyramidDecoder(net, client.snapshot(m + 1), group=4)
        for dtype in (None, torch.uint8):
            filled = client.viewport(rect, out_hw, unit, mark=m, dtype=dtype, fill=True)
            assert torch.equal(filled, snap.viewport(rect, out_hw, unit, mark=m, dtype=dtype, fill=True)), i
            assert [(e[0], e[1]) for e in client.last_chain] == [(e[0], e[1]) for e in snap.last_chain] and client.last_chain[0][0] == k
            assert all(e[2] == [] for e in client.last_chain)
        assert torch.equal(filled, u8)                      # every tile of the window is there: nothing was filled
        if (k, win) not in canvases:
            canvases[(k, win)] = client.canvas(win, k)
        canvas = canvases[(k, win)]
        box = canvas.refresh(mark=m)
        assert (box is None) == (i == 4) and torch.equal(canvas.out, client.view(win, k, mark=m)) and client.last_decoded == []
        assert torch.equal(canvas.out, full.decode(win, level=k, mark=m))
    assert all(np.array_equal(client.have[j], server.have[j]) for j in range(3)) and sent < len(data)
    assert server.have[0].tolist() == [[4, 4, 4, 2]] * 3 and server.have[2].tolist() == [[4]]


def test_a_window_whose_tiles_hold_different_rounds_views_at_the_low_mark_and_names_the_tile_at_the_high_one():
    net, data = _net(), _coded()
    full = _fresh(data, len(data))
    server, client = SS.Server(data), SS.Client(net, group=4, cache_tiles=36)    # room for three keys of every tile of the window
    for rect, out_hw, unit, rounds in TOUR[:4]:
        client.merge(server.viewport(rect, out_hw, unit, rounds))
    g = client.level(0).grid
    win = PY.viewport_window(*VIEWS[1][:2], 0, H, W)                            # the first rect: columns 1 and 2 hold three rounds, column 3 one
    tiles = TL.tiles_for(g, win)
    assert sorted({int(client.level(0).tile_rounds[rc]) for rc in tiles}) == [1, 3]
    assert torch.equal(client.view(win, 0, mark=0), full.decode(win, level=0, mark=0)) and client.last_tiles == tiles
    assert client.available(win, 0, mark=0) == tiles and client.available(win, 0, mark=2) == [rc for rc in tiles if rc[1] < 3]
    before = (client.last_tiles, client.last_decoded, client.last_chain)
    with pytest.raises(ValueError, match=r"Client.view: level 0: the window .* needs tile \(0, 3\), which holds 1 whole rounds, 3 are needed"):
        client.view(win, 0, mark=2)
    with pytest.raises(ValueError, match=r"Client.view: level 1: the window .* needs tile \(0, 0\), which holds nothing: its head has not arrived"):
        client.view((0, 0, 10, 10), 1, mark=0)
    assert (client.last_tiles, client.last_decoded, client.last_chain) == before
    filled = client.view(win, 0, mark=2, fill=True)                             # the same window, filled: column 3 comes from the thumbnail
    snap = PY.PyramidDecoder(net, client.snapshot(3), group=4)
    assert torch.equal(filled, snap.decode(win, level=0, mark=2, fill=True)) and [e[0] for e in client.last_chain] == [0, 2]
    assert client.last_chain[0][1] == [rc for rc in tiles if rc[1] < 3] and not torch.equal(filled, full.decode(win, level=0, mark=2))
    # without a level every tile decodes from whatever it holds: the restatement's blend of the per-tile decodes
    got = client.view(win, 0)
    assert client.last_decoded == tiles
    cs = [EB.from_bytes(client.level(0).tile_bytes(r, c)) for r, c in tiles]
    assert [len(client.level(0).tile_bytes(r, c)) for r, c in tiles] == [int(client.level(0).held[rc]) for rc in tiles]
    with torch.no_grad():
        x_hat = torch.cat([EB.EmbeddedDecoder(net, cs[j:j + 5]).decode()["x_hat"] for j in range(0, len(cs), 5)]).cpu().numpy()
    want, missing = TR.blend(x_hat, TL._slot_table(g, tiles), g, win)
    assert not missing and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    client.view(win, 0)
    assert client.last_decoded == []                        # ("held", bytes): fresh until the tile's bytes grow
    grew = client.merge(server.viewport(*VIEWS[1][:3], 2))
    assert grew == [(0, r, 3) for r in range(3)]
    client.view(win, 0)
    assert client.last_decoded == [(r, 3) for r in range(3)]
    client.view(win, 0, mark=0)
    assert client.last_decoded == []                        # a level key never goes stale


def test_the_device_coder_serves_a_session():
    net = _net()
    data = _coded(coder="device", lanes=64, base_lanes=8)
    full = PY.PyramidDecoder(net, data, coder="device", group=4)
    server, client = SS.Server(data), SS.Client(net, coder="device", group=5)
    for i, (rect, out_hw, unit, rounds) in enumerate(TOUR[1:4]):
        message = server.viewport(rect, out_hw, unit, rounds)
        client.merge(message)
        assert torch.equal(client.viewport(rect, out_hw, unit, mark=rounds - 1), full.viewport(rect, out_hw, unit, mark=rounds - 1)), i
        assert client.last_decoded == _records(message, 0)
    assert torch.equal(client.viewport(None, (30, 40), mark=2, dtype=torch.uint8), full.viewport(None, (30, 40), mark=2, dtype=torch.uint8))


def test_picture_wide_marks_keep_their_thresholds_through_a_snapshot_and_pass_the_pooled_check():
    net, data = _net(), _coded(allocation="picture")
    full = PY.PyramidDecoder(net, data, group=4)
    server, client = SS.Server(data), SS.Client(net, group=4)
    for rect, out_hw, unit, rounds in TOUR[1:4]:
        client.merge(server.viewport(rect, out_hw, unit, rounds))
    rect, out_hw, unit, _ = TOUR[3]
    assert torch.equal(client.viewport(rect, out_hw, unit, mark=2), full.viewport(rect, out_hw, unit, mark=2)) and len(client.last_decoded) == 9
    assert torch.equal(client.viewport(rect, out_hw, unit, q=MARKS[2]), full.viewport(rect, out_hw, unit, mark=2))     # a marked quality is its mark
    with pytest.raises(ValueError, match="quality 1.0 is not marked"):
        client.viewport(rect, out_hw, unit, q=1.0)
    snap = client.snapshot(3)
    lay, whole = PY.layout(snap), PY.layout(data)
    assert [lv["present"] for lv in lay["levels"]] == [True, False, True]
    for k in (0, 2):
        tl = lay["levels"][k]["layout"]
        assert tl["allocation"] == "picture" and np.array_equal(tl["thresholds"], whole["levels"][k]["layout"]["thresholds"])
    assert snap == PY.extract_viewport(data, rect, out_hw, unit, rounds=3)
    dec = PY.PyramidDecoder(net, snap, group=4)
    assert torch.equal(dec.viewport(rect, out_hw, unit, mark=2, fill=True), full.viewport(rect, out_hw, unit, mark=2))


def test_a_scheduled_picture_is_viewed_by_stage():
    net = _net()
    S, _ = _schedules()
    data = PY.encode(net, _x(1, H, W)[0], schedule=S, **KW)
    full = PY.PyramidDecoder(net, data, group=4)
    server, client = SS.Server(data), SS.Client(net, group=4)
    rect, out_hw, unit = VIEWS[1][:3]
    for stage in (0, 1):
        message = server.viewport(rect, out_hw, unit, stage + 1)
        client.merge(message)
        got = client.viewport(rect, out_hw, unit, stage=stage)
        assert torch.equal(got, full.viewport(rect, out_hw, unit, stage=stage)) and client.last_decoded == client.last_tiles
        assert client.level(0).scheduled and client.level(0).stages == 2
        snap = PY.PyramidDecoder(net, client.snapshot(stage + 1), group=4)
        assert torch.equal(client.viewport(rect, out_hw, unit, stage=stage, fill=True), snap.viewport(rect, out_hw, unit, stage=stage, fill=True))
    with pytest.raises(ValueError, match="this picture is scheduled"):
        client.viewport(rect, out_hw, unit, q=0.5)
    assert PY.layout(client.snapshot(2))["levels"][0]["layout"]["stages"] == 2


_RD = {}


def _session_rd():
    if not _RD:
        tour = [dict(rect=rect, out_hw=out_hw, unit=unit, rounds=rounds) for rect, out_hw, unit, rounds in TOUR]
        _RD["rows"] = EV.session_rd(_net(), _x(1, H, W), tour, marks=MARKS, tile=64, overlap=16, group=4)
    return _RD["rows"]


def test_session_rd_counts_the_ledger_and_the_framing_and_sends_less_than_the_stateless_extracts_from_the_pan_on():
    data, rows = _coded(), _session_rd()
    server = SS.Server(data)
    opening = SS.layout(server.open())                                          # the same session on the same bytes, by hand
    assert opening["headers"] and opening["records"] == [] and opening["segment_bytes"] == 0
    lengths, framing = [], opening["total"]
    for rect, out_hw, unit, rounds in TOUR:
        lay = SS.layout(server.viewport(rect, out_hw, unit, rounds))
        assert not lay["headers"]
        lengths.append(lay["total"])
        framing += lay["header_end"]
    assert [r["bytes"] for r in rows] == lengths and [r["bytes_total"] for r in rows] == (opening["total"] + np.cumsum(lengths)).tolist()
    tables = PY.layout(data)
    ledger = 0
    for k, have in server.have.items():
        tl = tables["levels"][k]["layout"]
        ledger += sum(([tl["head"]] + tl["piece"])[j][r][c][1] for (r, c), n in np.ndenumerate(have) for j in range(int(n)))
    assert rows[-1]["bytes_total"] == ledger + framing
    for i, (r, step) in enumerate(zip(rows, TOUR)):
        assert r["bytes_stateless"] == len(PY.extract_viewport(data, *step))
        assert i < 2 or r["bytes"] < r["bytes_stateless"]
        assert np.isfinite(r["psnr"]) and r["dec_s"] > 0 and r["decoded"] <= r["tiles"]
    assert [r["tiles"] for r in rows] == [1, 9, 9, 9, 9, 4] and [r["decoded"] for r in rows] == [1, 9, 3, 9, 0, 4]


def test_session_rd_sends_no_more_than_the_stateless_extract_at_every_step():
    """``bytes <= bytes_stateless`` at EVERY step.  The session opens with ``Server.open()``, so a step's message is records and
    segments alone; the headers are counted once, in ``bytes_total``."""
    rows = _session_rd()
    print([(r["bytes"], r["bytes_stateless"], r["bytes_total"]) for r in rows])
    for i, r in enumerate(rows):
        assert r["bytes"] <= r["bytes_stateless"], (i, r["bytes"], r["bytes_stateless"])
