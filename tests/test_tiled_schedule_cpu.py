"""Scheduled tiled pictures on the host: the properties of the NumPy restatement of a tile's schedule
(tests/tiled_schedule_ref.py) and the version-3 framing of fabricated scheduled tile codestreams (pack / layout / tile_stream /
extract and the refusals of a header that cannot be trusted).  No model and no GPU are needed."""
import struct

import numpy as np
import pytest
import torch

import test_embedded_stream_cpu as ES
import tiled_schedule_ref as SR
from test_tiled_cpu import _reseal, _tile
from vampic import embedded as EB, evaluate as EV, tiled as TL

NS = ES.NS


# ---------------------------------------------------------------------------------------------------- the restatement
def _monotone(L, H, W, seed):
    """A random schedule [L, H, W] that never decreases from stage to stage: patches of 11 x 13 pixels (no divisor of 16, so
    cells straddle them) of a few qualities, and single pixels that stand out of their patch."""
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.float32([0, 0.05, 0.5, 2.5, 5]), (L, -(-H // 11), -(-W // 13)), p=[0.3, 0.3, 0.2, 0.1, 0.1])
    S = np.repeat(np.repeat(coarse, 11, axis=1), 13, axis=2)[:, :H, :W].copy()
    for k, y, x in zip(rng.integers(0, L, 12), rng.integers(0, H, 12), rng.integers(0, W, 12)):
        S[k, y, x] = 7.5
    return np.maximum.accumulate(S, axis=0).astype(np.float32)


def test_on_the_16_grid_the_restatement_is_a_crop_of_latent_quality_map():
    g = TL.grid(160, 208, 64, 16)                                               # stride 48; 64 + 2 * 48 = 160, 64 + 3 * 48 = 208
    assert (g["R"], g["C"], g["Sy"] % 16, g["Sx"] % 16) == (3, 4, 0, 0)
    S = _monotone(3, 160, 208, 1)
    lat = EV.latent_quality_map(torch.from_numpy(S)).numpy()                    # float64 [3, 10, 13]
    coords = TL.tiles_for(g)
    out = SR.tile_schedule(S, g, coords)
    assert out.dtype == np.float32 and out.shape == (12, 3, 4, 4)
    for i, (r, c) in enumerate(coords):
        assert np.array_equal(out[i], lat[:, 3 * r:3 * r + 4, 3 * c:3 * c + 4]), (r, c)


@pytest.mark.parametrize("H,W,tile,V", [(150, 200, 64, 16), (150, 200, 64, 7), (37, 53, 64, 0), (60, 200, 128, 32)])
def test_a_schedule_that_never_decreases_gives_tile_schedules_that_never_decrease(H, W, tile, V):
    g = TL.grid(H, W, tile, V)
    out = SR.tile_schedule(_monotone(4, H, W, H + V), g, TL.tiles_for(g))
    assert out.shape == (g["R"] * g["C"], 4, g["th"] // 16, g["tw"] // 16)
    assert (np.diff(out, axis=1) >= 0).all() and len(np.unique(out)) > 1
    for i in range(out.shape[0]):                                               # and a valid one for the embedded encoder
        EB.check_schedule([out[i:i + 1, k] for k in range(4)], 1, g["th"] // 16, g["tw"] // 16)


def test_a_cell_that_touches_a_box_takes_the_box_s_quality():
    H, W = 150, 200
    g = TL.grid(H, W, 64, 7)                                                    # stride 57: cells straddle the picture's 16-grid
    y0, x0, y1, x1 = 56, 104, 88, 136
    S = EV.picture_roi_schedule(H, W, [(y0, x0, y1, x1)], [5.0], [0.5], "cpu").numpy()
    assert S.shape == (1, H, W) and S.dtype == np.float32 and S[0, 56, 104] == 5 and S[0, 55, 104] == 0.5 and S[0, 87, 136] == 0.5
    coords = TL.tiles_for(g)
    out = SR.tile_schedule(S, g, coords)
    touched = 0
    for i, (r, c) in enumerate(coords):
        for a in range(4):
            for b in range(4):
                ys = [min(r * g["Sy"] + 16 * a + y, H - 1) for y in range(16)]
                xs = [min(c * g["Sx"] + 16 * b + x, W - 1) for x in range(16)]
                touches = any(y0 <= y < y1 for y in ys) and any(x0 <= x < x1 for x in xs)
                assert out[i, 0, a, b] == (5.0 if touches else 0.5), (r, c, a, b)
                touched += touches
    assert 0 < touched < out.size


def test_replicated_cells_take_the_last_row_s_and_column_s_quality():
    H, W = 37, 53
    g = TL.grid(H, W, 64, 0)
    S = np.full((2, H, W), 1.0, dtype=np.float32)
    S[0, H - 1, :] = 7.0                                                        # stage 0: the last row; stage 1: the last column too
    S[1, H - 1, :] = 7.0
    S[1, :, W - 1] = 9.0
    out = SR.tile_schedule(S, g, [(0, 0)])[0]
    assert np.array_equal(out[0], np.float32([[1] * 4, [1] * 4, [7] * 4, [7] * 4]))           # rows 32 .. 63 hold or repeat row 36
    assert np.array_equal(out[1], np.float32([[1, 1, 1, 9], [1, 1, 1, 9], [7, 7, 7, 9], [7, 7, 7, 9]]))   # columns 48 .. 63: column 52
    g = TL.grid(150, 200, 64, 16)                                               # the corner tile of a grid: rows 96 .. 159 of 150
    S = np.full((1, 150, 200), 1.0, dtype=np.float32)
    S[0, 149, 199] = 3.0
    out = SR.tile_schedule(S, g, [(2, 3), (2, 2), (1, 3)])
    want = np.ones((4, 4), dtype=np.float32)
    want[3, 3] = 3.0                                                            # cell rows 144 .. 159, columns 192 .. 207 of tile (2, 3)
    assert np.array_equal(out[0, 0], want) and (out[1:] == 1).all()


def test_a_nan_propagates_and_the_host_refuses_it_afterwards():
    H, W = 150, 200
    g = TL.grid(H, W, 64, 16)
    S = _monotone(2, H, W, 9)
    S[1, 50, 60] = np.nan                                                       # rows 48 .. 63 and columns 48 .. 63 lie in two tiles each
    coords = TL.tiles_for(g)
    out = SR.tile_schedule(S, g, coords)
    assert not np.isnan(out[:, 0]).any()
    hit = {(coords[i], a, b) for i, a, b in np.argwhere(np.isnan(out[:, 1]))}
    assert hit == {((0, 0), 3, 3), ((0, 1), 3, 0), ((1, 0), 0, 3), ((1, 1), 0, 0)}
    assert SR.same(out, out.copy()) and not SR.same(out, np.nan_to_num(out)) and SR.same(np.float32([-0.0, np.nan]), np.float32([0.0, np.nan]))
    with pytest.raises(ValueError, match=r"schedule: stage 1: quality map: qualities must be >= 0 \(and not NaN\), got NaN"):
        EB.check_schedule([out[:1, k] for k in range(2)], 1, 4, 4)


# ------------------------------------------------------------------------------------------------------------ framing
H, W, TILE, V = 60, 500, 128, 32                                                # 1 x 5 tiles of 64 x 128, the shape ES.make gives
_MADE = {}


def picture(L=3, K=1, Kb=1):
    """(grid, scheduled tile streams in raster order, picture codestream), made once per case."""
    key = (L, K, Kb)
    if key not in _MADE:
        g = TL.grid(H, W, TILE, V)
        assert (g["R"], g["C"], g["th"], g["tw"]) == (1, 5, 64, 128)
        streams = [ES.make(K, Kb, True, L, ("random", "zeros")[i % 2])[1] for i in range(5)]
        _MADE[key] = (g, streams, TL.pack(H, W, TILE, V, streams, stages=L))
    return _MADE[key]


CASES = [dict(), dict(L=1), dict(L=3, K=8, Kb=8)]


@pytest.mark.parametrize("case", CASES)
def test_the_whole_stream_returns_every_tile_stream(case):
    g, streams, data = picture(**case)
    L = case.get("L", 3)
    lay = TL.layout(data)
    assert data[:4] == b"VAMp" and data[4] == 3 and lay["scheduled"] is True and lay["stages"] == L
    assert lay["marks"] == list(range(L)) and lay["allocation"] == "tile" and lay["thresholds"] is None
    assert lay["lanes"] == case.get("K", 1) and lay["base_lanes"] == case.get("Kb", 1)
    assert lay["format"] == ("embedded-4" if case.get("Kb", 1) > 1 else "embedded-3")
    assert lay["total"] == len(data) and lay["n_rounds"] == L + 1 and lay["round_end"][-1] == len(data)
    assert lay["header_end"] == 16 + 20 + 4 * 5 * (L + 2) + 8 + 8              # version 1's, and kind, n_stages, reserved
    assert struct.unpack_from("<HHI", data, lay["header_end"] - 16) == (1, L, 0)
    assert lay["need_bytes"] == TL.need_bytes(data) == lay["header_end"] + sum(EB.layout(s)["base_end"] for s in streams)
    for c, s in enumerate(streams):
        assert TL.tile_stream(data, 0, c) == s and lay["present"][0][c]         # head + pieces == embedded.to_bytes(tile)
        o, n = lay["head"][0][c]
        assert data[o:o + n] == s[:EB.layout(s)["base_end"]]                    # the head is the tile's own, schedule included
        assert EB.from_bytes(TL.tile_stream(data, 0, c))["schedule"]["index"].shape[0] == L
    assert TL.layout(data[:lay["header_end"]])["stages"] == L and TL.layout(data[:lay["header_end"]])["marks"] is None
    assert TL.pack(H, W, TILE, V, [streams], stages=L) == data                  # [R][C]
    plain = [_tile(7 + i, shape=(1, 2)) for i in range(5)]
    v1 = TL.pack(H, W, TILE, V, plain)
    assert v1[4] == 1 and TL.layout(v1)["scheduled"] is False and TL.layout(v1)["stages"] == 0


@pytest.mark.parametrize("case", CASES)
def test_a_round_end_gives_every_tile_its_own_stage(case):
    g, streams, data = picture(**case)
    lay = TL.layout(data)
    for k in range(case.get("L", 3)):
        for cut in (data[:lay["round_end"][k]], TL.extract(data, rounds=k + 1)):
            for c, s in enumerate(streams):
                assert TL.tile_stream(cut, 0, c) == s[:EB.layout(s)["round_end"][k]], (k, c)
    need = lay["need_bytes"]
    for n in list(range(need, len(data) + 1, 11)) + [len(data)]:
        got = [TL.tile_stream(data[:n], 0, c) for c in range(5)]
        assert all(s[:len(t)] == t for s, t in zip(streams, got)) and sum(len(t) for t in got) == n - lay["header_end"], n


def test_extracts_keep_version_and_stages_compose_and_are_idempotent():
    g, streams, data = picture()
    lay = TL.layout(data)
    assert TL.extract(data) == data and TL.extract(bytearray(data)) == data
    win = (10, 200, 30, 50)
    keep = TL.tiles_for(g, win)
    assert keep == [(0, 1), (0, 2)]
    for rounds in (None, 4, 2, 1, 0):
        ex = TL.extract(data, win, rounds)
        nr = 4 if rounds is None else rounds
        el = TL.layout(ex)
        assert ex[4] == 3 and el["scheduled"] and el["stages"] == 3 and el["marks"] == [0, 1, 2] and el["n_rounds"] == nr
        assert len(ex) < len(data) and len(ex) == el["total"]
        for c, s in enumerate(streams):
            assert el["present"][0][c] == ((0, c) in keep)
            if (0, c) in keep:
                e = EB.layout(s)
                assert TL.tile_stream(ex, 0, c) == s[:([e["base_end"]] + e["round_end"] + [e["total"]])[nr]]
            else:
                with pytest.raises(ValueError, match=rf"tile \(0, {c}\) is absent"):
                    TL.tile_stream(ex, 0, c)
        assert TL.extract(ex) == ex
    assert TL.extract(TL.extract(data, (0, 0, 60, 300)), win, 2) == TL.extract(TL.extract(data, rounds=3), win, 2) == TL.extract(data, win, 2)
    assert TL.extract(data, rounds=1) == TL.extract(data[:lay["round_end"][0]], rounds=1)
    with pytest.raises(ValueError, match=r"end before round 1 of tile \(0, 0\)"):
        TL.extract(data[:lay["round_end"][0]], rounds=2)


@pytest.mark.parametrize("case", [CASES[0], CASES[2]])
def test_every_single_byte_change_of_preamble_and_header_is_refused(case):
    g, streams, data = picture(**case)
    hend = TL.layout(data)["header_end"]
    for at in range(hend):
        for flip in (0x01, 0x80):
            bad = data[:at] + bytes([data[at] ^ flip]) + data[at + 1:]
            with pytest.raises(ValueError):
                TL.layout(bad)
            with pytest.raises(ValueError):
                TL.tile_stream(bad, 0, 0)
            with pytest.raises(ValueError):
                TL.extract(bad, rounds=1)


def _as_version(data, version, ext_old, ext_new):
    """``data`` with the ``ext_old`` bytes before its total replaced by ``ext_new``, the total adjusted, the version byte set
    and the preamble made right again."""
    def edit(h):
        total = struct.unpack_from("<Q", h, len(h) - 8)[0]
        h[len(h) - 8 - ext_old:len(h) - 8] = ext_new
        struct.pack_into("<Q", h, len(h) - 8, total - ext_old + len(ext_new))
    return _reseal(data[:4] + bytes([version]) + data[5:], edit)


def test_contradictions_under_a_matching_crc_are_refused_by_message():
    g, streams, data = picture()
    ext = 20 + 4 * 5 * 5                                                        # kind, n_stages, reserved follow the table
    assert _reseal(data, lambda h: None) == data
    v3 = "version 3: the header contradicts itself: "
    with pytest.raises(ValueError, match=v3 + r".*the schedule fields take 136 bytes, it states 140"):
        TL.layout(_reseal(data, lambda h: h.extend(b"\0" * 4)))                 # four bytes too many
    with pytest.raises(ValueError, match=v3 + r".* it states 128"):
        TL.layout(_reseal(data, lambda h: h.__delitem__(slice(ext, ext + 8))))  # a version-1 header read as version 3
    with pytest.raises(ValueError, match=v3 + r".* it states"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 18, 3)))    # n_rounds against the header's length
    with pytest.raises(ValueError, match=v3 + r"kind 2 .*this reader knows kind 1"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext, 2)))
    with pytest.raises(ValueError, match=v3 + r"kind 0"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext, 0)))
    with pytest.raises(ValueError, match=v3 + r"kind 1 \(reserved field 5\)"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<I", h, ext + 4, 5)))
    with pytest.raises(ValueError, match=v3 + r"0 stages and 4 rounds"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext + 2, 0)))
    with pytest.raises(ValueError, match=v3 + r"2 stages and 4 rounds"):        # a whole stream of L stages has L + 1 rounds
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext + 2, 2)))
    with pytest.raises(ValueError, match=v3 + r"2 stages and 4 rounds"):
        TL.extract(_reseal(data, lambda h: struct.pack_into("<H", h, ext + 2, 2)), rounds=1)
    with pytest.raises(ValueError, match=r"tile \(0, 0\) is marked at the stages \[0, 1, 2\]; the tiles of this picture have 5 stages"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext + 2, 5)))           # more stages than the tiles carry
    assert TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext + 2, 5))[:TL.layout(data)["header_end"]])["stages"] == 5
    # plain tiles under version 3
    plain = TL.pack(H, W, TILE, V, [_tile(7 + i, shape=(1, 2)) for i in range(5)])
    with pytest.raises(ValueError, match=r"tile \(0, 0\) is plain \('embedded-1'\); a scheduled picture codestream \(version 3\)"):
        TL.layout(_as_version(plain, 3, 0, struct.pack("<HHI", 1, 3, 0)))
    # scheduled tiles under versions 1 and 2
    with pytest.raises(ValueError, match=r"tile \(0, 0\) is scheduled \('embedded-3'\); a picture codestream carries no schedules"):
        TL.layout(_as_version(data, 1, 8, b""))
    with pytest.raises(ValueError, match=r"tile \(0, 0\) is scheduled \('embedded-3'\); a picture codestream carries no schedules"):
        TL.layout(_as_version(data, 2, 8, struct.pack("<HHHH", 1, 3, NS, 0) + b"\0" * (4 * 3 * NS)))
    with pytest.raises(ValueError, match="this reader knows versions 1, 2 and 3"):
        TL.layout(data[:4] + b"\x04" + data[5:])


def test_pack_refuses_what_a_scheduled_picture_cannot_carry_and_is_unchanged_without_stages():
    g, streams, data = picture()
    with pytest.raises(ValueError, match=r"tile \(0, 0\) is scheduled \('embedded-3'\); a picture codestream carries no schedules"):
        TL.pack(H, W, TILE, V, streams)                                         # today's text, without stages
    plain = [_tile(7 + i, shape=(1, 2)) for i in range(5)]
    assert TL.pack(H, W, TILE, V, plain)[4] == 1 and TL.pack(H, W, TILE, V, plain, stages=None) == TL.pack(H, W, TILE, V, plain)
    with pytest.raises(ValueError, match=r"pack: tile \(0, 1\) is plain \('embedded-1'\)"):
        TL.pack(H, W, TILE, V, [streams[0], plain[1]] + streams[2:], stages=3)
    one = ES.make(1, 1, True, 1, "random")[1]
    with pytest.raises(ValueError, match=r"pack: tile \(0, 2\) is marked at the stages \[0\]; the tiles of this picture have 3 stages"):
        TL.pack(H, W, TILE, V, streams[:2] + [one] + streams[3:], stages=3)
    with pytest.raises(ValueError, match=r"pack: tile \(0, 0\) is marked at the stages \[0, 1, 2\]; the tiles of this picture have 2 stages"):
        TL.pack(H, W, TILE, V, streams, stages=2)
    with pytest.raises(ValueError, match="pack: give thresholds or stages, not both"):
        TL.pack(H, W, TILE, V, streams, thresholds=np.zeros((3, NS), np.float32), stages=3)
    with pytest.raises(ValueError, match=r"tile \(0, 3\) and tile \(0, 0\) differ in their lanes"):
        TL.pack(H, W, TILE, V, streams[:3] + [ES.make(8, 1, True, 3, "random")[1]] + streams[4:], stages=3)
    with pytest.raises(ValueError, match=r"differ in their base_lanes"):
        TL.pack(H, W, TILE, V, [ES.make(8, 8, True, 3, "random")[1]] + [ES.make(8, 1, True, 3, "random")[1]] * 4, stages=3)
    for bad in (0, -1, 1 << 16, 2.0, True):
        with pytest.raises(ValueError, match="stages is 1 .. 65535|is an integer"):
            TL.pack(H, W, TILE, V, streams, stages=bad)
    absent = TL.pack(H, W, TILE, V, [None] + streams[1:], stages=3)             # an absent tile is framed as a head of 0 bytes
    assert not TL.layout(absent)["present"][0][0] and TL.tile_stream(absent, 0, 1) == streams[1] and TL.layout(absent)["stages"] == 3


def test_random_corruptions_raise_nothing_but_valueerror():
    g, streams, data = picture()
    rng = np.random.default_rng(5)
    for _ in range(300):
        bad = bytearray(data[:int(rng.integers(0, len(data) + 1))])
        for at in rng.integers(0, max(len(bad), 1), int(rng.integers(0, 4))):
            if len(bad):
                bad[int(at)] = int(rng.integers(0, 256))
        for fn in (TL.layout, TL.need_bytes, lambda d: TL.tile_stream(d, 0, 2), lambda d: TL.extract(d, (10, 200, 30, 50), 1)):
            try:
                fn(bytes(bad))
            except ValueError:
                pass


# ------------------------------------------------------------------------------------------------ the schedule builder
def test_picture_roi_schedule_follows_roi_schedule_s_ladder():
    S = EV.picture_roi_schedule(150, 200, [(56, 104, 88, 136), (140, 190, 150, 200)], (0.5, 2.5, 5), (0.05, 0.5, 2.5), "cpu")
    assert S.dtype == torch.float32 and tuple(S.shape) == (5, 150, 200)
    assert [float(S[k, 60, 110]) for k in range(5)] == [0.5, 2.5, 5, 5, 5] == [float(S[k, 149, 199]) for k in range(5)]
    assert [round(float(S[k, 0, 0]), 6) for k in range(5)] == [0.05, 0.05, 0.05, 0.5, 2.5]
    assert bool((S[1:] >= S[:-1]).all())
    lat = EV.roi_schedule(1, 160, 208, [(0, 56, 104, 88, 136)], (0.5, 2.5, 5), (0.05, 0.5, 2.5))       # the same ladder per stage
    pic = EV.picture_roi_schedule(160, 208, [(56, 104, 88, 136)], (0.5, 2.5, 5), (0.05, 0.5, 2.5), "cpu")
    assert all(torch.equal(EV.latent_quality_map(pic[k:k + 1]).float(), lat[k].float()) for k in range(5))
    with pytest.raises(ValueError, match="lies outside the picture of 150x200"):
        EV.picture_roi_schedule(150, 200, [(0, 0, 151, 10)], (1,), (0.5,), "cpu")
    with pytest.raises(ValueError, match="at least one quality each"):
        EV.picture_roi_schedule(150, 200, [], (), (0.5,), "cpu")
