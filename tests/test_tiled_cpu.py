"""Tiled picture codestreams on the host (vampic.tiled): the geometry, the framing of fabricated tile
codestreams (pack / layout / tile_stream / extract), the refusals of a header that cannot be trusted, and the properties of
the NumPy restatement of the blend (tests/tiled_ref.py).  No model and no GPU are needed."""
import struct
import zlib

import numpy as np
import pytest

import tiled_ref as TR
from vampic import embedded as EB, tiled as TL

NS = 3
_MADE = {}


def _tile(seed, shape=(1, 1), K=1, Kb=1, L=3, q=(0.5, 2.5, 10.0)):
    """An embedded codestream of random bytes with consistent marks, in the style of test_embedded_stream_cpu.make: three
    slices, ``shape`` = (th / 64, tw / 64), its byte lengths drawn from ``seed``."""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(40, 90, NS)]
    rows = np.sort(rng.integers(4, 36, (L, NS)), axis=0) // 4 * 4
    c = {"format": EB._format_of(K, Kb, False), "shape": shape, "z": [rng.bytes(10 + K)],
         "base": [[rng.bytes(int(n))] for n in rng.integers(5, 30, NS)], "embedded": [rng.bytes(n) for n in lens],
         "marks": {"q": list(q[:L]), "count": [[int(v) for v in row] for row in rows // 2], "bytes": [[int(v) for v in row] for row in rows]}}
    if c["format"] != "embedded-1":
        c["lanes"] = K
    if Kb > 1:
        c["base_lanes"] = Kb
    return EB.to_bytes(c)


def picture(H=150, W=200, tile=64, overlap=16, shape=(1, 1), **kw):
    """(grid, tile streams in raster order, picture codestream), made once per case."""
    key = (H, W, tile, overlap, shape, tuple(sorted(kw.items())))
    if key not in _MADE:
        g = TL.grid(H, W, tile, overlap)
        streams = [_tile(100 * H + i, shape, **kw) for i in range(g["R"] * g["C"])]
        _MADE[key] = (g, streams, TL.pack(H, W, tile, overlap, streams))
    return _MADE[key]


CASES = [dict(), dict(H=60, W=200, tile=128, overlap=32, shape=(1, 2)), dict(H=37, W=53, tile=256, overlap=0),
         dict(H=100, W=70, tile=64, overlap=32, K=8, Kb=8, L=1)]


# --------------------------------------------------------------------------------------------------------------- grid
@pytest.mark.parametrize("H,W,tile,V", [(150, 200, 64, 16), (60, 200, 128, 32), (37, 53, 64, 0), (4000, 3000, 256, 32), (1, 1, 64, 32),
                                        (64, 65, 64, 32), (1000, 1500, 1024, 512), (129, 257, 128, 0), (96, 96, 64, 1)])
def test_grid_covers_the_picture_and_is_never_three_deep(H, W, tile, V):
    g = TL.grid(H, W, tile, V)
    c64 = lambda n: (n + 63) // 64 * 64
    assert (g["th"], g["tw"]) == (min(tile, c64(H)), min(tile, c64(W))) and g["th"] % 64 == 0 and g["tw"] % 64 == 0
    assert (g["Sy"], g["Sx"], g["V"]) == (g["th"] - V, g["tw"] - V, V)
    for n, S, t, N in ((g["R"], g["Sy"], g["th"], H), (g["C"], g["Sx"], g["tw"], W)):
        assert n >= 1 and (n - 1) * S + t >= N                                  # coverage
        assert n == 1 or (n - 2) * S + t < N                                    # and no tile too many: the last one is needed
        cover = np.zeros(N, dtype=np.int64)
        for k in range(n):
            cover[k * S:k * S + t] += 1
        assert cover.min() >= 1 and cover.max() <= 2                            # never three tiles deep
        assert V > 0 or cover.max() == 1


def test_grid_small_pictures_overlap_zero_and_refusals():
    g = TL.grid(37, 53, 256, 32)
    assert (g["th"], g["tw"], g["R"], g["C"]) == (64, 64, 1, 1)                 # H <= tile: one tile of ceil64
    g = TL.grid(60, 200, 128, 32)
    assert (g["th"], g["tw"], g["R"], g["C"]) == (64, 128, 1, 2)
    g = TL.grid(150, 200, 64, 16)
    assert (g["R"], g["C"]) == (3, 4)
    g = TL.grid(128, 192, 64, 0)
    assert (g["R"], g["C"], g["Sy"], g["Sx"]) == (2, 3, 64, 64)
    assert TL.grid(4000, 3000)["tile"] == 256 and TL.grid(4000, 3000)["V"] == 32
    for bad in (100, 0, 32, 1088, 96.0):
        with pytest.raises(ValueError, match="tile is a multiple of 64|is an integer"):
            TL.grid(100, 100, bad, 0)
    with pytest.raises(ValueError, match="overlap 33: tiles of 64 x 64 take 0 <= overlap <= 32"):
        TL.grid(100, 100, 64, 33)
    with pytest.raises(ValueError, match="overlap 40"):                        # the smaller side of 64 x 128 tiles decides
        TL.grid(60, 200, 128, 40)
    with pytest.raises(ValueError, match="overlap -1"):
        TL.grid(100, 100, 64, -1)
    with pytest.raises(ValueError, match="sides are 1"):
        TL.grid(0, 100, 64, 0)


def test_tiles_for_is_what_the_blend_reads():
    g = TL.grid(150, 200, 64, 16)
    assert TL.tiles_for(g) == [(r, c) for r in range(3) for c in range(4)]
    assert TL.tiles_for(g, (20, 20, 10, 10)) == [(0, 0)]                        # inside one tile's core
    assert TL.tiles_for(g, (48, 48, 1, 1)) == [(0, 0), (0, 1), (1, 0), (1, 1)]  # a corner of four
    assert TL.tiles_for(g, (63, 0, 2, 10)) == [(0, 0), (1, 0)]                  # the last band row, the first core row
    assert TL.tiles_for(g, (64, 0, 1, 10)) == [(1, 0)]
    assert TL.tiles_for(g, (149, 199, 1, 1)) == [(2, 3)]
    for win in [(0, 0, 150, 200), (40, 90, 30, 17), (95, 143, 3, 9), (149, 0, 1, 200)]:   # against the restatement's own reads
        need = set()
        for r, c in TL.tiles_for(g):
            slot = np.full((3, 4), 0)
            slot[r, c] = -1
            if TR.blend(np.zeros((1, 3, 64, 64), np.float32), slot, g, win)[1]:
                need.add((r, c))
        assert set(TL.tiles_for(g, win)) == need, win
    for bad in [(0, 0, 151, 1), (-1, 0, 1, 1), (0, 0, 0, 1), (0, 199, 1, 2), (0, 0, 1)]:
        with pytest.raises(ValueError):
            TL.tiles_for(g, bad)


# ------------------------------------------------------------------------------------------------------------ framing
@pytest.mark.parametrize("case", CASES)
def test_the_whole_stream_returns_every_tile_stream(case):
    g, streams, data = picture(**case)
    lay = TL.layout(data)
    L = case.get("L", 3)
    assert all(lay[k] == g[k] for k in ("H", "W", "th", "tw", "V", "Sy", "Sx", "R", "C"))
    assert lay["total"] == len(data) and lay["n_rounds"] == L + 1 and lay["round_end"][-1] == len(data)
    assert lay["marks"] == [0.5, 2.5, 10.0][:L] and lay["lanes"] == case.get("K", 1) and lay["base_lanes"] == case.get("Kb", 1)
    assert lay["need_bytes"] == TL.need_bytes(data) == lay["header_end"] + sum(EB.layout(s)["base_end"] for s in streams)
    assert lay["header_end"] == 16 + 20 + 4 * len(streams) * (L + 2) + 8
    assert data[:4] == b"VAMp" and TL.layout(data[:lay["header_end"]])["head"] == lay["head"]
    at = lay["header_end"]
    for i, s in enumerate(streams):
        r, c = divmod(i, g["C"])
        assert TL.tile_stream(data, r, c) == s and lay["present"][r][c]
        assert lay["head"][r][c] == (at, EB.layout(s)["base_end"])              # heads in raster order, each up to its base_end
        at += lay["head"][r][c][1]
        assert data[lay["head"][r][c][0]:at] == s[:EB.layout(s)["base_end"]]
    for k in range(L + 1):                                                      # then the rounds, each in raster order
        for i, s in enumerate(streams):
            r, c = divmod(i, g["C"])
            el = EB.layout(s)
            edges = [el["base_end"]] + el["round_end"] + [el["total"]]
            assert lay["piece"][k][r][c] == (at, edges[k + 1] - edges[k])
            at += edges[k + 1] - edges[k]
        assert at == lay["round_end"][k]
    assert TL.pack(g["H"], g["W"], g["tile"], g["V"], [streams[r * g["C"]:(r + 1) * g["C"]] for r in range(g["R"])]) == data


@pytest.mark.parametrize("case", CASES[:2])
def test_every_prefix_from_need_bytes_on(case):
    g, streams, data = picture(**case)
    lay = TL.layout(data)
    need = lay["need_bytes"]
    for n in list(range(need, len(data) + 1, 7)) + [len(data)] + lay["round_end"]:
        got = [TL.tile_stream(data[:n], *divmod(i, g["C"])) for i in range(len(streams))]
        assert all(s[:len(t)] == t for s, t in zip(streams, got)), n
        assert sum(len(t) for t in got) == n - lay["header_end"], n              # every byte received is some tile's
        assert all(len(t) >= EB.layout(s)["base_end"] for s, t in zip(streams, got))
        assert all(EB.from_bytes(t) is not None for t in got)
    for n in (0, 5, 16, lay["header_end"] - 1):
        assert TL.need_bytes(data[:n]) == (16 if n < 16 else lay["header_end"])
        with pytest.raises(ValueError, match="bytes are needed"):
            TL.layout(data[:n])
    assert TL.need_bytes(data[:lay["header_end"]]) == need
    assert TL.layout(data[:lay["header_end"]])["marks"] is None                 # no head held yet


@pytest.mark.parametrize("case", CASES)
def test_a_round_end_gives_every_tile_its_own_round_end(case):
    g, streams, data = picture(**case)
    lay = TL.layout(data)
    for k in range(case.get("L", 3)):
        cut = data[:lay["round_end"][k]]
        for i, s in enumerate(streams):
            assert TL.tile_stream(cut, *divmod(i, g["C"])) == s[:EB.layout(s)["round_end"][k]], (k, i)


def test_extract_is_shorter_composes_and_is_the_identity_without_arguments():
    g, streams, data = picture()
    lay = TL.layout(data)
    assert TL.extract(data) == data and TL.extract(bytearray(data)) == data
    win = (40, 90, 30, 17)
    keep = TL.tiles_for(g, win)
    assert 0 < len(keep) < 12
    for rounds in (None, 4, 2, 1, 0):
        ex = TL.extract(data, win, rounds)
        nr = 4 if rounds is None else rounds
        el = TL.layout(ex)
        assert len(ex) < len(data) and len(ex) == el["total"] and el["n_rounds"] == nr
        assert all(el[k] == lay[k] for k in ("H", "W", "th", "tw", "V", "R", "C", "marks", "lanes", "base_lanes"))
        for i, s in enumerate(streams):
            r, c = divmod(i, g["C"])
            assert el["present"][r][c] == ((r, c) in keep)
            if (r, c) in keep:
                e = EB.layout(s)
                end = ([e["base_end"]] + e["round_end"] + [e["total"]])[nr]
                assert TL.tile_stream(ex, r, c) == s[:end]
            else:
                with pytest.raises(ValueError, match=rf"tile \({r}, {c}\) is absent"):
                    TL.tile_stream(ex, r, c)
        assert TL.extract(ex) == ex
    a = TL.extract(TL.extract(data, (0, 0, 100, 200)), win, 2)                  # an extract of an extract is an extract
    assert a == TL.extract(TL.extract(data, rounds=3), win, 2) == TL.extract(data, win, 2)
    assert TL.extract(data, rounds=1) == TL.extract(data[:lay["round_end"][0]], rounds=1)
    assert len(TL.extract(data, rounds=1)) == lay["round_end"][0] - 4 * 12 * 3   # the table loses three columns
    small = TL.extract(data, (20, 20, 10, 10), 1)
    with pytest.raises(ValueError, match=r"needs tile \(0, 1\), which is absent"):
        TL.extract(small, (20, 20, 10, 40))
    with pytest.raises(ValueError, match="rounds is 0 .. 1"):
        TL.extract(small, rounds=2)
    with pytest.raises(ValueError, match=r"end before round 1 of tile \(0, 0\)"):
        TL.extract(data[:lay["round_end"][0]], rounds=2)
    with pytest.raises(ValueError, match="does not lie inside"):
        TL.extract(data, (0, 0, 151, 10))


# ----------------------------------------------------------------------------------------------------------- refusals
def _reseal(data, edit):
    """``data`` with its header edited by ``edit(bytearray)`` and the preamble's length and CRC made right again."""
    hlen = struct.unpack_from("<I", data, 8)[0]
    header = bytearray(data[16:16 + hlen])
    edit(header)
    return data[:8] + struct.pack("<II", len(header), zlib.crc32(bytes(header)) & 0xFFFFFFFF) + bytes(header) + data[16 + hlen:]


def _u32(header, off, delta):
    struct.pack_into("<I", header, off, struct.unpack_from("<I", header, off)[0] + delta)


def test_a_header_that_cannot_be_trusted_is_refused():
    g, streams, data = picture()
    hend = TL.layout(data)["header_end"]
    with pytest.raises(ValueError, match="CRC-32 does not match"):
        TL.layout(data[:20] + bytes([data[20] ^ 1]) + data[21:])
    with pytest.raises(ValueError, match="not a picture codestream"):
        TL.layout(b"VAMe" + data[4:])
    with pytest.raises(ValueError, match="not a picture codestream"):
        TL.layout(streams[0])                                                   # a tile's own codestream is no picture
    with pytest.raises(ValueError, match="version 2"):
        TL.layout(data[:4] + b"\x02" + data[5:])
    with pytest.raises(ValueError, match="bytes follow the codestream"):
        TL.layout(data + b"\0")
    with pytest.raises(ValueError, match="a bytes-like object"):
        TL.layout("VAMp")
    T0 = 20                                                                     # the table follows the eight fixed fields
    with pytest.raises(ValueError, match="its table adds up to"):               # a table that contradicts total
        TL.layout(_reseal(data, lambda h: _u32(h, T0 + 4, 4)))
    with pytest.raises(ValueError, match="its table adds up to"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<Q", h, len(h) - 8, len(data) + 1)))

    def both(h):                                                                # table and total agree, the tile does not
        _u32(h, T0 + 4, 4)
        struct.pack_into("<Q", h, len(h) - 8, len(data) + 4)
    with pytest.raises(ValueError, match=r"contradicts tile \(0, 0\)"):
        TL.layout(_reseal(data, both) + b"\0" * 4)

    def absent(h):                                                              # tile (0, 1): no head, but its pieces stay
        struct.pack_into("<I", h, T0 + 4 * 5, 0)
    with pytest.raises(ValueError, match=r"tile \(0, 1\) is absent \(a head of 0 bytes\) and has round pieces"):
        TL.layout(_reseal(data, absent))
    with pytest.raises(ValueError, match="is no grid of"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 14, 4)))    # R
    with pytest.raises(ValueError, match="overlap 40"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 12, 40)))   # V
    with pytest.raises(ValueError, match="sides are 64 .. 1024"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 8, 0)))     # th / 64
    with pytest.raises(ValueError, match="it states"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, 18, 3)))    # n_rounds against the header's length
    assert TL.layout(_reseal(data, lambda h: None)) == TL.layout(data) and hend == 16 + 20 + 4 * 12 * 5 + 8


def test_tiles_that_differ_and_tiles_the_format_cannot_carry_are_refused():
    g, streams, data = picture()
    n = len(streams)
    with pytest.raises(ValueError, match="has 3 x 4 = 12 tiles, got 11"):
        TL.pack(150, 200, 64, 16, streams[:-1])
    with pytest.raises(ValueError, match=r"tile \(0, 1\) and tile \(0, 0\) differ in their marks"):
        TL.pack(150, 200, 64, 16, [streams[0], _tile(7, q=(0.5, 2.0, 10.0))] + streams[2:])
    with pytest.raises(ValueError, match=r"tile \(2, 3\) and tile \(0, 0\) differ in their marks"):
        TL.pack(150, 200, 64, 16, streams[:-1] + [_tile(7, L=2)])
    with pytest.raises(ValueError, match=r"tile \(0, 2\) and tile \(0, 0\) differ in their lanes"):
        TL.pack(150, 200, 64, 16, streams[:2] + [_tile(7, K=8)] + streams[3:])
    with pytest.raises(ValueError, match=r"differ in their base_lanes"):
        TL.pack(150, 200, 64, 16, [_tile(7, K=8, Kb=8)] + [_tile(8, K=8, Kb=4)] * (n - 1))
    with pytest.raises(ValueError, match=r"tile \(1, 0\) is an image of 64 x 128, the tiles of this picture are 64 x 64"):
        TL.pack(150, 200, 64, 16, streams[:4] + [_tile(7, shape=(1, 2))] + streams[5:])
    with pytest.raises(ValueError, match=r"tile \(0, 0\): .* a picture is packed from whole tile codestreams"):
        TL.pack(150, 200, 64, 16, [streams[0][:-1]] + streams[1:])
    with pytest.raises(ValueError, match="no tile"):
        TL.pack(150, 200, 64, 16, [None] * n)
    import test_embedded_stream_cpu as ES
    sched = ES.make(1, 1, True, 3, "random")[1]                                 # shape (1, 2): the tiles of 60 x 200 at 128
    with pytest.raises(ValueError, match=r"tile \(0, 0\) is scheduled \('embedded-3'\); a picture codestream carries no schedules"):
        TL.pack(60, 200, 128, 32, [sched, sched])
    # the same refusals from the bytes: a stream whose second head is another tile's, sealed with a right table
    other = _tile(7, K=8)
    e0, e1 = EB.layout(streams[1]), EB.layout(other)
    swapped = data[:TL.layout(data)["head"][0][1][0]] + other[:e1["base_end"]] + data[TL.layout(data)["head"][0][2][0]:]

    def row(h):
        edges = [0, e1["base_end"]] + e1["round_end"] + [e1["total"]]
        struct.pack_into("<5I", h, 20 + 4 * 5, *[b - a for a, b in zip(edges, edges[1:])])
        struct.pack_into("<Q", h, len(h) - 8, len(data) - e0["total"] + e1["total"])
    bad = _reseal(swapped, row)
    bad = bad + b"\0" * (len(data) - e0["total"] + e1["total"] - len(bad)) if e1["total"] > e0["total"] else bad
    with pytest.raises(ValueError, match=r"tile \(0, 1\) and tile \(0, 0\) differ in their lanes"):
        TL.layout(bad[:TL.need_bytes(bad[:TL.layout(data)['header_end']])])
    absent = TL.pack(150, 200, 64, 16, [None] + streams[1:])                    # an absent tile is framed as a head of 0 bytes
    assert not TL.layout(absent)["present"][0][0] and TL.tile_stream(absent, 0, 1) == streams[1]


@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
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


def test_random_corruptions_raise_nothing_but_valueerror():
    g, streams, data = picture()
    rng = np.random.default_rng(5)
    for _ in range(300):
        bad = bytearray(data[:int(rng.integers(0, len(data) + 1))])
        for at in rng.integers(0, max(len(bad), 1), int(rng.integers(0, 4))):
            if len(bad):
                bad[int(at)] = int(rng.integers(0, 256))
        for fn in (TL.layout, TL.need_bytes, lambda d: TL.tile_stream(d, 1, 2), lambda d: TL.extract(d, (10, 10, 50, 50), 1)):
            try:
                fn(bytes(bad))
            except ValueError:
                pass


# ---------------------------------------------------------------------------------------------------- the restatement
def test_the_ramps_are_the_package_s_and_sum_to_one():
    for V in (1, 2, 16, 32, 33, 512):
        lo, hi = TR.ramps(V)
        plo, phi = TL.ramps(V)
        assert lo.dtype == hi.dtype == np.float32 and np.array_equal(lo, plo) and np.array_equal(hi, phi)
        assert np.array_equal(hi, ((np.arange(V) + 0.5) / V).astype(np.float32)) and np.array_equal(lo, np.float32(1) - hi)
        assert (np.diff(hi) > 0).all() and 0 < hi[0] and hi[-1] < 1
    assert TL.ramps(0)[0].size == 0


@pytest.mark.parametrize("H,W,tile,V", [(150, 200, 64, 16), (60, 200, 128, 32), (37, 53, 64, 32), (128, 130, 64, 0)])
def test_extraction_replicates_the_edge_and_the_blend_copies_outside_the_bands(H, W, tile, V):
    g = TL.grid(H, W, tile, V)
    rng = np.random.default_rng(H)
    img = rng.random((3, H, W), dtype=np.float32)
    coords = TL.tiles_for(g)
    tiles = TR.extract(img, g, coords)
    for i, (r, c) in enumerate(coords):
        for y, x in [(0, 0), (g["th"] - 1, g["tw"] - 1), (g["th"] // 2, g["tw"] - 1)]:
            assert np.array_equal(tiles[i, :, y, x], img[:, min(r * g["Sy"] + y, H - 1), min(c * g["Sx"] + x, W - 1)])
    slot = np.arange(len(coords)).reshape(g["R"], g["C"])
    out, missing = TR.blend(tiles, slot, g)
    assert not missing and out.dtype == np.float32 and out.shape == (3, H, W)
    assert np.abs(out - img).max() <= 2.0 ** -22                                # tiles of one picture blend back to it
    noise = rng.random(tiles.shape, dtype=np.float32)                           # unrelated tiles: outside the bands a copy
    out, _ = TR.blend(noise, slot, g)
    for i, (r, c) in enumerate(coords):
        ys = [y for y in range(g["th"]) if r * g["Sy"] + y < H and (r == 0 or y >= V) and (r == g["R"] - 1 or y < g["Sy"])]
        xs = [x for x in range(g["tw"]) if c * g["Sx"] + x < W and (c == 0 or x >= V) and (c == g["C"] - 1 or x < g["Sx"])]
        core = noise[i][:, ys][:, :, xs]
        assert core.size and np.array_equal(out[:, r * g["Sy"] + ys[0]:r * g["Sy"] + ys[-1] + 1, c * g["Sx"] + xs[0]:c * g["Sx"] + xs[-1] + 1],
                                            core), (r, c)
    win = (g["Sy"] - 3 if g["R"] > 1 else 5, g["Sx"] + 1 if g["C"] > 1 else 7, 9, 11)
    assert np.array_equal(TR.blend(noise, slot, g, win)[0], out[:, win[0]:win[0] + 9, win[1]:win[1] + 11])


@pytest.mark.parametrize("V", [1, 16, 31, 32])
def test_a_constant_field_stays_within_two_ulp(V):
    g = TL.grid(150, 200, 64, V)
    slot = np.arange(g["R"] * g["C"]).reshape(g["R"], g["C"])
    for value in (0.7, 1.0, 0.3333, 1.0e-3, 250.0):
        v = np.float32(value)
        out, _ = TR.blend(np.full((g["R"] * g["C"], 3, 64, 64), v, dtype=np.float32), slot, g)
        assert np.abs(out.astype(np.float64) - float(v)).max() <= 2 * float(np.spacing(v)), (V, value)


def test_to_u8_rounds_half_to_even():
    x = np.array([0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1.0, 1.5, -0.2, 0.999], dtype=np.float32).reshape(1, 1, -1).repeat(3, 0)
    want = np.rint(np.clip(x.astype(np.float32), 0, 1) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(TR.to_u8(x), want.transpose(1, 2, 0)) and TR.to_u8(x).shape == (1, 8, 3)
    import torch
    t = torch.from_numpy(x)
    assert np.array_equal(TR.to_u8(x), t.clamp(0, 1).mul(255.0).round().to(torch.uint8).permute(1, 2, 0).numpy())   # write_image
