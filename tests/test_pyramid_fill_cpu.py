"""Filled pyramid views on the host: ``pyramid.source_window`` against brute force, the properties of
the NumPy restatement (tests/fill_ref.py), and the per-tile readiness of ``tiled.PictureFeed`` (``tile_ready``,
``tile_rounds``) on fabricated codestreams fed in chunks that end inside a head.  No model and no GPU are needed."""
import numpy as np
import pytest

import fill_ref as FR
import tiled_ref as TR
from test_tiled_cpu import picture
from test_tiled_schedule_cpu import picture as picture_v3
from vampic import pyramid as PY, tiled as TL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ source_window
@pytest.mark.parametrize("d", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (38, 50), (75, 100)])
def test_source_window_is_the_brute_force_over_every_window(H, W, d):
    Hj, Wj = -(-H // 2 ** d), -(-W // 2 ** d)

    def spans(N, Nj):
        """{(first, length) of a window: (first, length) of the sources}, each source found pixel by pixel with floor division."""
        lo, hi = [], []
        for P in range(N):
            a = (2 * P + 1 - 2 ** d) // 2 ** (d + 1)
            lo.append(min(max(a, 0), Nj - 1))
            hi.append(min(max(a + 1, 0), Nj - 1))
        return {(p0, n): (min(lo[p0:p0 + n]), max(hi[p0:p0 + n]) - min(lo[p0:p0 + n]) + 1) for p0 in range(N) for n in range(1, N - p0 + 1)}
    rows, cols = spans(H, Hj), spans(W, Wj)
    assert all(y + h <= Hj for y, h in rows.values()) and all(x + w <= Wj for x, w in cols.values())
    for (y0, h), (sy, sh) in rows.items():                                      # the axes are independent: every row span with two
        for x0, w in ((0, W), (W // 2, W - W // 2)):                            # column spans, every column span with two row spans
            sx, sw = cols[(x0, w)]
            assert PY.source_window((y0, x0, h, w), d, Hj, Wj) == (sy, sx, sh, sw)
    for (x0, w), (sx, sw) in cols.items():
        for y0, h in ((0, H), (H - 1, 1)):
            sy, sh = rows[(y0, h)]
            assert PY.source_window((y0, x0, h, w), d, Hj, Wj) == (sy, sx, sh, sw) == FR.source_window((y0, x0, h, w), d, Hj, Wj)


def test_source_window_refuses_what_is_no_window_or_shift():
    assert PY.source_window((0, 0, 150, 200), 1, 75, 100) == (0, 0, 75, 100) and PY.source_window((0, 0, 1, 1), 15, 1, 1) == (0, 0, 1, 1)
    for bad, text in (((0, 0, 1), "a window is"), ((0, 0, 0, 1), "h, w >= 1"), ((-1, 0, 1, 1), "y0, x0 >= 0"), ((0.0, 0, 1, 1), "is an integer")):
        with pytest.raises(ValueError, match=f"source_window: .*{text}"):
            PY.source_window(bad, 1, 4, 4)
    for d in (0, 16, 1.0):
        with pytest.raises(ValueError, match="source_window: d is"):
            PY.source_window((0, 0, 1, 1), d, 4, 4)
    with pytest.raises(ValueError, match="at least 1 x 1"):
        PY.source_window((0, 0, 1, 1), 1, 0, 4)


# ---------------------------------------------------------------------------------------------------- the restatement
def _level(H, W, V=16, seed=0):
    g = TL.grid(H, W, 64, V)
    n = g["R"] * g["C"]
    tiles = (np.random.default_rng(seed + n + H).random((n, 3, 64, 64), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    return g, tiles, np.arange(n).reshape(g["R"], g["C"])


@pytest.mark.parametrize("d", [1, 2, 5])
def test_restatement_a_constant_stays_constant_bit_for_bit(d):
    H, W = 75, 100
    Hj, Wj = -(-H // 2 ** d), -(-W // 2 ** d)
    for value in (np.float32(0.1), np.float32(-3.7e-5), np.float32(1) / np.float32(3), np.float32(255.5)):
        up = FR.upsample(np.full((3, Hj, Wj), value, dtype=np.float32), (0, 0, Hj, Wj), (0, 0, H, W), d, Hj, Wj)
        assert up.dtype == np.float32 and up.shape == (3, H, W) and (_bits(up) == _bits(np.float32(value))).all()


def test_restatement_at_d_1_the_weights_are_a_quarter_and_three_quarters():
    r0, r1, f = FR.axis(np.arange(8), 1, 4)
    assert r0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and r1.tolist() == [0, 1, 1, 2, 2, 3, 3, 3]
    assert f.dtype == np.float32 and f.tolist() == [0.75, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]
    for d in (2, 5, 15):                                                        # never 0 or 1, and exact: odd numerators over 2^(d+1)
        _, _, f = FR.axis(np.arange(3 * 2 ** d), d, 3)
        assert ((f > 0) & (f < 1)).all() and (f.astype(np.float64) * 2 ** (d + 1) % 2 == 1).all()
    src = np.zeros((3, 1, 2), dtype=np.float32)
    src[:, 0, 1] = 1
    up = FR.upsample(src, (0, 0, 1, 2), (0, 0, 2, 4), 1, 1, 2)                  # the edge is replicated: 0, 1/4, 3/4, 1
    assert up[0].tolist() == [[0, 0.25, 0.75, 1]] * 2


@pytest.mark.parametrize("V", [0, 16, 32])
def test_restatement_all_tiles_is_the_blend_none_is_the_upsample_and_sharp_is_all_tiles_available(V):
    g, tiles, slot = _level(150, 200, V)
    Hj, Wj = 75, 100
    below = np.random.default_rng(3).random((3, Hj, Wj), dtype=np.float32)
    for win in [(0, 0, 150, 200), (40, 31, 70, 101), (149, 199, 1, 1)]:
        src = FR.source_window(win, 1, Hj, Wj)
        crop = np.ascontiguousarray(below[:, src[0]:src[0] + src[2], src[1]:src[1] + src[3]])
        up = FR.upsample(below, (0, 0, Hj, Wj), win, 1, Hj, Wj)
        assert np.array_equal(_bits(up), _bits(FR.upsample(crop, src, win, 1, Hj, Wj)))       # the source window suffices
        assert np.array_equal(_bits(FR.compose(tiles, slot, g, win, crop, src, 1, Hj, Wj)), _bits(TR.blend(tiles, slot, g, win)[0]))
        assert np.array_equal(_bits(FR.compose(tiles, np.full_like(slot, -1), g, win, crop, src, 1, Hj, Wj)), _bits(up))
        assert np.array_equal(_bits(FR.compose(None, None, None, win, crop, src, 1, Hj, Wj)), _bits(up))
    # sharp exactly when all of the pixel's tiles are available: the blend sums the tiles whose extent holds the pixel
    # (test_tiles_for_is_what_the_blend_reads), so a tile that is not available takes its whole extent with it
    win = (0, 0, 150, 200)
    rng = np.random.default_rng(V)
    for _ in range(4):
        part = np.where(rng.random(slot.shape) < 0.5, slot, -1)
        want = np.ones((150, 200), dtype=bool)
        for r, c in zip(*np.nonzero(part < 0)):
            want[r * g["Sy"]:r * g["Sy"] + 64, c * g["Sx"]:c * g["Sx"] + 64] = False
        assert np.array_equal(FR.sharp(part, g, win), want) and 0 < want.sum() < want.size
        assert all(want[y, x] == all(part[rc] >= 0 for rc in TL.tiles_for(g, (y, x, 1, 1))) for y in range(0, 150, 7) for x in range(0, 200, 3))
        got = FR.compose(tiles, part, g, win, below, (0, 0, Hj, Wj), 1, Hj, Wj)
        full, up = TR.blend(tiles, slot, g, win)[0], FR.upsample(below, (0, 0, Hj, Wj), win, 1, Hj, Wj)
        assert np.array_equal(_bits(got), _bits(np.where(want[None], full, up)))


def test_restatement_chain_skips_a_level_that_is_not_usable():
    shapes = [(150, 200), (75, 100), (38, 50)]
    lv = [_level(*s, seed=k) for k, s in enumerate(shapes)]
    none0 = (lv[0][1], np.full_like(lv[0][2], -1), lv[0][0])
    full2 = (lv[2][1], lv[2][2], lv[2][0])
    win = (40, 31, 70, 101)
    src = FR.source_window(win, 2, 38, 50)
    want = FR.upsample(TR.blend(lv[2][1], lv[2][2], lv[2][0], src)[0], src, win, 2, 38, 50)
    assert np.array_equal(_bits(FR.chain([none0, None, full2], shapes, win, 0)), _bits(want))
    assert np.array_equal(_bits(FR.chain([None, None, full2], shapes, win, 0)), _bits(want))
    half1 = (lv[1][1], np.where(np.eye(2, dtype=bool), lv[1][2], -1), lv[1][0])
    got = FR.chain([none0, half1, full2], shapes, win, 0)
    assert not np.array_equal(_bits(got), _bits(want)) and got.shape == (3, 70, 101)


# ------------------------------------------------------------------------------------------- tile_ready and tile_rounds
def _want(data, n):
    """(tile_ready, tile_rounds) of ``data[:n]`` from ``_Picture``'s offsets alone."""
    s = TL._parse(data[:max(n, TL.layout(data)["header_end"])], "test")[1]
    R, C = s.g["R"], s.g["C"]
    ready = np.array([bool(s.present[i]) and int(s.off[0, i] + s.size[0, i]) <= n for i in range(R * C)])
    rounds = np.full(R * C, -1, dtype=np.int64)
    for i in np.flatnonzero(ready):
        rounds[i] = 0
        for k in range(1, 1 + s.nr):
            if int(s.off[k, i] + s.size[k, i]) > n and s.size[k, i] > 0:
                break
            rounds[i] = k
    return ready.reshape(R, C), rounds.reshape(R, C)


@pytest.mark.parametrize("name", ["v1-3x4", "v3-1x5", "extract"])
def test_tile_ready_and_tile_rounds_follow_the_bytes_head_by_head(name):
    data = {"v1-3x4": lambda: picture()[2], "v3-1x5": lambda: picture_v3()[2],
            "extract": lambda: TL.extract(picture()[2], (10, 70, 30, 60), 2)}[name]()
    lay = TL.layout(data)
    f = TL.PictureFeed()
    assert f.tile_ready is None and f.tile_rounds is None
    f.feed(data[:lay["header_end"] - 1])
    assert f.tile_ready is None and f.tile_rounds is None                       # they exist once the header is complete
    heads = [o + n for row in lay["head"] for o, n in row if n]
    cuts = sorted({lay["header_end"]} | {e + dlt for e in heads for dlt in (-7, -1, 0, 3)} | set(lay["round_end"])
                  | {o + n + dlt for k in lay["piece"] for row in k for o, n in row if n for dlt in (-1, 0)} | {len(data)})
    at = len(f)
    seen = set()
    for n in [c for c in cuts if at < c <= len(data)]:
        f.feed(data[at:n])
        at = n
        ready, rounds = _want(data, n)
        assert f.tile_ready.dtype == bool and np.array_equal(f.tile_ready, ready) and np.array_equal(f.tile_rounds, rounds), n
        assert (f.tile_rounds >= 0).tolist() == f.tile_ready.tolist()
        assert (f.rounds is None) == (n < lay["need_bytes"]) and (f.rounds is None or np.array_equal(f.rounds, f.tile_rounds))
        seen.add(int(ready.sum()))
    present = sum(p for row in lay["present"] for p in row)
    assert seen == set(range(present + 1))                                      # the heads came in one by one, cuts inside them
    assert int(f.tile_rounds.max()) == lay["n_rounds"] and (name != "extract" or (f.tile_rounds == -1).sum() == 12 - present)


def test_a_refused_feed_leaves_tile_ready_and_tile_rounds_as_they_were():
    data = picture()[2]
    lay = TL.layout(data)
    o, n = lay["head"][0][2]
    f = TL.PictureFeed()
    f.feed(data[:o + 3])
    ready, rounds = f.tile_ready.copy(), f.tile_rounds.copy()
    assert ready.sum() == 2
    with pytest.raises(ValueError, match=r"PictureFeed.feed: .*tile \(0, 2\)"):  # the head that would complete contradicts the table
        f.feed(data[o + 3:o + 20] + bytes([data[o + 20] ^ 0x40]) + data[o + 21:o + n])
    with pytest.raises(ValueError, match="bytes follow the codestream"):
        f.feed(data[o + 3:] + b"\0")
    assert np.array_equal(f.tile_ready, ready) and np.array_equal(f.tile_rounds, rounds)
    f.feed(data[o + 3:o + n])
    assert f.tile_ready.sum() == 3 and f.tile_rounds[0, 2] == 0
