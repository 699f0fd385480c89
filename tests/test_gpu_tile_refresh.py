"""vam_tile_refresh on the GPU without a model: a persistent canvas re-blended only where a dirty tile
contributes.  Every result is bit-exact against the NumPy restatement of tests/tiled_stream_ref.py (which is built on
tests/tiled_ref.py's blend); pixels without a dirty tile keep their sentinel; guards of 1024 elements around the canvas stay
intact; a clean tile that no dirty pixel needs may be absent; malformed calls are errors through vam_last_error and write
nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiled_ref as TR                                # noqa: E402
import tiled_stream_ref as RR                         # noqa: E402
from vampic import _lib as L, ops, tiled as TL        # noqa: E402

GRIDS = [(37, 53, 64, 0), (150, 200, 64, 16), (150, 200, 64, 7), (60, 200, 128, 32), (129, 70, 64, 0)]
GUARD = 1024
_TILES = {}


def _tiles(g):
    key = (g["H"], g["W"], g["th"], g["tw"])
    if key not in _TILES:
        n = g["R"] * g["C"]
        t = (np.random.default_rng(n + g["H"]).random((n, 3, g["th"], g["tw"]), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
        _TILES[key] = (t, torch.from_numpy(t).cuda())
    return _TILES[key]


def _sentinel(window, u8):
    """A canvas that no blend produces: per pixel another value, fp32 below -7 or bytes from a seeded draw."""
    _, _, h, w = window
    rng = np.random.default_rng(h * 1000 + w)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if u8 else (-7 - rng.random((3, h, w), dtype=np.float32)).astype(np.float32)


def _refresh(g, slot, dirty, window, box, u8=False, canvas=None):
    """(canvas afterwards, status) of one ops.tile_refresh on a guarded canvas; a uint8 canvas starts at an odd byte."""
    tiles_dev = _tiles(g)[1]
    canvas = _sentinel(window, u8) if canvas is None else canvas
    numel, fill = canvas.size, (0x5A if u8 else -3.0)
    whole = torch.full((numel + 2 * GUARD + 1,), fill, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    view = whole[GUARD + 1:GUARD + 1 + numel]
    assert not u8 or view.data_ptr() % 2 == 1
    out = view.view(canvas.shape)
    out.copy_(torch.from_numpy(canvas))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(g["V"])) if g["V"] else (None, None)
    ops.tile_refresh(tiles_dev, torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32)).cuda(),
                     torch.from_numpy(np.ascontiguousarray(dirty, dtype=np.int32)).cuda(), w_lo, w_hi, g["H"], g["W"], g["V"], window, box,
                     out, status)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD + 1] == fill).all()) and bool((whole[GUARD + 1 + numel:] == fill).all())
    return out.cpu().numpy(), int(status.item())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _windows(g):
    """The whole picture, and windows at odd x0 of widths 1, 3, 17 and one that is no multiple of 4."""
    H, W = g["H"], g["W"]
    wins = [(0, 0, H, W), (H // 2, 5, 3, 1), (1, 7, H - 2, 3), (2, W // 2 - 9, H - 5, 17), (3, 1, H - 3, W - 3 - (W - 3) % 4 + 2)]
    return [(y0, x0, h, min(w, W - x0)) for y0, x0, h, w in wins]


def _bbox(g, dirty, window):
    cy0, cx0, ch, cw = window
    rows, cols = np.flatnonzero(dirty.any(1)), np.flatnonzero(dirty.any(0))
    y0, y1 = max(cy0, rows[0] * g["Sy"]), min(cy0 + ch, rows[-1] * g["Sy"] + g["th"])
    x0, x1 = max(cx0, cols[0] * g["Sx"]), min(cx0 + cw, cols[-1] * g["Sx"] + g["tw"])
    return (int(y0), int(x0), int(y1 - y0), int(x1 - x0)) if y1 > y0 and x1 > x0 else None


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
@pytest.mark.parametrize("H,W,tile,V", GRIDS)
def test_none_all_each_tile_and_a_checkerboard_against_the_restatement(H, W, tile, V, u8):
    g = TL.grid(H, W, tile, V)
    R, C = g["R"], g["C"]
    tiles, tiles_dev = _tiles(g)
    slot = np.arange(R * C).reshape(R, C)
    assert (R, C) == {37: (1, 1), 150: (3, 4), 60: (1, 2), 129: (3, 2)}[H] or V == 7
    singles = [np.eye(1, R * C, i, dtype=np.int32).reshape(R, C) for i in range(R * C)]
    checker = (np.add.outer(np.arange(R), np.arange(C)) % 2).astype(np.int32)
    for win in _windows(g):
        y0, x0, h, w = win
        start = _sentinel(win, u8)
        got, status = _refresh(g, np.full((R, C), -1), np.zeros((R, C)), win, win, u8)        # nothing dirty: nothing read, nothing written
        assert status == 0 and _same(got, start), win
        got, status = _refresh(g, slot, np.ones((R, C)), win, win, u8)                         # everything dirty: the blend of the window
        blend = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") if u8 else torch.empty((3, h, w), device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(V)) if V else (None, None)
        ops.tile_blend(tiles_dev, torch.from_numpy(slot.astype(np.int32)).cuda(), w_lo, w_hi, H, W, V, win, blend, st)
        assert status == 0 and _same(got, blend.cpu().numpy()) and _same(got, RR.refresh(start, tiles, slot, np.ones((R, C)), g, win, win)[0]), win
        for dirty in singles + ([checker] if R * C > 1 else []):
            box = _bbox(g, dirty, win)
            if box is None:                                                     # the dirty tiles do not meet this window
                continue
            want, missing = RR.refresh(start, tiles, slot, dirty, g, win, box)
            got, status = _refresh(g, slot, dirty, win, box, u8)
            assert status == 0 and not missing and _same(got, want), (win, dirty.tolist())
            assert _same(_refresh(g, slot, dirty, win, win, u8)[0], want)       # a box larger than needed visits clean pixels only
            by, bx, bh, bw = box
            small = (by + (bh > 2), bx + (bw > 3), max(1, bh - 2), max(1, bw - 5))          # a box smaller than the dirty one
            want, _ = RR.refresh(start, tiles, slot, dirty, g, win, small)
            assert _same(_refresh(g, slot, dirty, win, small, u8)[0], want), (win, small)


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
def test_clean_absent_tiles_are_never_read_and_a_needed_one_sets_the_status(u8):
    g = TL.grid(150, 200, 64, 16)
    tiles, _ = _tiles(g)
    full = np.arange(12).reshape(3, 4)
    win = (0, 0, 150, 200)
    dirty = np.zeros((3, 4), dtype=np.int32)
    dirty[1, 1] = 1
    slot = np.full((3, 4), -1)
    slot[0:3, 0:3] = full[0:3, 0:3]                                             # the neighbours of (1, 1); column 3 is absent
    start = _sentinel(win, u8)
    want, missing = RR.refresh(start, tiles, slot, dirty, g, win, win)
    got, status = _refresh(g, slot, dirty, win, win, u8)
    assert not missing and status == 0 and _same(got, want)
    assert _same(got, RR.refresh(start, tiles, full, dirty, g, win, win)[0])    # what the absent tiles held does not show
    slot[0, 1] = -1                                                             # the band rows 48 .. 63 of tile (1, 1) need (0, 1)
    want, missing = RR.refresh(start, tiles, slot, dirty, g, win, win)
    got, status = _refresh(g, slot, dirty, win, win, u8)
    assert missing and status == 1 and _same(got, want)                         # that term is skipped, as in vam_tile_blend
    got, status = _refresh(g, slot, dirty, win, (64, 64, 32, 32), u8)           # a box in the core of (1, 1) does not need it
    assert status == 0 and _same(got, RR.refresh(start, tiles, slot, dirty, g, win, (64, 64, 32, 32))[0])
    slot[0, 1] = 12                                                             # a slot beyond the buffer is absent, too
    assert _refresh(g, slot, dirty, win, win, u8)[1] == 1


def test_a_sequence_of_refreshes_keeps_the_canvas_equal_to_the_blend():
    g = TL.grid(150, 200, 64, 7)
    tiles, _ = _tiles(g)
    slot = np.arange(g["R"] * g["C"]).reshape(g["R"], g["C"])
    win = (9, 13, 120, 150)
    canvas = _sentinel(win, False)
    seen = np.zeros_like(slot)
    for r, c in [(1, 1), (0, 0), (2, 2), (1, 2), (0, 1), (1, 0), (0, 2), (2, 0), (2, 1)]:
        dirty = np.zeros_like(slot)
        dirty[r, c] = 1
        seen |= dirty
        canvas, status = _refresh(g, slot, dirty, win, _bbox(g, dirty, win), canvas=canvas)
        assert status == 0
        assert _same(canvas, RR.refresh(_sentinel(win, False), tiles, slot, seen, g, win, win)[0]), (r, c)
    assert TL.tiles_for(g, win) == [(r, c) for r in range(3) for c in range(3)]
    assert _same(canvas, TR.blend(tiles, slot, g, win)[0])


def test_malformed_calls_are_errors_and_write_nothing():
    lib = L.load()
    g = TL.grid(150, 200, 64, 16)
    tiles = _tiles(g)[1]
    slot = torch.arange(12, dtype=torch.int32, device="cuda").view(3, 4)
    dirty = torch.ones((3, 4), dtype=torch.int32, device="cuda")
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(16))
    out = torch.full((3 * 150 * 200,), -7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = ops.stream_ptr()
    ptr = lambda t: t.data_ptr() if t is not None else None

    def call(H=150, W=200, th=64, tw=64, V=16, cwin=(0, 0, 150, 200), box=(0, 0, 150, 200), n=12, u8=0, lo=w_lo, hi=w_hi, st=status,
             sl=slot, di=dirty, ti=tiles, o=out):
        return lib.vam_tile_refresh(ptr(ti), n, ptr(sl), ptr(di), ptr(lo), ptr(hi), H, W, th, tw, V, *cwin, *box, ptr(o), u8, ptr(st), s)

    cases = [(lambda: call(V=33), "overlap 33"), (lambda: call(H=0), "a picture of 0 x 200"), (lambda: call(th=0), "tiles of 0 x 64"),
             (lambda: call(cwin=(0, 0, 151, 200)), "the canvas window (y0 0, x0 0, h 151, w 200) does not lie inside the 150 x 200 picture"),
             (lambda: call(cwin=(-1, 0, 10, 10), box=(0, 0, 5, 5)), "the canvas window"),
             (lambda: call(cwin=(0, 190, 10, 11), box=(0, 190, 5, 5)), "the canvas window"),
             (lambda: call(cwin=(10, 10, 0, 10), box=(10, 10, 1, 1)), "the canvas window"),
             (lambda: call(cwin=(10, 20, 50, 60), box=(9, 20, 5, 5)), "the box (y0 9, x0 20, h 5, w 5) does not lie inside the canvas window (y0 10, x0 20, h 50, w 60)"),
             (lambda: call(cwin=(10, 20, 50, 60), box=(10, 19, 5, 5)), "the box"), (lambda: call(cwin=(10, 20, 50, 60), box=(10, 20, 51, 5)), "the box"),
             (lambda: call(cwin=(10, 20, 50, 60), box=(30, 70, 5, 11)), "the box"), (lambda: call(cwin=(10, 20, 50, 60), box=(30, 70, 0, 5)), "the box"),
             (lambda: call(cwin=(10, 20, 50, 60), box=(2147483647, 20, 1, 1)), "the box"),
             (lambda: call(H=1 << 20, W=64, cwin=(0, 0, 1 << 20, 64), box=(0, 0, 4 * 65535 + 1, 64)), "a box of 262141 rows exceeds one launch"),
             (lambda: call(n=0), "a buffer of 0 tiles"), (lambda: call(u8=2), "out_u8 is 0"), (lambda: call(lo=None), "needs the two ramp tables"),
             (lambda: call(di=None), "need tiles, slot, dirty, out and status"), (lambda: call(st=None), "need tiles"), (lambda: call(o=None), "need tiles")]
    for fn, text in cases:
        assert fn() != 0, text
        assert "vam_tile_refresh" in lib.vam_last_error().decode() and text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and int(status.item()) == 0
    with pytest.raises(L.VamError, match="vam_tile_refresh failed .*the box .* does not lie inside the canvas window"):
        ops.tile_refresh(tiles, slot, dirty, w_lo, w_hi, 150, 200, 16, (100, 100, 50, 10), (100, 100, 51, 10), torch.empty((3, 50, 10), device="cuda"), status)
    assert call() == 0                                                          # and the well-formed call goes through
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and not bool((out == -7.0).any())
