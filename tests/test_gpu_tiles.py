"""The tile kernels on the GPU without a model (vam_tile_extract, vam_tile_blend): every result is
bit-exact against the NumPy float32 restatement of tests/tiled_ref.py; guard regions around the outputs stay untouched;
malformed geometry is an error through vam_last_error and writes nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiled_ref as TR                                # noqa: E402
from vampic import _lib as L, ops, tiled as TL        # noqa: E402

GRIDS = [(37, 53, 64, 32), (150, 200, 64, 16), (60, 200, 128, 32)]      # one replicated tile; 3 x 4; tiles of 64 x 128, 1 x 2
GUARD = 1024
_PICTURES, _TILES = {}, {}


def _picture(H, W):
    if (H, W) not in _PICTURES:
        _PICTURES[(H, W)] = np.random.default_rng(H * W).random((3, H, W), dtype=np.float32)
    return _PICTURES[(H, W)]


def _tiles(g, n=None):
    """Random tile buffers, unrelated from tile to tile (a blend of them shows every weight), with values outside [0, 1]."""
    n = g["R"] * g["C"] if n is None else n
    key = (g["H"], g["W"], g["th"], g["tw"], n)
    if key not in _TILES:
        _TILES[key] = (np.random.default_rng(n + g["H"]).random((n, 3, g["th"], g["tw"]), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    return _TILES[key]


def _guarded(numel, dtype, fill):
    """(whole buffer, the view of ``numel`` elements between two guards of GUARD elements)."""
    whole = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + numel]


def _guards_intact(whole, numel, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + numel:] == fill).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _extract(img, g, coords):
    n = len(coords)
    whole, view = _guarded(n * 3 * g["th"] * g["tw"], torch.float32, -7.0)
    out = view.view(n, 3, g["th"], g["tw"])
    ops.tile_extract(img, torch.tensor(coords, dtype=torch.int32, device="cuda"), out, g["V"])
    torch.cuda.synchronize()
    assert _guards_intact(whole, out.numel(), -7.0)
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W,tile,V", GRIDS + [(129, 70, 64, 0)])
def test_extract_in_one_launch_and_in_two(H, W, tile, V):
    g = TL.grid(H, W, tile, V)
    pic = _picture(H, W)
    img = torch.from_numpy(pic).cuda()
    coords = TL.tiles_for(g)
    want = TR.extract(pic, g, coords)
    got = _extract(img, g, coords)
    assert np.array_equal(_bits(got), _bits(want))
    order = coords[::-1]                                                        # any list, any order; then two launches
    assert np.array_equal(_bits(_extract(img, g, order)), _bits(want[::-1]))
    if len(coords) > 1:
        k = (len(coords) + 1) // 2
        two = np.concatenate([_extract(img, g, coords[:k]), _extract(img, g, coords[k:])])
        assert np.array_equal(_bits(two), _bits(want))
    if H < g["th"] and W < g["tw"]:                                             # everything below and right of the picture is its edge
        assert np.array_equal(got[0][:, H:, :W], np.broadcast_to(pic[:, H - 1:H, :], (3, g["th"] - H, W)))
        assert np.array_equal(got[0][:, :, W:], np.broadcast_to(got[0][:, :, W - 1:W], (3, g["th"], g["tw"] - W)))


def test_extract_from_an_unaligned_picture_and_a_coordinate_outside_the_grid():
    g = TL.grid(150, 200, 64, 16)
    base = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), _picture(150, 200).reshape(-1)])).cuda()
    img = base[1:].view(3, 150, 200)                                           # 4 bytes off a 16-byte boundary: the scalar loads
    assert img.data_ptr() % 16 == 4
    want = TR.extract(_picture(150, 200), g, TL.tiles_for(g))
    assert np.array_equal(_bits(_extract(img, g, TL.tiles_for(g))), _bits(want))
    got = _extract(img, g, [(0, 0), (3, 0), (0, 4), (-1, 2), (2, 3)])          # not tiles of a 3 x 4 grid: left unwritten
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[4]), _bits(want[11]))
    assert (got[1:4] == -7.0).all()


def _blend(tiles_dev, slot, g, window, dtype=torch.float32, ramps=True):
    y0, x0, h, w = window
    fill = -7.0 if dtype == torch.float32 else 0x5A
    whole, view = _guarded(3 * h * w, dtype, fill)
    out = view.view(3, h, w) if dtype == torch.float32 else view.view(h, w, 3)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(g["V"]))
    use = ramps and g["V"] > 0
    ops.tile_blend(tiles_dev, torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32)).cuda(), w_lo if use else None,
                   w_hi if use else None, g["H"], g["W"], g["V"], window, out, status)
    torch.cuda.synchronize()
    assert _guards_intact(whole, out.numel(), fill)
    return out.cpu().numpy(), int(status.item())


def _windows(g):
    """The whole picture; 1 x 1 at a four-tile corner (or the last pixel); windows that start and end inside bands, with odd
    x0 and widths that are no multiple of 4; single rows and columns at the edges."""
    H, W, Sy, Sx, V = g["H"], g["W"], g["Sy"], g["Sx"], g["V"]
    wins = [(0, 0, H, W), (H - 1, W - 1, 1, 1), (0, 1, H, 1), (H - 1, 0, 1, W), (3, 5, min(H - 3, 9), min(W - 5, 6))]
    if g["R"] > 1 and g["C"] > 1:
        wins += [(Sy, Sx, 1, 1), (Sy + V - 1, Sx + V - 1, 1, 1), (Sy + 1, Sx + 3, V + Sy - 2, V + Sx - 5), (Sy - 2, Sx - 3, V + 5, V + 7)]
    if g["C"] > 1:
        wins += [(0, Sx + 1, min(H, 7), max(1, V - 2)), (1, 1, min(H - 1, 5), W - 2), (2, Sx - 1, 3, 2 * V + 3 if 2 * V + 3 + Sx - 1 <= W else 3)]
    return [(y0, x0, min(h, H - y0), min(w, W - x0)) for y0, x0, h, w in wins if y0 < H and x0 < W]


@pytest.mark.parametrize("H,W,tile,V", GRIDS + [(150, 200, 64, 0), (150, 200, 64, 32), (100, 131, 64, 7)])
def test_blend_every_window_against_the_restatement(H, W, tile, V):
    g = TL.grid(H, W, tile, V)
    tiles = _tiles(g)
    dev = torch.from_numpy(tiles).cuda()
    slot = np.arange(g["R"] * g["C"]).reshape(g["R"], g["C"])
    full, missing = TR.blend(tiles, slot, g)
    assert not missing
    for win in _windows(g):
        y0, x0, h, w = win
        got, status = _blend(dev, slot, g, win)
        assert status == 0 and np.array_equal(_bits(got), _bits(full[:, y0:y0 + h, x0:x0 + w])), win
        u8, status = _blend(dev, slot, g, win, torch.uint8)
        assert status == 0 and np.array_equal(u8, TR.to_u8(got)), win           # the write_image formula on the fp32 output
    assert full.min() < 0 and full.max() > 1                                    # the uint8 output clamps on both sides
    if V == 0:                                                                  # no band: every pixel is a copy; no tables are read
        got, _ = _blend(dev, slot, g, (0, 0, H, W), ramps=False)
        assert np.array_equal(_bits(got), _bits(full))


def test_blend_through_permuted_slots_with_unneeded_tiles_absent():
    g = TL.grid(150, 200, 64, 16)
    win = (40, 90, 30, 17)                                                      # rows 40..69, columns 90..106: tiles (0..1, 1..2)
    need = TL.tiles_for(g, win)
    assert need == [(0, 1), (0, 2), (1, 1), (1, 2)]
    tiles = _tiles(g, 6)                                                        # a buffer larger than the tiles in use
    order = [4, 0, 5, 2]
    slot = np.full((3, 4), -1)
    for s, (r, c) in zip(order, need):
        slot[r, c] = s
    want, missing = TR.blend(tiles, slot, g, win)
    assert not missing
    dense = np.zeros((12, 3, 64, 64), dtype=np.float32)                         # the same tiles in raster slots
    for s, (r, c) in zip(order, need):
        dense[r * 4 + c] = tiles[s]
    assert np.array_equal(_bits(want), _bits(TR.blend(dense, np.arange(12).reshape(3, 4), g, win)[0]))
    got, status = _blend(torch.from_numpy(tiles).cuda(), slot, g, win)
    assert status == 0 and np.array_equal(_bits(got), _bits(want))
    # the guard: a window that needs an absent tile sets the status word, skips that term and still writes inside its output only
    wide = (40, 90, 30, 60)
    want, missing = TR.blend(tiles, slot, g, wide)
    got, status = _blend(torch.from_numpy(tiles).cuda(), slot, g, wide)
    assert missing and status == 1 and np.array_equal(_bits(got), _bits(want))
    slot[0, 1] = 6                                                              # a slot beyond the buffer is absent, too
    assert _blend(torch.from_numpy(tiles).cuda(), slot, g, win)[1] == 1


def test_malformed_geometry_is_an_error_and_writes_nothing():
    lib = L.load()
    g = TL.grid(150, 200, 64, 16)
    tiles = torch.from_numpy(_tiles(g)).cuda()
    img = torch.from_numpy(_picture(150, 200)).cuda()
    coords = torch.tensor(TL.tiles_for(g), dtype=torch.int32, device="cuda")
    slot = torch.arange(12, dtype=torch.int32, device="cuda").view(3, 4)
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(16))
    out = torch.full((12 * 3 * 64 * 64,), -7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = ops.stream_ptr()

    def extract(H=150, W=200, th=64, tw=64, V=16, n=12, image=img, co=coords, o=out):
        return lib.vam_tile_extract(image.data_ptr() if image is not None else None, H, W, th, tw, V,
                                    co.data_ptr() if co is not None else None, n, o.data_ptr() if o is not None else None, s)

    def blend(H=150, W=200, th=64, tw=64, V=16, win=(0, 0, 150, 200), n=12, u8=0, lo=w_lo, hi=w_hi, st=status):
        return lib.vam_tile_blend(tiles.data_ptr(), n, slot.data_ptr(), lo.data_ptr() if lo is not None else None,
                                  hi.data_ptr() if hi is not None else None, H, W, th, tw, V, *win, out.data_ptr(), u8,
                                  st.data_ptr() if st is not None else None, s)

    cases = [(lambda: extract(V=33), "overlap 33"), (lambda: extract(V=-1), "overlap -1"), (lambda: extract(H=0), "a picture of 0 x 200"),
             (lambda: extract(th=0), "tiles of 0 x 64"), (lambda: extract(n=0), "1 .. 65535 tiles"), (lambda: extract(image=None), "need image"),
             (lambda: extract(co=None), "need image, coords and out"), (lambda: extract(W=(1 << 24) + 1), "sides are 1"),
             (lambda: blend(V=33), "overlap 33"), (lambda: blend(tw=16), "overlap 16"), (lambda: blend(win=(0, 0, 151, 200)), "does not lie inside"),
             (lambda: blend(win=(-1, 0, 10, 10)), "does not lie inside"), (lambda: blend(win=(0, 190, 10, 11)), "does not lie inside"),
             (lambda: blend(win=(0, 0, 0, 10)), "does not lie inside"), (lambda: blend(n=0), "a buffer of 0 tiles"),
             (lambda: blend(u8=2), "out_u8 is 0"), (lambda: blend(lo=None), "needs the two ramp tables"), (lambda: blend(st=None), "need tiles")]
    for call, text in cases:
        assert call() != 0, text
        assert text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and int(status.item()) == 0
    with pytest.raises(L.VamError, match="vam_tile_blend failed .*does not lie inside"):
        ops.tile_blend(tiles, slot, w_lo, w_hi, 150, 200, 16, (100, 100, 51, 10), torch.empty((3, 51, 10), device="cuda"), status)
    assert extract() == 0 and blend() == 0                                      # and the well-formed calls go through
