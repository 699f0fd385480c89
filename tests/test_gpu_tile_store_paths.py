"""vam_tile_blend, vam_tile_compose and vam_tile_refresh share one store (csrc/tiles.hip, store_pixels): where its paths
switch -- the window's first column and width decide which rows are aligned and how many of a thread's four pixels exist --
the three agree bit for bit, in fp32 and uint8; and a write mask that is neither empty nor full (refresh across the edge of a
dirty tile) writes exactly its pixels of a uint8 canvas."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import ops, tiled as TL                   # noqa: E402

H, W, TILE = 37, 45, 16
WINDOWS = [(y0, x0, h, w) for y0 in (0, 5) for h in (1, 6) for x0 in range(5) for w in range(1, 10)]


def _setup(V):
    g = TL._geometry(H, W, TILE, TILE, V, "test")
    n = g["R"] * g["C"]
    tiles = (torch.from_numpy(np.random.default_rng(n + V).random((n, 3, TILE, TILE), dtype=np.float32)) * 1.5 - 0.25).cuda()
    slot = torch.arange(n, dtype=torch.int32, device="cuda").view(g["R"], g["C"])
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(V)) if V else (None, None)
    return g, tiles, slot, w_lo, w_hi


def _new(h, w, dtype, fill=None):
    shape = (3, h, w) if dtype == torch.float32 else (h, w, 3)
    return torch.empty(shape, dtype=dtype, device="cuda") if fill is None else torch.full(shape, fill, dtype=dtype, device="cuda")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "uint8"])
@pytest.mark.parametrize("V", [3, 0])
def test_blend_compose_and_refresh_agree_where_the_store_switches_paths(V, dtype):
    g, tiles, slot, w_lo, w_hi = _setup(V)
    assert (g["R"], g["C"]) == ((3, 4) if V else (3, 3))
    Hj, Wj = (H + 1) // 2, (W + 1) // 2
    below = torch.from_numpy(np.random.default_rng(5).random((3, Hj, Wj), dtype=np.float32)).cuda() + 1000.0     # a value that leaks would show
    dirty = torch.ones_like(slot)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for win in WINDOWS:
        _, _, h, w = win
        blend, compose, canvas = _new(h, w, dtype), _new(h, w, dtype), _new(h, w, dtype, 0)
        ops.tile_blend(tiles, slot, w_lo, w_hi, H, W, V, win, blend, status)
        ops.tile_compose(tiles, slot, w_lo, w_hi, H, W, V, win, below, (0, 0, Hj, Wj), 1, compose, status)
        ops.tile_refresh(tiles, slot, dirty, w_lo, w_hi, H, W, V, win, win, canvas, status)
        assert _same(blend, compose) and _same(blend, canvas), win
    assert int(status.item()) == 0


def test_a_partial_write_mask_writes_exactly_the_dirty_pixels_of_a_uint8_canvas():
    g, tiles, slot, _, _ = _setup(0)                                            # overlap 0: every pixel has a single tile
    Sx = g["Sx"]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    blend = _new(H, W, torch.uint8)
    ops.tile_blend(tiles, slot, None, None, H, W, 0, (0, 0, H, W), blend, status)
    dirty = torch.zeros_like(slot)
    dirty[:, 1] = 1
    for x0 in (Sx - 1, Sx - 2, Sx - 3):                                         # a thread's four pixels straddle both edges of column 1
        canvas = _new(H, W, torch.uint8, 0xAB)
        ops.tile_refresh(tiles, slot, dirty, None, None, H, W, 0, (0, 0, H, W), (0, x0, H, W - x0), canvas, status)
        want = torch.full_like(canvas, 0xAB)
        want[:, Sx:2 * Sx] = blend[:, Sx:2 * Sx]
        assert _same(canvas, want), x0
    assert int(status.item()) == 0
