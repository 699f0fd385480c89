"""vam_tile_schedule on the GPU without a model: a picture-wide schedule at pixel resolution brought
down onto the tiles' latent grids.  Every result equals the NumPy restatement of tests/tiled_schedule_ref.py value for value
(-0 equal to +0, NaNs at equal positions; a maximum rounds nothing); guard regions around the outputs stay untouched;
malformed calls are errors through vam_last_error and write nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tiled_schedule_ref as SR                          # noqa: E402
from test_tiled_schedule_cpu import _monotone            # noqa: E402
from vampic import _lib as L, ops, tiled as TL           # noqa: E402

GRIDS = [(37, 53, 64, 0), (150, 200, 64, 16), (150, 200, 64, 7), (60, 200, 128, 32), (129, 70, 64, 0)]
GUARD = 1024
FILL = -7.0
_MAPS = {}


def _maps(H, W):
    """A schedule of 32 stages, made once per picture size and left unchanged; its first L stages are a schedule of L."""
    if (H, W) not in _MAPS:
        _MAPS[(H, W)] = _monotone(32, H, W, 31 * H + W)
    return _MAPS[(H, W)]


def _run(maps_dev, g, coords, V=None):
    """The kernel's output for ``coords`` as a NumPy array, its guards checked."""
    n, nl, h, w = len(coords), int(maps_dev.shape[0]), g["th"] // 16, g["tw"] // 16
    whole = torch.full((n * nl * h * w + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
    out = whole[GUARD:GUARD + n * nl * h * w].view(n, nl, h, w)
    ops.tile_schedule(maps_dev, torch.tensor(coords, dtype=torch.int32, device="cuda"), out, g["th"], g["tw"], g["V"] if V is None else V)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + out.numel():] == FILL).all())
    return out.cpu().numpy()


@pytest.mark.parametrize("L_", [1, 3, 32])
@pytest.mark.parametrize("H,W,tile,V", GRIDS)
def test_the_tile_list_in_one_launch_reversed_and_in_two(H, W, tile, V, L_):
    g = TL.grid(H, W, tile, V)
    S = _maps(H, W)[:L_]
    dev = torch.from_numpy(S).cuda()
    coords = TL.tiles_for(g)
    want = SR.tile_schedule(S, g, coords)
    assert len(np.unique(want)) > 2
    got = _run(dev, g, coords)
    assert got.dtype == np.float32 and SR.same(got, want)
    assert SR.same(_run(dev, g, coords[::-1]), want[::-1])
    if len(coords) > 1:
        k = (len(coords) + 1) // 2
        assert SR.same(np.concatenate([_run(dev, g, coords[:k]), _run(dev, g, coords[k:])]), want)


@pytest.mark.parametrize("H,W,tile,V", [(150, 200, 64, 7), (37, 53, 64, 0)])
def test_maps_four_bytes_off_a_16_byte_boundary(H, W, tile, V):
    g = TL.grid(H, W, tile, V)
    S = _maps(H, W)[:3]
    base = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), S.reshape(-1)])).cuda()
    dev = base[1:].view(3, H, W)                                                # every row start is off by 4 bytes at least
    assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    assert SR.same(_run(dev, g, TL.tiles_for(g)), SR.tile_schedule(S, g, TL.tiles_for(g)))


def test_a_single_nan_and_a_single_inf_pixel():
    H, W = 150, 200
    g = TL.grid(H, W, 64, 16)
    coords = TL.tiles_for(g)
    for value, y, x in [(np.nan, 50, 60), (np.inf, 50, 60), (np.nan, 149, 199), (np.nan, 0, 0), (np.inf, 100, 3)]:
        S = _maps(H, W)[:2].copy()
        S[1, y, x] = value
        want = SR.tile_schedule(S, g, coords)
        got = _run(torch.from_numpy(S).cuda(), g, coords)
        assert SR.same(got, want), (value, y, x)
        hit = np.isnan(got) if np.isnan(value) else np.isinf(got)
        assert hit.any() and not hit[:, 0].any() and np.array_equal(hit, np.isnan(want) if np.isnan(value) else np.isinf(want))
    S = _maps(H, W)[:2].copy()                                                  # a NaN beside larger values: fmaxf alone would drop it
    S[0, 50, 60], S[0, 50, 61] = np.nan, 100.0
    got = _run(torch.from_numpy(S).cuda(), g, coords)
    assert np.isnan(got[0, 0, 3, 3]) and np.isnan(got[5, 0, 0, 0]) and SR.same(got, SR.tile_schedule(S, g, coords))


def test_coordinates_outside_the_grid_leave_their_rows_unwritten():
    g = TL.grid(150, 200, 64, 16)
    S = _maps(150, 200)[:3]
    want = SR.tile_schedule(S, g, TL.tiles_for(g))
    got = _run(torch.from_numpy(S).cuda(), g, [(0, 0), (3, 0), (0, 4), (-1, 2), (2, 3)])      # a 3 x 4 grid
    assert SR.same(got[0], want[0]) and SR.same(got[4], want[11]) and (got[1:4] == FILL).all()


def test_replicated_cells_take_the_last_row_and_column():
    g = TL.grid(37, 53, 64, 0)
    S = np.full((2, 37, 53), 1.0, dtype=np.float32)
    S[:, 36, :] = 7.0
    S[1, :, 52] = 9.0
    dev = torch.from_numpy(S).cuda()
    got = _run(dev, g, [(0, 0)])[0]
    assert np.array_equal(got[0], np.float32([[1] * 4, [1] * 4, [7] * 4, [7] * 4]))
    assert np.array_equal(got[1], np.float32([[1, 1, 1, 9], [1, 1, 1, 9], [7, 7, 7, 9], [7, 7, 7, 9]]))


def test_malformed_calls_are_errors_and_write_nothing():
    lib = L.load()
    S = torch.from_numpy(_maps(150, 200)[:3]).cuda()
    coords = torch.tensor(TL.tiles_for(TL.grid(150, 200, 64, 16)), dtype=torch.int32, device="cuda")
    out = torch.full((12 * 32 * 4 * 4,), FILL, device="cuda")
    s = ops.stream_ptr()

    def call(nl=3, H=150, W=200, th=64, tw=64, V=16, n=12, maps=S, co=coords, o=out):
        return lib.vam_tile_schedule(maps.data_ptr() if maps is not None else None, nl, H, W, th, tw, V,
                                     co.data_ptr() if co is not None else None, n, o.data_ptr() if o is not None else None, s)

    cases = [(lambda: call(th=72, V=0), "tiles of 72 x 64"), (lambda: call(tw=40), "tiles of 64 x 40"), (lambda: call(nl=0), "1 .. 32 stages, got 0"),
             (lambda: call(nl=33), "1 .. 32 stages, got 33"), (lambda: call(nl=-1), "1 .. 32 stages"), (lambda: call(V=33), "overlap 33"),
             (lambda: call(V=-1), "overlap -1"), (lambda: call(H=0), "a picture of 0 x 200"), (lambda: call(W=(1 << 24) + 1), "sides are 1"),
             (lambda: call(th=0), "tiles of 0 x 64"), (lambda: call(n=0), "tiles per launch at 3 stages, got 0"),
             (lambda: call(n=21846), "1 .. 21845 tiles per launch at 3 stages"), (lambda: call(maps=None), "need maps, coords and out"),
             (lambda: call(co=None), "need maps"), (lambda: call(o=None), "need maps")]
    for fn, text in cases:
        assert fn() != 0, text
        assert text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
        assert "vam_tile_schedule" in lib.vam_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    with pytest.raises(L.VamError, match="vam_tile_schedule failed .*overlap 40"):
        ops.tile_schedule(S, coords, out[:12 * 3 * 16].view(12, 3, 4, 4), 64, 64, 40)
    assert call() == 0                                                          # and the well-formed call goes through
    torch.cuda.synchronize()
    assert bool((out[:12 * 3 * 16] != FILL).all()) and bool((out[12 * 3 * 16:] == FILL).all())
