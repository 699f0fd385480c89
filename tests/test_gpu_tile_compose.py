"""vam_tile_compose on the GPU without a model: the blend where all tiles of a pixel are available, the
upsample of a coarser window elsewhere.  Every result is bit-exact against the NumPy restatement of tests/fill_ref.py (built
on tests/tiled_ref.py's blend); guards of 1024 elements around the output stay intact; all tiles available is
``ops.tile_blend``'s output, no tiles the pure upsample; malformed calls are errors through vam_last_error and write nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fill_ref as FR                                 # noqa: E402
import tiled_ref as TR                                # noqa: E402
from vampic import _lib as L, ops, pyramid as PY, tiled as TL        # noqa: E402

GRIDS = [(150, 200, 64, 16), (150, 200, 64, 0), (150, 200, 64, 32), (1, 1, 64, 16), (70, 64, 64, 16)]
GUARD = 1024
_TILES, _BELOW = {}, {}


def _tiles(g):
    key = (g["H"], g["W"], g["th"], g["tw"], g["V"])
    if key not in _TILES:
        n = g["R"] * g["C"]
        t = (np.random.default_rng(n + g["H"]).random((n, 3, g["th"], g["tw"]), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
        _TILES[key] = (t, torch.from_numpy(t).cuda())
    return _TILES[key]


def _below(H, W, d):
    """The whole picture of the level d below, values that no tile holds (some outside 0 .. 1 for the uint8 clamp)."""
    if (H, W, d) not in _BELOW:
        Hj, Wj = -(-H // 2 ** d), -(-W // 2 ** d)
        _BELOW[(H, W, d)] = (np.random.default_rng(100 * d + H).random((3, Hj, Wj), dtype=np.float32) * 1.25 - 0.125).astype(np.float32)
    return _BELOW[(H, W, d)]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _compose(g, slot, window, below, below_window, d, u8=False, n=None):
    """(out, status) of one ops.tile_compose into a guarded buffer; a uint8 output starts at an odd byte, ``below`` 4 bytes
    off a 16-byte boundary."""
    _, _, h, w = window
    numel = 3 * h * w
    fill = 0x5A if u8 else -3.0
    whole = torch.full((numel + 2 * GUARD + 1,), fill, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out = whole[GUARD + 1:GUARD + 1 + numel].view((h, w, 3) if u8 else (3, h, w))
    assert not u8 or out.data_ptr() % 2 == 1
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    held = torch.empty(below.size + 1, device="cuda")
    below_dev = held[1:].view(below.shape)
    below_dev.copy_(torch.from_numpy(below))
    if slot is None:
        ops.tile_compose(None, None, None, None, g["H"], g["W"], 0, window, below_dev, below_window, d, out, None)
    else:
        tiles_dev = _tiles(g)[1] if n is None else _tiles(g)[1][:n]
        w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(g["V"])) if g["V"] else (None, None)
        ops.tile_compose(tiles_dev, torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32)).cuda(), w_lo, w_hi, g["H"], g["W"], g["V"],
                         window, below_dev, below_window, d, out, status)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD + 1] == fill).all()) and bool((whole[GUARD + 1 + numel:] == fill).all())
    return out.cpu().numpy(), int(status.item())


def _windows(g):
    """The whole picture; odd first columns with widths 1, 3 and 5; the picture's last row and column; across a band."""
    H, W = g["H"], g["W"]
    wins = {(0, 0, H, W), (H // 2, min(5, W - 1), min(3, H - H // 2), 1), (min(1, H - 1), min(7, W - 1), max(1, H - 2), 3),
            (H - 1, max(0, W - 6) | 1 if W > 1 else 0, 1, 5), (max(0, H - 9), max(0, W - 13), min(9, H), min(13, W)),
            (min(40, H - 1), min(31, W - 1), max(1, min(70, H - 40)), max(1, min(101, W - 31)))}
    return sorted((y0, x0, h, min(w, W - x0)) for y0, x0, h, w in wins)


def _slots(g, rng):
    """Slot tables with -1 entries: a seeded half, one tile alone, all but one; the available slots are a permutation."""
    R, C = g["R"], g["C"]
    perm = rng.permutation(R * C).reshape(R, C)
    tables = [np.where(rng.random((R, C)) < 0.5, perm, -1)]
    if R * C > 1:
        one = rng.integers(0, R * C)
        tables += [np.where(np.arange(R * C).reshape(R, C) == one, perm, -1), np.where(np.arange(R * C).reshape(R, C) == one, -1, perm)]
    return tables


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
@pytest.mark.parametrize("d", [1, 2, 5])
@pytest.mark.parametrize("H,W,tile,V", GRIDS)
def test_random_slot_tables_against_the_restatement(H, W, tile, V, d, u8):
    g = TL.grid(H, W, tile, V)
    assert (g["R"], g["C"]) == {(150, 16): (3, 4), (150, 0): (3, 4), (150, 32): (4, 6), (1, 16): (1, 1), (70, 16): (2, 1)}[(H, V)]
    tiles = _tiles(g)[0]
    Hj, Wj = -(-H // 2 ** d), -(-W // 2 ** d)
    below = _below(H, W, d)
    rng = np.random.default_rng(7 * H + d)
    cast = (lambda a: TR.to_u8(a)) if u8 else (lambda a: a)
    for win in _windows(g):
        src = PY.source_window(win, d, Hj, Wj)
        assert src == FR.source_window(win, d, Hj, Wj)
        crop = np.ascontiguousarray(below[:, src[0]:src[0] + src[2], src[1]:src[1] + src[3]])
        for slot in _slots(g, rng):
            want = cast(FR.compose(tiles, slot, g, win, crop, src, d, Hj, Wj))
            got, status = _compose(g, slot, win, crop, src, d, u8)              # below: exactly the source window
            assert status == 0 and _same(got, want), (win, slot.tolist())
            got, status = _compose(g, slot, win, below, (0, 0, Hj, Wj), d, u8)  # and a larger window with another origin
            assert status == 0 and _same(got, want), (win, slot.tolist())


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
@pytest.mark.parametrize("H,W,tile,V", GRIDS)
def test_all_tiles_is_the_blend_and_no_tiles_is_the_upsample(H, W, tile, V, u8):
    g = TL.grid(H, W, tile, V)
    tiles, tiles_dev = _tiles(g)
    slot = np.arange(g["R"] * g["C"]).reshape(g["R"], g["C"])
    d, Hj, Wj = 1, -(-H // 2), -(-W // 2)
    below = _below(H, W, d)
    cast = (lambda a: TR.to_u8(a)) if u8 else (lambda a: a)
    for win in _windows(g):
        _, _, h, w = win
        blend = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") if u8 else torch.empty((3, h, w), device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(V)) if V else (None, None)
        ops.tile_blend(tiles_dev, torch.from_numpy(slot.astype(np.int32)).cuda(), w_lo, w_hi, H, W, V, win, blend, st)
        got, status = _compose(g, slot, win, below, (0, 0, Hj, Wj), d, u8)
        assert status == 0 and _same(got, blend.cpu().numpy()), win
        up = cast(FR.upsample(below, (0, 0, Hj, Wj), win, d, Hj, Wj))
        got, status = _compose(g, None, win, below, (0, 0, Hj, Wj), d, u8)      # slot = NULL, n = 0
        assert status == 0 and _same(got, up), win
        got, status = _compose(g, np.full_like(slot, -1), win, below, (0, 0, Hj, Wj), d, u8)
        assert status == 0 and _same(got, up), win


def test_a_constant_below_stays_constant_and_an_unavailable_tile_is_never_read():
    g = TL.grid(150, 200, 64, 16)
    for d in (1, 2, 5):
        Hj, Wj = -(-150 // 2 ** d), -(-200 // 2 ** d)
        value = np.float32(1) / np.float32(3)
        got, _ = _compose(g, None, (0, 0, 150, 200), np.full((3, Hj, Wj), value, dtype=np.float32), (0, 0, Hj, Wj), d)
        assert (got.view(np.uint32) == value.view(np.uint32)).all()
    slot = np.full((3, 4), -1)
    slot[1, 1] = 0                                                              # a buffer of ONE tile: any other read would leave it
    below = _below(150, 200, 1)
    got, status = _compose(g, slot, (0, 0, 150, 200), below, (0, 0, 75, 100), 1, n=1)
    assert status == 0 and _same(got, FR.compose(_tiles(g)[0][:1], slot, g, (0, 0, 150, 200), below, (0, 0, 75, 100), 1, 75, 100))
    assert _same(got[:, 64:96, 64:96], _tiles(g)[0][0][:, 16:48, 16:48])        # its core is the tile, bit for bit


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
def test_a_slot_beyond_the_buffer_sets_the_status(u8):
    g = TL.grid(150, 200, 64, 16)
    slot = np.arange(12).reshape(3, 4)
    below = _below(150, 200, 1)
    assert _compose(g, slot, (0, 0, 150, 200), below, (0, 0, 75, 100), 1, u8)[1] == 0
    slot[1, 2] = 12
    assert _compose(g, slot, (0, 0, 150, 200), below, (0, 0, 75, 100), 1, u8)[1] == 1
    assert _compose(g, slot, (0, 0, 40, 40), below, (0, 0, 75, 100), 1, u8)[1] == 0            # a window that does not meet it


def test_capture_in_a_graph_and_one_replay():
    g = TL.grid(150, 200, 64, 16)
    tiles, tiles_dev = _tiles(g)
    win, d, Hj, Wj = (40, 31, 70, 101), 1, 75, 100
    slot = np.where(np.eye(3, 4, dtype=bool) | np.eye(3, 4, 1, dtype=bool), np.arange(12).reshape(3, 4), -1)
    slot_dev = torch.from_numpy(slot.astype(np.int32)).cuda()
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(16))
    a, b = _below(150, 200, d), np.random.default_rng(9).random((3, Hj, Wj), dtype=np.float32)
    below = torch.from_numpy(a).cuda()
    out = torch.full((3, 70, 101), -3.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    run = lambda: ops.tile_compose(tiles_dev, slot_dev, w_lo, w_hi, 150, 200, 16, win, below, (0, 0, Hj, Wj), d, out, status)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # the code object is loaded before the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), FR.compose(tiles, slot, g, win, a, (0, 0, Hj, Wj), d, Hj, Wj))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    below.copy_(torch.from_numpy(b))
    out.fill_(-3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), FR.compose(tiles, slot, g, win, b, (0, 0, Hj, Wj), d, Hj, Wj)) and int(status.item()) == 0


def test_malformed_calls_are_errors_and_write_nothing():
    lib = L.load()
    g = TL.grid(150, 200, 64, 16)
    tiles = _tiles(g)[1]
    slot = torch.arange(12, dtype=torch.int32, device="cuda").view(3, 4)
    w_lo, w_hi = (torch.from_numpy(t).cuda() for t in TL.ramps(16))
    below = torch.from_numpy(_below(150, 200, 1)).cuda()
    out = torch.full((3 * 150 * 200,), -7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = ops.stream_ptr()
    ptr = lambda t: t.data_ptr() if t is not None else None

    def call(H=150, W=200, th=64, tw=64, V=16, win=(0, 0, 150, 200), bwin=(0, 0, 75, 100), Hj=75, Wj=100, d=1, n=12, u8=0, lo=w_lo, hi=w_hi,
             st=status, sl=slot, ti=tiles, be=below, o=out):
        return lib.vam_tile_compose(ptr(ti), n, ptr(sl), ptr(lo), ptr(hi), H, W, th, tw, V, *win, ptr(be), *bwin, Hj, Wj, d, ptr(o), u8, ptr(st), s)

    cases = [(lambda: call(be=None), "need below and out"), (lambda: call(o=None), "need below and out"),
             (lambda: call(d=0), "d is 1 .. 15"), (lambda: call(d=16), "d is 1 .. 15"), (lambda: call(d=-1), "d is 1 .. 15"),
             (lambda: call(Hj=76), "a level of 76 x 100 below a 150 x 200 picture at d = 1: it is ceil(H / 2^d) x ceil(W / 2^d) = 75 x 100"),
             (lambda: call(Wj=99), "a level of 75 x 99"), (lambda: call(d=2), "a level of 75 x 100 below a 150 x 200 picture at d = 2"),
             (lambda: call(bwin=(0, 0, 76, 100)), "the window of below (y0 0, x0 0, h 76, w 100) does not lie inside the 75 x 100 level"),
             (lambda: call(bwin=(-1, 0, 75, 100)), "does not lie inside the 75 x 100 level"),
             (lambda: call(bwin=(0, 1, 75, 100)), "does not lie inside the 75 x 100 level"),
             (lambda: call(bwin=(0, 0, 0, 100)), "does not lie inside the 75 x 100 level"),
             (lambda: call(bwin=(0, 0, 74, 100)), "does not cover the source window (y0 0, x0 0, h 75, w 100)"),
             (lambda: call(bwin=(0, 1, 75, 99)), "does not cover the source window"),
             (lambda: call(win=(10, 21, 20, 30), bwin=(5, 10, 10, 16)), "does not cover the source window (y0 4, x0 10, h 12, w 16)"),
             (lambda: call(win=(10, 21, 20, 30), bwin=(4, 10, 12, 15)), "does not cover the source window"),
             (lambda: call(V=33), "overlap 33"), (lambda: call(H=0), "a picture of 0 x 200"), (lambda: call(th=0), "tiles of 0 x 64"),
             (lambda: call(win=(0, 0, 151, 200)), "the window (y0 0, x0 0, h 151, w 200) does not lie inside the 150 x 200 picture"),
             (lambda: call(win=(-1, 0, 10, 10)), "does not lie inside"), (lambda: call(win=(0, 0, 0, 10)), "does not lie inside"),
             (lambda: call(win=(2147483647, 0, 1, 1)), "does not lie inside"),
             (lambda: call(H=1 << 20, W=64, win=(0, 0, 4 * 65535 + 1, 64), Hj=1 << 19, Wj=32), "a window of 262141 rows exceeds one launch"),
             (lambda: call(n=0), "a buffer of 0 tiles"), (lambda: call(sl=None), "need tiles, slot and status"), (lambda: call(ti=None), "need tiles"),
             (lambda: call(st=None), "need tiles"), (lambda: call(u8=2), "out_u8 is 0"), (lambda: call(lo=None), "needs the two ramp tables"),
             (lambda: call(sl=None, ti=None, n=0, H=0), "a picture of 0 x 200"), (lambda: call(sl=None, ti=None, n=0, be=None), "need below and out")]
    for fn, text in cases:
        assert fn() != 0, text
        assert "vam_tile_compose" in lib.vam_last_error().decode() and text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and int(status.item()) == 0
    with pytest.raises(L.VamError, match="vam_tile_compose failed .*does not cover the source window"):
        ops.tile_compose(tiles, slot, w_lo, w_hi, 150, 200, 16, (0, 0, 150, 200), below[:, :74].contiguous(), (0, 0, 74, 100), 1,
                         torch.empty((3, 150, 200), device="cuda"), status)
    assert call(win=(10, 21, 20, 30), bwin=(4, 10, 12, 16)) == 0                # exactly the source window goes through
    assert call(sl=None, ti=None, n=0, th=0, tw=0, V=-5, lo=None, hi=None, st=None) == 0       # no tiles: th, tw, V, status are not looked at
    assert call() == 0                                                          # and the well-formed call
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and not bool((out == -7.0).any())
