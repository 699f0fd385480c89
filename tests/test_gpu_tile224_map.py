"""The block map of the wave-specialised 128x224 convolution tile (csrc/conv_igemm.hip, MAP22): its 4 x 7 blocks of 32x32
are dealt to the four consumer waves as 2x2 groups, and column block 3 of a row pair is shared by the pair's two waves.
The map must be invisible: the same bits as every other tile, every block at its own place in the output.

Shapes are the smallest that reach every part of the map (3x3 stride 1, N = 224 unless stated):
  full     Cin 512, one image of 16x16: P = 256 is two full M tiles, 144 K chunks
  ragged   three images of 10x10: P = 300, the last M tile has rows of both wave pairs outside the problem
  n200     N = 200 (Npad 224): column block 6 partly dead, block 3 live
  planes   `full` with a bf16x3-plane input (View3): the AIN = 1 instantiation
  cin496   `full` with Cin = 496: a half-empty last chunk
Everything is compared bit for bit, so no tolerance is involved anywhere except in the float64 anchor of the window
test, which uses the contract's own worst-case bound (K + 4) 2^-24 sum |x| |w|."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import ops, _lib as L  # noqa: E402

SENTINEL = -12345.678
GUARD = 4                                    # guard channels on either side of the output window
OTHER_TILES = ((64, 64, 0), (128, 128, 0))
CASES = {  # name: (Cin, N, images, H, W, plane input)
    "full": (512, 224, 1, 16, 16, False),
    "ragged": (512, 224, 3, 10, 10, False),
    "n200": (512, 200, 1, 16, 16, False),
    "planes": (512, 224, 1, 16, 16, True),
    "cin496": (496, 224, 1, 16, 16, False),
}


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32)


class _Problem:
    """One 3x3 problem with a bias and a ``pre`` operand that differ in every element, writing a channel window of a
    wider sentinel-filled buffer."""

    def __init__(self, name, seed=0):
        cin, n, b, h, w, planes = CASES[name]
        self.cin, self.n, self.shape = cin, n, (b, h, w)
        self.weight = _rand((n, cin, 3, 3), 100 + seed) / (3.0 * cin ** 0.5)
        self.bias = _rand((n,), 200 + seed)
        self.packed = ops.pack_conv(self.weight.cuda(), self.bias.cuda())
        if planes:
            # any bf16 triple is a valid plane input; every tile consumes the planes alike
            self.x = ops.new_view3(b, h, w, cin)
            g = torch.Generator().manual_seed(300 + seed)
            bits = torch.randint(0x3C00, 0x4000, (self.x.buf.numel() * 2,), generator=g, dtype=torch.int16)
            self.x.buf.view(torch.int16).copy_(bits.view(self.x.buf.view(torch.int16).shape))
        else:
            self.x = ops.new_view(b, h, w, cin)
            self.x.buf.copy_(_rand((b, h, w, cin), 300 + seed))
        self.pre = ops.new_view(b, h, w, n)
        self.pre.buf.copy_(_rand((b, h, w, n), 400 + seed))

    def problem(self):
        b, h, w = self.shape
        obuf = torch.full((b, h, w, GUARD + self.n + GUARD), SENTINEL, dtype=torch.float32, device="cuda")
        out = ops.View(obuf, GUARD, self.n)
        return ops.conv_problem(self.packed, [self.x], out, L.ACT_NONE, pre=self.pre), obuf


def _last_tile():
    bm, bn, bk = C.c_int(), C.c_int(), C.c_int()
    L.load().vam_conv_last_tile(C.byref(bm), C.byref(bn), C.byref(bk))
    return bm.value, bn.value


def _run(problems, tile):
    """Launch the problems as one group with the tile forced; returns the output buffers."""
    lib = L.load()
    built = [p.problem() for p in problems]
    lib.vam_conv_force_tile(*tile)
    try:
        ops.conv_group([c for c, _ in built])
        torch.cuda.synchronize()
        assert _last_tile() == tile[:2], f"asked for tile {tile[:2]}, the launch took {_last_tile()}"
    finally:
        lib.vam_conv_force_tile(0, 0, 0)
    return [obuf for _, obuf in built]


@functools.lru_cache(maxsize=None)
def _single(name, seed):
    """(problem, its output buffer from a single launch on the 128x224 tile), shared by the tests."""
    p = _Problem(name, seed)
    return p, _run([p], (128, 224, 0))[0]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_other_tiles(name):
    p, o224 = _single(name, 0)
    for tile in OTHER_TILES:
        o = _run([p], tile)[0]
        diff = int((o.view(torch.int32) != o224.view(torch.int32)).sum())
        assert diff == 0, f"{name}: 128x224 differs from {tile[0]}x{tile[1]} in {diff} elements"


@pytest.mark.parametrize("name", list(CASES))
def test_window_and_guards(name):
    """Every element of the window is written, the guard channels keep the sentinel's bits."""
    p, o = _single(name, 0)
    sent = torch.full((1,), SENTINEL, dtype=torch.float32, device="cuda")
    assert _same_bits(o[..., :GUARD], sent.expand_as(o[..., :GUARD]).contiguous())
    assert _same_bits(o[..., GUARD + p.n:], sent.expand_as(o[..., GUARD + p.n:]).contiguous())
    assert not bool((o[..., GUARD:GUARD + p.n] == SENTINEL).any()), f"{name}: part of the window was not written"


def test_every_block_lands_at_its_own_place():
    """`full` against float64 with the contract's worst-case bound for an fp32 accumulation of exact products,
    (K + 4) 2^-24 sum |x| |w|.  Bias and ``pre`` are of order one and differ in every element, the bound is of order
    1e-5: a block stored at another block's coordinates, or given another block's operands, cannot pass."""
    p, o = _single("full", 0)
    x64 = p.x.buf.cpu().double().permute(0, 3, 1, 2)
    w64 = p.weight.double()
    z = torch.nn.functional.conv2d(x64, w64, p.bias.double(), padding=1) + p.pre.buf.cpu().double().permute(0, 3, 1, 2)
    mag = torch.nn.functional.conv2d(x64.abs(), w64.abs(), padding=1)
    bound = (9 * p.cin + 4) * 2.0 ** -24 * (mag + p.bias.double().abs()[None, :, None, None] + p.pre.buf.cpu().double().permute(0, 3, 1, 2).abs())
    got = o[..., GUARD:GUARD + p.n].cpu().double().permute(0, 3, 1, 2)
    worst = float(((got - z).abs() / bound).max())
    print(f"128x224 tile against float64: largest error / bound {worst:.3g}")
    assert worst <= 1.0


def test_group_of_eight_equals_single_launches():
    """Eight problems (all the fp32-input cases, two seeds each) in one grouped launch on the 128x224 tile."""
    names = [n for n in CASES if not CASES[n][5]]
    singles = [_single(n, seed) for seed in (0, 1) for n in names]
    assert len(singles) == 8
    outs = _run([p for p, _ in singles], (128, 224, 0))
    for (p, o1), og in zip(singles, outs):
        diff = int((og.view(torch.int32) != o1.view(torch.int32)).sum())
        assert diff == 0, f"Cin {p.cin} N {p.n} {p.shape}: {diff} elements differ between the group and the single launch"
