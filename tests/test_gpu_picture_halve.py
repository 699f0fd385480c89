"""vam_picture_halve on the GPU (ops.picture_halve): the next level of a resolution pyramid, bit for bit
the NumPy restatement (tests/pyramid_ref.py) viewed as uint32, in both modes, on either path of the kernel (16-byte loads;
single loads for clamped columns and rows off a 16-byte boundary); guards of 1024 elements around every output stay intact;
malformed calls are errors through vam_last_error and write nothing.  No model is needed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pyramid_ref as PR                                           # noqa: E402
from vampic import _lib as L, ops                                  # noqa: E402

GUARD = 1024
FILL = -7.0
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53), (64, 66), (129, 70), (150, 200)]
_VALUES = {}


def _values(C, Hs, Ws):
    """float32 [C, Hs, Ws], made once per shape: normal values of many magnitudes and, where there is room, +-0, denormals,
    +-inf, magnitudes near FLT_MAX (a block's sum overflows before the * 0.25) and a single NaN."""
    key = (C, Hs, Ws)
    if key not in _VALUES:
        rng = np.random.default_rng(1000 * Hs + 10 * Ws + C)
        x = (rng.standard_normal((C, Hs, Ws)) * 10.0 ** rng.integers(-3, 4, (C, Hs, Ws))).astype(np.float32)
        flat = x.reshape(-1)
        if flat.size >= 64:
            special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-40, np.inf, -np.inf, 3.4e38, 3.3e38, -3.4e38, 2.5e38, 1e38, 9e37],
                               dtype=np.float32)
            at = rng.choice(flat.size, size=min(flat.size // 4, 12 * special.size), replace=False)
            flat[at] = special[np.arange(at.size) % special.size]
            flat[int(rng.integers(0, flat.size))] = np.nan
        if Hs >= 8 and Ws >= 8:                                                 # blocks that hold what a random draw rarely puts together
            x[0, 0:2, 0:2] = [[0.0, -0.0], [-0.0, -0.0]]
            x[0, 2:4, 2:4] = [[-0.0, 0.0], [-0.0, -0.0]]
            x[0, 4:6, 4:6] = [[np.inf, -np.inf], [1.0, 2.0]]                   # inf - inf
            x[0, 6:8, 6:8] = [[3.4e38, 3.4e38], [-3.4e38, 3.4e38]]             # (inf) + (0): overflows, then stays inf
            x[0, 0:2, 6:8] = [[1e-45, 1e-45], [1e-45, 0.0]]                    # 3 denormal units * 0.25 = 0.75 of one: rounds up
        _VALUES[key] = x
    return _VALUES[key]


def _halve(x, mode, off=0):
    """ops.picture_halve of ``x`` (NumPy) into a guarded output; the source lies ``off`` floats past a 256-byte boundary."""
    C, Hs, Ws = x.shape
    shape = (C, (Hs + 1) // 2, (Ws + 1) // 2)
    numel = int(np.prod(shape))
    raw = torch.empty((x.size + 8,), dtype=torch.float32, device="cuda")
    src = raw[off:off + x.size].view(C, Hs, Ws)
    src.copy_(torch.from_numpy(x))
    assert src.data_ptr() % 16 == (4 * off) % 16
    whole = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
    out = whole[GUARD:GUARD + numel].view(shape)
    assert ops.picture_halve(src, mode, out=out) is out
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + numel:] == FILL).all())
    return out.cpu().numpy()


def _same(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("Hs,Ws", SIZES)
@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_a_level_is_the_restatement_bit_for_bit(mode, C, Hs, Ws):
    x = _values(C, Hs, Ws)
    want = PR.halve(x, mode)
    assert _same(_halve(x, mode), want)
    if C == 3:
        assert _same(_halve(x, mode, off=1), want)                              # a source 4 bytes off a 16-byte boundary
        assert _same(_halve(x, mode, off=2), want)


def test_the_special_values_are_there_and_come_out_as_the_arithmetic_gives_them():
    x = _values(3, 150, 200)
    assert np.isnan(x).sum() == 1 and np.isinf(x).sum() >= 4 and (np.abs(x[x != 0]) < 1.2e-38).sum() >= 4 and np.signbit(x[x == 0]).any()
    mean, big = PR.halve(x, "mean"), PR.halve(x, "max")
    assert mean.view(np.uint32)[0, 0, 0] == 0 and big.view(np.uint32)[0, 0, 0] == 0            # (+0 + -0) + (-0 + -0); the first of equals
    assert big.view(np.uint32)[0, 1, 1] == 0x80000000 and mean.view(np.uint32)[0, 1, 1] == 0
    assert mean.view(np.uint32)[0, 2, 2] == PR.QNAN and big[0, 2, 2] == np.inf
    assert np.isposinf(mean[0, 3, 3]) and big[0, 3, 3] == np.float32(3.4e38)
    assert mean.view(np.uint32)[0, 0, 3] == 1 and big.view(np.uint32)[0, 0, 3] == 1            # 0.75 units: to the nearest
    assert np.isnan(mean).sum() >= 2 and np.isposinf(mean).sum() >= 2
    for mode, want in (("mean", mean), ("max", big)):
        assert _same(_halve(x, mode), want)


def test_five_halvings_in_a_row():
    x = np.random.default_rng(7).random((3, 150, 200), dtype=np.float32)
    for mode in ("mean", "max"):
        dev, ref = torch.from_numpy(x).cuda(), x
        for shape in [(75, 100), (38, 50), (19, 25), (10, 13), (5, 7)]:
            dev, ref = ops.picture_halve(dev, mode), PR.halve(ref, mode)
            assert tuple(dev.shape) == (3,) + shape and _same(dev.cpu().numpy(), ref)


def test_rows_beyond_one_grid_dimension():
    """More than 4 * 32768 output rows: the row blocks are split over two grid dimensions."""
    Hs = 2 * 4 * 32768 + 2 * 4 * 5 + 3
    x = np.random.default_rng(11).standard_normal((2, Hs, 3)).astype(np.float32)
    for mode in ("mean", "max"):
        assert _same(_halve(x, mode), PR.halve(x, mode))


def test_capture_in_a_graph_and_one_replay():
    a, b = _values(3, 37, 53), np.random.default_rng(9).random((3, 37, 53), dtype=np.float32)
    src = torch.from_numpy(a).cuda()
    out = torch.full((3, 19, 27), FILL, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # the code object is loaded before the capture
        ops.picture_halve(src, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), PR.halve(a))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.picture_halve(src, out=out)
    src.copy_(torch.from_numpy(b))
    out.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), PR.halve(b))


def test_malformed_calls_are_errors_and_write_nothing():
    lib = L.load()
    src = torch.zeros((3, 16, 16), device="cuda")
    out = torch.full((3 * 8 * 8 + 2 * GUARD,), FILL, device="cuda")
    s = ops.stream_ptr()

    def call(C=3, Hs=16, Ws=16, mode=0, a=src.data_ptr(), o=out.data_ptr() + 4 * GUARD):
        return lib.vam_picture_halve(a, C, Hs, Ws, o, mode, s)

    most = L.VAM_MAX_LAYER_LEVELS
    cases = [(lambda: call(a=None), "need src and dst"), (lambda: call(o=None), "need src and dst"),
             (lambda: call(C=0), f"1 .. {most} planes, got 0"), (lambda: call(C=most + 1), f"1 .. {most} planes, got {most + 1}"),
             (lambda: call(C=-1), "planes, got -1"), (lambda: call(Hs=0), "a picture of 0 x 16"), (lambda: call(Ws=0), "a picture of 16 x 0"),
             (lambda: call(Hs=-4), "a picture of -4 x 16"), (lambda: call(Hs=(1 << 24) + 1), "a picture of 16777217 x 16: sides are 1 .. 16777216"),
             (lambda: call(Ws=(1 << 24) + 1), "a picture of 16 x 16777217"), (lambda: call(mode=2), "mode is 0 (mean) or 1 (max), got 2"),
             (lambda: call(mode=-1), "mode is 0"), (lambda: call(C=32, Hs=1 << 24, Ws=1 << 24), "exceed one launch")]
    for fn, text in cases:
        assert fn() == -1, text                                               # VAM_EINVAL
        assert "vam_picture_halve" in lib.vam_last_error().decode() and text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    with pytest.raises(ValueError, match="picture_halve: mode is one of"):
        ops.picture_halve(src, "median")
    assert call() == 0 and call(mode=1) == 0                                    # and the well-formed calls go through
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == FILL).all()) and bool((out[GUARD + 192:] == FILL).all()) and bool((out[GUARD:GUARD + 192] == 0).all())
