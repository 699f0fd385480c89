"""vam_picture_resample on the GPU without a model (ops.picture_resample): a viewport of a picture read
from one pyramid level at any zoom and pan.  Every result is bit-equal, as uint32 / uint8, to the NumPy restatement of
tests/resample_ref.py; guards of 1024 elements around the output stay intact; the fp32 output starts 4 bytes off a 16-byte
boundary and the uint8 output at an odd byte; ``src`` exactly the support window and the whole level give the same bits;
malformed calls are errors through vam_last_error and write nothing.

The bound against the float64 evaluation with the exact rational weights.  A result is the sum of t_y t_x terms wy wx s.  An
fp32 weight is float(u) / float(S): two conversions and one division, each within a relative 2^-24 =: e of its exact
operands' result, so it is the exact u / S times (1 + d)^3 with |d| <= e.  A term is then multiplied by s (one rounding), summed
with the other column taps in t_x - 1 additions at the most (the first two terms meet t_x - 1 of them, later ones fewer),
multiplied by wy (three roundings in wy, one in the product) and summed in at most t_y - 1 additions: a term carries at most
m = (3 + 1 + t_x - 1) + (3 + 1 + t_y - 1) = t_y + t_x + 6 factors (1 + d).  The exact weights are positive and add up to 1, so
|result - exact| <= ((1 + e)^m - 1) max|s| <= m e / (1 - m e) max|s|.  That is the issue's (t_y + t_x + 6) 2^-24 max|s| with the
second-order term kept, which the first-order constant drops: the derived bound is larger by a factor of at most 1 + 5e-6
(m <= 70).  The float64 evaluation rounds as well: m 2^-53 max|s| is added for it.  No underflow occurs: the values are multiples
of 2^-24 of size 1 and a weight is at least 2^-46."""
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_ref as RR                             # noqa: E402
from vampic import _lib as L, ops, pyramid as PY      # noqa: E402

SOURCES = [(1, 1), (5, 7), (37, 53), (150, 200)]
OUTPUTS = [(1, 1), (3, 5), (64, 64), (97, 131)]
SCALES = {"1": (Fraction(1), Fraction(1)), "2": (Fraction(2), Fraction(2)), "1.37": (Fraction(137, 100),) * 2, "1/3.3": (Fraction(10, 33),) * 2,
          "16": (Fraction(16), Fraction(16)), "1.2 x 5": (Fraction(6, 5), Fraction(5)), "1 x 3": (Fraction(1), Fraction(3))}
GUARD = 1024
_SRC = {}


def _picture(Hk, Wk, k):
    """A picture whose level k is Hk x Wk, with sides that are no multiple of 2^k for k > 0."""
    return Hk * 2 ** k - k, Wk * 2 ** k - k


def _src(Hk, Wk, C):
    """The level's picture, values partly outside 0 .. 1 for the uint8 clamp: (NumPy, device)."""
    if (Hk, Wk, C) not in _SRC:
        a = (np.random.default_rng(Hk + 7 * C).random((C, Hk, Wk), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
        _SRC[(Hk, Wk, C)] = (a, torch.from_numpy(a).cuda())
    return _SRC[(Hk, Wk, C)]


def _viewports(Hk, Wk, k):
    """[(scale name, rect, unit, out_hw)] of the picture of this level: per unit, output and scale that fit, the rect at the
    picture's origin, at its far corner and at an odd origin inside; the whole picture into every output it may go to."""
    H, W = _picture(Hk, Wk, k)
    out = []
    for unit in (1, 3):
        for oh, ow in OUTPUTS:
            if max(RR.scales((0, 0, H * unit, W * unit), (oh, ow), k, unit)) <= 16:
                out.append(("whole", (0, 0, H * unit, W * unit), unit, (oh, ow)))
            for name, (sy, sx) in SCALES.items():
                h, w = max(1, round(sy * oh * unit * 2 ** k)), max(1, round(sx * ow * unit * 2 ** k))
                if h > H * unit or w > W * unit:
                    continue
                for y0, x0 in sorted({(0, 0), (H * unit - h, W * unit - w), (min(H * unit - h, 1), min(W * unit - w, 3)),
                                      ((H * unit - h) // 2 | 1 if H * unit - h > 1 else 0, (W * unit - w) // 2 | 1 if W * unit - w > 1 else 0)}):
                    out.append((name, (y0, x0, h, w), unit, (oh, ow)))
    return out


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _resample(src_dev, src_window, level_hw, k, rect, unit, out_hw, u8=False):
    """One ops.picture_resample into a guarded output that starts 4 bytes off a 16-byte boundary (uint8: at an odd byte);
    ``src`` lies 4 bytes off one as well."""
    C = src_dev.shape[0]
    numel = C * out_hw[0] * out_hw[1]
    fill = 0x5A if u8 else -3.0
    whole = torch.full((numel + 2 * GUARD + 1,), fill, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out = whole[GUARD + 1:GUARD + 1 + numel].view(tuple(out_hw) + (3,) if u8 else (C,) + tuple(out_hw))
    assert out.data_ptr() % (2 if u8 else 16) == (1 if u8 else 4)
    held = torch.empty(src_dev.numel() + 1, device="cuda")
    src = held[1:].view(src_dev.shape)
    src.copy_(src_dev)
    assert ops.picture_resample(src, src_window, level_hw, k, rect, unit, out_hw, out=out) is out
    torch.cuda.synchronize()
    assert bool((whole[:GUARD + 1] == fill).all()) and bool((whole[GUARD + 1 + numel:] == fill).all())
    return out.cpu().numpy()


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("Hk,Wk", SOURCES)
def test_viewports_against_the_restatement(Hk, Wk, k):
    H, W = _picture(Hk, Wk, k)
    assert RR.level_shape(H, W, k) == (Hk, Wk)
    cases = _viewports(Hk, Wk, k)
    seen = {"names": set(), "units": set(), "outs": set(), "loop": set(), "clamped": 0, "taps": set()}
    for n, (name, rect, unit, out_hw) in enumerate(cases):
        C = (1, 3, 5)[n % 3]
        a, dev = _src(Hk, Wk, C)
        win = PY.viewport_window(rect, out_hw, k, H, W, unit)
        assert win == RR.support_window(rect, out_hw, k, H, W, unit)
        want = RR.resample(a, (0, 0, Hk, Wk), (Hk, Wk), k, rect, unit, out_hw)
        crop = dev[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]].contiguous()
        got = _resample(dev, (0, 0, Hk, Wk), (Hk, Wk), k, rect, unit, out_hw)           # src: the whole level
        assert _same(got, want), (name, rect, unit, out_hw, C)
        assert _same(_resample(crop, win, (Hk, Wk), k, rect, unit, out_hw), want), (name, rect, unit, out_hw, C)     # exactly the support window
        if C == 3:
            assert _same(_resample(crop, win, (Hk, Wk), k, rect, unit, out_hw, u8=True), RR.to_u8(want)), (name, rect, unit, out_hw)
        exact, t_y, t_x = RR.resample_exact(a, (0, 0, Hk, Wk), (Hk, Wk), k, rect, unit, out_hw)
        m = t_y + t_x + 6
        bound = (m * 2.0 ** -24 / (1 - m * 2.0 ** -24) + m * 2.0 ** -53) * float(np.abs(a).max())
        assert float(np.abs(got.astype(np.float64) - exact).max()) <= bound, (name, rect, unit, out_hw, C)
        taps = [RR.axis_taps(rect[i], rect[2 + i], out_hw[i], k, unit) for i in (0, 1)]
        seen["names"].add(name); seen["units"].add(unit); seen["outs"].add(out_hw); seen["taps"].add((t_y, t_x))
        seen["loop"].add(max(RR.scales(rect, out_hw, k, unit)) > 2)
        seen["clamped"] += any(first < 0 or first + len(u) > N for i, N in ((0, Hk), (1, Wk)) for first, u in taps[i])
        if name == "1" and unit == 1 and (rect[0] % 2 ** k, rect[1] % 2 ** k) == (0, 0):  # an aligned scale 1: the source values
            assert _same(got, a[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]]) and (t_y, t_x) == (1, 1)
    assert seen["units"] == {1, 3} and seen["clamped"] >= 2 and "whole" in seen["names"]
    if (Hk, Wk) == (150, 200):                                                  # the large source meets every scale, output and path
        assert seen["names"] == set(SCALES) | {"whole"} and seen["outs"] == set(OUTPUTS) and seen["loop"] == {False, True}
        assert max(t for t, _ in seen["taps"]) == 32 and (1, 1) in seen["taps"]


def test_an_aligned_scale_of_one_returns_the_source_and_a_constant_stays_within_the_bound():
    a, dev = _src(150, 200, 3)
    for rect, unit, out_hw, k in [((12, 24, 192, 192), 3, (32, 32), 1), ((40, 60, 97, 131), 1, (97, 131), 0), ((8, 4, 388, 524), 1, (97, 131), 2)]:
        H, W = _picture(150, 200, k)
        win = PY.viewport_window(rect, out_hw, k, H, W, unit)
        assert win[2:] == out_hw
        assert _same(_resample(dev, (0, 0, 150, 200), (150, 200), k, rect, unit, out_hw), a[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    value = np.float32(1) / np.float32(3)
    const = torch.full((2, 37, 53), float(value), device="cuda")
    for rect, out_hw, k in [((0, 0, 37, 53), (64, 64), 0), ((3, 5, 30, 41), (3, 5), 0), ((0, 0, 72, 104), (3, 5), 1)]:
        H, W = _picture(37, 53, k)
        got = _resample(const, (0, 0, 37, 53), (37, 53), k, rect, 1, out_hw)
        m = sum(max(len(u) for _, u in RR.axis_taps(rect[i], rect[2 + i], out_hw[i], k, 1)) for i in (0, 1)) + 6
        assert float(np.abs(got.astype(np.float64) - float(value)).max()) <= m * 2.0 ** -24 / (1 - m * 2.0 ** -24) * float(value)
        assert _same(got, RR.resample(const.cpu().numpy(), (0, 0, 37, 53), (37, 53), k, rect, 1, out_hw))


def test_wide_outputs_across_the_blocks_and_the_scales_where_the_kernel_changes():
    """A block is 4 x 256 pixels.  Column scales from 1.9 to 2 go through the kernel that stages the source in LDS, scales below
    1.9 and magnifications through cached reads, scales above 2 through the loop: each at an output wider than one block and
    than two, at 1.9 exactly and just below, at 2 exactly and just above, with clamped taps at both ends."""
    Hk, Wk = 23, 1300
    a = (np.random.default_rng(3).random((3, Hk, Wk), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
    dev = torch.from_numpy(a).cuda()
    for ow, w in [(300, 600), (300, 570), (300, 569), (300, 601), (600, 1200), (600, 1300), (257, 514), (513, 1026), (520, 1000), (650, 1300), (300, 299)]:
        for oh, y0, h in [(5, 0, 10), (9, 2, 17), (11, 0, 23)]:
            rect, out_hw = (y0, (Wk - w) // 2, h, w), (oh, ow)
            path = "loop" if max(RR.scales(rect, out_hw, 0)) > 2 else "staged" if RR.scales(rect, out_hw, 0)[1] >= Fraction(19, 10) else "cached"
            assert path == {(300, 600): "staged", (300, 570): "staged", (300, 569): "cached", (300, 601): "loop", (600, 1200): "staged",
                            (600, 1300): "loop", (257, 514): "staged", (513, 1026): "staged", (520, 1000): "staged", (650, 1300): "staged",
                            (300, 299): "cached"}[(ow, w)] or (path == "loop" and h > 2 * oh)
            win = PY.viewport_window(rect, out_hw, 0, Hk, Wk)
            want = RR.resample(a, (0, 0, Hk, Wk), (Hk, Wk), 0, rect, 1, out_hw)
            crop = dev[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]].contiguous()
            assert _same(_resample(dev, (0, 0, Hk, Wk), (Hk, Wk), 0, rect, 1, out_hw), want), (rect, out_hw, path)
            assert _same(_resample(crop, win, (Hk, Wk), 0, rect, 1, out_hw), want), (rect, out_hw, path)
            assert _same(_resample(crop, win, (Hk, Wk), 0, rect, 1, out_hw, u8=True), RR.to_u8(want)), (rect, out_hw, path)


def test_capture_in_a_graph_and_one_replay():
    a, dev = _src(150, 200, 3)
    b = np.random.default_rng(9).random((3, 150, 200), dtype=np.float32)
    src = dev.clone()
    rect, unit, out_hw, k = (3 * 41 + 1, 3 * 33 + 2, 3 * 97, 3 * 131), 3, (64, 64), 0   # scales 1.52 and 2.05: the loop path
    out = torch.full((3, 64, 64), -3.0, device="cuda")
    small = torch.full((64, 64, 3), 7, dtype=torch.uint8, device="cuda")
    rect2 = (40, 60, 20, 20)                                                    # a magnification: the unrolled path

    def run():
        ops.picture_resample(src, (0, 0, 150, 200), (150, 200), k, rect, unit, out_hw, out=out)
        ops.picture_resample(src, (0, 0, 150, 200), (150, 200), k, rect2, 1, out_hw, out=small)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # the code object is loaded before the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), RR.resample(a, (0, 0, 150, 200), (150, 200), k, rect, unit, out_hw))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    src.copy_(torch.from_numpy(b))
    out.fill_(-3.0)
    small.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), RR.resample(b, (0, 0, 150, 200), (150, 200), k, rect, unit, out_hw))
    assert _same(small.cpu().numpy(), RR.to_u8(RR.resample(b, (0, 0, 150, 200), (150, 200), k, rect2, 1, out_hw)))


def test_the_binding_allocates_in_the_dtype_asked_for():
    a, dev = _src(37, 53, 3)
    want = RR.resample(a, (0, 0, 37, 53), (37, 53), 0, (1, 3, 30, 40), 1, (22, 29))
    got = ops.picture_resample(dev, (0, 0, 37, 53), (37, 53), 0, (1, 3, 30, 40), 1, (22, 29))
    assert got.dtype == torch.float32 and _same(got.cpu().numpy(), want)
    got = ops.picture_resample(dev, (0, 0, 37, 53), (37, 53), 0, (1, 3, 30, 40), 1, (22, 29), dtype=torch.uint8)
    assert got.dtype == torch.uint8 and _same(got.cpu().numpy(), RR.to_u8(want))
    with pytest.raises(ValueError, match="picture_resample: dtype is torch.float32 or torch.uint8"):
        ops.picture_resample(dev, (0, 0, 37, 53), (37, 53), 0, (1, 3, 30, 40), 1, (22, 29), dtype=torch.float16)
    with pytest.raises(L.VamError, match="vam_picture_resample failed .*a uint8 output is \\[oh, ow, 3\\]: it takes 3 planes, got 5"):
        ops.picture_resample(_src(37, 53, 5)[1], (0, 0, 37, 53), (37, 53), 0, (1, 3, 30, 40), 1, (22, 29), dtype=torch.uint8)
    with pytest.raises(L.VamError, match="vam_picture_resample failed .*does not cover the support window"):
        ops.picture_resample(dev[:, :30].contiguous(), (0, 0, 30, 53), (37, 53), 0, (1, 3, 30, 40), 1, (22, 29))


def test_malformed_calls_are_errors_and_write_nothing():
    lib = L.load()
    src = _src(150, 200, 3)[1]
    out = torch.full((3 * 75 * 100,), -7.0, device="cuda")
    s = ops.stream_ptr()
    ptr = lambda t: t.data_ptr() if t is not None else None

    def call(sr=src, C=3, win=(0, 0, 150, 200), Hk=150, Wk=200, shift=1, rect=(0, 0, 299, 399), unit=1, oh=75, ow=100, o=out, u8=0):
        return lib.vam_picture_resample(ptr(sr), C, *win, Hk, Wk, shift, *rect, unit, oh, ow, ptr(o), u8, s)

    cases = [(lambda: call(sr=None), "need src and out"), (lambda: call(o=None), "need src and out"),
             (lambda: call(C=0), "1 .. 32 planes, got 0"), (lambda: call(C=33), "1 .. 32 planes, got 33"),
             (lambda: call(u8=2), "out_u8 is 0"), (lambda: call(C=1, u8=1), "a uint8 output is [oh, ow, 3]: it takes 3 planes, got 1"),
             (lambda: call(unit=0), "unit is 1 .. 256, got 0"), (lambda: call(unit=257), "unit is 1 .. 256, got 257"),
             (lambda: call(oh=0), "an output of 0 x 100: sides are 1 .. 65536"), (lambda: call(ow=65537), "an output of 75 x 65537"),
             (lambda: call(oh=-3), "an output of -3 x 100"),
             (lambda: call(shift=-1), "shift is 0 .. 15 (the level), got -1"), (lambda: call(shift=16), "shift is 0 .. 15 (the level), got 16"),
             (lambda: call(Hk=0), "a level of 0 x 200 at shift 1 is ceil(. / 2^shift) of no picture"),
             (lambda: call(Wk=(1 << 23) + 2), "a level of 150 x 8388610 at shift 1 is ceil(. / 2^shift) of no picture with sides 1 .. 16777216"),
             (lambda: call(rect=(0, 0, 301, 399)), "the rect (y0 0, x0 0, h 301, w 399) / 1 does not lie inside the 300 x 400 picture of this 150 x 200 level at shift 1"),
             (lambda: call(rect=(-1, 0, 10, 10)), "does not lie inside"), (lambda: call(rect=(0, 0, 0, 10)), "does not lie inside"),
             (lambda: call(rect=(0, 395, 10, 10)), "does not lie inside"), (lambda: call(rect=(1 << 62, 0, 1 << 62, 10)), "does not lie inside"),
             (lambda: call(rect=(0, 0, 10, 1201), unit=3), "/ 3 does not lie inside"), (lambda: call(rect=(0, 0, -5, 10)), "does not lie inside"),
             (lambda: call(win=(0, 0, 151, 200)), "the window of src (y0 0, x0 0, h 151, w 200) does not lie inside the 150 x 200 level"),
             (lambda: call(win=(-1, 0, 150, 200)), "does not lie inside the 150 x 200 level"), (lambda: call(win=(0, 1, 150, 200)), "does not lie inside the 150 x 200 level"),
             (lambda: call(win=(0, 0, 0, 200)), "does not lie inside the 150 x 200 level"),
             (lambda: call(win=(0, 0, 149, 200)), "does not cover the support window (y0 0, x0 0, h 150, w 200)"),
             (lambda: call(win=(0, 1, 150, 199)), "does not cover the support window"),
             (lambda: call(rect=(41, 61, 60, 80), oh=30, ow=40, win=(20, 31, 30, 40)), "does not cover the support window (y0 20, x0 30, h 31, w 41)"),
             (lambda: call(rect=(41, 61, 60, 80), oh=30, ow=40, win=(20, 30, 30, 41)), "does not cover the support window"),
             (lambda: call(rect=(0, 0, 97, 399), oh=3, ow=100), "has a scale of 16.17 x 1.995: above 16; a pyramid of 3 levels has a level (shift 2)"),
             (lambda: call(shift=0, rect=(0, 0, 150, 200), oh=1, ow=1), "has a scale of 150 x 200: above 16; a pyramid of 5 levels has a level (shift 4)")]
    for fn, text in cases:
        assert fn() != 0, text
        assert "vam_picture_resample" in lib.vam_last_error().decode() and text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert PY.viewport_window((41, 61, 60, 80), (30, 40), 1, 299, 399) == (20, 30, 31, 41)
    assert call(rect=(41, 61, 60, 80), oh=30, ow=40, win=(20, 30, 31, 41)) == 0    # exactly the support window goes through
    assert call(rect=(0, 0, 96, 399), oh=3, ow=100) == 0                        # a scale of exactly 16
    torch.cuda.synchronize()
    assert not bool((out[:3 * 3 * 100] == -7.0).any()) and bool((out[3 * 30 * 40:] == -7.0).all())
    assert call() == 0                                                          # and the well-formed call
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())
