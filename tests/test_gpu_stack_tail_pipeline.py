"""csrc/stack_tail.hip, the pipeline of the fused stack tail: weight slabs and input chunks by LDS-DMA into a ring / a double
buffer, counted waits and raw barriers between the 18 steps, fragment reads one group ahead of the MFMAs.  Every comparison is
``torch.equal`` against what the launch replaces: the two ``conv_group`` launches with bf16x3 planes between them.  The shapes
are those at which a ring, a role split or a double buffer can go wrong: one tile with both halo rows outside the image (H = 4),
no interior tile (H = 8), an interior tile (H = 12, 16), one image and several, stack counts around the eight-problem launch
limit, outputs and epilogue operands as channel windows of wider buffers, and launches of different extents one after another."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                                     # noqa: E402
from vampic import layers as Ly, ops, _lib as L  # noqa: E402

SENTINEL = -77.0
W = 16


def _rand(shape, seed, scale=1.0):
    return vampic.synth.normal(shape, seed, scale)


def _fill(m, seed):
    m.load_state_dict(vampic.synth.synth_state_dict(m.state_dict(), seed))
    return m


@functools.lru_cache(maxsize=None)
def _stack(k):
    """Layers 3, 4, 5 of stack k: its own weights."""
    return (_fill(Ly.Conv2d(32, 128, 3, 1).cuda(), 150 + 3 * k), _fill(Ly.Conv2d(128, 64, 3, 1).cuda(), 151 + 3 * k),
            _fill(Ly.Conv2d(64, 32, 3, 1).cuda(), 152 + 3 * k))


def _epilogue(k):
    """Stack k's epilogue: plain, LRP with one operand, LRP with two, plain again, ... mixed within every group of K >= 2."""
    return (L.ACT_NONE, False, False) if k % 3 == 0 else (L.ACT_HALF_TANH, True, k % 3 == 2)


def _wide(B, H, K):
    """An output / operand buffer 8 + 32 K + 8 channels wide, stack k's window at 8 + 32 k, pre-filled with the sentinel."""
    v = ops.new_view(B, H, W, 32 * K + 16)
    v.buf.fill_(SENTINEL)
    return v


def _outside_is_sentinel(v, K):
    return bool((v.buf[..., :8] == SENTINEL).all()) and bool((v.buf[..., 8 + 32 * K:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _case(B, H, K):
    """Inputs of K stacks on B images of H x 16 and the reference: the two conv_group launches, computed once."""
    assert ops.split_mode()
    post, post2 = _wide(B, H, K), _wide(B, H, K)
    post.buf.copy_(_rand((B, H, W, 32 * K + 16), 170 + H).cuda())
    post2.buf.copy_(_rand((B, H, W, 32 * K + 16), 171 + H).cuda())
    ref = _wide(B, H, K)
    xs, two = [], [[], []]
    keep = []
    for k in range(K):
        m3, m4, m5 = _stack(k)
        x = ops.from_nchw(_rand((B, 32, H, W), 160 + 7 * k + H).cuda())
        x3 = ops.new_view3(B, H, W, 128)
        ops.conv_group([ops.conv_problem(m3.packed(), [x], x3, L.ACT_GELU)])            # the stack's third layer writes planes
        mid = ops.new_view3(B, H, W, 64)
        act, p1, p2 = _epilogue(k)
        two[0].append(ops.conv_problem(m4.packed(), [x3], mid, L.ACT_GELU))
        two[1].append(ops.conv_problem(m5.packed(), [mid], ref.window(8 + 32 * k, 32), act, post=post.window(8 + 32 * k, 32) if p1 else None,
                                       post2=post2.window(8 + 32 * k, 32) if p2 else None))
        xs.append(x3)
        keep += [x, mid]
    ops.conv_group(two[0])
    ops.conv_group(two[1])
    torch.cuda.synchronize()
    assert torch.isfinite(ref.buf).all() and float(ref.buf[..., 8:8 + 32 * K].abs().max()) > 1e-3
    assert _outside_is_sentinel(ref, K)
    return dict(B=B, H=H, K=K, xs=xs, post=post, post2=post2, ref=ref, keep=keep)


def _fused(c, out, stacks=None):
    """The fused problems of case c (all stacks, or the listed ones) writing into the wide buffer `out`."""
    probs = []
    for k in (range(c["K"]) if stacks is None else stacks):
        _, m4, m5 = _stack(k)
        act, p1, p2 = _epilogue(k)
        o = out.window(8 + 32 * k, 32)
        kw = dict(act=act, post=c["post"].window(8 + 32 * k, 32) if p1 else None, post2=c["post2"].window(8 + 32 * k, 32) if p2 else None)
        assert ops.stack_tail_ok(c["xs"][k], m4, m5, o, kw)
        probs.append(ops.stack_tail_problem(c["xs"][k], m4.packed(), m5.packed(), o, act, kw["post"], kw["post2"]))
    return probs


def _launch(c, stacks=None):
    out = _wide(c["B"], c["H"], c["K"])
    ops.stack_tail_group(_fused(c, out, stacks))
    torch.cuda.synchronize()
    return out


def _needs_planes():
    if not ops.split_mode():
        pytest.skip("the fused tail reads bf16x3 planes")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [4, 8, 12, 16])
def test_tile_rows(H, B):
    """H = 4: one tile, both halo rows outside the image; 8: a top and a bottom tile, no interior one; 12, 16: interior tiles with
    both halos inside.  One image (the grid is H / 4 workgroups per stack) and three.  Plain and both LRP epilogues in the group."""
    _needs_planes()
    c = _case(B, H, 3)
    out = _launch(c)
    assert torch.equal(out.buf, c["ref"].buf)


@pytest.mark.parametrize("K", [1, 8, 9, 17])
def test_stack_counts_around_the_launch_limit(K):
    """One launch takes eight stacks: K = 8 fills it, 9 adds a launch of one, 17 is two full launches and one more.  Every stack
    has its own weights and input; the epilogues are mixed within each launch.  Outputs are 32-channel windows of a buffer 16
    channels wider, post / post2 windows of buffers with ld = 32 K + 16 > 32: what lies outside the windows keeps the sentinel."""
    _needs_planes()
    c = _case(2, 8, K)
    out = _launch(c)
    assert torch.equal(out.buf, c["ref"].buf)
    assert _outside_is_sentinel(out, K)
    assert c["post"].ld > 32 and c["post2"].ld > 32


def test_windows_written_one_by_one_leave_the_rest_alone():
    """Each stack launched alone into its window: every other channel of the wide buffer, the other stacks' windows included,
    keeps the sentinel bit for bit."""
    _needs_planes()
    c = _case(2, 8, 8)
    for k in (0, 4, 7):                                         # plain, LRP with one operand, LRP with two
        out = _launch(c, [k])
        lo, hi = 8 + 32 * k, 8 + 32 * k + 32
        assert torch.equal(out.buf[..., lo:hi], c["ref"].buf[..., lo:hi])
        assert bool((out.buf[..., :lo] == SENTINEL).all()) and bool((out.buf[..., hi:] == SENTINEL).all())


def test_no_state_leaks_between_launches():
    """Nothing survives a launch — LDS contents, the ring's phase, the per-device attribute: the same group twice into two
    buffers, two stacks after nine, and one-tile images (H = 4) after four-tile ones (H = 16) all give the reference's bits."""
    _needs_planes()
    big, small, tall, flat = _case(2, 8, 9), _case(2, 8, 9), _case(3, 16, 3), _case(3, 4, 3)
    a = _launch(big)
    b = _launch(big)
    assert torch.equal(a.buf, b.buf) and torch.equal(a.buf, big["ref"].buf)
    two = _launch(small, [0, 1])                                # K = 2 right after K = 9
    assert torch.equal(two.buf[..., 8:72], small["ref"].buf[..., 8:72])
    assert bool((two.buf[..., :8] == SENTINEL).all()) and bool((two.buf[..., 72:] == SENTINEL).all())
    t = _launch(tall)
    f = _launch(flat)                                           # H = 4 right after H = 16
    assert torch.equal(t.buf, tall["ref"].buf) and torch.equal(f.buf, flat["ref"].buf)
    # and back to back on the stream, nothing waiting in between
    outs = [_wide(2, 8, 9), _wide(3, 4, 3), _wide(2, 8, 9)]
    ops.stack_tail_group(_fused(big, outs[0]))
    ops.stack_tail_group(_fused(flat, outs[1]))
    ops.stack_tail_group(_fused(big, outs[2], [0, 1]))
    torch.cuda.synchronize()
    assert torch.equal(outs[0].buf, big["ref"].buf) and torch.equal(outs[1].buf, flat["ref"].buf)
    assert torch.equal(outs[2].buf[..., 8:72], big["ref"].buf[..., 8:72])


def test_refusals_are_unchanged():
    """Rows that are no multiple of four, another width, a channel window of a wider plane tensor and a `pre` operand are
    refused — by ops.stack_tail_ok, and by the library where the problem can be written down — and the output keeps the sentinel."""
    _needs_planes()
    B = 2
    _, m4, m5 = _stack(0)
    out = _wide(B, 8, 1)
    o = out.window(8, 32)

    def refused(x3):
        p = ops.stack_tail_problem(x3, m4.packed(), m5.packed(), ops.View(torch.full((x3.B, x3.H, x3.W, 48), SENTINEL, device="cuda"), 8, 32))
        with pytest.raises(L.VamError):
            ops.stack_tail_group([p])
        torch.cuda.synchronize()
        assert bool((p._keep[3].buf == SENTINEL).all())

    x6 = ops.new_view3(B, 6, W, 128)                            # H = 6
    assert not ops.stack_tail_ok(x6, m4, m5, None, {})
    refused(x6)
    x32 = ops.new_view3(B, 8, 32, 128)                          # W = 32
    assert not ops.stack_tail_ok(x32, m4, m5, None, {})
    refused(x32)
    xw = ops.new_view3(B, 8, W, 256).window(128, 128)           # a window of a wider plane tensor
    assert not ops.stack_tail_ok(xw, m4, m5, o, {})
    refused(xw)
    good = _case(B, 8, 1)["xs"][0]
    assert ops.stack_tail_ok(good, m4, m5, o, {})
    assert not ops.stack_tail_ok(good, m4, m5, o, {"pre": _case(B, 8, 1)["post"].window(8, 32)})     # a `pre` operand: no launch exists
    assert bool((out.buf == SENTINEL).all())
