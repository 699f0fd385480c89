"""Rate control without a GPU: the bracket arithmetic of qualities_for_bpp on synthetic step curves, the
layer identity behind vam_gauss_layer_bits in the oracle's own numbers, and the loud refusal of the entry points on a CPU model."""
import argparse
import math
import sys

import numpy as np
import pytest
import torch

import vampic
import vampic.synth as synth
import vampic_oracle as O

M = sys.modules["vampic.models"]


# ----------------------------------------------------------------------------------------------- bracket arithmetic
def _step_curve(seed, base=0.1, first=0.3, n_jumps=40, flat_to=None):
    """A non-decreasing step curve on [0, 10]: ``base`` at 0, a jump of ``first`` right after 0 (the progressive slices'
    constant term), then n_jumps jumps at random places; flat stretches between them (and up to ``flat_to``)."""
    r = np.random.default_rng(seed)
    xs = np.sort(r.uniform(flat_to or 0.0, 10.0, n_jumps))
    js = r.uniform(0.0, 0.05, n_jumps)

    def f(q):
        q = np.asarray(q, dtype=np.float64)
        return base + first * (q > 0) + (js * (q[..., None] >= xs)).sum(-1)
    return f


def _curve_of(fs, calls):
    def curve(q, need):
        calls.append(int(need.sum()))
        out = np.full(q.shape, np.nan)             # what the search does not ask for, it must not read
        for b, f in enumerate(fs):
            out[:, b] = np.where(need[:, b], f(q[:, b]), np.nan)
        return out
    return curve


def test_rate_search_step_picks_largest_grid_point_within_budget():
    q = np.array([[0.0, 1.0, 2.0, 3.0, 4.0]] * 4)
    r = np.array([[1.0, 1.0, 2.0, 2.0, 5.0]] * 4)             # flat stretches and jumps
    t = np.array([0.5, 1.0, 2.5, 7.0])
    lo, r_lo, hi, r_hi, ok = M.rate_search_step(q, r, t)
    assert ok.tolist() == [False, True, True, True]
    assert lo.tolist() == [0.0, 1.0, 3.0, 4.0]                # the LARGEST point of a flat stretch within the budget
    assert hi.tolist() == [0.0, 2.0, 4.0, 4.0]                # above the end of the grid: hi == lo
    assert r_lo.tolist() == [1.0, 1.0, 2.0, 5.0] and r_hi.tolist() == [1.0, 2.0, 5.0, 5.0]


def test_rate_search_grid_is_even_and_ends_at_hi():
    g = M.rate_search_grid(np.array([0.0, 2.5]), np.array([10.0, 2.8125]))
    assert g.shape == (2, M.RATE_GRID) and g[0, -1] == 10.0 and g[1, -1] == 2.8125
    assert np.all(np.diff(g, axis=-1) > 0) and g[0, 0] == 10.0 / 32 and np.all(g[1] > 2.5)


@pytest.mark.parametrize("q_tol,n_grid", [(1e-3, 32), (1e-2, 32), (1e-4, 32), (0.5, 32), (1e-3, 2)])
def test_rate_search_contract_and_pass_count(q_tol, n_grid):
    fs = [_step_curve(1), _step_curve(2, flat_to=6.0), _step_curve(3, n_jumps=3)]
    bpp0 = np.array([float(f(0.0)) for f in fs])
    full = np.array([float(f(10.0)) for f in fs])
    fr = np.array([0.1, 0.5, 0.9])[:, None]
    t = np.concatenate([bpp0[None] - 0.01,                               # below the curve's start: unreached
                        bpp0[None],                                      # exactly the base
                        bpp0[None] + 0.1,                                # between the base and the first progressive rate
                        (bpp0 + 0.3)[None] + fr * (full - bpp0 - 0.3)[None],
                        full[None],                                      # exactly the full rate
                        full[None] + 1.0])                               # above the curve's end
    calls = []
    q, r, ok = M.rate_search(_curve_of(fs, calls), bpp0, t, q_tol, n_grid)
    passes = M.rate_search_passes(q_tol, n_grid)
    assert passes == max(0, math.ceil(round(math.log(10.0 / q_tol) / math.log(n_grid), 9)))
    assert len(calls) == passes                                          # one curve evaluation (= host sync) per pass
    assert calls[0] <= t.size * n_grid and all(c <= t.size * (n_grid - 1) for c in calls[1:])
    assert ok.tolist() == [[False] * 3] + [[True] * 3] * 7
    for ti in range(t.shape[0]):
        for b, f in enumerate(fs):
            if not ok[ti, b]:
                assert q[ti, b] == 0.0 and f(0.0) > t[ti, b]
                continue
            assert 0.0 <= q[ti, b] <= 10.0
            assert f(q[ti, b]) <= t[ti, b], (ti, b, q[ti, b])
            assert r[ti, b] == f(q[ti, b])
            assert q[ti, b] == 10.0 or f(min(10.0, q[ti, b] + q_tol)) > t[ti, b], (ti, b, q[ti, b])
    assert (q[1] == 0).all() and (q[2] == 0).all() and (q[-2] == 10).all() and (q[-1] == 10).all()


def test_rate_search_passes_is_ceil_log32():
    assert [M.rate_search_passes(t) for t in (10.0, 1.0, 10 / 32, 1e-2, 1e-3, 10 / 32 ** 3, 1e-4)] == [0, 1, 1, 2, 3, 3, 4]


# ----------------------------------------------------------------------------------------------- the layer identity
def test_layer_binned_sums_equal_the_oracles_masked_sums():
    """Σ_{layer<=k} log2 L_in + (#outside) log2 L(0,0) == the oracle's masked likelihood sum at q_k, for 32 qualities."""
    S, C, h, w = 3, 32, 4, 4                                             # three segments of 512 elements
    sg = synth.normal((S, C, h, w), 11).abs() * 0.6
    sg[0, :4] = 0.05                                                     # under the 0.11 bound, and a 64-fold tie
    sg[1, 5:9] = sg[1, 0:4]                                              # ties across the segment
    sg[2] = torch.round(sg[2] * 8) / 8                                   # a coarse grid: many ties, some exact zeros
    mu = synth.normal((S, C, h, w), 12) * 2
    r = mu + synth.normal((S, C, h, w), 13) * 3
    qs = sorted([0.0, 0.003, 0.05, 0.1, 0.25, 0.5, 0.5, 0.75, 1, 1.25, 1.5, 2, 2.5, 2.5, 3, 3.5, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5,
                 8, 8.5, 9, 9.5, 9.9, 9.999, 10, 10])
    assert len(qs) == 32
    masks = [O.variance_mask(sg, q).bool() for q in qs]
    layer = torch.full(sg.shape, 255, dtype=torch.int64)
    for k in reversed(range(len(qs))):
        layer[masks[k]] = k                                              # ends as the FIRST level whose mask holds the element
    l_in = torch.log2(O.gaussian_likelihood(r - mu, sg, None).double())
    zero = torch.zeros(1)
    l_out = float(torch.log2(O.gaussian_likelihood(zero, zero, None).double()))
    assert l_out < 0 and (l_in <= l_out + 1e-12).all()                   # in the mask an element never costs less: the rate grows with q
    n = C * h * w
    prev = None
    for k, q in enumerate(qs):
        assert torch.equal(layer <= k, masks[k]), (k, q)                 # nested masks: layer <= k  <=>  mask_k
        m = masks[k].float()
        want = O.log2_sum_per_image(O.gaussian_likelihood((r - mu) * m, sg * m, None))
        inside = layer <= k
        got = (l_in * inside).flatten(1).sum(1) + (n - inside.flatten(1).sum(1)).double() * l_out
        rel = ((got - want).abs() / want.abs()).max().item()
        assert rel < 1e-12, (k, q, rel)
        if prev is not None:
            assert (got <= prev + 1e-9).all()                            # log2 sums fall, the rate rises
        prev = got
    assert (layer[0] == 255).sum() == 0 and (layer == 255).sum() == 0    # q = 10 takes every element
    assert (layer == 0).sum() == 0                                       # q = 0 takes none


# ----------------------------------------------------------------------------------------------- entry points on the CPU
def test_rate_entry_points_need_a_gpu(monkeypatch):
    from conftest import README_ARGS
    net = vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu").eval()
    x = synth.synth_image(1, 64, 64, seed=0)
    L = vampic._lib
    if torch.cuda.is_available():                   # on a GPU box: what require_gpu answers without a device

        def no_device():
            raise L.VamError("no HIP device")
        monkeypatch.setattr(L, "require_gpu", no_device)
    with pytest.raises(L.VamError):
        net.rate_curve(x, [0, 1, 10])
    with pytest.raises(L.VamError):
        net.qualities_for_bpp(x, [0.5])
    from vampic import evaluate as EV, progressive as PR
    with pytest.raises(L.VamError):
        EV.rate_curve(net, x, [0, 1])
    with pytest.raises(L.VamError):
        PR.q_list_for_bpps(net, x, [0.5])
    with pytest.raises(ValueError):
        PR.q_list_for_bpps(net, torch.cat([x, x]), [0.5])
    with pytest.raises(ValueError):
        net.qualities_for_bpp(x, [0.5], mask_pol="two-levels")
