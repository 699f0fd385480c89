"""Coded-size control without a GPU: the stream-length bound of the range coder against the host
pricing (every stream's length is one of the at most two values predicted), the layer identity behind
vam_coded_layer_bits on synthetic symbols, and the level-by-level arithmetic of q_list_for_bytes on synthetic curves."""
import sys

import numpy as np
import pytest
import torch

import rans_oracle as R
import vampic
from vampic import bitstream as bs
from vampic import progressive as P

M = sys.modules["vampic.models"]


def _tables(widths=(1, 2, 3, 5, 8, 12, 20, 40)):
    """Discretised Gaussians of growing width plus a tail entry, quantised by the library: table i covers -w..w."""
    cdfs, sizes, offs = [], [], []
    for w in widths:
        k = np.arange(-w, w + 1)
        pmf = np.exp(-0.5 * (k / (0.3 * w + 0.2)) ** 2).astype(np.float32)
        pmf /= pmf.sum()
        prob = torch.from_numpy(np.concatenate([pmf, [np.float32(1e-4)]]).astype(np.float32))
        c = bs.pmf_to_quantized_cdf(prob, 16).numpy()
        cdfs.append(c)
        sizes.append(len(c))
        offs.append(-w)
    tab = np.zeros((len(cdfs), max(sizes)), dtype=np.int32)
    for i, c in enumerate(cdfs):
        tab[i, :len(c)] = c
    return bs.Tables(tab, np.array(sizes, dtype=np.int32), np.array(offs, dtype=np.int32))


def _streams(t, n_streams=220, seed=0):
    """(symbols, indexes[, layer, sel]) jobs: lengths 1..50 000, mixed tables, all-zero streams, layer selectors, and
    bypass-heavy streams (at least a tenth of the symbols outside their table, raw values up to all 8 nibbles)."""
    rng = np.random.default_rng(seed)
    nt = t.cdf.shape[0]
    jobs, kinds = [], []
    for s in range(n_streams):
        kind = ("plain", "zeros", "layer", "bypass", "single-table")[s % 5]
        n = int(rng.integers(1, 50001)) if s % 11 == 0 else int(rng.integers(1, 4000))
        if s < 3:
            n = (1, 2, 50000)[s]
        idx = rng.integers(0, nt, n).astype(np.int32)
        sym = np.round(rng.normal(0, 1, n) * (0.4 + idx)).astype(np.int32)
        if kind == "zeros":
            sym[:] = 0
            if s % 2:
                idx[:] = 0
        elif kind == "single-table":
            idx[:] = int(rng.integers(0, nt))
        elif kind == "bypass":
            out = rng.random(n) < 0.25
            mag = (2.0 ** rng.uniform(0, 31, n)).astype(np.int64)
            far = np.where(rng.random(n) < 0.5, mag, -mag)
            far[rng.random(n) < 0.1] = 2 ** 31 - 1                  # raw values that need all 8 nibbles, both signs
            far[rng.random(n) < 0.1] = -2 ** 31 + 1
            sym = np.where(out, far, sym).astype(np.int32)
        if kind == "layer":
            layer = rng.integers(0, 4, n).astype(np.uint8)
            layer[rng.random(n) < 0.2] = 0xFF
            jobs.append((sym, idx, layer, int(rng.integers(0, 4))))
        else:
            jobs.append((sym, idx))
        kinds.append(kind)
    return jobs, kinds


def test_every_stream_length_is_one_of_the_two_predicted():
    t = _tables()
    jobs, kinds = _streams(t)
    assert len(jobs) >= 200
    got = bs.encode_streams(jobs, t)
    cost = bs.cost_table(t)
    n_bypass_heavy = n_full = 0
    worst_lo, worst_hi = np.inf, -np.inf
    for j, kind, b in zip(jobs, kinds, got):
        pr = bs.price(j[0], j[1], t, *(j[2:] if len(j) > 2 else ()), cost=cost)
        S, n = float(pr.sum()), j[0].size
        lo, hi = bs.stream_bytes(S, n)
        assert hi - lo in (0, 4), (kind, n, S, lo, hi)              # at most two values, 4 bytes apart
        assert len(b) in (int(lo), int(hi)), (kind, n, S, len(b), lo, hi)
        # the derived bound of DESIGN section 9i: len - S / 8 in (4 + e / 8, 8 + e / 8], |e| <= n log2(e) (2^-15 + 9 * 2^-27)
        e = n * bs.LOG2E * (2.0 ** -15 + 9 * 2.0 ** -27)
        assert 4 - e / 8 - 1e-9 < len(b) - S / 8 <= 8 + e / 8 + 1e-9, (kind, n, S, len(b))
        worst_lo, worst_hi = min(worst_lo, len(b) - S / 8), max(worst_hi, len(b) - S / 8)
        if kind == "bypass":
            v = j[0].astype(np.int64) - t.offsets[j[1]]
            outside = (v < 0) | (v >= t.sizes[j[1]] - 2)
            n_bypass_heavy += outside.mean() >= 0.1
            raw = np.where(v < 0, -2 * v - 1, 2 * (v - (t.sizes[j[1]] - 2)))
            n_full += bool((raw[outside] >= 2 ** 28).any())
    assert n_bypass_heavy >= 40 and n_full >= 20, (n_bypass_heavy, n_full)
    print(f"len - S/8 over {len(jobs)} streams: [{worst_lo:.5f}, {worst_hi:.5f}]")


def test_short_streams_against_the_python_oracle():
    t = _tables()
    jobs, _ = _streams(t, n_streams=40, seed=5)
    short = [j for j in jobs if len(j) == 2 and j[0].size <= 1500][:10]
    assert len(short) >= 6
    for sym, idx in short:
        b = R.encode(sym.tolist(), idx.tolist(), t.cdf.tolist(), t.sizes.tolist(), t.offsets.tolist())
        lo, hi = bs.stream_bytes(bs.price(sym, idx, t).sum(), sym.size)
        assert len(b) in (int(lo), int(hi))


def test_price_counts_bypass_nibbles_and_the_selector():
    t = _tables(widths=(2,))
    c = bs.cost_table(t)
    mx = int(t.sizes[0]) - 2                                      # 5 entries -2..2, the escape is entry 5
    assert mx == 5 and np.all(c[0, :mx + 1] > 0) and np.all(c[0, mx + 1:] == 0)
    sym = np.array([0, 2, 3, 3 + 7, 3 + 8, -3, -3 - 7, -3 - 8, 2 ** 31 - 1], dtype=np.int32)
    # value = sym + 2; >= 5 escapes with raw = 2 (value - 5): 0 -> 0 nibbles, 14 -> 1, 16 -> 2; < 0 with raw = -2 value - 1
    nib = [None, None, 0, 1, 2, 1, 1, 2, 8]
    pr = bs.price(sym, np.zeros(sym.size, dtype=np.int32), t)
    for p_, s_, nb in zip(pr, sym, nib):
        want = c[0, s_ + 2] if nb is None else c[0, mx] + 4 * (1 + nb)
        assert p_ == want, (s_, p_, want)
    layer = np.array([0, 1, 1, 0, 255, 1, 0, 1, 1], dtype=np.uint8)
    pl = bs.price(sym, np.zeros(sym.size, dtype=np.int32), t, layer, 1)
    assert np.array_equal(pl, np.where(layer == 1, pr, c[0, 2]))


def test_cost_table_refuses_what_the_coder_refuses():
    t = _tables(widths=(2, 3))
    bad = bs.Tables(t.cdf.copy(), t.sizes.copy(), t.offsets)
    bad.sizes[0] = t.cdf.shape[1] + 1
    with pytest.raises(ValueError):
        bs.cost_table(bad)
    bad = bs.Tables(t.cdf.copy(), t.sizes, t.offsets)
    bad.cdf[1, 2] = bad.cdf[1, 1]
    with pytest.raises(ValueError):
        bs.cost_table(bad)


def test_layer_identity_of_both_cumulative_formulas():
    """compress at level k: sum_{j<=k} bits_j + (n - sum_{j<=k} count_j) * c_out;  container layer k: bits_k +
    (n - count_k) * c_out0 — against the masked arrays priced directly, 32 levels, 1e-12 relative."""
    t = _tables()
    rng = np.random.default_rng(3)
    n, nl = 20000, 32
    idx = rng.integers(0, t.cdf.shape[0], n).astype(np.int32)
    sym = np.round(rng.normal(0, 1.5, n) * (0.4 + idx)).astype(np.int32)
    sym[rng.random(n) < 0.02] = 5000                               # some bypass symbols
    layer = rng.integers(0, nl, n).astype(np.uint8)
    layer[rng.random(n) < 0.15] = 0xFF
    layer[layer == 7] = 8                                          # an empty layer
    pr = bs.price(sym, idx, t)
    bits = np.array([pr[layer == k].sum() for k in range(nl)])
    count = np.array([(layer == k).sum() for k in range(nl)])
    idx0 = 2                                                       # where compress puts an out-of-mask element
    zero = bs.price(np.zeros(t.cdf.shape[0], dtype=np.int32), np.arange(t.cdf.shape[0]), t)
    for k in range(nl):
        m = layer <= k                                             # compress at q_k: sym * mask, build_indexes(sigma * mask)
        direct = bs.price(np.where(m, sym, 0), np.where(m, idx, idx0), t).sum()
        ident = bits[:k + 1].sum() + (n - count[:k + 1].sum()) * zero[idx0]
        assert abs(ident - direct) <= 1e-12 * abs(direct), (k, ident, direct)
        direct = bs.price(sym, idx, t, layer, k).sum()             # container layer k: 0 in table 0 elsewhere
        ident = bits[k] + (n - count[k]) * zero[0]
        assert abs(ident - direct) <= 1e-12 * abs(direct), (k, ident, direct)
        b = bs.encode_streams([(sym, idx, layer, k)], t)[0]
        assert len(b) in [int(v) for v in bs.stream_bytes(ident, n)]


# ----------------------------------------------------------------------------------------------- level-by-level solver
def _layer_curve(seed, overhead=90.0, n_jumps=60):
    """A synthetic container: jumps of size at random qualities; a layer from q_prev to q weighs ``overhead`` (its stream
    headers and out-of-layer constant) plus the jumps in (q_prev, q]."""
    r = np.random.default_rng(seed)
    xs = np.sort(r.uniform(0.0, 10.0, n_jumps))
    js = np.floor(r.uniform(1.0, 400.0, n_jumps))
    calls = []

    def layer_hi(q_prev, qs):
        qs = np.asarray(qs, dtype=np.float64)
        calls.append(qs.size)
        assert np.all(qs >= q_prev) and np.all(np.diff(qs) >= 0) and qs.size <= 31
        return overhead + (js * ((qs[:, None] >= xs) & (q_prev < xs))).sum(-1)
    return layer_hi, xs, js, calls


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_q_list_for_bytes_level_by_level(seed):
    layer_hi, xs, js, calls = _layer_curve(seed)
    fixed, q_tol = 1000.0, 1e-3
    total = fixed + 4 * 90.0 + js.sum()
    targets = [500.0, fixed + 10.0, fixed + 0.2 * total, fixed + 0.2 * total + 50.0, 0.5 * total, 0.9 * total, 3 * total, 4 * total]
    qs, kept, sizes = P.solve_q_list_for_bytes(layer_hi, fixed, list(reversed(targets)), q_tol)
    # below the base, and base + less than one empty layer: dropped; the second target above everything: after q = 10
    assert 500.0 not in kept and fixed + 10.0 not in kept and kept == sorted(kept)
    assert qs == sorted(qs) and qs[-1] == 10.0 and 4 * total not in kept
    assert P.check_q_list(qs) == qs
    used, q_prev = fixed, 0.0
    for q, t_, s_ in zip(qs, kept, sizes):
        used += float(layer_hi(q_prev, [q])[0])
        assert used == s_ and used <= t_                           # the guarantee, with every earlier layer's overhead
        if q < 10.0:                                               # maximal: the layer up to q + q_tol does not fit
            assert used - float(layer_hi(q_prev, [q])[0]) + float(layer_hi(q_prev, [min(10.0, q + q_tol)])[0]) > t_
        q_prev = q
    # the level that only admits an empty layer repeats the previous quality
    assert qs[1] == qs[0] or kept[1] != targets[3]
    assert max(calls) <= 31


def test_q_list_for_bytes_passes_shrink_by_the_grid():
    layer_hi, _, js, calls = _layer_curve(7)
    P.solve_q_list_for_bytes(layer_hi, 0.0, [0.5 * js.sum()], q_tol=1e-3)
    # one call for the empty layer, then ceil(log31(10 / 1e-3)) = 3 grids
    assert calls == [1, 31, 31, 31]


def test_entry_points_refuse_a_cpu_model():
    import argparse
    args = argparse.Namespace(model="pic", N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True,
                              dim_chunk=32, division_dimension=[320, 640], mask_policy="point-based-std",
                              support_progressive_slices=5, delta_encode=True, total_mu_rep=True, all_scalable=True)
    net = vampic.get_model(args, "cpu").eval()
    x = torch.zeros(1, 3, 64, 64)
    for call in (lambda: net.coded_size_curve(x, [0, 1]), lambda: net.qualities_for_bytes(x, [1000.0]),
                 lambda: P.container_sizes(net, x, [1.0]), lambda: P.q_list_for_bytes(net, x, [1000.0])):
        with pytest.raises(Exception):
            call()
    with pytest.raises(ValueError):
        net.qualities_for_bytes(x, [1000.0], mask_pol="two-levels")
    with pytest.raises(ValueError):
        P.q_list_for_bytes(net, torch.zeros(2, 3, 64, 64), [1000.0])
