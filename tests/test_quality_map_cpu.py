"""Quality maps without a GPU: the validation that splits a map into sorted levels and an index map, the
host table of vam_variance_mask_map against vam_variance_layer_params called directly, the per-position rate identity in the
oracle's own numbers, the budget solver's contract on a synthetic curve with grids of 24 points, the pixel-map helpers, and
the argument validation of the model functions that precedes any GPU work."""
import ctypes as C

import numpy as np
import pytest
import torch

import vampic.synth as synth
import vampic_oracle as O
from vampic import _lib as L, control as CT, evaluate as EV, ops

FIELDS = ("k_lo", "k_hi", "w", "mode")


# ----------------------------------------------------------------------------------------------- quality_map_levels
def test_levels_and_index_of_a_hand_made_map():
    qmap = torch.zeros(2, 4, 8)
    qmap[0, :2, :4] = 2.5
    qmap[0, 2:, 4:] = 10.0
    qmap[0, 3, 0] = 12.0
    qmap[0, 0, 7] = 2.5                                                  # a repeat away from its block
    qmap[1] = 0.75                                                       # a constant image
    levels, index = CT.quality_map_levels((2, 3, 64, 128), qmap, "point-based-std")
    assert [lv.dtype for lv in levels] == [np.float64] * 2
    assert levels[0].tolist() == [0.0, 2.5, 10.0, 12.0] and levels[1].tolist() == [0.75]
    assert index.dtype == np.uint8 and index.shape == (2, 4, 8)
    want = np.zeros((4, 8), dtype=np.uint8)
    want[:2, :4] = 1
    want[2:, 4:] = 2
    want[3, 0] = 3
    want[0, 7] = 1
    assert np.array_equal(index[0], want) and not index[1].any()
    for b in range(2):                                                   # levels[index] is the map again
        assert np.array_equal(levels[b][index[b].astype(np.int64)], qmap[b].double().numpy())
    # the same through a list and an integer tensor
    lv2, ix2 = CT.quality_map_levels((2, 3, 64, 128), qmap.long().tolist(), "point-based-std")
    assert lv2[0].tolist() == [0.0, 2.0, 10.0, 12.0] and np.array_equal(ix2, index)


def test_two_levels_collapses_the_map_to_0_and_10():
    qmap = torch.tensor([[[0.0, 0.3, 5.0, 12.0]] * 4, [[1.0, 1.0, 2.0, 2.0]] * 4])
    levels, index = CT.quality_map_levels((2, 3, 64, 64), qmap, "two-levels")
    assert levels[0].tolist() == [0.0, 10.0] and levels[1].tolist() == [10.0]
    assert np.array_equal(index[0], np.array([[0, 1, 1, 1]] * 4, dtype=np.uint8)) and not index[1].any()


def test_map_refusals():
    ok = torch.ones(2, 4, 4)
    CT.quality_map_levels((2, 3, 64, 64), ok, "point-based-std")
    for bad in (torch.ones(2, 4, 5), torch.ones(1, 4, 4), torch.ones(2, 64, 64), torch.ones(2, 1, 4, 4), torch.ones(4, 4), 1.0):
        with pytest.raises(ValueError, match=r"\[2, 4, 4\]"):            # the message names the expected shape
            CT.quality_map_levels((2, 3, 64, 64), bad, "point-based-std")
    nan = ok.clone()
    nan[1, 2, 3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        CT.quality_map_levels((2, 3, 64, 64), nan, "point-based-std")
    neg = ok.clone()
    neg[0, 0, 0] = -0.5
    with pytest.raises(ValueError, match=">= 0"):
        CT.quality_map_levels((2, 3, 64, 64), neg, "point-based-std")
    many = torch.ones(1, 8, 8)
    many.view(-1)[:33] = torch.arange(33, dtype=torch.float32) * 0.25    # 33 distinct values
    with pytest.raises(ValueError, match=rf"33 distinct.*{L.VAM_MAX_LAYER_LEVELS}"):
        CT.quality_map_levels((1, 3, 128, 128), many, "point-based-std")
    many.view(-1)[32] = 0.0                                              # 32: accepted
    assert CT.quality_map_levels((1, 3, 128, 128), many, "point-based-std")[0][0].size == 32
    CT.quality_map_levels((1, 3, 128, 128), many * 1e-3 + (many > 0), "two-levels")     # and two-levels never has more than two


# ----------------------------------------------------------------------------------------------- ops.layer_table
def _records(raw: np.ndarray):
    n = raw.size // C.sizeof(L.VamLayerParams)
    return [L.VamLayerParams.from_buffer_copy(raw[i * C.sizeof(L.VamLayerParams):(i + 1) * C.sizeof(L.VamLayerParams)].tobytes())
            for i in range(n)]


def _layer_params(lists, n_pix, ch):
    """vam_variance_layer_params called directly."""
    width = max(len(r) for r in lists)
    flat = (C.c_double * (width * len(lists)))(*[v for r in lists for v in list(r) + [0.0] * (width - len(r))])
    nl = (C.c_int * len(lists))(*[len(r) for r in lists])
    raw = np.zeros(len(lists) * C.sizeof(L.VamLayerParams), dtype=np.uint8)
    L.check(L.load().vam_variance_layer_params(flat, nl, len(lists), width, n_pix, ch, raw.ctypes.data), "vam_variance_layer_params")
    return _records(raw)


@pytest.mark.parametrize("n_pix,ch", [(256, 32), (1536, 32)])
def test_layer_table_equals_layer_params(n_pix, ch):
    lists = [[0.0, 0.05, 0.5, 2.5, 9.99, 10.0, 12.0], [1.25], [i * 0.3 for i in range(L.VAM_MAX_LAYER_LEVELS)]]
    raw = ops.layer_table(lists, n_pix, ch)
    assert raw.dtype == np.uint8 and raw.size == 3 * C.sizeof(L.VamLayerParams)
    got, want = _records(raw), _layer_params(lists, n_pix, ch)
    for g, w_, r in zip(got, want, lists):
        assert g.n_levels == w_.n_levels == len(r) and g.any_select == w_.any_select
        for f in FIELDS:
            ga, gb = list(getattr(g, f)), list(getattr(w_, f))
            if f == "w":                                  # bit patterns, not values
                ga, gb = (np.array(v, dtype=np.float32).view(np.uint32).tolist() for v in (ga, gb))
            assert ga == gb, f
        assert [g.mode[k] for k in range(len(r))] == [2 if q >= 10 else 1 if q == 0 else 0 for q in r]
    with pytest.raises(L.VamError):
        ops.layer_table([[2.0, 1.0]], n_pix, ch)                         # not sorted
    with pytest.raises(L.VamError):
        ops.layer_table([[0.5] * (L.VAM_MAX_LAYER_LEVELS + 1)], n_pix, ch)
    with pytest.raises(L.VamError):
        ops.layer_table([[1.0], []], n_pix, ch)


# ----------------------------------------------------------------------------------------------- the rate identity
def test_per_position_layer_sums_equal_the_sum_under_the_composite_mask():
    """quality_map_rate's formula, from numpy layer ids and per-element likelihoods, against the direct sum of log2
    likelihoods under the composite mask (each position masked at its own quality): 1e-12 relative, the bound
    tests/test_rate_control_cpu.py uses for the same identity at a uniform quality."""
    S, C_, h, w = 3, 32, 4, 4                                            # three segments (slices of one image) of 512 elements
    sg = synth.normal((S, C_, h, w), 11).abs() * 0.6
    sg[0, :4] = 0.05                                                     # under the 0.11 bound, and a 64-fold tie
    sg[1, 5:9] = sg[1, 0:4]                                              # ties across the segment
    sg[2] = torch.round(sg[2] * 8) / 8                                   # a coarse grid: many ties, some exact zeros
    mu = synth.normal((S, C_, h, w), 12) * 2
    r = mu + synth.normal((S, C_, h, w), 13) * 3
    levels = [0.0, 1.75, 6.5]
    kmap = np.zeros((h, w), dtype=np.int64)                              # the level index of every position: three values
    kmap[:2, 2:] = 1
    kmap[2:, :] = 2
    kmap[0, 0] = 2
    masks = [O.variance_mask_np(sg.numpy(), q).astype(bool) for q in levels]           # [S, C, h, w] each
    layer = np.full(sg.shape, 255, dtype=np.int64)
    for k in reversed(range(len(levels))):
        layer[masks[k]] = k                                              # the first level whose mask holds the element
    l_in = torch.log2(O.gaussian_likelihood(r - mu, sg, None).double()).numpy()
    zero = torch.zeros(1)
    l_out = float(torch.log2(O.gaussian_likelihood(zero, zero, None).double()))
    # the bins of one vam_gauss_layer_bits at pix_per_item = 1: per position, by level (slot 3: no level)
    bits, count = np.zeros((h, w, 4)), np.zeros((h, w, 4), dtype=np.int64)
    for k in range(4):
        sel = layer == (k if k < 3 else 255)
        bits[..., k] = (l_in * sel).sum((0, 1))
        count[..., k] = sel.sum((0, 1))
    n_p = count.sum(-1)
    assert (n_p == S * C_).all()
    got = 0.0
    for y in range(h):
        for x_ in range(w):
            k = kmap[y, x_]
            got += bits[y, x_, :k + 1].sum() + (n_p[y, x_] - count[y, x_, :k + 1].sum()) * l_out
    # the composite mask: position p of every slice and channel masked as at its own quality
    comp = np.zeros(sg.shape, dtype=np.float32)
    for k in range(3):
        comp += masks[k] * (kmap == k)[None, None]
    assert 0 < comp.sum() < comp.size and not comp[:, :, kmap == 0].any()
    m = torch.from_numpy(comp)
    want = float(torch.log2(O.gaussian_likelihood((r - mu) * m, sg * m, None).double()).sum())
    rel = abs(got - want) / abs(want)
    print(f"rate identity: formula {got!r}, direct {want!r}, rel {rel:.3e}")
    assert rel <= 1e-12, rel


# ----------------------------------------------------------------------------------------------- the solver's contract
def test_rate_search_with_grids_of_24_meets_the_contract():
    assert CT.MAP_GRID == 24 and CT.MAP_FLOOR_LEVELS + CT.MAP_GRID <= L.VAM_MAX_LAYER_LEVELS
    rng = np.random.default_rng(5)
    xs, js = np.sort(rng.uniform(0.0, 10.0, (3, 60)), axis=1), rng.uniform(0.0, 0.05, (3, 60))
    floor = np.array([0.8, 0.45, 1.3])                                   # the floor map's rate: a map max(floor, q) never costs less

    def f(b, q):                                                         # a monotone step curve per image
        q = np.asarray(q, dtype=np.float64)
        return floor[b] + (js[b] * (q[..., None] >= xs[b])).sum(-1)
    calls = []

    def curve(q, need):
        calls.append(int(need.sum()))
        out = np.full(q.shape, np.nan)
        for b in range(3):
            out[:, b] = np.where(need[:, b], f(b, q[:, b]), np.nan)
        return out
    bpp0 = np.array([float(f(b, 0.0)) for b in range(3)])
    full = np.array([float(f(b, 10.0)) for b in range(3)])
    t = np.stack([bpp0 - 0.01, bpp0 + 0.25 * (full - bpp0), bpp0 + 0.5 * (full - bpp0), bpp0 + 0.9 * (full - bpp0), full + 1.0])
    q_tol = 1e-3
    q, r, ok = CT.rate_search(curve, bpp0, t, q_tol, n_grid=CT.MAP_GRID)
    assert len(calls) == CT.rate_search_passes(q_tol, 24) == 3
    assert calls[0] <= t.size * 24 and all(c <= t.size * 23 for c in calls[1:])
    assert ok.tolist() == [[False] * 3] + [[True] * 3] * 4
    for ti in range(t.shape[0]):
        for b in range(3):
            if not ok[ti, b]:
                assert q[ti, b] == 0.0 and f(b, 0.0) > t[ti, b]
                continue
            assert f(b, q[ti, b]) <= t[ti, b] and r[ti, b] == f(b, q[ti, b])
            assert q[ti, b] == 10.0 or f(b, min(10.0, q[ti, b] + q_tol)) > t[ti, b], (ti, b, q[ti, b])
    assert (q[-1] == 10).all() and ((q[1:4] > 0) & (q[1:4] < 10)).all()


# ----------------------------------------------------------------------------------------------- pixel-map helpers
def test_latent_quality_map_takes_the_block_maximum():
    pm = torch.zeros(2, 32, 48)
    pm[0, 15, 15] = 3.0                                                  # one pixel in the corner of block (0, 0)
    pm[0, 16:20, 30:34] = 7.0                                            # straddles blocks (1, 1) and (1, 2)
    pm[0, 17, 31] = 2.0                                                  # a lower value inside it: the maximum wins
    pm[1] = 1.5
    lm = EV.latent_quality_map(pm)
    assert lm.dtype == torch.float64 and tuple(lm.shape) == (2, 2, 3)
    assert lm[0].tolist() == [[3.0, 0.0, 0.0], [0.0, 7.0, 7.0]] and (lm[1] == 1.5).all()
    assert torch.equal(EV.latent_quality_map(pm.unsqueeze(1)), lm)
    for bad in (torch.zeros(2, 30, 48), torch.zeros(32, 48), torch.zeros(2, 3, 32, 48)):
        with pytest.raises(ValueError):
            EV.latent_quality_map(bad)


def test_quality_map_from_boxes_later_boxes_win():
    lm = EV.quality_map_from_boxes(2, 64, 64, 1.0, [(0, 0, 0, 32, 32, 8.0), (0, 16, 16, 48, 48, 4.0), (1, 60, 60, 64, 64, 10.0)])
    assert tuple(lm.shape) == (2, 4, 4)
    # image 0: the first box covers blocks [0:2, 0:2]; the second overwrites pixels 16..47, so block (0, 0) keeps 8 from its
    # untouched pixels, blocks (0, 1), (1, 0) too (their first-box pixels outside the second box), block (1, 1) is all 4
    assert lm[0].tolist() == [[8.0, 8.0, 1.0, 1.0], [8.0, 4.0, 4.0, 1.0], [1.0, 4.0, 4.0, 1.0], [1.0, 1.0, 1.0, 1.0]]
    want1 = torch.ones(4, 4, dtype=torch.float64)
    want1[3, 3] = 10.0
    assert torch.equal(lm[1], want1)
    assert (EV.quality_map_from_boxes(1, 64, 64, 0.0, []) == 0).all()
    with pytest.raises(ValueError):
        EV.quality_map_from_boxes(1, 64, 64, 0.0, [(1, 0, 0, 8, 8, 5.0)])
    with pytest.raises(ValueError):
        EV.quality_map_from_boxes(1, 64, 64, 0.0, [(0, 0, 0, 8, 72, 5.0)])


# ----------------------------------------------------------------------------------------------- the model functions
def test_model_functions_validate_before_any_gpu_work(synth_model_cpu):
    net, _ = synth_model_cpu                  # a CPU REM model: what passes validation is refused (REM) before any GPU work
    x = torch.zeros(2, 3, 64, 64)
    good = torch.ones(2, 4, 4)
    nan = good.clone()
    nan[0, 0, 0] = float("nan")
    many = torch.arange(64, dtype=torch.float32).reshape(1, 8, 8).repeat(2, 1, 1)
    fns = [lambda m_: net.forward_quality_map(x, m_), lambda m_: net.compress_quality_map(x, m_),
           lambda m_: net.quality_map_rate(x, m_), lambda m_: net.quality_map_for_bpp(x, m_, 1.0)]
    for fn in fns:
        with pytest.raises(ValueError, match=r"\[2, 4, 4\]"):
            fn(torch.ones(2, 4, 5))
        with pytest.raises(ValueError, match=r"\[2, 4, 4\]"):
            fn(torch.ones(2, 64, 64))
        with pytest.raises(ValueError, match="NaN"):
            fn(nan)
        with pytest.raises(ValueError, match=">= 0"):
            fn(-good)
        with pytest.raises(NotImplementedError, match="REM"):
            fn(good)
    x2 = torch.zeros(2, 3, 128, 128)
    for fn in (net.forward_quality_map, net.compress_quality_map, net.quality_map_rate):
        with pytest.raises(ValueError, match="64 distinct"):
            fn(x2, many)
    nine = torch.arange(64, dtype=torch.float32).reshape(1, 8, 8).repeat(2, 1, 1) % 9
    with pytest.raises(ValueError, match=r"9 distinct.*8"):             # a floor map: at most 8 values per image
        net.quality_map_for_bpp(x2, nine, 1.0)
    with pytest.raises(ValueError, match="point-based-std"):
        net.quality_map_for_bpp(x, good, 1.0, mask_pol="two-levels")
    with pytest.raises(ValueError, match="q_tol"):
        net.quality_map_for_bpp(x, good, 1.0, q_tol=0.0)
    with pytest.raises(ValueError):
        net.forward_quality_map(torch.zeros(2, 3, 60, 64), good)
    # decompress_quality_map: items and their maps
    item = {"strings": [[], []], "shape": (1, 1), "quality_map": {"levels": [1.0], "index": np.zeros((4, 4), dtype=np.uint8)}}
    with pytest.raises(ValueError, match="no items"):
        net.decompress_quality_map([])
    with pytest.raises(ValueError, match="same shape"):
        net.decompress_quality_map([item, dict(item, shape=(1, 2))])
    for qm in ({"levels": [1.0], "index": np.zeros((4, 5), dtype=np.uint8)},            # not the latent grid
               {"levels": [1.0], "index": np.zeros((4, 4), dtype=np.int64)},            # not uint8
               {"levels": [1.0], "index": np.ones((4, 4), dtype=np.uint8)},             # an index beyond the list
               {"levels": [2.0, 1.0], "index": np.zeros((4, 4), dtype=np.uint8)},       # not sorted
               {"levels": [-1.0], "index": np.zeros((4, 4), dtype=np.uint8)},
               {"levels": [], "index": np.zeros((4, 4), dtype=np.uint8)}):
        with pytest.raises(ValueError, match="item 0"):
            net.decompress_quality_map([dict(item, quality_map=qm)])
    with pytest.raises(ValueError, match="quality_map"):
        net.decompress_quality_map([{"strings": [[], []], "shape": (1, 1), "quality": 1.0}])
    with pytest.raises(NotImplementedError, match="REM"):
        net.decompress_quality_map([item])
