"""Scheduled embedded streams on the host: the numpy statements of the two device contracts that
tests/test_gpu_embedded_schedule.py holds the kernels to — the stage id (vam_stage_ids) and the scheduled rank order
(vam_variance_rank_staged) —, prefix = quality-map mask on random segments, the 64-bit key, embedded.check_schedule and
embedded.truncate on a hand-built "embedded-3" container."""
import numpy as np
import pytest
import torch

from vampic import embedded as EB

import test_embedded_cpu as EC                         # rank_order, rank_keys: the contracts of section 9m

NONE = 0xFF


# ------------------------------------------------------------------------------------------------ the device contracts
def level_mask(s, q: float) -> np.ndarray:
    """The variance mask of one segment at quality q, as layers/channel_mask.py builds it: nothing at 0, everything at
    >= 10, else sigma >= the (1 - q/10) quantile (all False in a segment that holds a NaN: no comparison with NaN holds)."""
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    if q <= 0:
        return np.zeros(s.size, dtype=bool)
    if q >= 10:
        return np.ones(s.size, dtype=bool)
    return s >= torch.quantile(torch.from_numpy(s), 1 - q / 10).item()


def layer_ids(s, levels) -> np.ndarray:
    """What vam_variance_layers_per_image writes for one segment and the sorted list ``levels``: the first level whose
    mask holds the element, 0xFF when none does."""
    out = np.full(np.asarray(s).size, NONE, dtype=np.uint8)
    for k in reversed(range(len(levels))):
        out[level_mask(s, float(levels[k]))] = k
    return out


def stage_ids(layer, index, n_pix: int) -> np.ndarray:
    """THE stage contract of vam_stage_ids for one segment flattened in canonical [C, h, w] order (element e lies at latent
    position p = e % n_pix): ``index`` uint8 [L, n_pix], stage(e) = min{k : index[k][p] >= layer[e]}, 0xFF when none."""
    layer = np.asarray(layer, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64).reshape(len(index), n_pix)
    p = np.arange(layer.size) % n_pix
    hit = index[:, p] >= layer[None, :]                                     # [L, n]
    return np.where(hit.any(0), hit.argmax(0), NONE).astype(np.uint8)


def scheduled_order(s, stage) -> np.ndarray:
    """THE ordering contract of vam_variance_rank_staged: ascending stage, within a stage the order of section 9m."""
    o = EC.rank_order(s)
    return o[np.argsort(np.asarray(stage)[o], kind="stable")]


def scheduled_keys(s, stage) -> np.ndarray:
    """The 64-bit keys the kernel sorts ascending: stage << 56 | ~ordered_bits(sigma) << 24 | e, e < 2^24."""
    k = EC.rank_keys(s)
    d, e = k >> np.uint64(32), k & np.uint64(0xFFFFFFFF)
    assert e.size <= 1 << 24
    return (np.asarray(stage, dtype=np.uint64) << np.uint64(56)) | (d << np.uint64(24)) | e


def random_schedule(rng, B, n_stages, h, w, values):
    """[n_stages, B, h, w] float64, non-decreasing along the stages, entries drawn from ``values``."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    idx = np.sort(rng.integers(0, v.size, (n_stages, B, h, w)), axis=0)
    return v[idx]


def _segment(rng, n, ties=True, nan=False):
    s = (rng.random(n) * 4 + 0.05).astype(np.float32)
    if ties:
        s = np.round(s * 2) / 2
    if nan:
        s[rng.integers(0, n)] = np.nan
    return s


def test_stage_contract_small_case():
    # two positions, two channels: e = c * 2 + p
    layer = np.array([0, 1, 2, NONE], dtype=np.uint8)
    index = np.array([[0, 0], [1, 0], [2, 2]], dtype=np.uint8)            # position 0 climbs 0, 1, 2; position 1: 0, 0, 2
    assert stage_ids(layer, index, 2).tolist() == [0, 2, 2, NONE]
    s = np.array([1.0, 3.0, 3.0, 2.0], dtype=np.float32)
    assert scheduled_order(s, [0, 2, 2, NONE]).tolist() == [0, 1, 2, 3]
    assert scheduled_order(s, [2, 0, NONE, 0]).tolist() == [1, 3, 0, 2]
    assert scheduled_order(s, [NONE] * 4).tolist() == EC.rank_order(s).tolist()      # no stage: the plain order


@pytest.mark.parametrize("nan", [False, True])
def test_prefix_of_the_scheduled_order_is_the_quality_map_mask(nan):
    """perm[:count_k] is the support of the mask of S[k] (per position its own quantile threshold), with q = 0 and q >= 10
    positions, two equal consecutive stages and heavy ties; a NaN segment keeps only its q >= 10 positions."""
    rng = np.random.default_rng(11 + nan)
    C, h, w = 8, 4, 6
    n_pix, n = h * w, 8 * 4 * 6
    S = random_schedule(rng, 1, 5, h, w, [0, 0, 0.5, 2.5, 7, 10, 12])[:, 0]          # [5, h, w]
    S[3] = S[2]                                                            # an empty increment
    levels, index = EB.check_schedule(S[:, None], 1, h, w)
    assert 0.0 in levels[0] and levels[0].max() >= 10 and index.shape == (1, 5, h, w)
    for trial in range(4):
        s = _segment(rng, n, ties=True, nan=nan)
        stage = stage_ids(layer_ids(s, levels[0]), index[0], n_pix)
        perm = scheduled_order(s, stage)
        assert sorted(perm.tolist()) == list(range(n))
        p = np.arange(n) % n_pix
        last = 0
        for k in range(5):
            qmap = S[k].reshape(-1)
            mask = np.zeros(n, dtype=bool)
            for q in np.unique(qmap):
                mask |= level_mask(s, float(q)) & (qmap[p] == q)
            count = int((stage <= k).sum())
            assert count == int(mask.sum()) and count >= last, (trial, k)
            assert set(perm[:count].tolist()) == set(np.nonzero(mask)[0].tolist()), (trial, k)
            if nan:
                assert np.array_equal(mask, qmap[p] >= 10)
            last = count
        assert int((stage <= 3).sum()) == int((stage <= 2).sum())


@pytest.mark.parametrize("n", [64, 3072, 8192])
def test_scheduled_keys_sort_to_the_contract(n):
    rng = np.random.default_rng(n)
    s = _segment(rng, n)
    s[rng.integers(0, n, 6)] = [np.nan, np.inf, -0.0, 0.0, -np.inf, -np.nan]
    stage = rng.choice(np.array([0, 1, 2, 31, NONE], dtype=np.uint8), n)
    keys = scheduled_keys(s, stage)
    assert np.unique(keys).size == n and keys.max() < np.uint64(0xFFFFFFFFFFFFFFFF)     # below the sentinel
    assert np.array_equal(np.argsort(keys), scheduled_order(s, stage))
    assert np.array_equal(keys & np.uint64(0xFFFFFF), np.arange(n, dtype=np.uint64))    # what the final write keeps
    # one stage everywhere: the plain order, whatever the stage
    assert np.array_equal(np.argsort(scheduled_keys(s, np.full(n, 7, dtype=np.uint8))), EC.rank_order(s))


# ------------------------------------------------------------------------------------------------ check_schedule
def test_check_schedule_accepts():
    rng = np.random.default_rng(0)
    S = random_schedule(rng, 2, 4, 3, 5, [0, 0.5, 1, 2.5, 10])
    for given in (S, list(S), [torch.from_numpy(m) for m in S], torch.from_numpy(S).float()):
        levels, index = EB.check_schedule(given, 2, 3, 5)
        assert len(levels) == 2 and index.shape == (2, 4, 3, 5) and index.dtype == np.uint8
        for b in range(2):
            assert levels[b].dtype == np.float64 and np.array_equal(levels[b], np.unique(S[:, b]))
            assert np.array_equal(levels[b][index[b]], S[:, b])
            assert (np.diff(index[b].astype(int), axis=0) >= 0).all()
    levels, index = EB.check_schedule([np.full((1, 2, 2), 3.0)] * 32, 1, 2, 2)         # 32 stages, one value
    assert levels[0].tolist() == [3.0] and index.shape == (1, 32, 2, 2) and not index.any()
    wide = np.arange(32, dtype=np.float64).reshape(1, 4, 8) / 4                         # 32 distinct values in one stage
    levels, index = EB.check_schedule([wide], 1, 4, 8)
    assert levels[0].size == 32 and np.array_equal(index[0, 0], np.arange(32).reshape(4, 8))


def test_check_schedule_refuses():
    ok = np.ones((2, 3, 5))
    with pytest.raises(ValueError, match=r"shape .*\[2, 3, 5\].*got \[2, 5, 3\]"):
        EB.check_schedule([ok, np.ones((2, 5, 3))], 2, 3, 5)
    with pytest.raises(ValueError, match="shape"):
        EB.check_schedule([np.ones((3, 5))], 2, 3, 5)
    bad = ok.copy()
    bad[1, 2, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        EB.check_schedule([ok, bad], 2, 3, 5)
    bad[1, 2, 4] = -0.5
    with pytest.raises(ValueError, match=">= 0"):
        EB.check_schedule([bad], 2, 3, 5)
    bad[1, 2, 4] = np.inf
    with pytest.raises(ValueError, match="finite"):
        EB.check_schedule([bad], 2, 3, 5)
    low = 2 * ok
    low[1, 0, 3] = 0.5
    with pytest.raises(ValueError, match=r"image 1, position \(0, 3\): stage 2 lowers"):
        EB.check_schedule([ok, 2 * ok, low], 2, 3, 5)
    with pytest.raises(ValueError, match="1..32 stages, got 33"):
        EB.check_schedule([ok] * 33, 2, 3, 5)
    with pytest.raises(ValueError, match="1..32 stages, got 0"):
        EB.check_schedule([], 2, 3, 5)
    many = np.arange(30, dtype=np.float64).reshape(1, 5, 6)                            # 30 + 3 distinct values over two stages
    with pytest.raises(ValueError, match="image 0 holds 33 distinct"):
        EB.check_schedule([many, np.maximum(many, 100 + (many % 3))], 1, 5, 6)
    with pytest.raises(ValueError, match="schedule"):
        EB.check_schedule(3.5, 2, 3, 5)


# ------------------------------------------------------------------------------------------------ truncate
def _container():
    index = np.zeros((3, 4, 8), dtype=np.uint8)
    index[1:, :2] = 1
    index[2] = 2
    return {"format": "embedded-3", "lanes": 1, "shape": (1, 2), "z": [b"z" * 10], "base": [[b"a" * 4], [b"b" * 6]],
            "embedded": [bytes(range(40)), bytes(range(100, 160))],
            "schedule": {"levels": [0.0, 2.5, 10.0], "index": index}, "side_bytes": 8 * 3 + 3 * 4 * 8,
            "marks": {"stage": [0, 1, 2], "count": [[3, 5], [9, 11], [20, 30]], "bytes": [[8, 12], [16, 24], [40, 60]]}}


def _lens(c):
    return [len(s) for s in c["embedded"]]


def test_truncate_at_a_stage():
    c = _container()
    t = EB.truncate(c, stage=1)
    assert _lens(t) == [16, 24] and t["embedded"][0] == bytes(range(16)) and t["embedded"][1] == bytes(range(100, 124))
    assert _lens(c) == [40, 60]                                                # the original is left alone
    for key in ("z", "base", "marks", "format", "lanes", "side_bytes"):
        assert t[key] == c[key]
    assert t["schedule"] is c["schedule"]
    assert _lens(EB.truncate(c, stage=2)) == [40, 60] and _lens(EB.truncate(c, stage=0)) == [8, 12]
    assert _lens(EB.truncate(t, stage=0)) == [8, 12]
    with pytest.raises(ValueError, match="stage 3 is not marked"):
        EB.truncate(c, stage=3)
    with pytest.raises(ValueError, match="already cut"):
        EB.truncate(t, stage=2)
    with pytest.raises(ValueError, match="stage="):                            # a uniform quality is no prefix
        EB.truncate(c, q=2.5)
    with pytest.raises(ValueError, match="exactly one"):
        EB.truncate(c, stage=1, max_bytes=500)
    with pytest.raises(ValueError, match="exactly one"):
        EB.truncate(c, stage=1, slice_bytes=[1, 2])
    with pytest.raises(ValueError, match="not an embedded container"):         # the format promises a schedule
        EB.truncate({k: v for k, v in c.items() if k != "schedule"}, stage=1)
    plain = dict(c, format="embedded-1", marks=dict(c["marks"], q=[0.5, 1, 2]))
    with pytest.raises(ValueError, match="scheduled container"):
        EB.truncate(plain, stage=1)


def test_truncate_to_a_byte_budget_counts_the_side_bytes():
    c = _container()                                                           # z + base = 20, schedule 120; marks 20 / 40 / 100
    side = c["side_bytes"]
    assert side == 120 and EB.container_bytes(c) == [10, 10, 100]
    for budget, want in ((10 ** 6, [40, 60]), (240, [40, 60]), (239, [16, 24]), (180, [16, 24]), (179, [8, 12]), (160, [8, 12]),
                         (159, [0, 0]), (140, [0, 0])):
        t = EB.truncate(c, max_bytes=budget)
        assert _lens(t) == want, budget
        assert sum(EB.container_bytes(t)) + side <= budget
    with pytest.raises(ValueError, match="schedule"):
        EB.truncate(c, max_bytes=139)


def test_truncate_at_explicit_lengths_is_unchanged():
    c = _container()
    assert EB.truncate(c, slice_bytes=[3, 0])["embedded"] == [bytes(range(3)), b""]
    assert _lens(EB.truncate(c, slice_bytes=[1000, 7])) == [40, 7]
    with pytest.raises(ValueError, match="slice_bytes"):
        EB.truncate(c, slice_bytes=[1])
