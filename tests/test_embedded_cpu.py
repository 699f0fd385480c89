"""Embedded streams on the host: the tolerant prefix decoder and prefix_bytes behind the C ABI against
the independent pure-Python coder (oracle/rans_oracle.py), embedded.truncate on a hand-built container, and the numpy
statements of the two device contracts that tests/test_gpu_embedded.py holds the kernels to: the rank order
(vam_variance_rank) and the level-id rule (vam_rank_scatter)."""
import numpy as np
import pytest
import torch

import rans_oracle as R
import vampic
from vampic import bitstream as bs
from vampic import embedded as EB


# ------------------------------------------------------------------------------------------------ the device contracts
def rank_order(s) -> np.ndarray:
    """THE ordering contract of vam_variance_rank for one segment ``s`` flattened in canonical [C, h, w] order: descending
    sigma, equal values by ascending index, -0.0 == +0.0, +inf first, NaN last (the NaNs again by index)."""
    return np.argsort(-np.asarray(s, dtype=np.float32).reshape(-1), kind="stable")


def rank_keys(s) -> np.ndarray:
    """The 64-bit keys the kernel sorts ascending: (~ordered_bits(sigma) << 32) | index, zeros and NaNs canonicalised."""
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    u = s.view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    k = np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    d = np.where(np.isnan(s), 0xFFFFFFFF, k ^ 0xFFFFFFFF).astype(np.uint64)
    return (d << np.uint64(32)) | np.arange(s.size, dtype=np.uint64)


def level_ids(count, n: int) -> np.ndarray:
    """THE level-id rule of vam_rank_scatter for one segment: for every rank r < n the smallest g with r < count[g], 0xFF
    if there is none (count non-decreasing)."""
    count = np.asarray(count, dtype=np.int64)
    r = np.arange(n)[:, None]
    inside = r < count[None, :]
    return np.where(inside.any(1), inside.argmax(1), 0xFF).astype(np.uint8)


def test_rank_order_contract_special_values():
    nan, inf = float("nan"), float("inf")
    s = np.array([1, nan, 0.0, -0.0, inf, 1, -inf, nan, 0.5], dtype=np.float32)
    assert rank_order(s).tolist() == [4, 0, 5, 8, 2, 3, 6, 1, 7]
    assert rank_order(np.array([-0.0, 0.0, -0.0], dtype=np.float32)).tolist() == [0, 1, 2]
    assert rank_order(np.full(5, 1.25, dtype=np.float32)).tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("n", [1, 64, 3072, 8192])
def test_rank_keys_sort_to_the_contract(n):
    rng = np.random.default_rng(n)
    for ties in (False, True):
        s = (rng.random(n) * 4 + 0.05).astype(np.float32)
        if ties:
            s = np.round(s * 2) / 2
        if n >= 64:
            s[rng.integers(0, n, 6)] = [np.nan, np.inf, -0.0, 0.0, -np.inf, -np.nan]
            s[rng.integers(0, n, 2)] = np.float32(-1.5)
        keys = rank_keys(s)
        assert np.unique(keys).size == n                                   # unique: any correct sort gives the contract
        assert np.array_equal(np.argsort(keys), rank_order(s))


def test_prefix_of_rank_order_is_the_quantile_mask():
    """The masks of all qualities are prefixes of the rank order (torch.quantile, as layers/channel_mask.py builds them)."""
    rng = np.random.default_rng(7)
    for n, ties in ((64, False), (64, True), (8192, False), (8192, True)):
        s = (rng.random(n) * 4 + 0.05).astype(np.float32)
        if ties:
            s = np.round(s * 2) / 2
        order = rank_order(s)
        for q in (0.05, 0.5, 1, 2.5, 3.3, 7, 9.99):
            thr = torch.quantile(torch.from_numpy(s), 1 - q / 10)
            mask = s >= thr.item()
            assert set(order[:int(mask.sum())].tolist()) == set(np.nonzero(mask)[0].tolist()), (n, ties, q)


def test_level_id_rule():
    assert level_ids([2, 2, 5], 7).tolist() == [0, 0, 2, 2, 2, 255, 255]
    assert level_ids([0, 0], 3).tolist() == [255, 255, 255]
    assert level_ids([3], 3).tolist() == [0, 0, 0]
    assert level_ids([0, 1, 1, 4], 4).tolist() == [1, 3, 3, 3]


# ------------------------------------------------------------------------------------------------ the host coder
def _tables(widths=(1, 3, 8, 20, 40)):
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


def _stream(n, seed, t):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 5, n).astype(np.int32)
    sym = np.round(rng.normal(0, 0.3 * np.array([1, 3, 8, 20, 40])[idx] + 0.2)).astype(np.int32)
    sym[3::17] = 500             # far out of range: bypass coding, several 4-bit chunks
    sym[5::23] = -777
    sym[7::11] = 41              # just outside the widest table
    return sym, idx, bs.encode(sym, idx, t)


UNTOUCHED = -123456


def _prefix(stream, idx, t):
    out = np.full(idx.size, UNTOUCHED, dtype=np.int32)
    got = bs.decode_prefix_streams([(stream, idx, out)], t)
    assert len(got) == 1
    return got[0], out


@pytest.mark.parametrize("n, seed", [(40, 0), (150, 1), (333, 2)])
def test_prefix_decoder_agrees_with_the_oracle_on_every_word_prefix(n, seed):
    t = _tables()
    sym, idx, stream = _stream(n, seed, t)
    tab = (t.cdf.tolist(), t.sizes.tolist(), t.offsets.tolist())
    last = 0
    for nb in range(0, len(stream) + 1, 4):
        cnt, out = _prefix(stream[:nb], idx, t)
        assert np.array_equal(out[:cnt], sym[:cnt]), nb
        assert (out[cnt:] == UNTOUCHED).all(), nb                              # the rest is left untouched
        assert cnt >= last, nb                                                 # monotone in the length
        last = cnt
        if nb < 8:
            assert cnt == 0, nb
            continue
        assert R.decode(stream[:nb], idx[:cnt].tolist(), *tab) == sym[:cnt].tolist(), nb
        if cnt < n:
            with pytest.raises(IndexError):                                    # one more symbol runs out of words
                R.decode(stream[:nb], idx[:cnt + 1].tolist(), *tab)
    assert last == n


def test_prefix_decoder_any_byte_length_and_short_prefixes():
    t = _tables()
    sym, idx, stream = _stream(150, 4, t)
    for nb in range(0, 8):
        assert _prefix(stream[:nb], idx, t)[0] == 0
    for nb in (9, 13, 30, 31, len(stream) - 1):
        a, out_a = _prefix(stream[:nb], idx, t)
        b, out_b = _prefix(stream[:nb // 4 * 4], idx, t)
        assert a == b and np.array_equal(out_a, out_b), nb
    assert _prefix(stream + b"\x01\x02\x03", idx, t)[0] == 150                 # bytes beyond the stream are not read
    assert _prefix(b"", idx, t)[0] == 0
    with pytest.raises(vampic._lib.VamError):
        _prefix(stream, idx + 100, t)                                          # table index out of range


def test_prefix_decoder_many_streams_equals_one_by_one():
    t = _tables()
    jobs, want = [], []
    for seed in range(24):
        sym, idx, stream = _stream(60 + 5 * seed, 10 + seed, t)
        cut = stream[:(seed * 7) % (len(stream) + 3)]
        jobs.append((cut, idx, np.full(idx.size, UNTOUCHED, dtype=np.int32)))
        want.append(_prefix(cut, idx, t))
    for threads in (1, 4, None):
        for j in jobs:
            j[2][:] = UNTOUCHED
        got = bs.decode_prefix_streams(jobs, t, threads=threads)
        assert got == [w[0] for w in want]
        assert all(np.array_equal(j[2], w[1]) for j, w in zip(jobs, want))
    assert bs.decode_prefix_streams([], t) == []


def test_existing_decoder_still_refuses_a_truncated_stream():
    t = _tables()
    sym, idx, stream = _stream(150, 5, t)
    with pytest.raises(vampic._lib.VamError, match="truncated"):
        bs.decode(stream[:len(stream) // 2 // 4 * 4], idx, t)
    assert np.array_equal(bs.decode(stream, idx, t), sym)


@pytest.mark.parametrize("n, seed", [(40, 0), (333, 2), (3000, 3)])
def test_prefix_bytes_is_minimal(n, seed):
    t = _tables()
    sym, idx, stream = _stream(n, seed, t)
    counts = sorted({0, 1, 2, 3, n // 7, n // 2, n - 1, n})
    cuts = bs.prefix_bytes(stream, idx, counts, t)
    assert len(cuts) == len(counts) and cuts == sorted(cuts) and cuts[-1] <= len(stream)
    for c, nb in zip(counts, cuts):
        assert nb % 4 == 0
        if c == 0:
            assert nb == 0
            continue
        assert nb >= 8
        assert _prefix(stream[:nb], idx, t)[0] >= c, (c, nb)
        assert _prefix(stream[:nb - 4], idx, t)[0] < c, (c, nb)
    assert bs.prefix_bytes(stream, idx, [], t) == []
    assert bs.prefix_bytes(stream, idx, [5, 5], t) == [bs.prefix_bytes(stream, idx, [5], t)[0]] * 2
    with pytest.raises(vampic._lib.VamError, match="decode"):
        bs.prefix_bytes(stream[:8], idx, [n], t)                               # the bytes given do not reach that count
    with pytest.raises(vampic._lib.VamError, match="sorted"):
        bs.prefix_bytes(stream, idx, [3, 2], t)


# ------------------------------------------------------------------------------------------------ truncate
def _container():
    return {"format": "embedded-1", "shape": (1, 2), "z": [b"z" * 10], "base": [[b"a" * 4], [b"b" * 6]],
            "embedded": [bytes(range(40)), bytes(range(100, 160))],
            "marks": {"q": [0.5, 1, 2], "count": [[3, 5], [9, 11], [20, 30]], "bytes": [[8, 12], [16, 24], [40, 60]]}}


def _lens(c):
    return [len(s) for s in c["embedded"]]


def test_truncate_at_a_mark():
    c = _container()
    t = EB.truncate(c, q=1)
    assert _lens(t) == [16, 24] and t["embedded"][0] == bytes(range(16)) and t["embedded"][1] == bytes(range(100, 124))
    assert _lens(c) == [40, 60]                                                # the original is left alone
    assert t["z"] == c["z"] and t["base"] == c["base"] and t["marks"] == c["marks"] and t["format"] == "embedded-1"
    assert _lens(EB.truncate(c, q=2)) == [40, 60] and _lens(EB.truncate(c, q=0.5)) == [8, 12]
    assert _lens(EB.truncate(t, q=0.5)) == [8, 12]                             # cutting a cut container further
    with pytest.raises(ValueError, match="not marked"):
        EB.truncate(c, q=3.3)
    with pytest.raises(ValueError, match="already cut"):
        EB.truncate(t, q=2)


def test_truncate_to_a_byte_budget():
    c = _container()                                                           # z + base = 20 bytes; marks 40 / 60 / 120
    assert EB.container_bytes(c) == [10, 10, 100]
    for budget, want in ((10 ** 6, [40, 60]), (120, [40, 60]), (119, [16, 24]), (60, [16, 24]), (59, [8, 12]), (40, [8, 12]),
                         (39, [0, 0]), (20, [0, 0])):
        t = EB.truncate(c, max_bytes=budget)
        assert _lens(t) == want, budget
        assert sum(EB.container_bytes(t)) <= budget
    with pytest.raises(ValueError, match="base"):
        EB.truncate(c, max_bytes=19)


def test_truncate_at_explicit_lengths_and_bad_calls():
    c = _container()
    t = EB.truncate(c, slice_bytes=[3, 0])
    assert t["embedded"] == [bytes(range(3)), b""]
    assert _lens(EB.truncate(c, slice_bytes=[1000, 7])) == [40, 7]
    for bad in ([1], [1, 2, 3], [-1, 2]):
        with pytest.raises(ValueError, match="slice_bytes"):
            EB.truncate(c, slice_bytes=bad)
    with pytest.raises(ValueError, match="exactly one"):
        EB.truncate(c)
    with pytest.raises(ValueError, match="exactly one"):
        EB.truncate(c, q=1, max_bytes=100)
    with pytest.raises(ValueError, match="embedded container"):
        EB.truncate({"q_list": [1], "progressive": []}, q=1)
