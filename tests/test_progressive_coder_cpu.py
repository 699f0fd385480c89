"""Host stream coder of the batched progressive container (vam_rans_encode_streams / vam_rans_decode_streams) against the
single-stream coder and oracle/rans_oracle.py, and the container's pure helpers (quality-list checks, bit accounting)."""
import numpy as np
import pytest
import torch

import rans_oracle as R
import vampic
from vampic import bitstream as bs
from vampic import progressive as P


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


def _jobs(t, n_streams=23, seed=0):
    rng = np.random.default_rng(seed)
    jobs = []
    for s in range(n_streams):
        n = int(rng.integers(0, 700)) if s % 5 else 0 if s == 0 else 333
        idx = rng.integers(0, t.cdf.shape[0], n).astype(np.int32)
        sym = np.round(rng.normal(0, 1, n) * (1 + 3 * idx)).astype(np.int32)
        jobs.append((sym, idx))
    return jobs


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_streams_equal_single_coder_and_oracle(threads):
    t = _tables()
    jobs = _jobs(t)
    got = bs.encode_streams(jobs, t, threads=threads)
    assert len(got) == len(jobs)
    for (sym, idx), b in zip(jobs, got):
        assert b == bs.encode(sym, idx, t)
    for (sym, idx), b in list(zip(jobs, got))[:6]:
        assert b == R.encode(sym.tolist(), idx.tolist(), t.cdf.tolist(), t.sizes.tolist(), t.offsets.tolist())
    outs = [np.full(sym.size, -7, dtype=np.int32) for sym, _ in jobs]
    bs.decode_streams([(b, idx, o) for (sym, idx), b, o in zip(jobs, got, outs)], t, threads=threads)
    for (sym, _), o in zip(jobs, outs):
        assert np.array_equal(o, sym)


def test_bypass_extremes_round_trip():
    t = _tables()
    big = np.array([0, 1, -1, 2 ** 20, -2 ** 20, 2 ** 30, -2 ** 30, 40, -41, 41, 2 ** 31 - 1, -2 ** 31 + 1], dtype=np.int32)
    jobs = [(big, np.full(big.size, k, dtype=np.int32)) for k in range(t.cdf.shape[0])]
    got = bs.encode_streams(jobs, t, threads=4)
    outs = [np.empty(big.size, dtype=np.int32) for _ in jobs]
    bs.decode_streams([(b, j[1], o) for j, b, o in zip(jobs, got, outs)], t, threads=4)
    for (sym, idx), b, o in zip(jobs, got, outs):
        assert b == bs.encode(sym, idx, t)
        assert np.array_equal(o, big)


@pytest.mark.parametrize("threads", [1, 5])
def test_layer_selector_equals_explicit_masking(threads):
    t = _tables()
    rng = np.random.default_rng(3)
    n, n_layers = 2000, 6
    idx = rng.integers(0, t.cdf.shape[0], n).astype(np.int32)
    sym = np.round(rng.normal(0, 4, n)).astype(np.int32)
    layer = rng.integers(0, n_layers, n).astype(np.uint8)
    layer[rng.random(n) < 0.2] = 0xFF                              # in no layer
    got = bs.encode_streams([(sym, idx, layer, k) for k in range(n_layers)], t, threads=threads)
    acc = np.zeros(n, dtype=np.int32)
    for k in range(n_layers):
        delta = (layer == k).astype(np.int32)
        assert got[k] == bs.encode(sym * delta, idx * delta, t)   # r_sym * delta, idx * delta
        ref = bs.decode(got[k], idx * delta, t)
        acc += ref * delta
    out = np.full(n, 12345, dtype=np.int32)
    bs.decode_streams([(got[k], idx, out, layer, k) for k in range(n_layers)], t, threads=threads)
    inside = layer != 0xFF
    assert np.array_equal(out[inside], sym[inside]) and np.array_equal(out[inside], acc[inside])
    assert (out[~inside] == 12345).all()                          # elements of no layer are never written


def test_errors_raise():
    t = _tables()
    sym, idx = np.arange(-5, 5, dtype=np.int32), np.zeros(10, dtype=np.int32)
    st = (L := vampic._lib).VamRansStream
    arr = (st * 1)()
    out = np.empty(4, dtype=np.uint8)                              # over capacity
    arr[0] = st(sym.ctypes.data, None, idx.ctypes.data, None, sym.size, 0, 0, out.ctypes.data, out.size, 0)
    with pytest.raises(L.VamError, match="too small"):
        L.check(L.load().vam_rans_encode_streams(arr, 1, t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                                 t.offsets.ctypes.data, t.cdf.shape[0], 2), "vam_rans_encode_streams")
    bad = idx.copy()
    bad[3] = 99
    with pytest.raises(L.VamError, match="out of range"):
        bs.encode_streams([(sym, idx), (sym, bad)], t, threads=2)
    good = bs.encode_streams([(sym, idx)] * 3, t, threads=2)
    o = [np.empty(10, dtype=np.int32) for _ in range(3)]
    with pytest.raises(L.VamError, match="stream 1"):
        bs.decode_streams([(good[0], idx, o[0]), (good[1][:8], idx, o[1]), (good[2], idx, o[2])], t, threads=3)
    with pytest.raises(L.VamError):
        bs.decode_streams([(good[0][:-4], idx, o[0])], t, threads=1)
    with pytest.raises(L.VamError):
        bs.decode_streams([(good[0], bad, o[0])], t, threads=1)


def test_thread_count_clamped():
    t = _tables()
    jobs = _jobs(t, 40, seed=1)
    assert bs.encode_streams(jobs, t, threads=1000) == bs.encode_streams(jobs, t, threads=1)
    assert 1 <= bs.coder_threads(1000) <= vampic._lib.VAM_RANS_MAX_THREADS == 16
    assert bs.coder_threads(1) == 1
    with pytest.raises(vampic._lib.VamError):
        bs.encode_streams(jobs, t, threads=0)


def test_q_list_validation():
    assert P.check_q_list(P.Q_LIST) == [float(q) for q in P.Q_LIST]
    assert P.check_q_list([0, 0.5, 0.5, 10, 12]) == [0.0, 0.5, 0.5, 10.0, 12.0]
    for bad in ([], [1, 0.5], [-1, 2], [float("nan")], list(range(33))):
        with pytest.raises(ValueError):
            P.check_q_list(bad)


def test_bit_accounting():
    c = {"q_list": [0.5, 1, 2], "shape": (1, 1), "z": [b"abcd"], "base": [[b"x" * 8] for _ in range(10)],
         "progressive": [[b"y" * 4] * 10, [b"z" * 12] * 10, [b"" for _ in range(10)]]}
    assert P.container_bits(c) == [32.0, 640.0, [320.0, 960.0, 0.0]]
    assert [P.bits_up_to(c, k) for k in range(4)] == [672.0, 992.0, 1952.0, 1952.0]
    with pytest.raises(ValueError):
        P.bits_up_to(c, 4)
