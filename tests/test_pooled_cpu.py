"""Picture-wide quality marks on the host: the NumPy / torch.quantile restatement of the definition
(tests/pooled_ref.py) and the version-2 framing of vampic.tiled on fabricated tile codestreams.  No model and no GPU."""
import struct

import numpy as np
import pytest
import torch

import pooled_ref as PR
from test_tiled_cpu import NS, _reseal, picture
from vampic import tiled as TL

QS = [0.05, 0.5, 2.5, 5.0, 9.99, 10.0]


def _sig(T, n, seed, ns=2, tied=True):
    rng = np.random.default_rng(seed)
    s = np.abs(rng.standard_normal((T, ns, n))).astype(np.float32) * np.linspace(0.2, 3.0, T, dtype=np.float32)[:, None, None]
    return np.round(s, 2).astype(np.float32) if tied else s


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("T,n", [(1, 512), (3, 7), (12, 512), (130, 64)])
def test_the_restatement_is_torch_quantile_of_the_concatenation(T, n):
    sig = _sig(T, n, T + n)
    thr = PR.thresholds(sig, QS)
    for k, q in enumerate(QS[:-1]):
        for j in range(sig.shape[1]):
            pool = torch.cat([torch.from_numpy(sig[t, j]) for t in range(T)])
            want = torch.quantile(pool, torch.tensor(1 - 0.1 * q, dtype=torch.float32), interpolation="linear")
            assert thr[k, j].tobytes() == want.numpy().tobytes(), (q, j)
    assert np.isneginf(thr[-1]).all()
    assert (np.diff(thr, axis=0) <= 0).all()                                    # thresholds never rise with q


def test_a_pool_of_one_tile_is_the_per_segment_rule():
    sig = _sig(1, 512, 3)
    thr = PR.thresholds(sig, QS)
    cnt = PR.counts(sig, thr)
    for k, q in enumerate(QS[:-1]):
        for j in range(2):
            t = torch.quantile(torch.from_numpy(sig[0, j]), torch.tensor(1 - 0.1 * q, dtype=torch.float32))
            assert float(t) == thr[k, j] and cnt[k, 0, j] == int((torch.from_numpy(sig[0, j]) >= t).sum())
    assert (cnt[-1] == 512).all()


def test_counts_are_monotone_and_sum_to_the_pool_count():
    sig = _sig(12, 64, 9)
    thr = PR.thresholds(sig, QS)
    cnt = PR.counts(sig, thr)
    assert cnt.shape == (len(QS), 12, 2) and cnt.dtype == np.int32
    assert (np.diff(cnt.astype(np.int64), axis=0) >= 0).all()
    for k in range(len(QS)):
        for j in range(2):
            assert cnt[k, :, j].sum() == (sig[:, j] >= thr[k, j]).sum()
    assert len({int(v) for v in cnt[2, :, 0]}) > 1                              # tiles of unlike scale keep unlike fractions
    # in rank order the kept set is a prefix whatever the ties
    o = PR.rank_order(sig[5, 1])
    assert (sig[5, 1][o][:cnt[2, 5, 1]] >= thr[2, 1]).all() and (sig[5, 1][o][cnt[2, 5, 1]:] < thr[2, 1]).all()


def test_keys_canonicalise_zeros_and_nans_and_sort_like_the_rank_order():
    s = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1.5, 1.0], dtype=np.float32)
    k = PR.keys(s)
    assert k[0] == k[1] and k[5] == k[6] == 0xFFFFFFFF and k[3] == k.min() and k[4] == 0xFF800000
    with np.errstate(invalid="ignore"):
        assert list(PR.rank_order(s)) == list(np.argsort(-np.where(np.isnan(s), -np.inf, s) + 0.0, kind="stable")[:8]) + [5, 6]
    one = _sig(1, 64, 1)
    one[0, 0, 7] = np.nan
    thr = PR.thresholds(one, QS)
    assert np.isnan(thr[:-1, 0]).all() and not np.isnan(thr[:, 1]).any()
    assert (PR.counts(one, thr)[:-1, 0, 0] == 0).all() and PR.counts(one, thr)[-1, 0, 0] == 64


# ------------------------------------------------------------------------------------------------- version-2 framing
def _thr(L=3, seed=0):
    rng = np.random.default_rng(seed)
    t = -np.sort(-rng.random((L, NS)).astype(np.float32), axis=0)               # never rising with the mark
    t[-1] = -np.inf
    return t


def pooled(**case):
    g, streams, v1 = picture(**case)
    thr = _thr(case.get("L", 3))
    return g, streams, v1, thr, TL.pack(g["H"], g["W"], g["tile"], g["V"], streams, thresholds=thr)


def test_version_2_round_trip_and_version_1_unchanged():
    g, streams, v1, thr, data = pooled()
    lay1, lay = TL.layout(v1), TL.layout(data)
    assert lay1["allocation"] == "tile" and lay1["thresholds"] is None and v1[4] == 1
    assert TL.pack(g["H"], g["W"], g["tile"], g["V"], streams) == v1            # no thresholds: version 1 byte for byte
    assert lay["allocation"] == "picture" and data[4] == 2
    assert lay["thresholds"].dtype == np.float32 and lay["thresholds"].tobytes() == thr.tobytes()
    extra = 8 + 4 * thr.size
    assert len(data) == len(v1) + extra and lay["header_end"] == lay1["header_end"] + extra
    assert lay["need_bytes"] == TL.need_bytes(data) == lay1["need_bytes"] + extra
    assert lay["round_end"] == [e + extra for e in lay1["round_end"]] and lay["marks"] == lay1["marks"]
    assert data[lay["header_end"]:] == v1[lay1["header_end"]:]                  # the body is the same
    for i, s in enumerate(streams):
        assert TL.tile_stream(data, *divmod(i, g["C"])) == s
    assert TL.tiles_for(lay, (40, 90, 30, 17)) == TL.tiles_for(lay1, (40, 90, 30, 17))
    assert TL.layout(data[:lay["header_end"]])["thresholds"].tobytes() == thr.tobytes()
    for n in (lay["header_end"], lay["need_bytes"], lay["round_end"][0], len(data) - 1):
        assert TL.need_bytes(data[:n]) == lay["need_bytes"]


def test_extract_keeps_version_and_thresholds_and_composes():
    g, streams, v1, thr, data = pooled()
    win = (40, 90, 30, 17)
    assert TL.extract(data) == data
    for rounds in (None, 2, 0):
        ex = TL.extract(data, win, rounds)
        el = TL.layout(ex)
        assert ex[4] == 2 and el["allocation"] == "picture" and el["thresholds"].tobytes() == thr.tobytes()
        assert el["marks"] == [0.5, 2.5, 10.0] and len(ex) < len(data)
        e1 = TL.extract(v1, win, rounds)                                        # the same cut of the version-1 stream
        assert ex[el["header_end"]:] == e1[TL.layout(e1)["header_end"]:]
    assert TL.extract(TL.extract(data, (0, 0, 100, 200)), win, 2) == TL.extract(TL.extract(data, rounds=3), win, 2) \
        == TL.extract(data, win, 2)
    lay = TL.layout(data)
    assert TL.extract(data, rounds=1) == TL.extract(data[:lay["round_end"][0]], rounds=1)


def test_every_single_byte_change_of_preamble_and_header_is_refused():
    g, streams, v1, thr, data = pooled()
    hend = TL.layout(data)["header_end"]
    for at in range(hend):
        for flip in (0x01, 0x80):
            bad = data[:at] + bytes([data[at] ^ flip]) + data[at + 1:]
            with pytest.raises(ValueError):
                TL.layout(bad)
            with pytest.raises(ValueError):
                TL.tile_stream(bad, 0, 0)
            with pytest.raises(ValueError):
                TL.extract(bad, rounds=1)


def test_contradictions_under_a_matching_crc_are_refused_by_message():
    g, streams, v1, thr, data = pooled()
    ext = 20 + 4 * 12 * 5                                                       # the allocation fields follow the table
    assert _reseal(data, lambda h: None) == data
    with pytest.raises(ValueError, match=r"version 2: the header contradicts itself: .* thresholds of 4 marks x 3 slices take .* it states"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext + 2, 4)))        # n_marks against the header's length
    with pytest.raises(ValueError, match=r"version 2: the header contradicts itself: .* it states"):
        TL.layout(_reseal(data, lambda h: h.extend(b"\0" * 4)))                          # four bytes too many
    with pytest.raises(ValueError, match=r"version 2: the header contradicts itself: .* at least"):
        TL.layout(data[:4] + b"\x02" + v1[5:])                                           # a version-1 header read as version 2
    with pytest.raises(ValueError, match=r"allocation 2 .*this reader knows allocation 1"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext, 2)))
    with pytest.raises(ValueError, match=r"allocation 0"):
        TL.layout(_reseal(data, lambda h: struct.pack_into("<H", h, ext, 0)))

    def rises(h):                                                                        # slice 1: mark 1 above mark 0
        struct.pack_into("<f", h, ext + 8 + 4 * (1 * NS + 1), float(thr[0, 1]) + 1.0)
    with pytest.raises(ValueError, match=r"the threshold of slice 1 rises from mark 0 .* to mark 1"):
        TL.layout(_reseal(data, rises))
    with pytest.raises(ValueError, match=r"the threshold of slice 1 rises"):
        TL.extract(_reseal(data, rises), rounds=1)

    def fewer(h):                                                                        # two rows, consistently framed: not the tiles' marks
        del h[ext + 8 + 4 * 2 * NS:ext + 8 + 4 * 3 * NS]
        struct.pack_into("<H", h, ext + 2, 2)
        struct.pack_into("<Q", h, len(h) - 8, len(data) - 4 * NS)
    with pytest.raises(ValueError, match=r"contradicts tile \(0, 0\): thresholds of 2 marks x 3 slices, the tile carries 3 marks"):
        TL.layout(_reseal(data, fewer))
    with pytest.raises(ValueError, match=r"thresholds are float32 \[3 marks\]\[3 slices\]"):
        TL.pack(g["H"], g["W"], g["tile"], g["V"], streams, thresholds=thr[:2])
    with pytest.raises(ValueError, match="a threshold rises with the mark"):
        TL.pack(g["H"], g["W"], g["tile"], g["V"], streams, thresholds=thr[::-1])
    nan = thr.copy()
    nan[:2, 0] = np.nan                                                                  # a pool with a NaN: NaN rows are no rise
    assert np.isnan(TL.layout(TL.pack(g["H"], g["W"], g["tile"], g["V"], streams, thresholds=nan))["thresholds"][:2, 0]).all()
