"""The cut-table kernel (csrc/rans_device.hip): vam_rans_interleaved_cut_table_device against the host
coder's table of the strings the host export writes for the same elements, bit for bit; refused streams, guard words,
malformed calls; and the encode launch beside it, whose strings and marks it must not change.  No model."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import _lib as L, bitstream as bs, ops        # noqa: E402
from cut_table_cases import CONTENTS, LENGTHS, content, tables        # noqa: E402

# (streams, lanes): one stream, more streams than a wave holds (65 > 64, 9 > 8, 3 > 1), and waves with idle lanes
GEOMETRIES = [(1, 1), (7, 1), (65, 1), (1, 8), (9, 8), (1, 64), (3, 64)]
FILL, GUARD = -7, 64


@pytest.fixture(scope="module")
def dt():
    return bs.DeviceCoderTables.build(tables(), "cuda")


def _streams(t, kind, S, n, seed):
    pairs = [content(t, kind, n, seed + 31 * s) for s in range(S)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _launch(sym, idx, dt, K):
    """(cut [S, n + 1], status [S]) of one launch; both sit between guard words that must stay untouched."""
    S, n = sym.shape
    cut = torch.full((2 * GUARD + S * (n + 1),), FILL, dtype=torch.int32, device="cuda")
    status = torch.full((2 * GUARD + S,), FILL, dtype=torch.int32, device="cuda")
    bs.cut_table_launch(torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda(), dt, K,
                        cut[GUARD:GUARD + S * (n + 1)].view(S, n + 1), status[GUARD:GUARD + S])
    c, st = cut.cpu().numpy(), status.cpu().numpy()
    for a in (c, st):
        assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all()
    return c[GUARD:-GUARD].reshape(S, n + 1), st[GUARD:-GUARD]


def _host(sym, idx, t, K):
    strings = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(sym.shape[0])], t, lanes=K)
    return strings, np.stack([bs.cut_table(strings[s], idx[s], t, K) for s in range(sym.shape[0])])


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_kernel_equals_the_host_table(dt, geometry, n):
    S, K = geometry
    for kind in CONTENTS:
        sym, idx = _streams(dt.host, kind, S, n, seed=S + n + K)
        strings, want = _host(sym, idx, dt.host, K)
        got, status = _launch(sym, idx, dt, K)
        assert not status.any(), kind
        assert np.array_equal(got, want), (kind, np.argwhere(got != want)[:4])
        assert (got[:, 0] == 0).all() and (np.diff(got, axis=1) >= 0).all()
        assert (got[:, n] <= [len(s) for s in strings]).all()
        if kind == "zeros" and n >= 63:
            assert (got[:, min(n, 8 * K)] == 8 * K).all()     # a run that reads no word


def test_wrapper_returns_the_table_on_the_device(dt):
    sym, idx = _streams(dt.host, "bypass", 6, 500, seed=3)
    got = bs.cut_table_device(torch.from_numpy(sym.reshape(2, 3, 500)).cuda(), torch.from_numpy(idx.reshape(2, 3, 500)).cuda(), dt, 8)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (6, 501)
    assert np.array_equal(got.cpu().numpy(), _host(sym, idx, dt.host, 8)[1])


@pytest.mark.parametrize("K", [1, 8, 64])
def test_a_bad_index_zeroes_its_own_row_only(dt, K):
    n = 1000
    sym, idx = _streams(dt.host, "mixed", 3, n, seed=11 + K)
    _, want = _host(sym, idx, dt.host, K)
    for where, value in ((0, -1), (517, dt.host.cdf.shape[0]), (999, 1 << 30)):
        bad = idx.copy()
        bad[1, where] = value
        got, status = _launch(sym, bad, dt, K)
        assert status.tolist() == [0, 2, 0]
        assert not got[1].any() and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    with pytest.raises(L.VamError, match="embedded stream 1: index out of range"):
        bs.cut_table_device(torch.from_numpy(sym).cuda(), torch.from_numpy(bad).cuda(), dt, K)


@pytest.mark.parametrize("K", [1, 8, 64])
def test_a_zero_frequency_symbol_is_status_5(K):
    t = tables(zero_freq=True)
    dz = bs.DeviceCoderTables.build(t, "cuda")
    n = 300
    sym, idx = _streams(t, "mixed", 3, n, seed=5 + K)
    hit = (idx == 0) & (sym == t.offsets[0])                  # table 0's first entry has no mass
    sym[hit] += 1
    _, want = _host(sym, idx, t, K)
    sym[1, 123], idx[1, 123] = t.offsets[0], 0
    got, status = _launch(sym, idx, dz, K)
    assert status.tolist() == [0, 5, 0]
    assert not got[1].any() and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    with pytest.raises(L.VamError, match="zero-frequency symbol"):
        bs.cut_table_device(torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda(), dz, K)


def test_malformed_calls_say_why_and_write_nothing(dt):
    S, n = 2, 64
    sym, idx = _streams(dt.host, "mixed", S, n, seed=1)
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    cut = torch.full((S, n + 1), FILL, dtype=torch.int32, device="cuda")
    status = torch.full((S,), FILL, dtype=torch.int32, device="cuda")
    lib, tb = L.load(), C.byref(dt.struct)
    good = dict(sym=d_sym.data_ptr(), idx=d_idx.data_ptr(), S=S, n=n, K=8, t=tb, cut=cut.data_ptr(), status=status.data_ptr())
    for change, text in ((dict(sym=None), "need sym, idx, cut, status"), (dict(idx=None), "need sym, idx, cut, status"),
                         (dict(cut=None), "need sym, idx, cut, status"), (dict(status=None), "need sym, idx, cut, status"),
                         (dict(t=None), "tables need"), (dict(n=0), "n = 0"), (dict(n=-3), "n = -3"),
                         (dict(n=(1 << 31) - 1), "2\\^28 symbols"), (dict(n=(1 << 28) + 1), "2\\^28 symbols"),
                         (dict(S=0), "1 .. 2\\^20 streams"), (dict(K=0), "power of two"), (dict(K=3), "power of two"),
                         (dict(K=128), "power of two")):
        a = dict(good, **change)
        rc = lib.vam_rans_interleaved_cut_table_device(a["sym"], a["idx"], a["S"], a["n"], a["K"], a["t"], a["cut"], a["status"],
                                                       ops.stream_ptr())
        assert rc == -1, change                               # VAM_EINVAL
        with pytest.raises(L.VamError, match="vam_rans_interleaved_cut_table_device: .*" + text):
            L.check(rc, "cut table")
    torch.cuda.synchronize()
    assert (cut == FILL).all() and (status == FILL).all()
    for bad in (cut[:, :n], cut.to(torch.int64), cut.cpu()):
        with pytest.raises(ValueError, match=rf"cut is a contiguous int32 \[{S}, {n + 1}\] device buffer"):
            bs.cut_table_launch(d_sym, d_idx, dt, 8, bad, status)
    with pytest.raises(ValueError, match="power of two"):
        bs.cut_table_device(d_sym, d_idx, dt, 3)
    assert np.array_equal(bs.cut_table_device(d_sym, d_idx, dt, 8).cpu().numpy(), _host(sym, idx, dt.host, 8)[1])


@pytest.mark.parametrize("K", [1, 8, 64])
def test_the_encode_launch_is_unchanged_and_its_marks_are_table_entries(dt, K):
    S, n, marks = 5, 1000, 32
    sym, idx = _streams(dt.host, "bypass", S, n, seed=17 + K)
    strings, want = _host(sym, idx, dt.host, K)
    rng = np.random.default_rng(K)
    counts = np.sort(rng.integers(0, n + 1, (marks, S)), axis=0).astype(np.int32)         # non-decreasing in the mark
    counts[0, 0], counts[-1, -1] = 0, n
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    got, mark_bytes = bs.encode_embedded_device(d_sym, d_idx, dt, K, torch.from_numpy(counts).cuda())
    table, status = _launch(sym, idx, dt, K)
    assert not status.any() and np.array_equal(table, want)
    assert np.array_equal(mark_bytes, np.take_along_axis(table, counts.T.astype(np.int64), axis=1).T)
    assert got == strings                                     # the host export's strings, as before the table existed
    assert bs.encode_embedded_device(d_sym, d_idx, dt, K)[0] == strings
