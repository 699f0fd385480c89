"""Embedded streams on the device coder, with interleaved lanes (csrc/rans_device.hip): the kernels on
flat ranked buffers against the host exports — strings, marks, the tolerant decode at every kind of cut, refused inputs —
and embedded.encode_batch / EmbeddedDecoder with ``coder`` and ``lanes`` against the host coder and
forward_single_quality.  Everything is bit-exact."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import _lib as L, bitstream as bs, embedded as EB, progressive as P   # noqa: E402
from test_gpu_progressive_batch import _net, _x                                  # noqa: E402
from test_gpu_rans_device import _buffers                                        # noqa: E402

LANES = [1, 8, 64]
GEOMETRIES = [(6, 12),       # a partial group; at K = 64 it has 52 empty lanes
              (6, 512),      # a slice of the 64x64 image
              (3, 1000)]     # no multiple of 8 or 64
FILL = -7
NS, QS = 10, [0, 0.5, 2.5, 10, 1.0]


# ----------------------------------------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def dt():
    d = bs.DeviceCoderTables.of(_net().gaussian_conditional, "cuda")
    assert d.packed is not None and 0 < d.lds_bytes <= d.lds_limit                # the LDS path
    return d


def _flat(t, streams, n, seed):
    sym, idx = _buffers(t, streams, 1, 1, n, seed)
    return np.ascontiguousarray(sym.reshape(streams, n)), np.ascontiguousarray(idx.reshape(streams, n))


def _host_prefix(prefix, idx, t, K):
    """(count, status, symbols with zeros beyond the count) from the host export."""
    i = bs._i32(idx)
    out = np.zeros(i.size, dtype=np.int32)
    src = np.frombuffer(prefix, dtype=np.uint8)
    st = np.full(1, -1, dtype=np.int32)
    got = L.load().vam_rans_interleaved_decode_prefix(src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size,
                                                      t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data, t.offsets.ctypes.data,
                                                      t.cdf.shape[0], K, out.ctypes.data, st.ctypes.data)
    assert got >= 0
    out[got:] = 0
    return int(got), int(st[0]), out


def _device_prefix(strings, d_idx, dt, K, up=None):
    """(available, status, symbols) of one device launch; the output sits inside a larger buffer that must stay untouched."""
    streams, n = d_idx.shape
    guard = torch.full((streams + 2, n), FILL, dtype=torch.int32, device="cuda")
    out = guard[1:streams + 1]
    meta = torch.full((2, streams), -1, dtype=torch.int32, device="cuda")
    up = bs.upload_streams(strings, "cuda") if up is None else up
    bs.decode_embedded_uploaded(up, 0, d_idx, out, dt, K, meta)
    g = guard.cpu().numpy()
    assert (g[0] == FILL).all() and (g[-1] == FILL).all()
    m = meta.cpu().numpy()
    return m[0], m[1], g[1:-1]


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_kernels_equal_the_host_exports(dt, geometry, K):
    streams, n = geometry
    t = dt.host
    sym, idx = _flat(t, streams, n, seed=streams + n + K)
    want = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(streams)], t, lanes=K)
    counts = np.array(sorted({0, 1, n // 3, n}), dtype=np.int32)
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    d_count = torch.from_numpy(np.ascontiguousarray(np.repeat(counts[:, None], streams, 1))).cuda()
    got, marks = bs.encode_embedded_device(d_sym, d_idx, dt, K, d_count)
    assert got == want                                        # device strings == the host export's
    if K == 1:
        assert got == bs.encode_streams([(sym[s], idx[s]) for s in range(streams)], t)
    assert marks.shape == (len(counts), streams)
    for s in range(streams):                                  # the marks from the encoder's word positions == the host's pass
        assert marks[:, s].tolist() == bs.prefix_bytes(want[s], idx[s], counts.tolist(), t, lanes=K), s
    assert bs.encode_embedded_device(d_sym, d_idx, dt, K)[0] == want             # and without marks
    # the tolerant decode, every stream cut at its own length
    cuts = {"0": [0] * streams, "7": [7] * streams, "8K-1": [8 * K - 1] * streams, "8K": [8 * K] * streams,
            "odd": [(len(s) * (k + 2) // (streams + 3)) | 1 for k, s in enumerate(want)],
            "odd2": [(len(s) // 2) | 3 for s in want], "whole": [len(s) for s in want]}
    for m in range(len(counts)):
        cuts[f"mark {m}"] = marks[m].tolist()
    assert all(c % 4 for c in cuts["odd"] + cuts["odd2"])
    for name, cut in cuts.items():
        strings = [s[:c] for s, c in zip(want, cut)]
        avail, status, out = _device_prefix(strings, d_idx, dt, K)
        for s in range(streams):
            count, st, ref = _host_prefix(strings[s], idx[s], t, K)
            assert (avail[s], status[s]) == (count, st) and st == 0, (name, s)
            assert np.array_equal(out[s], ref), (name, s)     # the host's symbols, zeros beyond
            assert np.array_equal(ref[:count], sym[s][:count])
        if name.startswith("mark"):
            assert (avail >= counts[int(name.split()[1])]).all()
        if name == "whole":
            assert (avail == n).all()


@pytest.mark.parametrize("K", LANES)
def test_kernels_refuse_bad_indexes_offsets_and_lengths(dt, K):
    streams, n = 3, 1000
    t = dt.host
    sym, idx = _flat(t, streams, n, seed=77 + K)
    want = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(streams)], t, lanes=K)
    bad = idx.copy()
    bad[0, 0], bad[1, 517], bad[2, 999] = -1, t.cdf.shape[0], 1 << 30
    avail, status, out = _device_prefix(want, torch.from_numpy(bad).cuda(), dt, K)
    for s, where in enumerate((0, 517, 999)):
        count, st, ref = _host_prefix(want[s], bad[s], t, K)
        assert (avail[s], status[s]) == (count, st) and st == 2 and where // K * K <= count <= where
        assert np.array_equal(out[s], ref) and (out[s][count:] == 0).all()
    d_idx = torch.from_numpy(idx).cuda()
    with pytest.raises(L.VamError, match="index out of range"):
        bs.encode_embedded_device(torch.from_numpy(sym).cuda(), torch.from_numpy(bad).cuda(), dt, K)
    # a byte offset that is misaligned, negative or past the upload, and a length that leaves it: status 6, nothing read
    for offsets, lengths in (([2, None, None], None), ([-4, None, None], None), ([None, 1 << 40, None], None),
                             (None, [None, None, 1 << 30]), (None, [-1, None, None])):
        up = bs.upload_streams(want, "cuda")
        o = up.buf[:8 * streams].view(torch.int64)
        ln = up.buf[8 * streams:12 * streams].view(torch.int32)
        touched = set()
        for arr, vals in ((o, offsets), (ln, lengths)):
            for s, v in enumerate(vals or []):
                if v is not None:
                    arr[s] = v if arr is ln or v < 0 or v > (1 << 30) else int(arr[s]) + v
                    touched.add(s)
        avail, status, out = _device_prefix(want, d_idx, dt, K, up=up)
        for s in range(streams):
            if s in touched:
                assert (avail[s], status[s]) == (0, 6) and (out[s] == 0).all(), (offsets, lengths, s)
            else:
                assert (avail[s], status[s]) == (n, 0) and np.array_equal(out[s], sym[s])
    for lanes in (0, 3, 128):
        with pytest.raises(ValueError, match="power of two"):
            bs.encode_embedded_device(torch.from_numpy(sym).cuda(), d_idx, dt, lanes)


def test_kernels_read_tables_too_large_for_lds_from_global_memory():
    n_t, size = 48, 2050                                      # 48 x 2049 x 2 bytes: above a CU's LDS
    rng = np.random.default_rng(1)
    cdf = np.zeros((n_t, size), dtype=np.int32)
    for k in range(n_t):
        cdf[k, 1:-1] = np.sort(rng.choice(np.arange(1, 65536), size=size - 2, replace=False))
        cdf[k, -1] = 65536
    t = bs.Tables(cdf, np.full(n_t, size, dtype=np.int32), rng.integers(-1000, 0, n_t).astype(np.int32))
    big = bs.DeviceCoderTables.build(t, "cuda")
    assert big.packed is None and big.lds_bytes > big.lds_limit
    sym, idx = _flat(t, 3, 1000, seed=9)
    want = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(3)], t, lanes=8)
    d_idx = torch.from_numpy(idx).cuda()
    assert bs.encode_embedded_device(torch.from_numpy(sym).cuda(), d_idx, big, 8)[0] == want
    strings = [s[:len(s) * 2 // 3 | 1] for s in want]
    avail, status, out = _device_prefix(strings, d_idx, big, 8)
    for s in range(3):
        count, st, ref = _host_prefix(strings[s], idx[s], t, 8)
        assert (avail[s], status[s]) == (count, 0) and 0 < count < 1000 and np.array_equal(out[s], ref)


# ----------------------------------------------------------------------------------------------- model
_CODED = {}


def _coded(coder, K):
    """(x, containers) of the 2 x 64 x 64 batch per (coder, lanes), encoded once per session."""
    if "x" not in _CODED:
        _CODED["x"] = _x(2, 64, 64)
    if (coder, K) not in _CODED:
        _CODED[coder, K] = EB.encode_batch(_net(), _CODED["x"], coder=coder, lanes=K)
    return _CODED["x"], _CODED[coder, K]


@pytest.fixture(scope="module")
def forward():
    net, x = _net(), _coded("host", 1)[0]
    with torch.no_grad():
        return {q: net.forward_single_quality(x, q) for q in QS}


def _same(a, b):
    return torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"])


@contextlib.contextmanager
def host_coder_forbidden(monkeypatch):
    """Any call of a host coder entry point fails the test: without it the comparisons would pass with ``coder`` ignored."""
    def refuse(*a, **k):
        raise AssertionError("the host coder ran in a coder='device' call")
    with monkeypatch.context() as mp:
        for name in ("encode", "decode", "encode_streams", "decode_streams", "encode_lanes", "decode_lanes", "encode_interleaved",
                     "encode_interleaved_streams", "decode_prefix_streams", "prefix_bytes"):
            mp.setattr(bs, name, refuse)
        yield


@pytest.mark.parametrize("K", LANES)
def test_device_containers_equal_the_host_containers(K):
    x, host = _coded("host", K)
    _, dev = _coded("device", K)
    assert dev == host
    for c in host:
        if K == 1:
            assert c["format"] == "embedded-1" and set(c) == {"format", "shape", "z", "base", "embedded", "marks"}
        else:
            assert c["format"] == "embedded-2" and c["lanes"] == K and set(c) == {"format", "shape", "z", "base", "embedded", "marks", "lanes"}
        for counts, row in zip(c["marks"]["count"], c["marks"]["bytes"]):
            assert all((b == 0) == (n_ == 0) and (b == 0 or 8 * K <= b <= len(s)) for n_, b, s in zip(counts, row, c["embedded"]))
    if K == 1:
        assert host == EB.encode_batch(_net(), x)             # as it is called today
    else:                                                     # z and the base are the K = 1 container's
        one = _coded("host", 1)[1]
        assert all(a["z"] == b["z"] and a["base"] == b["base"] and a["marks"]["count"] == b["marks"]["count"] for a, b in zip(host, one))


@pytest.mark.parametrize("K", [1, 64])
def test_device_session_never_calls_the_host_coder(monkeypatch, forward, K):
    net = _net()
    x, want = _coded("host", K)
    with host_coder_forbidden(monkeypatch):
        cs = EB.encode_batch(net, x, coder="device", lanes=K)
        dec = EB.EmbeddedDecoder(net, cs, coder="device")
        assert dec.idx_r is None                              # _front copied no ranked indexes to the host
        assert (dec.available() == 512).all()
        assert _same(dec.decode(), forward[10])
        outs = dec.decode_qualities(QS)
        assert dec.idx_r is None
    assert cs == want
    for q, o in zip(QS, outs):
        assert _same(o, forward[q]), q
    assert dec.bits(2.5) == EB.EmbeddedDecoder(net, want, coder="host").bits(2.5) and dec.idx_r is not None


@pytest.mark.parametrize("K", [1, 64])
def test_either_coder_reads_the_others_containers(forward, K):
    net = _net()
    dev_dec = EB.EmbeddedDecoder(net, _coded("host", K)[1], coder="device")
    host_dec = EB.EmbeddedDecoder(net, _coded("device", K)[1], coder="host")
    assert dev_dec.lanes == host_dec.lanes == K and dev_dec.dp is not host_dec.dp
    a, b = dev_dec.decode_qualities(QS), host_dec.decode_qualities(QS)
    for q, oa, ob in zip(QS, a, b):
        assert _same(oa, forward[q]) and _same(ob, forward[q]), q
    assert np.array_equal(dev_dec.available(), host_dec.available())


@pytest.mark.parametrize("K", [1, 64])
def test_truncated_containers_decode_alike_on_both_coders(K):
    net = _net()
    x, cs = _coded("host", K)
    lens = [len(s) for s in cs[1]["embedded"]]
    cut = [(8 * K + (ln - 8 * K) * (j + 1) // 12) | 1 for j, ln in enumerate(lens)]     # odd lengths inside the words: mid-group cuts
    cut[2], cut[5], cut[8] = 0, 8 * K - 1, lens[8] + 3                            # one slice gone, one below the states, one whole
    assert all(c % 4 for c in cut[:2] + cut[3:8] + cut[9:])
    pair = [EB.truncate(cs[0], q=2.5), EB.truncate(cs[1], slice_bytes=cut)]
    dev, host = EB.EmbeddedDecoder(net, pair, coder="device"), EB.EmbeddedDecoder(net, pair, coder="host")
    avail = host.available()
    assert np.array_equal(dev.available(), avail)
    assert avail[1, 2] == 0 and avail[1, 5] == 0 and avail[1, 8] == 512 and ((avail[1] > 0) & (avail[1] < 512)).any()
    if K > 1:
        assert (avail[1] % K != 0).any()                      # a cut inside a group
    k25 = P.Q_LIST.index(2.5)
    assert (avail[0] >= np.asarray(cs[0]["marks"]["count"][k25])).all() and (avail[0] < 512).any()
    assert _same(dev.decode(), host.decode())
    errors = []
    for d in (dev, host):
        with pytest.raises(ValueError, match=r"quality 7.0 needs \d+ elements of slice \d+ of image \d+, its container holds \d+") as e:
            d.decode_qualities([7])
        errors.append(str(e.value))
    assert errors[0] == errors[1]
    one = [EB.truncate(c, q=2.5) for c in cs]                 # every image cut at the mark: that quality is still whole
    d1, h1 = EB.EmbeddedDecoder(net, one, coder="device"), EB.EmbeddedDecoder(net, one, coder="host")
    with torch.no_grad():
        assert _same(d1.decode_qualities([2.5])[0], net.forward_single_quality(x, 2.5))
    assert d1.bits(2.5) == h1.bits(2.5) == [8.0 * sum(EB.container_bytes(c)) for c in one]
    assert d1.bits(0.5) == h1.bits(0.5) and d1.bits(0) == h1.bits(0)


def test_one_graph_per_group_size_on_the_device_decoder(forward):
    net = _net()
    assert net.use_graph
    _, cs = _coded("device", 8)
    dec = EB.EmbeddedDecoder(net, cs, coder="device")
    a = dec.decode_qualities([0.5, 2.5])
    b = dec.decode_qualities([1.0, 10])                       # other cuts: the same graph, another count table
    other = EB.EmbeddedDecoder(net, [EB.truncate(c, q=1) for c in cs], coder="device")     # another decoder on the same plans
    e = other.decode_qualities([1.0])[0]
    a2 = dec.decode_qualities([0.5, 2.5])                     # the first one again after the plans served another
    assert dec.dp is other.dp and {1, 2} <= set(dec.dp.tails)
    assert all(len(t.runner.graphs) == 1 for t in dec.dp.tails.values())
    for o, q in zip(a + b + [e] + a2, [0.5, 2.5, 1.0, 10, 1.0, 0.5, 2.5]):
        assert _same(o, forward[q]), q


def test_lanes_are_read_from_the_containers_and_checked():
    net = _net()
    x, c1 = _coded("host", 1)
    _, c8 = _coded("host", 8)
    for coder in ("host", "device"):
        with pytest.raises(ValueError, match="same lanes per embedded stream"):
            EB.EmbeddedDecoder(net, [c1[0], c8[1]], coder=coder)
    for bad in (0, 3, 128, "8", None):
        with pytest.raises(ValueError, match="power of two"):
            EB.encode_batch(net, x, lanes=bad)
        with pytest.raises(ValueError, match="power of two"):
            EB.EmbeddedDecoder(net, [dict(c, lanes=bad) for c in c8])
    with pytest.raises(ValueError, match="coder is 'host' or 'device'"):
        EB.encode_batch(net, x, coder="gpu")
    with pytest.raises(ValueError, match="coder is 'host' or 'device'"):
        EB.EmbeddedDecoder(net, c1, coder="gpu")
    net.coder_lanes = 8                                       # never read: lanes is the argument's
    try:
        assert EB.encode_batch(net, x[:1]) == c1[:1]
    finally:
        net.coder_lanes = 1


def test_a_slice_that_is_no_power_of_two_round_trips_at_64_lanes():
    net = _net()
    x = _x(1, 128, 192, seed=4)                               # n = 32 * 8 * 12 = 3072 per slice
    cs = EB.encode_batch(net, x, coder="device", lanes=64)
    assert cs == EB.encode_batch(net, x, coder="host", lanes=64)
    dec = EB.EmbeddedDecoder(net, [EB.truncate(cs[0], q=2.5)], coder="device")
    assert (dec.available() < 3072).any()
    with torch.no_grad():
        assert _same(dec.decode_qualities([2.5])[0], net.forward_single_quality(x, 2.5))
        assert _same(EB.EmbeddedDecoder(net, cs, coder="device").decode(), net.forward_single_quality(x, 10))
