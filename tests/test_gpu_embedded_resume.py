"""Resumable embedded decode (csrc/rans_device.hip): the resume kernel against the host resume export and
the one-shot kernel on the concatenation, step by step through chains of cuts, and EmbeddedDecoder(resumable=True).extend
against a fresh decoder on the same prefixes.  Everything is bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import _lib as L, bitstream as bs, embedded as EB                            # noqa: E402
from test_gpu_progressive_batch import _net, _x                                         # noqa: E402
from test_gpu_embedded_device import _device_prefix, _flat, _same, host_coder_forbidden  # noqa: E402
import test_gpu_embedded_schedule as GS                                                 # noqa: E402

FILL = -7
STREAMS = 5                        # an odd count: a wave holds a partial set of streams
STATE_FILL = 0x5A5A5A5A5A5A5A5A


# ----------------------------------------------------------------------------------------------- kernel
@pytest.fixture(scope="module")
def dt():
    d = bs.DeviceCoderTables.of(_net().gaussian_conditional, "cuda")
    assert d.packed is not None and 0 < d.lds_bytes <= d.lds_limit                # the LDS path
    return d


def _big_tables():
    n_t, size = 48, 2050                                      # 48 x 2049 x 2 bytes: above a CU's LDS
    rng = np.random.default_rng(1)
    cdf = np.zeros((n_t, size), dtype=np.int32)
    for k in range(n_t):
        cdf[k, 1:-1] = np.sort(rng.choice(np.arange(1, 65536), size=size - 2, replace=False))
        cdf[k, -1] = 65536
    t = bs.Tables(cdf, np.full(n_t, size, dtype=np.int32), rng.integers(-1000, 0, n_t).astype(np.int32))
    big = bs.DeviceCoderTables.build(t, "cuda")
    assert big.packed is None and big.lds_bytes > big.lds_limit
    return big


class Pair:
    """The same streams received on the device and on the host.  The device's symbols and states sit inside larger
    buffers whose guard rows must stay untouched."""

    def __init__(self, idx, dt, K):
        self.idx, self.dt, self.K = idx, dt, K
        self.ns, self.n = idx.shape
        self.d_idx = torch.from_numpy(idx).cuda()
        self.guard = torch.full((self.ns + 2, self.n), FILL, dtype=torch.int32, device="cuda")
        self.sguard = torch.full((self.ns + 2, K), STATE_FILL, dtype=torch.int64, device="cuda")
        self.sguard[1:-1] = 0
        self.ck = bs.Checkpoints(self.sguard[1:-1], torch.zeros(self.ns, dtype=torch.int32, device="cuda"),
                                 torch.zeros(self.ns, dtype=torch.int32, device="cuda"))
        self.meta = torch.full((3, self.ns), -1, dtype=torch.int32, device="cuda")
        self.host = bs.Checkpoints.fresh(self.ns, K)
        self.h_out = np.full((self.ns, self.n), FILL, dtype=np.int32)
        self.pos = np.zeros(self.ns, dtype=np.int64)          # what the host knows from the last read of meta

    def device(self, prefixes, up=None):
        """One launch on the bytes from 4 * pos on; returns (available, status, symbols, done, pos, states)."""
        before, done_in = self.guard.cpu().numpy(), self.ck.done.cpu().numpy()
        up = bs.upload_streams([p[4 * int(q):] for p, q in zip(prefixes, self.pos)], "cuda") if up is None else up
        bs.resume_embedded_uploaded(up, 0, self.d_idx, self.guard[1:-1], self.dt, self.K, self.ck, self.meta)
        g, sg, m = self.guard.cpu().numpy(), self.sguard.cpu().numpy(), self.meta.cpu().numpy()
        assert (g[0] == FILL).all() and (g[-1] == FILL).all()                     # the guard rows around sym_out
        assert (sg[0] == np.int64(STATE_FILL)).all() and (sg[-1] == np.int64(STATE_FILL)).all()   # and around the states
        for s in range(self.ns):                              # nothing outside [done_in, available) is touched
            keep = np.ones(self.n, dtype=bool)
            keep[done_in[s]:max(m[0, s], done_in[s])] = False
            assert np.array_equal(g[1 + s][keep], before[1 + s][keep]), s
        assert np.array_equal(m[2], self.ck.pos.cpu().numpy())
        return m[0], m[1], g[1:-1], self.ck.done.cpu().numpy(), m[2], sg[1:-1].view(np.uint64)

    def both(self, prefixes, want_status=0):
        """A step on both sides and the one-shot kernel on the whole prefixes: everything agrees."""
        avail, status, out, done, pos, states = self.device(prefixes)
        st = np.full(self.ns, -1, dtype=np.int32)
        try:
            got = bs.resume_prefix_streams([(p[4 * int(self.host.pos[s]):], self.idx[s], self.h_out[s]) for s, p in enumerate(prefixes)],
                                           self.dt.host, self.host, lanes=self.K, status=st)
        except L.VamError:
            assert want_status
            got = None
        a1, s1, o1 = _device_prefix(prefixes, self.d_idx, self.dt, self.K)        # zeros beyond the count
        assert np.array_equal(avail, a1) and np.array_equal(status, s1) and np.array_equal(status, st)
        assert got is None or got == avail.tolist()
        for s in range(self.ns):
            assert np.array_equal(out[s][:avail[s]], o1[s][:avail[s]]) and (out[s][avail[s]:] == FILL).all(), s
            assert np.array_equal(out[s], self.h_out[s]), s
        assert np.array_equal(done, self.host.done) and np.array_equal(pos, self.host.pos)
        assert np.array_equal(states, self.host.states)
        assert (done == np.where(avail == self.n, self.n, avail // self.K * self.K)).all()
        self.pos[:] = pos
        return avail, status


def _chain(strings, idx, t, K, n):
    """Per stream the cuts 0, 4, 8K - 4, 8K, a length with L mod 4 = 3, the middle of a group, an exact group boundary, the
    end, and the end once more — each stream at its own groups."""
    rows = []
    for s, (string, i) in enumerate(zip(strings, idx)):
        g = (n // K) * (s + 1) // (len(strings) + 1)          # a group of this stream's own
        inside = min(n, g * K + max(K // 2, 1))
        boundary = min(n, (g + 1) * K)
        b_in, b_at = bs.prefix_bytes(string, i, sorted([inside, boundary]), t, lanes=K)
        odd = (8 * K + (b_in - 8 * K) // 2) | 3
        rows.append(sorted([0, 4, 8 * K - 4, 8 * K, odd, b_in, b_at]) + [len(string), len(string)])
        assert odd % 4 == 3 and b_in <= b_at <= len(string)
    return [list(step) for step in zip(*rows)]


@pytest.mark.parametrize("K", [1, 8, 64])
@pytest.mark.parametrize("n", [64, 1000])
def test_the_resume_kernel_equals_the_host_export_and_the_one_shot_kernel_step_by_step(dt, n, K):
    t = dt.host
    sym, idx = _flat(t, STREAMS, n, seed=n + K)
    strings = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(STREAMS)], t, lanes=K)
    pair = Pair(idx, dt, K)
    last = np.zeros(STREAMS, dtype=np.int64)
    for cuts in _chain(strings, idx, t, K, n):
        avail, status = pair.both([s[:c] for s, c in zip(strings, cuts)])
        assert (status == 0).all() and (avail >= last).all()
        last = avail
    assert (last == n).all() and np.array_equal(pair.h_out, sym)
    if K > 1 and n > K:
        assert (pair.pos > 2 * K).all()


def test_the_resume_kernel_reads_tables_too_large_for_lds_from_global_memory():
    big = _big_tables()
    t, K, n = big.host, 8, 1000
    sym, idx = _flat(t, STREAMS, n, seed=9)
    strings = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(STREAMS)], t, lanes=K)
    pair = Pair(idx, big, K)
    for cuts in _chain(strings, idx, t, K, n):
        avail, status = pair.both([s[:c] for s, c in zip(strings, cuts)])
        assert (status == 0).all()
    assert (avail == n).all() and np.array_equal(pair.h_out, sym)


@pytest.mark.parametrize("K", [1, 8, 64])
def test_a_bad_index_gives_status_2_at_the_one_shot_count(dt, K):
    t, n = dt.host, 1000
    sym, idx = _flat(t, STREAMS, n, seed=31 + K)
    strings = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(STREAMS)], t, lanes=K)
    bad = idx.copy()
    where = [0, 300, 517, 999]                                # stream 4 stays whole
    for s, (w, v) in enumerate(zip(where, (-1, t.cdf.shape[0], 1 << 30, -5))):
        bad[s, w] = v
    pair = Pair(bad, dt, K)
    for frac in (0.0, 0.25, 0.6, 1.0, 1.0):                   # before, around and after the bad elements; recomputed every call
        cuts = [min(len(s), int(len(s) * frac) | (3 if frac < 1 else 0)) for s in strings]
        avail, status = pair.both([s[:c] for s, c in zip(strings, cuts)], want_status=2)
    assert status.tolist() == [2, 2, 2, 2, 0] and avail[4] == n
    for s, w in enumerate(where):
        assert w // K * K <= avail[s] <= w


@pytest.mark.parametrize("K", [8, 64])
def test_refused_offsets_lengths_and_checkpoints_give_status_6_and_write_nothing(dt, K):
    t, n = dt.host, 1000
    sym, idx = _flat(t, STREAMS, n, seed=55 + K)
    strings = bs.encode_interleaved_streams([(sym[s], idx[s]) for s in range(STREAMS)], t, lanes=K)
    half = [s[:len(s) // 2 | 1] for s in strings]
    for what in ("offset", "negative offset", "length", "negative length", "done", "done > n", "pos", "negative pos"):
        pair = Pair(idx, dt, K)
        pair.both(half)
        done0, pos0 = pair.ck.done.cpu().numpy().copy(), pair.ck.pos.cpu().numpy().copy()
        states0, out0 = pair.sguard.cpu().numpy().copy(), pair.guard.cpu().numpy().copy()
        up = bs.upload_streams([s[4 * int(q):] for s, q in zip(strings, pair.pos)], "cuda")
        o = up.buf[:8 * STREAMS].view(torch.int64)
        ln = up.buf[8 * STREAMS:12 * STREAMS].view(torch.int32)
        if what == "offset":
            o[1] += 2
        elif what == "negative offset":
            o[1] = -4
        elif what == "length":
            ln[1] = 1 << 30
        elif what == "negative length":
            ln[1] = -1
        elif what == "done":
            pair.ck.done[1] += 3
        elif what == "done > n":
            pair.ck.done[1] = n + K
        elif what == "pos":
            pair.ck.pos[1] = 2 * K - 1
        else:
            pair.ck.pos[1] = -1
        refused = (pair.ck.done.cpu().numpy().copy(), pair.ck.pos.cpu().numpy().copy())
        avail, status, out, done, pos, states = pair.device(strings, up=up)
        assert (avail[1], status[1]) == (0, 6), what
        assert done[1] == refused[0][1] and pos[1] == refused[1][1]               # the checkpoint is left as it was handed in
        assert np.array_equal(out[1], out0[2]) and np.array_equal(pair.sguard.cpu().numpy()[2], states0[2]), what
        for s in (0, 2, 3, 4):                                # the other streams of the wave are decoded
            assert (avail[s], status[s], done[s]) == (n, 0, n) and np.array_equal(out[s], sym[s]), (what, s)
        assert 0 < done0[1] < n and pos0[1] >= 2 * K
    for lanes in (0, 3, 128):
        with pytest.raises(ValueError, match="power of two"):
            bs.resume_embedded_uploaded(up, 0, pair.d_idx, pair.guard[1:-1], dt, lanes, pair.ck, pair.meta)
    with pytest.raises(ValueError, match=r"meta is a contiguous int32 \[3, 5\]"):
        bs.resume_embedded_uploaded(up, 0, pair.d_idx, pair.guard[1:-1], dt, K, pair.ck, pair.meta[:2])
    with pytest.raises(ValueError, match="device checkpoints of 5 streams"):
        bs.resume_embedded_uploaded(up, 0, pair.d_idx, pair.guard[1:-1], dt, K, bs.Checkpoints.fresh(5, K), pair.meta)


# ----------------------------------------------------------------------------------------------- model
_CODED, _FULL = {}, {}
SHAPES = {"2x64x64": (2, 64, 64, 3), "1x128x192": (1, 128, 192, 4)}       # n = 512 and n = 3072 per slice


def _coded(shape, K):
    """(x, host-coded containers) per (shape, lanes), encoded once per session."""
    if (shape, K) not in _CODED:
        B, H, W, seed = SHAPES[shape]
        if shape not in _FULL:
            x = _x(B, H, W, seed=seed)
            with torch.no_grad():
                _FULL[shape] = (x, _net().forward_single_quality(x, 10))
        _CODED[shape, K] = EB.encode_batch(_net(), _FULL[shape][0], coder="host", lanes=K)
    return _FULL[shape][0], _CODED[shape, K]


def _steps(cs, K):
    """Per step the container every image holds: each image its own cuts, image 0 of a batch standing still once."""
    qs = cs[0]["marks"]["q"]
    m0, m1, m2 = qs[2], qs[6], qs[10]
    steps = [[EB.truncate(c, q=m0) for c in cs], [EB.truncate(c, q=m1) for c in cs], [EB.truncate(c, q=m2) for c in cs]]
    if len(cs) > 1:
        steps[1][0] = steps[0][0]                             # image 0 receives b"" in this step ...
        steps[2][1] = EB.truncate(cs[1], q=qs[8])             # ... and image 1 reaches another mark
    odd = []
    for b, c in enumerate(cs):
        at = [len(s) for s in steps[2][b]["embedded"]]
        cut = [min(len(s) - 1, a + (len(s) - a) * (j + 2 + b) // 14) | 1 for j, (s, a) in enumerate(zip(c["embedded"], at))]
        marked = {int(v) for row in c["marks"]["bytes"] for v in row}
        assert all(v % 4 and v not in marked and a <= v <= len(s) for v, a, s in zip(cut, at, c["embedded"]))
        odd.append(EB.truncate(c, slice_bytes=cut))
    return steps + [odd, list(cs)], m0


@pytest.mark.parametrize("shape,coder,K", [(s, c, K) for s in SHAPES for c in ("host", "device") for K in (1, 64)]
                         + [("2x64x64", "device", 8)])
def test_extend_leaves_the_decoder_a_fresh_one_on_the_concatenation(shape, coder, K):
    net = _net()
    x, cs = _coded(shape, K)
    B, ns = len(cs), net.ns0
    steps, q0 = _steps(cs, K)
    dec = EB.EmbeddedDecoder(net, steps[0], coder=coder, resumable=True)
    held = steps[0]
    for k, now in enumerate(steps):
        if k:
            more = [EB.delta(c, h) for c, h in zip(now, held)]
            if k == 1 and B > 1:
                assert more[0] == [b""] * ns
            got = dec.extend(more)
            assert np.array_equal(got, dec.available())
            if coder == "device":                             # the upload: the new bytes and at most one group per stream
                assert dec.extend_bytes <= sum(len(s) for row in more for s in row) + B * ns * (8 * K + 4), (k, dec.extend_bytes)
            held = now
        fresh = EB.EmbeddedDecoder(net, now, coder=coder)      # it uses the same plans: the next extend goes through _own()
        assert fresh.dp is dec.dp and dec.dp.owner is fresh
        assert [c["embedded"] for c in dec.containers] == [c["embedded"] for c in now]
        assert np.array_equal(dec.available(), fresh.available()), k
        a = dec.decode()
        assert dec.dp.owner is dec and _same(a, fresh.decode()), k
        for oa, ob in zip(dec.decode_qualities([q0, 0, 0.3]), fresh.decode_qualities([q0, 0, 0.3])):
            assert _same(oa, ob), k
        if k == 3:
            assert dec.bits(q0) == fresh.bits(q0)
    assert (dec.available() == net.dim_chunk * (x.shape[2] // 16) * (x.shape[3] // 16)).all()
    assert _same(dec.decode(), _FULL[shape][1])               # the whole stream: forward_single_quality(x, 10)
    assert all(len(t.runner.graphs) == 1 for t in dec.dp.tails.values())          # still one graph per group size


def test_the_device_extend_never_calls_the_host_coder(monkeypatch):
    net = _net()
    x, cs = _coded("2x64x64", 64)
    steps, q0 = _steps(cs, 64)
    with host_coder_forbidden(monkeypatch):
        monkeypatch.setattr(bs, "resume_prefix_streams", bs.decode_prefix_streams)      # refused like the others
        dec = EB.EmbeddedDecoder(net, steps[0], coder="device", resumable=True)
        for held, now in zip(steps, steps[1:]):
            dec.extend([EB.delta(c, h) for c, h in zip(now, held)])
        assert dec.idx_r is None                              # no ranked indexes came to the host
        out = dec.decode()
    assert _same(out, _FULL["2x64x64"][1])


@pytest.mark.parametrize("coder", ["host", "device"])
def test_a_scheduled_container_is_extended_stage_by_stage(coder):
    net = GS._net()
    x, S, cs = GS._coded(2, 64, 128, lanes=8)
    n_stages = len(cs[0]["marks"]["stage"])
    held = [EB.truncate(c, stage=0) for c in cs]
    dec = EB.EmbeddedDecoder(net, held, coder=coder, resumable=True)
    for k in range(n_stages):
        if k:
            now = [EB.truncate(c, stage=k) for c in cs]
            dec.extend([EB.delta(c, h) for c, h in zip(now, held)])
            held = now
        fresh = EB.EmbeddedDecoder(net, held, coder=coder)
        assert np.array_equal(dec.available(), fresh.available())
        assert _same(dec.decode_stages([k])[0], fresh.decode_stages([k])[0]), k
    assert all(len(t.runner.graphs) == 1 for t in dec.dp.tails.values())


@pytest.mark.parametrize("coder", ["host", "device"])
def test_a_status_in_extend_names_image_and_slice(coder):
    net = _net()
    x, cs = _coded("2x64x64", 8)
    held = [EB.truncate(c, q=1) for c in cs]
    dec = EB.EmbeddedDecoder(net, held, coder=coder, resumable=True)
    assert dec.available()[1, 3] < 504
    idx_r = dec.idx_r if coder == "host" else dec.dp.idx_r    # the ranked indexes the coder reads
    keep = int(idx_r[1, 3, 510])
    idx_r[1, 3, 510] = -1                                     # an element of the last group, not yet decoded
    try:
        with pytest.raises(L.VamError, match=r"EmbeddedDecoder: embedded stream \(image 1, slice 3\): .*out of range"):
            dec.extend([EB.delta(c, h) for c, h in zip(cs, held)])
    finally:
        idx_r[1, 3, 510] = keep
    assert np.array_equal(dec.extend([[b""] * net.ns0] * 2), EB.EmbeddedDecoder(net, cs, coder=coder).available())   # recomputed
    assert _same(dec.decode(), _FULL["2x64x64"][1])


def test_extend_refuses_a_decoder_without_checkpoints_and_malformed_arguments():
    net = _net()
    x, cs = _coded("2x64x64", 1)
    held = [EB.truncate(c, q=1) for c in cs]
    ns = net.ns0
    with pytest.raises(ValueError, match="resumable=True"):
        EB.EmbeddedDecoder(net, held).extend([[b""] * ns] * 2)
    dec = EB.EmbeddedDecoder(net, held, resumable=True)
    before = dec.available()
    for bad in ([[b""] * ns], [[b""] * ns] * 3, [[b""] * (ns - 1)] * 2, [[b""] * ns, [b""] * (ns - 1) + ["text"]],
                [[b""] * ns, [None] * ns], 5, [5, 6]):
        with pytest.raises(ValueError, match="EmbeddedDecoder.extend"):
            dec.extend(bad)
    assert np.array_equal(dec.available(), before) and [c["embedded"] for c in dec.containers] == [c["embedded"] for c in held]
    assert np.array_equal(dec.extend([[b""] * ns] * 2), before) and dec.extend_bytes < 2 * ns * (8 + 4)
