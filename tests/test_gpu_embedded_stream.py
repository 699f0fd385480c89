"""Embedded codestreams on the GPU (embedded.to_bytes / from_bytes / StreamDecoder): the decode of a
codestream and of its round ends against the forward passes, a StreamDecoder fed arbitrary cuts against a fresh
EmbeddedDecoder on from_bytes of the same prefix, chunked feeds, the use of a byte budget and mixed batches.  Model, inputs
and equality helpers are those of the existing embedded tests.  Every equality is bit-exact."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import embedded as EB                                                # noqa: E402
import test_gpu_embedded_base_lanes as BL                                        # noqa: E402
import test_gpu_embedded_schedule as GS                                          # noqa: E402
from test_gpu_embedded_base_lanes import _net, _same, host_coder_forbidden       # noqa: E402

LANES = [(1, 1), (8, 1), (64, 8)]
GRID = [(shape, coder, K, Kb) for shape in BL.SHAPES for coder in ("host", "device") for K, Kb in LANES]
_FORWARD, _SCHEDULED = {}, {}


def _streams(shape, K, Kb):
    """(x, containers, codestreams, layouts) per (shape, lanes, base_lanes); the containers are encoded once per session."""
    cs = BL._coded(shape, "host", K, Kb)
    data = [EB.to_bytes(c) for c in cs]
    return BL._input(shape), cs, data, [EB.layout(d) for d in data]


def _forward(shape, q):
    if (shape, q) not in _FORWARD:
        with torch.no_grad():
            _FORWARD[shape, q] = _net().forward_single_quality(BL._input(shape), q)
    return _FORWARD[shape, q]


def _forbidden(monkeypatch, coder):
    return host_coder_forbidden(monkeypatch) if coder == "device" else contextlib.nullcontext()


@pytest.mark.parametrize("shape,coder,K,Kb", GRID)
def test_the_codestream_and_its_round_ends_decode_to_the_forward_passes(shape, coder, K, Kb):
    net = _net()
    x, cs, data, lays = _streams(shape, K, Kb)
    back = [EB.from_bytes(d) for d in data]
    assert EB._same(back, cs)
    assert _same(EB.EmbeddedDecoder(net, back, coder=coder).decode(), EB.EmbeddedDecoder(net, cs, coder=coder).decode())
    assert _same(EB.EmbeddedDecoder(net, back, coder=coder).decode(), _forward(shape, 10))
    for k, q in enumerate(cs[0]["marks"]["q"]):
        cut = [EB.from_bytes(d[:lay["round_end"][k]]) for d, lay in zip(data, lays)]
        assert EB._same(cut, [EB.truncate(c, q=q) for c in cs])
        assert _same(EB.EmbeddedDecoder(net, cut, coder=coder).decode_qualities([q])[0], _forward(shape, q)), (k, q)


def _scheduled(Kb):
    """(x, two-stage schedule, containers) on the schedule fixtures: the region at 10 over background 0, then background 3.3."""
    if Kb not in _SCHEDULED:
        x = GS._x(2, 64, 128, seed=2)
        S = GS._schedule(2, 64, 128, roi=(10.0,), background=(0.0, 3.3))
        assert len(S) == 2
        _SCHEDULED[Kb] = (x, S, EB.encode_batch(_net(), x, schedule=S, lanes=8, base_lanes=Kb))
    return _SCHEDULED[Kb]


@pytest.mark.parametrize("coder", ["host", "device"])
@pytest.mark.parametrize("Kb", [1, 8])
def test_a_scheduled_codestream_ends_its_rounds_at_the_stages(coder, Kb):
    net = _net()
    x, S, cs = _scheduled(Kb)
    data = [EB.to_bytes(c) for c in cs]
    assert EB._same([EB.from_bytes(d) for d in data], cs) and cs[0]["format"] == ("embedded-4" if Kb > 1 else "embedded-3")
    dec = EB.StreamDecoder(net, 2, coder=coder)
    sent = [0, 0]
    for k in range(2):
        ends = [EB.layout(d)["round_end"][k] for d in data]
        cut = [EB.from_bytes(d[:e]) for d, e in zip(data, ends)]
        assert EB._same(cut, [EB.truncate(c, stage=k) for c in cs])
        with torch.no_grad():
            want = net.forward_quality_map(x, S[k])
        assert _same(EB.EmbeddedDecoder(net, cut, coder=coder).decode_stages([k])[0], want), k
        assert dec.feed([d[a:e] for d, a, e in zip(data, sent, ends)]) is not None
        sent = ends
        assert _same(dec.decode_stages([k])[0], want), k
    with pytest.raises(ValueError, match="decode_stages"):
        dec.decode_qualities([2.5])


def _chain(lay, b):
    """The cuts of image ``b``: one byte short of the need, the need, one byte of the body, a length = 3 mod 4 inside round
    1, the middle of a later round, a round end, the total — each image at rounds of its own."""
    ends, need = lay["round_end"], lay["base_end"]
    assert len(ends) >= 11
    r = next(k for k in range(1, 4) if ends[k] - ends[k - 1] >= 8)              # round 1, unless it cannot hold such a length
    odd = (ends[r - 1] + (ends[r] - ends[r - 1]) // 2) | 3
    later = 4 + 3 * b
    mid = (ends[later] + ends[later + 1]) // 2
    chain = [need - 1, need, need + 1, odd, mid, ends[8 + b], lay["total"]]
    assert odd % 4 == 3 and ends[r - 1] < odd < ends[r] and ends[later] <= mid <= ends[later + 1] and chain == sorted(chain)
    return chain


@pytest.mark.parametrize("shape,coder,K,Kb", GRID)
def test_a_stream_decoder_fed_arbitrary_cuts_equals_a_fresh_decoder_on_the_prefix(monkeypatch, shape, coder, K, Kb):
    net = _net()
    x, cs, data, lays = _streams(shape, K, Kb)
    B, ns = len(cs), net.ns0
    steps = list(zip(*[_chain(lay, b) for b, lay in enumerate(lays)]))           # [step][image]
    with _forbidden(monkeypatch, coder):
        dec = EB.StreamDecoder(net, B, coder=coder)
        sent, handed = [0] * B, 0
        for i, cuts in enumerate(steps):
            got = dec.feed([d[a:n] for d, a, n in zip(data, sent, cuts)])
            sent = list(cuts)
            handed += dec.extend_bytes
            if i == 0:
                assert got is None and not dec.ready and dec.need() == [1] * B and dec.available() is None
                with pytest.raises(ValueError, match="nothing to decode yet: image 0 lacks 1 bytes"):
                    dec.decode()
                continue
            assert dec.ready and dec.need() == [0] * B and np.array_equal(got, dec.available())
            prefix = [EB.from_bytes(d[:n]) for d, n in zip(data, cuts)]
            assert sum(len(s) for c in prefix for s in c["embedded"]) == sum(n - lay["base_end"] for n, lay in zip(cuts, lays))
            fresh = EB.EmbeddedDecoder(net, prefix, coder=coder)                   # on the same plans: the next feed goes through _own()
            assert EB._same(dec.decoder.containers, prefix), i
            assert np.array_equal(dec.available(), fresh.available()), i
            a = dec.decode()
            assert _same(a, fresh.decode()), i
            body = sum(n - lay["base_end"] for n, lay in zip(cuts, lays))
            assert handed <= body + i * B * ns * (8 * K + 4), (i, handed, body)    # the new bytes and one group's tail per stream and step
        assert _same(dec.decode(), _forward(shape, 10))
        if coder == "device":
            assert dec.decoder.idx_r is None                                      # no ranked indexes came to the host
    assert (dec.available() == 32 * (x.shape[2] // 16) * (x.shape[3] // 16)).all()


@pytest.mark.parametrize("coder", ["host", "device"])
@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_chunked_feeds_end_in_the_state_of_one_feed(coder, chunk):
    """The whole codestream of both images at every chunk size: through preamble, header, z and base, every round, the last
    round after the final mark and the end of the stream.  Every feed past the base that brings a body byte is a resume
    call."""
    import time
    net = _net()
    x, cs, data, lays = _streams("2x64x64", 8, 1)
    upto = [lay["total"] for lay in lays]
    one = EB.StreamDecoder(net, 2, coder=coder)
    want_avail = one.feed(data)
    want = one.decode()
    dec = EB.StreamDecoder(net, 2, coder=coder)
    t0, handed = time.perf_counter(), 0
    for at in range(0, max(upto), chunk):
        got = dec.feed([d[min(at, n):min(at + chunk, n)] for d, n in zip(data, upto)])
        handed += dec.extend_bytes
        assert (got is None) == any(min(at + chunk, n) < lay["base_end"] for n, lay in zip(upto, lays))
    torch.cuda.synchronize()
    feeds = -(-max(upto) // chunk)
    print(f"chunked feeds: coder {coder}, chunk {chunk}: {feeds} feeds of totals {upto} in {time.perf_counter() - t0:.2f} s")
    assert handed <= sum(n - lay["base_end"] for n, lay in zip(upto, lays)) + feeds * 2 * net.ns0 * (8 * 8 + 4)
    assert (dec.available() == 512).all() and _same(dec.decode(), _forward("2x64x64", 10))
    assert np.array_equal(dec.available(), want_avail) and _same(dec.decode(), want)
    assert EB._same(dec.decoder.containers, one.decoder.containers)
    assert EB._same(dec.decoder.containers, [EB.from_bytes(d[:n]) for d, n in zip(data, upto)])


@pytest.mark.parametrize("coder", ["host", "device"])
def test_a_byte_budget_between_two_round_ends_is_used(coder):
    """truncate(max_bytes=n) counts z, base and embedded bytes and not the codestream's header, so the budget is taken more
    than a header's length below the next round end: truncate then stops at mark k, the codestream goes on into round k + 1."""
    net = _net()
    x = BL._input("1x128x192")
    c, = EB.encode_batch(net, x, marks=[0.05, 2.5, 6.6], coder="host", lanes=8)
    data = EB.to_bytes(c)
    lay = EB.layout(data)
    ends = lay["round_end"]
    k = 0 if ends[1] - ends[0] >= ends[2] - ends[1] else 1
    assert ends[k + 1] - ends[k] > lay["header_end"] + 64
    n = ends[k] + (ends[k + 1] - ends[k] - lay["header_end"]) // 2
    cut = EB.truncate(c, max_bytes=n)
    assert [len(s) for s in cut["embedded"]] == c["marks"]["bytes"][k] and ends[k] < n < ends[k + 1]
    dec = EB.StreamDecoder(net, 1, coder=coder)
    got = dec.feed([data[:n]])
    marked = EB.EmbeddedDecoder(net, [cut], coder=coder).available()
    assert (got >= marked).all() and (got > marked).any()
    assert sum(len(s) for s in dec.decoder.containers[0]["embedded"]) == n - lay["base_end"] > sum(c["marks"]["bytes"][k])


def test_a_mixed_batch_is_refused_when_the_second_header_is_complete():
    net = _net()
    k1, k8 = EB.to_bytes(BL._coded("2x64x64", "host", 1, 1)[0]), EB.to_bytes(BL._coded("2x64x64", "host", 8, 1)[1])
    x, S, sched = _scheduled(1)
    plain = EB.to_bytes(EB.encode_batch(net, x, marks=[0.5, 2.5], lanes=8)[0])
    for first, second, why in ((k1, k8, "its lanes is 8, the others' 1"), (plain, EB.to_bytes(sched[1]), "it is scheduled, the others are plain")):
        for coder in ("host", "device"):
            dec = EB.StreamDecoder(net, 2, coder=coder)
            end = EB.layout(second)["header_end"]
            assert dec.feed([first, second[:end - 1]]) is None
            with pytest.raises(ValueError, match=f"image 1 does not belong to this batch: {why}; decode it separately"):
                dec.feed([b"", second[end - 1:]])
            assert not dec.ready and dec.need()[1] == 1


def test_embedded_stream_rd_reports_the_budgets_and_the_slack():
    from vampic import evaluate as EV
    net, x = _net(), BL._input("2x64x64")
    cs = BL._coded("2x64x64", "host", 8, 1)
    data = [EB.to_bytes(c) for c in cs]
    lo, hi = max(EB.need_bytes(d) for d in data), max(len(d) for d in data)
    budgets = [lo + (hi - lo) * i // 3 for i in range(4)]
    rows = EV.embedded_stream_rd(net, [x[0], x[1]], budgets, coder="device", lanes=8)
    assert [r["budget"] for r in rows] == budgets
    for r in rows:
        assert r["bytes"] == [min(r["budget"], len(d)) for d in data] and r["bpp"] == [8.0 * v / (64 * 64) for v in r["bytes"]]
        cut = [EB.truncate(c, max_bytes=r["budget"]) for c in cs]
        assert r["truncate_bytes"] == [sum(EB.container_bytes(c)) for c in cut]
        assert r["unused"] == [r["budget"] - v for v in r["truncate_bytes"]] and min(r["unused"]) >= 0
        assert all(np.isfinite(v) for v in r["psnr"] + r["truncate_psnr"])
    assert all(a["bytes"] <= b["bytes"] for a, b in zip(rows, rows[1:]))
    with pytest.raises(ValueError, match="ascending"):
        EV.embedded_stream_rd(net, [x[0]], budgets[::-1])
    with pytest.raises(ValueError, match="bytes are needed"):
        EV.embedded_stream_rd(net, [x[0]], [lo // 2])
