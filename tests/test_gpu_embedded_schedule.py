"""Scheduled embedded streams on the GPU (embedded.encode_batch(schedule=...) / truncate(stage=...) /
EmbeddedDecoder.decode_stages): vam_stage_ids and vam_variance_rank_staged against the numpy contracts of
tests/test_embedded_schedule_cpu.py, prefix = quality-map mask, bit-identity to the plain embedded format, and on models
every stage against forward_quality_map, cuts, both coders and lanes, graph replay and the refusals.  Every equality is
bit-exact."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_embedded_cpu as EC                        # noqa: E402  (the numpy contracts of section 9m)
import test_embedded_schedule_cpu as SC               # noqa: E402  (the numpy contracts of section 9r)
import vampic                                         # noqa: E402
import vampic.synth as synth                          # noqa: E402
from vampic import _lib as L, embedded as EB, evaluate as EV, ops   # noqa: E402

README_ARGS = dict(N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True, dim_chunk=32,
                   division_dimension=[320, 640], mask_policy="point-based-std", support_progressive_slices=5, delta_encode=True,
                   total_mu_rep=True, all_scalable=True)
NS, C = 10, 32
_NETS, _SIGMAS, _CODED = {}, {}, {}


def _net(kind="pic", **over):
    key = (kind,) + tuple(sorted(over.items()))
    if key not in _NETS:
        a = dict(README_ARGS, **over)
        if kind == "rem":
            a.update(check_levels=[0.01, 0.25, 1.75], mu_std=True, dimension="big")
        net = vampic.get_model(argparse.Namespace(model=kind, **a), "cpu").eval()
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
        net = net.cuda()
        net.update()
        _NETS[key] = net
    return _NETS[key]


def _x(B, H, W, seed=3):
    return synth.synth_image(B, H, W, seed=seed).cuda()


def _sigma(h, w, B):
    """(NCHW host tensor, NHWC device view) of a progressive-sigma-like input of 10 slices x 32 channels: slice 3 constant,
    slice 7 of image 0 holds a NaN, slice 9 heavy ties (so ties straddle every stage boundary), slice 5 holds +inf, -0.0
    and +0.0.  Computed once per shape and left unchanged."""
    if (h, w, B) not in _SIGMAS:
        g = torch.Generator().manual_seed(h * w)
        s = torch.rand((B, 320, h, w), generator=g) * 4 + 0.05
        s[:, 3 * 32:4 * 32] = 1.25
        s[0, 7 * 32 + 5, 1, 2] = float("nan")
        s[:, 9 * 32:10 * 32] = torch.round(s[:, 9 * 32:10 * 32] * 2) / 2
        s[B - 1, 5 * 32 + 2, 0, 1] = float("inf")
        s[:, 5 * 32 + 3, 0, :3] = -0.0
        s[:, 5 * 32 + 1, 2, 1:4] = 0.0
        s[0, 5 * 32 + 30, 3, 3] = -0.0
        _SIGMAS[(h, w, B)] = (s, ops.from_nchw(s.cuda()))
    return _SIGMAS[(h, w, B)]


def _segments(t):
    """[B, NS * C, h, w] -> [B, NS, n] in the canonical [C, h, w] order of a stream."""
    return t.reshape(t.shape[0], NS, -1)


def _nhwc_segments(t):
    """uint8 / float [B, h, w, NS * C] -> [B, NS, n] canonical."""
    return _segments(t.permute(0, 3, 1, 2).contiguous())


def _staged(sg, levels, index, n_stages=None):
    """(layer ids, stage ids, perm, table) of the device path for check_schedule's (levels, index) on the view ``sg``."""
    B, h, w = sg.B, sg.H, sg.W
    table, stage_map, ns_dev = EB.schedule_buffers(B, h * w, "cuda")
    EB.fill_schedule(table, stage_map, ns_dev, levels, index, h * w, C)
    if n_stages is not None:
        ns_dev.copy_(torch.tensor(n_stages, dtype=torch.int32))
    layer = torch.full((B, h, w, NS * C), 0x77, dtype=torch.uint8, device="cuda")
    stage = torch.full_like(layer, 0x55)
    perm = torch.full((B, NS, C * h * w), -7, dtype=torch.int32, device="cuda")
    ops.variance_layers_table(sg, table, layer, n_slice=NS)
    ops.stage_ids(layer, stage_map, ns_dev, stage)
    ops.variance_rank_staged(sg, stage, perm, n_slice=NS, workspace=ops.rank_workspace(sg, NS))
    return layer, stage, perm, table


VALUES32 = np.concatenate([[0.0], np.linspace(0.05, 9.9, 29), [10.0, 12.0]])       # 32 distinct, with 0 and >= 10


def _schedule32(B, h, w, seed):
    """32 stages of random monotone maps over 32 distinct values; position (0, 0) of every image climbs through all of them."""
    S = SC.random_schedule(np.random.default_rng(seed), B, 32, h, w, VALUES32)
    S[:, :, 0, 0] = VALUES32[:, None]
    return S


def _check_contract(s, layer, stage, perm, index, n_stages=None):
    B, n_pix = s.shape[0], s.shape[2] * s.shape[3]
    seg, lay, st, perm = _segments(s).numpy(), _nhwc_segments(layer).cpu().numpy(), _nhwc_segments(stage).cpu().numpy(), perm.cpu().numpy()
    for b in range(B):
        live = n_stages is None or 1 <= n_stages[b] <= 32
        for j in range(NS):
            want = SC.stage_ids(lay[b, j], index[b], n_pix) if live else np.full(lay[b, j].size, 0xFF, dtype=np.uint8)
            assert np.array_equal(st[b, j], want), (b, j)
            assert np.array_equal(perm[b, j], SC.scheduled_order(seg[b, j], want)), (b, j)
            if not live:
                assert np.array_equal(perm[b, j], EC.rank_order(seg[b, j])), (b, j)        # no stage: the plain order


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("hw, B", [((4, 8), 2), ((8, 12), 2), ((16, 24), 2), ((64, 128), 1)])
def test_stage_and_staged_rank_kernels_equal_the_numpy_contract(hw, B):
    """n = 1024 (LDS), 3072 (LDS, no power of two), 12288 (workspace, padded to 16384), 2^18 (the limit: e takes all 18
    bits under the 24-bit field).  32 stages over 32 distinct values; the segments hold a constant slice, ties across the
    stage boundaries, a NaN, +inf and both zeros."""
    h, w = hw
    s, sg = _sigma(h, w, B)
    n = C * h * w
    assert (ops.rank_workspace(sg, NS) is None) == (n <= 8192)
    S = _schedule32(B, h, w, seed=n)
    levels, index = EB.check_schedule(S, B, h, w)
    assert all(lv.size == 32 for lv in levels) and index.shape[1] == 32
    layer, stage, perm, _ = _staged(sg, levels, index)
    _check_contract(s, layer, stage, perm, index)
    st = _nhwc_segments(stage)
    assert (st[0, 7] == 0xFF).sum() > 0 and (st[0, 7] != 0xFF).sum() > 0        # the NaN segment: only its q >= 10 positions
    count = torch.empty((32, B, NS), dtype=torch.int32, device="cuda")
    ops.rank_counts(stage, perm, NS, 32, count)
    want = torch.stack([(st <= k).sum(-1) for k in range(32)])
    assert torch.equal(count.long(), want.long())


@pytest.mark.parametrize("hw", [(4, 8), (16, 24)])
def test_bad_stage_count_gives_no_stage_and_the_plain_order(hw):
    h, w = hw
    s, sg = _sigma(h, w, 2)
    S = SC.random_schedule(np.random.default_rng(5), 2, 3, h, w, [0, 0.5, 2.5, 10])
    levels, index = EB.check_schedule(S, 2, h, w)
    for bad in (0, 33, -1):
        layer, stage, perm, _ = _staged(sg, levels, index, n_stages=[3, bad])
        assert (stage[1] == 0xFF).all() and (stage[0] != 0xFF).any()
        _check_contract(s, layer, stage, perm, index, n_stages=[3, bad])


@pytest.mark.parametrize("hw", [(16, 16), (16, 24)])
def test_prefix_of_the_scheduled_order_is_the_map_mask(hw):
    h, w = hw
    s, sg = _sigma(h, w, 2)
    n = C * h * w
    S = SC.random_schedule(np.random.default_rng(h * w), 2, 6, h, w, [0, 0, 0.05, 0.5, 2.5, 7, 9.99, 10, 11])
    S[4] = S[3]                                                                 # an empty increment
    levels, index = EB.check_schedule(S, 2, h, w)
    layer, stage, perm, table = _staged(sg, levels, index)
    count = torch.empty((6, 2, NS), dtype=torch.int32, device="cuda")
    ops.rank_counts(stage, perm, NS, 6, count)
    mask = ops.new_view(2, h, w, 320, "cuda")
    r = torch.arange(n, device="cuda")
    for k in range(6):
        ops.variance_mask_map(sg, table, torch.from_numpy(np.ascontiguousarray(index[:, k])).cuda(), mask, n_slice=NS)
        m = _nhwc_segments(mask.buf)
        assert torch.equal(count[k].long(), m.sum(-1).long()), k
        ranked = torch.gather(m, 2, perm.long())                                # the mask along the scheduled order
        assert torch.equal(ranked == 1, r[None, None, :] < count[k][..., None]), k
    assert torch.equal(count[4], count[3]) and (count[1:] >= count[:-1]).all()


def test_constant_maps_give_the_plain_order_and_the_plain_kernel_is_unchanged():
    h, w = 8, 12
    s, sg = _sigma(h, w, 2)
    plain = torch.full((2, NS, C * h * w), -7, dtype=torch.int32, device="cuda")
    ops.variance_rank(sg, plain, n_slice=NS, workspace=ops.rank_workspace(sg, NS))
    seg = _segments(s).numpy()
    want = np.stack([np.stack([EC.rank_order(seg[b, j]) for j in range(NS)]) for b in range(2)])
    assert np.array_equal(plain.cpu().numpy(), want)                            # vam_variance_rank: its order as before
    qs = [0.05, 0.5, 2.5, 10]
    levels, index = EB.check_schedule([np.full((2, h, w), q) for q in qs], 2, h, w)
    layer, stage, perm, _ = _staged(sg, levels, index)
    assert torch.equal(perm, plain)
    ref = torch.empty_like(layer)
    ops.variance_layers(sg, qs, ref, n_slice=NS)
    assert torch.equal(layer, ref) and torch.equal(stage, ref)                  # constant maps: stage = layer


# ------------------------------------------------------------------------------------------------ models
def _boxes(B, H, W):
    """One box per image, each its own, none aligned to the 16-pixel grid."""
    return [(b, H // 4 + 3 * b, W // 4 - 5 * b, H // 2 + 9, W // 2 + 21 + 7 * b) for b in range(B)]


def _schedule(B, H, W, roi=(2.5, 10.0), background=(0.0, 0.5, 3.3)):
    return EV.roi_schedule(B, H, W, _boxes(B, H, W), roi, background)


def _coded(B, H, W, seed=2, coder="host", lanes=1):
    """(x, schedule, containers) of one input, encoded once per session."""
    key = (B, H, W, seed, coder, lanes)
    if key not in _CODED:
        x = _x(B, H, W, seed=seed)
        S = _schedule(B, H, W)
        _CODED[key] = (x, S, EB.encode_batch(_net(), x, schedule=S, coder=coder, lanes=lanes))
    return _CODED[key]


def _same(a, b):
    return torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"])


@pytest.mark.parametrize("shape", [(2, 64, 128), (1, 256, 320)])
def test_every_stage_equals_forward_quality_map(shape):
    """4 x 8 latents (LDS) and 16 x 20 (n = 10240: workspace)."""
    net = _net()
    B, H, W = shape
    x, S, cs = _coded(B, H, W)
    h, w = H // 16, W // 16
    n = C * h * w
    assert len(cs) == B and len(S) == 4
    for b, c in enumerate(cs):
        assert set(c) == {"format", "lanes", "shape", "z", "base", "embedded", "marks", "schedule", "side_bytes"}
        assert c["format"] == "embedded-3" and c["lanes"] == 1 and c["marks"]["stage"] == [0, 1, 2, 3] and "q" not in c["marks"]
        ix = c["schedule"]["index"]
        assert ix.dtype == np.uint8 and ix.shape == (4, h, w)
        assert np.array_equal(np.asarray(c["schedule"]["levels"])[ix], np.stack([m[b].numpy() for m in S]))
        assert c["side_bytes"] == 8 * len(c["schedule"]["levels"]) + 4 * h * w
        assert np.asarray(c["marks"]["count"]).shape == np.asarray(c["marks"]["bytes"]).shape == (4, NS)
        assert c["marks"]["count"][3] != [n] * NS                               # the last stage is not the whole stream
    dec = EB.EmbeddedDecoder(net, cs)
    assert dec.scheduled and dec.n_stages == 4 and (dec.available() == n).all()
    with torch.no_grad():
        fw = [net.forward_quality_map(x, m) for m in S]
        assert _same(dec.decode(), net.forward_single_quality(x, 10))           # the whole stream holds every element once
    for k in range(4):
        assert _same(dec.decode_stages([k])[0], fw[k]), k
    outs = dec.decode_stages([2, 0, 3, 0])                                      # any stages in any order
    assert all(_same(o, fw[k]) for o, k in zip(outs, [2, 0, 3, 0]))
    # the marks are the sizes of forward_quality_map's masks
    for k in range(4):
        want = _segments(fw[k]["mask"]).sum(-1).long().tolist()
        assert [c["marks"]["count"][k] for c in cs] == want, k
    # background 0 (stages 0 and 1): every element decoded lies at a region position
    perm = dec.dp.perm.cpu().numpy()
    for k in (0, 1):
        for b, c in enumerate(cs):
            region = (S[k][b] > 0).numpy().reshape(-1)
            assert 0 < region.sum() < region.size
            for j in range(NS):
                p = perm[b, j, :c["marks"]["count"][k][j]] % (h * w)
                assert region[p].all(), (k, b, j)


def test_image_alone_equals_image_in_the_batch():
    net = _net()
    x, S, cs = _coded(2, 64, 128)
    got = EB.EmbeddedDecoder(net, cs).decode_stages([1])[0]
    for b in range(2):
        one = EB.encode_batch(net, x[b:b + 1], schedule=[m[b:b + 1] for m in S])
        assert set(one[0]) == set(cs[b])
        for key in set(cs[b]) - {"schedule"}:
            assert one[0][key] == cs[b][key], key
        assert np.array_equal(one[0]["schedule"]["index"], cs[b]["schedule"]["index"])
        o = EB.EmbeddedDecoder(net, one).decode_stages([1])[0]
        assert torch.equal(o["x_hat"][0], got["x_hat"][b]) and torch.equal(o["y_hat"][0], got["y_hat"][b]), b


def test_constant_schedule_is_the_plain_container_byte_for_byte():
    net = _net()
    x = _x(2, 64, 128, seed=2)
    qs = [0.05, 0.5, 2.5, 10]
    plain = EB.encode_batch(net, x, marks=qs)
    sched = EB.encode_batch(net, x, schedule=[torch.full((2, 4, 8), q) for q in qs])
    for a, b in zip(plain, sched):
        assert a["format"] == "embedded-1" and b["format"] == "embedded-3"
        assert a["z"] == b["z"] and a["base"] == b["base"] and a["embedded"] == b["embedded"]
        assert a["marks"]["count"] == b["marks"]["count"] and a["marks"]["bytes"] == b["marks"]["bytes"]
    dp, ds = EB.EmbeddedDecoder(net, plain), EB.EmbeddedDecoder(net, sched)
    assert dp.dp is not ds.dp
    perm_plain = dp.dp.perm.clone()
    ds._own()
    assert torch.equal(ds.dp.perm, perm_plain)
    assert all(_same(a, b) for a, b in zip(dp.decode_qualities(qs), ds.decode_stages(range(4))))


def test_truncate_at_a_stage_then_decode():
    net = _net()
    x, S, cs = _coded(2, 64, 128)
    cut = [EB.truncate(c, stage=1) for c in cs]
    assert all(sum(EB.container_bytes(a)) < sum(EB.container_bytes(b)) for a, b in zip(cut, cs))
    assert [[len(s) for s in c["embedded"]] for c in cut] == [c["marks"]["bytes"][1] for c in cs]
    dec = EB.EmbeddedDecoder(net, cut)
    assert (dec.available() >= np.asarray([c["marks"]["count"][1] for c in cut])).all() and (dec.available() < C * 32).any()
    with torch.no_grad():
        for k in (0, 1):
            assert _same(dec.decode_stages([k])[0], net.forward_quality_map(x, S[k])), k
    with pytest.raises(ValueError, match=r"stage 2 needs \d+ elements of slice \d+ of image \d+, its container holds \d+"):
        dec.decode_stages([2])
    budget = [sum(EB.container_bytes(c)) + c["side_bytes"] for c in cut]
    again = [EB.truncate(c, max_bytes=v) for c, v in zip(cs, budget)]           # the budget of stage 1 buys stage 1
    assert [c["embedded"] for c in again] == [c["embedded"] for c in cut]


def test_cut_at_any_byte():
    """Every slice of image 0 cut at its own odd length, one to 0 bytes and one left whole; image 1 cut at a stage.  The
    quantised residual r_hat = symbol * present + mu is elementwise: it equals the full decode's where the scheduled rank
    is below `available` and the all-cut decode's (mu) elsewhere."""
    net = _net()
    x, S, cs = _coded(2, 64, 128)
    n = C * 4 * 8
    lens = [len(s) for s in cs[0]["embedded"]]
    cut = [max(9, ln * (j + 1) // 12) | 1 for j, ln in enumerate(lens)]
    cut[4], cut[8] = 0, lens[8] + 3
    c0, c1 = EB.truncate(cs[0], slice_bytes=cut), EB.truncate(cs[1], stage=0)
    dec = EB.EmbeddedDecoder(net, [c0, c1])
    avail = dec.available()
    assert avail[0, 4] == 0 and avail[0, 8] == n and (avail[0] < n).sum() == NS - 1
    assert (avail[1] >= np.asarray(cs[1]["marks"]["count"][0])).all()
    dec.decode()
    rq = dec.dp.tails[1].rq.buf.permute(0, 3, 1, 2).clone()
    perm = dec.dp.perm.long().clone()
    full_dec = EB.EmbeddedDecoder(net, cs)
    full_dec.decode()
    rq_full = full_dec.dp.tails[1].rq.buf.permute(0, 3, 1, 2).clone()
    assert torch.equal(full_dec.dp.perm.long(), perm)                           # the order does not depend on the cut
    none_dec = EB.EmbeddedDecoder(net, [EB.truncate(c, slice_bytes=[0] * NS) for c in cs])
    assert (none_dec.available() == 0).all()
    none_dec.decode()
    rq_none = none_dec.dp.tails[1].rq.buf.permute(0, 3, 1, 2).clone()
    rank = torch.empty_like(perm)
    rank.scatter_(2, perm, torch.arange(n, device="cuda").expand_as(perm).contiguous())
    present = rank < torch.from_numpy(avail).cuda()[..., None]
    assert torch.equal(_segments(rq), torch.where(present, _segments(rq_full), _segments(rq_none)))
    assert not torch.equal(rq_full, rq_none)


@pytest.mark.parametrize("lanes", [1, 8])
def test_both_coders_and_lanes(lanes):
    net = _net()
    x, S, host = _coded(2, 64, 128, coder="host", lanes=lanes)
    _, _, device = _coded(2, 64, 128, coder="device", lanes=lanes)
    one = _coded(2, 64, 128)[2]
    for a, b, c1 in zip(host, device, one):
        assert a["format"] == "embedded-3" and a["lanes"] == lanes
        assert set(a) == set(b)
        for key in set(a) - {"schedule"}:
            assert a[key] == b[key], key
        assert np.array_equal(a["schedule"]["index"], b["schedule"]["index"]) and a["schedule"]["levels"] == b["schedule"]["levels"]
        assert a["z"] == c1["z"] and a["base"] == c1["base"] and a["marks"]["count"] == c1["marks"]["count"]
        assert (a["embedded"] == c1["embedded"]) == (lanes == 1)
    with torch.no_grad():
        fw = net.forward_quality_map(x, S[1])
    cut = [EB.truncate(c, stage=2) for c in host]
    for coder in ("host", "device"):                                            # either decoder reads either's containers
        assert _same(EB.EmbeddedDecoder(net, device if coder == "host" else host, coder=coder).decode_stages([1])[0], fw), coder
        dec = EB.EmbeddedDecoder(net, cut, coder=coder)
        assert _same(dec.decode_stages([1])[0], fw), coder
        with pytest.raises(ValueError, match="stage 3 needs"):
            dec.decode_stages([3])


def test_one_graph_per_group_size_across_schedules_and_cuts():
    net = _net()
    assert net.use_graph
    x, S, cs = _coded(2, 64, 128)
    S2 = _schedule(2, 64, 128, roi=(1.0, 7.0), background=(0.0, 0.05, 7.0))     # another schedule, the same stage count
    cs2 = EB.encode_batch(net, x, schedule=S2)
    dec = EB.EmbeddedDecoder(net, cs)
    a = dec.decode_stages([0, 2])
    dec2 = EB.EmbeddedDecoder(net, cs2)                                         # another schedule on the same plans
    b = dec2.decode_stages([1, 3])
    c = dec2.decode()
    d = EB.EmbeddedDecoder(net, [EB.truncate(c_, stage=1) for c_ in cs])
    e = d.decode_stages([1])[0]
    a2 = dec.decode_stages([0, 2])                                              # the first one again after the plans served others
    assert dec.dp is dec2.dp is d.dp and {1, 2} <= set(dec.dp.tails)
    assert all(len(t.runner.graphs) == 1 for t in dec.dp.tails.values())
    key = [k for k, p in net._dec_plans.items() if p is dec.dp]
    assert len(key) == 1 and "scheduled" in key[0] and all(isinstance(v, (str, int)) for v in key[0])   # no schedule in the key
    with torch.no_grad():
        want = [net.forward_quality_map(x, S[0]), net.forward_quality_map(x, S[2]), net.forward_quality_map(x, S2[1]),
                net.forward_quality_map(x, S2[3]), net.forward_single_quality(x, 10), net.forward_quality_map(x, S[1]),
                net.forward_quality_map(x, S[0]), net.forward_quality_map(x, S[2])]
    for i, (o, r) in enumerate(zip(a + b + [c, e] + a2, want)):
        assert _same(o, r), i


def test_more_than_eight_stages_split_into_groups():
    net = _net()
    x = _x(2, 64, 128, seed=2)
    S = EV.roi_schedule(2, 64, 128, _boxes(2, 64, 128), [0.5, 1, 2.5, 5, 10], [0, 0.05, 0.5, 1, 2.5, 5, 10])    # 11 stages
    dec = EB.EmbeddedDecoder(net, EB.encode_batch(net, x, schedule=S))
    order = [10, 0, 5, 3, 9, 1, 7, 2, 8, 4, 6]
    outs = dec.decode_stages(order)
    with torch.no_grad():
        for k, o in zip(order, outs):
            assert _same(o, net.forward_quality_map(x, S[k])), k


def test_refusals(monkeypatch):
    net = _net()
    x1 = _x(1, 64, 64)
    x, S, cs = _coded(2, 64, 128)
    S1 = _schedule(1, 64, 64)
    with pytest.raises(ValueError, match="marks or schedule"):
        EB.encode_batch(net, x, marks=[1, 2], schedule=S)
    with pytest.raises(ValueError, match="lowers the quality"):
        EB.encode_batch(net, x, schedule=S[::-1])
    with pytest.raises(ValueError, match="shape"):
        EB.encode_batch(net, x, schedule=S1)
    plain = EB.encode_batch(net, x, marks=[0.5, 2.5])
    with pytest.raises(ValueError, match="scheduled .* or plain containers, not both"):
        EB.EmbeddedDecoder(net, [cs[0], plain[1]])
    five = EB.encode_batch(net, x[1:], schedule=[m[1:] for m in S] + [torch.full((1, 4, 8), 10.0)])
    with pytest.raises(ValueError, match="same number of stages"):
        EB.EmbeddedDecoder(net, [cs[0], five[0]])
    dec = EB.EmbeddedDecoder(net, cs)
    with pytest.raises(ValueError, match="decode_stages"):
        dec.decode_qualities([2.5])
    with pytest.raises(ValueError, match="decode_stages"):
        dec.bits(2.5)
    for bad in ([], [4], [-1], [1.5]):
        with pytest.raises(ValueError, match=r"stages must be integers in 0\.\.3"):
            dec.decode_stages(bad)
    with pytest.raises(ValueError, match="decode_qualities"):
        EB.EmbeddedDecoder(net, plain).decode_stages([0])
    with pytest.raises(ValueError, match="stage="):
        EB.truncate(cs[0], q=2.5)
    # section 9m's model refusals
    with pytest.raises(NotImplementedError, match="eager harness"):
        EB.encode_batch(_net("rem"), x1, schedule=S1)
    with pytest.raises(NotImplementedError, match="eager harness"):
        EB.EmbeddedDecoder(_net("rem"), cs)
    for over in (dict(all_scalable=False), dict(delta_encode=False)):
        with pytest.raises(NotImplementedError, match="all_scalable=True"):
            EB.encode_batch(_net(**over), x1, schedule=S1)
        with pytest.raises(NotImplementedError, match="all_scalable=True"):
            EB.EmbeddedDecoder(_net(**over), cs)
    with pytest.raises(NotImplementedError, match="up to 262144"):
        EB.encode_batch(net, torch.zeros((1, 3, 1024, 2112), device="cuda"), schedule=[torch.ones((1, 64, 132))])
    monkeypatch.setattr(net, "storage", "bf16")
    with pytest.raises(NotImplementedError, match="bf16 storage"):
        EB.encode_batch(net, x1, schedule=S1)
    with pytest.raises(NotImplementedError, match="bf16 storage"):
        EB.EmbeddedDecoder(net, cs)
    monkeypatch.setattr(net, "storage", "fp32")
    monkeypatch.setattr(ops, "f16x2_mode", lambda: True)
    with pytest.raises(NotImplementedError, match="f16x2"):
        EB.encode_batch(net, x1, schedule=S1)
    with pytest.raises(NotImplementedError, match="f16x2"):
        EB.EmbeddedDecoder(net, cs)


def test_roi_schedule_and_embedded_roi_rd():
    net = _net()
    x = _x(2, 64, 128, seed=2)
    boxes = _boxes(2, 64, 128)
    S = EV.roi_schedule(2, 64, 128, boxes, [1, 5, 10], [0, 0.5, 2.5, 10])
    assert len(S) == 6 and all(tuple(m.shape) == (2, 4, 8) for m in S)
    region = torch.zeros((2, 64, 128), dtype=torch.bool)
    for b, y0, x0, y1, x1 in boxes:
        region[b, y0:y1, x0:x1] = True
    lat = EV.latent_quality_map(region.double()) > 0                            # a block that touches the region belongs to it
    for k, (r, g) in enumerate([(1, 0), (5, 0), (10, 0), (10, 0.5), (10, 2.5), (10, 10)]):
        assert torch.equal(S[k], torch.where(lat, float(r), float(g)).double()), k
    EB.check_schedule(S, 2, 4, 8)
    rows = EV.embedded_roi_rd(net, x, S, region)
    assert [r["stage"] for r in rows] == list(range(6))
    cs = EB.encode_batch(net, x, schedule=S)
    for r in rows:
        k = r["stage"]
        assert r["bytes"] == [sum(EB.container_bytes(c)[:2]) + c["side_bytes"] + sum(c["marks"]["bytes"][k]) for c in cs]
        assert r["bpp"] == [8.0 * v / (64 * 128) for v in r["bytes"]]
        for key in ("psnr", "psnr_in", "psnr_out"):
            assert tuple(r[key].shape) == (2,) and r[key].dtype == torch.float64 and torch.isfinite(r[key]).all()
    for a, b in zip(rows, rows[1:]):
        assert all(v1 >= v0 for v0, v1 in zip(a["bytes"], b["bytes"]))
    assert all(v1 > v0 for v0, v1 in zip(rows[0]["bytes"], rows[-1]["bytes"]))
