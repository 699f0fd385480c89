"""Picture-wide quality marks end to end on the GPU (vampic.tiled.encode(allocation="picture"), PictureDecoder.decode(mark=),
EmbeddedDecoder.decode_marks, evaluate.tiled_rd(allocation=)): the header's thresholds and the tiles'
counts are the restatement's (tests/pooled_ref.py) on the sigmas a decoder computes, and every decode of a mark equals the
NumPy blend (tests/tiled_ref.py) of the tiles decoded at those counts through ``tail_counts``, bit for bit."""
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pooled_ref as PR                                            # noqa: E402
import tiled_ref as TR                                             # noqa: E402
from test_gpu_embedded_schedule import _coded as _scheduled, _net, _x   # noqa: E402
from test_tiled_cpu import _reseal                                 # noqa: E402
from vampic import embedded as EB, evaluate as EV, tiled as TL   # noqa: E402

MARKS = [0.05, 0.5, 2.5, 10]
MAIN = dict(H=150, W=200, tile=64, overlap=16)
_CODED, _REF = {}, {}


def _coded(H=150, W=200, tile=64, overlap=16, group=4, allocation="picture", **kw):
    key = (H, W, tile, overlap, group, allocation, tuple(sorted(kw.items())))
    if key not in _CODED:
        x = _x(1, H, W)[0]
        _CODED[key] = (x, TL.grid(H, W, tile, overlap),
                       TL.encode(_net(), x, tile=tile, overlap=overlap, marks=MARKS, group=group, allocation=allocation, **kw))
    return _CODED[key]


def _ref():
    """Of the main picture, once: the sigmas fp32 [T, ns, n] a decoder computes for every tile, the restatement's thresholds
    and counts on them, and per mark the tiles decoded through ``tail_counts`` at those counts, [T, 3, th, tw]."""
    if not _REF:
        net = _net()
        x, g, data = _coded()
        ns, C = net.ns0, net.dim_chunk
        cs = [EB.from_bytes(TL.tile_stream(data, r, c)) for r, c in TL.tiles_for(g)]
        sig, decs = [], []
        for i0 in (0, 6):
            dec = EB.EmbeddedDecoder(net, cs[i0:i0 + 6])
            std = dec.dp.sc.std_p.torch_nchw()[:, :ns * C].contiguous().cpu().numpy()      # [B, ns * C, h, w]
            sig.append(std.reshape(std.shape[0], ns, -1))
            decs.append(dec)
        sig = np.concatenate(sig)
        thr = PR.thresholds(sig, MARKS)
        cnt = PR.counts(sig, thr)
        x_hat = []
        with torch.no_grad():
            for k in range(len(MARKS)):
                parts = []
                for dec, i0 in zip(decs, (0, 6)):
                    dec._own()
                    t = dec.dp.tail_counts(np.ascontiguousarray(cnt[k:k + 1, i0:i0 + 6]), net.use_graph)
                    parts.append(t.x_hat[:6].clone().cpu().numpy())
                x_hat.append(np.concatenate(parts))
        _REF.update(sig=sig, thr=thr, cnt=cnt, x_hat=x_hat, cs=cs)
    return _REF


def _eq(got, want):
    return tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _blend(k, window=None):
    g = _coded()[1]
    return TR.blend(_ref()["x_hat"][k], np.arange(12).reshape(3, 4), g, window)[0]


def test_thresholds_and_counts_are_the_restatement_s_on_the_decoder_s_sigma():
    net = _net()
    x, g, data = _coded()
    ref, lay = _ref(), TL.layout(_coded()[2])
    n = net.dim_chunk * 16
    assert ref["sig"].shape == (12, net.ns0, n) and (g["R"], g["C"]) == (3, 4)
    assert lay["allocation"] == "picture" and lay["marks"] == [float(q) for q in MARKS] and data[4] == 2
    assert lay["thresholds"].shape == (4, net.ns0) and lay["thresholds"].tobytes() == ref["thr"].tobytes()
    got = np.stack([np.asarray(c["marks"]["count"]) for c in ref["cs"]], axis=1)             # [L, T, ns]
    assert np.array_equal(got, ref["cnt"])
    frac = ref["cnt"][2].sum(-1) / (net.ns0 * n)                                             # q = 2.5: the kept fraction per tile
    assert len(set(frac.tolist())) >= 2, frac                                                # not every tile's own 25 %
    for k in range(4):
        for j in range(net.ns0):
            with np.errstate(invalid="ignore"):
                pool = int((ref["sig"][:, j] >= ref["thr"][k, j]).sum()) if k < 3 else 12 * n
            assert int(ref["cnt"][k, :, j].sum()) == pool
    assert all(c["marks"]["q"] == [float(q) for q in MARKS] for c in ref["cs"])              # the heads are ordinary headers


def test_decode_mark_is_the_blend_of_the_tiles_at_the_picture_s_counts():
    net = _net()
    x, g, data = _coded()
    lay = TL.layout(data)
    dec = TL.PictureDecoder(net, data, group=5)
    window = (40, 90, 30, 17)                                                                # inside a band, four tiles
    for k, q in enumerate(MARKS):
        want = _blend(k)
        assert _eq(dec.decode(mark=k), want) and len(dec.last_tiles) == 12, k
        assert _eq(dec.decode(q=q), want), k                                                 # a marked quality means its mark
        assert _eq(dec.decode(window, mark=k), _blend(k, window)), k
        cut = TL.PictureDecoder(net, data[:lay["round_end"][k]], group=4)                   # exactly mark k of every tile
        assert _eq(cut.decode(mark=k), want), k
        ex = TL.extract(data, rounds=k + 1)
        assert TL.layout(ex)["allocation"] == "picture" and _eq(TL.PictureDecoder(net, ex).decode(mark=k), want), k
    ex = TL.extract(data, window, rounds=2)
    assert _eq(TL.PictureDecoder(net, ex).decode(window, mark=1), _blend(1, window))         # the pool stays the picture's
    with pytest.raises(ValueError, match=r"tile \(\d, \d\): .*mark 2 needs"):
        TL.PictureDecoder(net, data[:lay["round_end"][1]]).decode(mark=2)
    with pytest.raises(ValueError, match=r"quality 1.0 is not marked.*the marks are \[0.05, 0.5, 2.5, 10.0\]"):
        dec.decode(q=1.0)
    with pytest.raises(ValueError, match="mark is 0 .. 3"):
        dec.decode(mark=4)
    with pytest.raises(ValueError, match="give q or mark, not both"):
        dec.decode(q=0.5, mark=1)
    assert _eq(dec.decode(), TR.blend(_full_tiles(), np.arange(12).reshape(3, 4), g)[0])     # everything: q = 10 of every tile


def _full_tiles():
    ref = _ref()
    return ref["x_hat"][3]


def test_an_altered_threshold_is_refused_at_decode_naming_tile_mark_and_slice():
    net = _net()
    x, g, data = _coded()
    lay, ref = TL.layout(data), _ref()
    ext = 20 + 4 * 12 * 6                                                                    # fixed fields, the table of 12 x (1 + 5)
    k, j = 1, 0
    lower = float(np.sort(ref["sig"][:, j].reshape(-1))[::-1][int(ref["cnt"][k, :, j].sum()) + 40])   # keeps 40 elements more

    def edit(h):
        assert struct.unpack_from("<f", h, ext + 8 + 4 * (k * net.ns0 + j))[0] == lay["thresholds"][k, j]
        struct.pack_into("<f", h, ext + 8 + 4 * (k * net.ns0 + j), lower)
    bad = _reseal(data, edit)
    assert TL.layout(bad)["thresholds"][k, j] == np.float32(lower)                           # the framing has nothing against it
    with pytest.raises(ValueError, match=rf"PictureDecoder.decode: tile \(\d, \d\): tile \(\d, \d\), mark {k}, slice {j}: the header's "
                                         "picture-wide threshold"):
        TL.PictureDecoder(net, bad).decode(mark=2)


def test_one_tile_group_sizes_and_the_default_allocation():
    net = _net()
    x, g, data = _coded()
    assert _coded(group=1)[2] == data and _coded(group=5)[2] == data                         # the bytes do not depend on the group
    v1 = _coded(allocation="tile")[2]
    assert v1[4] == 1 and TL.layout(v1)["allocation"] == "tile" and TL.layout(v1)["thresholds"] is None
    assert TL.encode(net, x, tile=64, overlap=16, marks=MARKS, group=4) == v1                # the default is "tile", byte for byte
    assert v1 != data and any(TL.tile_stream(v1, r, c) != TL.tile_stream(data, r, c) for r, c in TL.tiles_for(g))
    k = 2                                                                                    # mark= on a version-1 stream: decode(q=q_k)
    d1 = TL.PictureDecoder(net, v1)
    assert torch.equal(d1.decode(mark=k), d1.decode(q=MARKS[k]))
    assert torch.equal(d1.decode(q=1.0), d1.decode(q=1.0))                                   # and any q stays accepted there
    a, _, one_p = _coded(60, 60)                                                             # one tile: the pool is the tile
    one_t = _coded(60, 60, allocation="tile")[2]
    assert TL.grid(60, 60, 64, 16)["R"] == 1 and TL.tile_stream(one_p, 0, 0) == TL.tile_stream(one_t, 0, 0)
    assert one_p[4] == 2 and one_t[4] == 1 and len(one_p) == len(one_t) + 8 + 4 * 4 * net.ns0
    assert torch.equal(TL.PictureDecoder(net, one_p).decode(mark=1), TL.PictureDecoder(net, one_t).decode(q=MARKS[1]))
    with pytest.raises(ValueError, match="allocation is one of"):
        TL.encode(net, x, tile=64, overlap=16, allocation="image")
    with pytest.raises(ValueError, match="a picture-wide mark is a quality > 0"):
        TL.encode(net, x, tile=64, overlap=16, marks=[0, 1], allocation="picture")


def test_the_device_coder_on_lanes_gives_the_host_coder_s_bytes():
    net = _net()
    x, g, host = _coded(lanes=64, base_lanes=8)
    dev = TL.encode(net, x, tile=64, overlap=16, marks=MARKS, coder="device", lanes=64, base_lanes=8, group=6, allocation="picture")
    assert dev == host and host != _coded()[2]
    lay = TL.layout(host)
    assert (lay["lanes"], lay["base_lanes"], lay["allocation"]) == (64, 8, "picture")
    assert lay["thresholds"].tobytes() == _ref()["thr"].tobytes()                            # the lanes do not touch the selection
    window = (40, 90, 30, 17)
    a = TL.PictureDecoder(net, host, coder="device").decode(window, mark=1)
    assert _eq(a, _blend(1, window))


def test_decode_marks_is_decode_qualities_on_an_ordinary_container():
    net = _net()
    x = _x(2, 64, 64)
    cs = EB.encode_batch(net, x, marks=MARKS)
    dec = EB.EmbeddedDecoder(net, cs)
    got = dec.decode_marks([2, 0, 3])
    want = dec.decode_qualities([MARKS[2], MARKS[0], MARKS[3]])
    for a, b in zip(got, want):
        assert torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"])
    with pytest.raises(ValueError, match="marks must be integers in 0..3"):
        dec.decode_marks([4])
    short = EB.EmbeddedDecoder(net, [EB.truncate(c, q=MARKS[1]) for c in cs])
    with pytest.raises(ValueError, match=r"mark 2 needs \d+ elements of slice \d of image \d, its container holds"):
        short.decode_marks([2])
    sched = EB.EmbeddedDecoder(net, _scheduled(2, 64, 128)[2])                               # a scheduled container: its stages
    for a, b in zip(sched.decode_marks([3, 1, 0]), sched.decode_stages([3, 1, 0])):
        assert torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"])


def test_tiled_rd_reports_the_kept_fractions():
    net = _net()
    x, g, data = _coded()
    lay, ref = TL.layout(data), _ref()
    rows = EV.tiled_rd(net, x, MARKS, tile=64, overlap=16, group=4, allocation="picture")
    n = net.ns0 * net.dim_chunk * 16
    for k, r in enumerate(rows):
        assert r["bytes"] == lay["round_end"][k] and np.isfinite(r["psnr"]) and r["allocation"] == "picture"
        frac = ref["cnt"][k].sum(-1) / n
        assert r["kept_min"] == float(frac.min()) and r["kept_max"] == float(frac.max())
    assert rows[2]["kept_min"] < rows[2]["kept_max"] and rows[3]["kept_min"] == rows[3]["kept_max"] == 1.0
    tile_rows = EV.tiled_rd(net, x, MARKS, tile=64, overlap=16, group=4)
    assert tile_rows[0]["allocation"] == "tile" and tile_rows[3]["kept_min"] == 1.0
