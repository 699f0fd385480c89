"""Progressive containers on the device coder: the layered kernels against the host coder's bytes on a
synthetic window, the level grouping, the two-level pack scan, and encode_batch / ProgressiveDecoder with ``coder="device"``
against the host path — the same containers byte for byte, decoded interchangeably, every level equal to
forward_single_quality bit for bit.  Everything is bit-exact; no time is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                                         # noqa: E402
from vampic import _lib as L, bitstream as bs, evaluate as EV, ops, progressive as P   # noqa: E402
from test_gpu_progressive_batch import _net, _x       # noqa: E402
from test_gpu_rans_device import _buffers             # noqa: E402

N_LEVELS = 4
SENTINEL = -7
#            B  h  w  ld   c0  C  n_slices
GEOMETRIES = [(2, 4, 4, 104, 5, 32, 3),       # n = 512: a multiple of 64
              (2, 1, 3, 11, 2, 4, 2)]         # n = 12: a partial wave, and at K = 64 empty lanes


def _window(a, b, c0, Cw, s):
    """Slice s of image b in stream order [C, h, w]."""
    return np.ascontiguousarray(a[b, :, :, c0 + s * Cw:c0 + (s + 1) * Cw].transpose(2, 0, 1))


@pytest.fixture(scope="module", autouse=True)
def layered_build():
    """Every test of this file is about the library that has the layered entry points; the two-level pack came with them."""
    lib = L.load()
    assert hasattr(lib, "vam_rans_layers_encode_device") and hasattr(lib, "vam_rans_layers_decode_device")


@pytest.fixture(scope="module")
def gauss():
    net = _net()
    return bs.DeviceCoderTables.of(net.gaussian_conditional, "cuda")


@pytest.fixture(scope="module", params=GEOMETRIES, ids=["n512", "n12"])
def window(request, gauss):
    """Symbols, indexes and layer ids of one geometry, on the host and on the device.  Layer ids cover the selectors
    0 .. 3: selector 2 owns no element, the ids 9 and 0xFF lie outside the range."""
    B, h, w, ld, c0, Cw, ns = request.param
    sym, idx = _buffers(gauss.host, B, h, w, ld, seed=sum(request.param))
    layer = np.random.default_rng(ld).choice(np.array([0, 1, 3, 9, 0xFF], dtype=np.uint8), size=(B, h, w, ld))
    d = {k: torch.from_numpy(v).cuda() for k, v in (("sym", sym), ("idx", idx), ("layer", layer))}
    return request.param, sym, idx, layer, d


def _host_layers(geometry, sym, idx, layer, t, K, levels):
    B, h, w, ld, c0, Cw, ns = geometry
    jobs = [(_window(sym, b, c0, Cw, s), _window(idx, b, c0, Cw, s), _window(layer, b, c0, Cw, s), k)
            for k in levels for s in range(ns) for b in range(B)]
    return bs.encode_streams(jobs, t, lanes=K)


def _flat(strings):
    return [s_ for level in strings for row in level for s_ in row]


@pytest.mark.parametrize("K", [1, 8, 64])
def test_layered_kernels_equal_the_host_coder(window, gauss, K):
    geometry, sym, idx, layer, d = window
    B, h, w, ld, c0, Cw, ns = geometry
    sv, iv = ops.IView(d["sym"], c0, Cw * ns), ops.IView(d["idx"], c0, Cw * ns)
    want = _host_layers(geometry, sym, idx, layer, gauss.host, K, range(N_LEVELS))
    got = bs.encode_layers_device(sv, iv, d["layer"], N_LEVELS, ns, Cw, gauss, lanes=K)
    assert len(got) == N_LEVELS and all(len(lv) == ns and all(len(row) == B for row in lv) for lv in got)
    assert _flat(got) == want                                 # stream (k, s, b) == the host coder's (layer, sel = k) job
    # a scratch bound of one level's regions: one launch per level, the same strings
    level_bytes = 2 * 4 * B * ns * K * (2 * (-(-(Cw * h * w) // K)) + 16)
    assert len(bs.layer_groups(N_LEVELS, level_bytes, level_bytes)) >= 3
    assert bs.encode_layers_device(sv, iv, d["layer"], N_LEVELS, ns, Cw, gauss, lanes=K, max_scratch_bytes=level_bytes) == got
    # and equal to the single-selector launches, selector by selector (K = 1 and the lane form)
    for k in (0, 2):
        assert got[k] == bs.encode_streams_device(sv, iv, ns, Cw, gauss, layer=d["layer"], sel=k, lanes=K)
    # one decode launch over all levels
    inside = np.zeros(sym.shape, dtype=bool)
    inside[..., c0:c0 + Cw * ns] = True
    out = torch.full_like(d["sym"], SENTINEL)
    up = bs.upload_streams(want, "cuda", K)
    bs.decode_layers_uploaded(up, 0, iv, ops.IView(out, c0, Cw * ns), d["layer"], 0, N_LEVELS, ns, Cw, gauss, lanes=K)
    bs.check_layer_status(up, B, ns)
    keep = inside & (layer < N_LEVELS)                        # ids 9 and 0xFF and everything outside the window: untouched
    assert np.array_equal(out.cpu().numpy(), np.where(keep, sym, SENTINEL))
    # a launch over the levels [1, 3) touches only those levels' elements
    out = torch.full_like(d["sym"], SENTINEL)
    per = ns * B
    up = bs.upload_streams(want[per:3 * per], "cuda", K)
    bs.decode_layers_uploaded(up, 0, iv, ops.IView(out, c0, Cw * ns), d["layer"], 1, 2, ns, Cw, gauss, lanes=K)
    bs.check_layer_status(up, B, ns, first_level=1)
    keep = inside & ((layer == 1) | (layer == 2))
    assert keep.any() and np.array_equal(out.cpu().numpy(), np.where(keep, sym, SENTINEL))


def test_layered_launches_refuse_bad_geometry_by_message(window, gauss):
    geometry, sym, idx, layer, d = window
    B, h, w, ld, c0, Cw, ns = geometry
    lib = L.load()
    words = torch.empty(64, dtype=torch.int32, device="cuda")

    def encode(layer_ptr=d["layer"].data_ptr(), sel0=0, n_sel=N_LEVELS, B_=B, c0_=c0, lanes=1):
        return lib.vam_rans_layers_encode_device(d["sym"].data_ptr(), d["idx"].data_ptr(), layer_ptr, sel0, n_sel, B_, h, w, ld, c0_, Cw,
                                                 ns, lanes, C.byref(gauss.struct), words.data_ptr(), 16, words.data_ptr(),
                                                 words.data_ptr(), None)
    for call, text in ((lambda: encode(layer_ptr=None), "need the layer ids"), (lambda: encode(sel0=254), "outside the layer ids"),
                       (lambda: encode(n_sel=0), "outside the layer ids"), (lambda: encode(c0_=ld - 1), "does not fit"),
                       (lambda: encode(lanes=3), "power of two"), (lambda: encode(n_sel=256, B_=1 << 16), "too large")):
        with pytest.raises(L.VamError, match=text):
            L.check(call(), "vam_rans_layers_encode_device")
    with pytest.raises(ValueError, match="layer ids"):
        bs.encode_layers_device(ops.IView(d["sym"], c0, Cw * ns), None, None, N_LEVELS, ns, Cw, gauss)
    with pytest.raises(ValueError, match="outside the layer ids"):
        bs.encode_layers_device(ops.IView(d["sym"], c0, Cw * ns), None, d["layer"], 300, ns, Cw, gauss)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_000])
def test_pack_scan_equals_cumsum(n):
    cap = 6
    rng = np.random.default_rng(n)
    lengths = rng.integers(0, cap + 1, n).astype(np.int32)
    lengths[rng.random(n) < 0.2] = 0
    regions = rng.integers(-2 ** 31, 2 ** 31, (n, cap)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])
    tails = regions[np.arange(cap)[None, :] >= cap - lengths[:, None]]        # every region's tail, back to back
    d_len, d_reg = torch.from_numpy(lengths).cuda(), torch.from_numpy(regions).cuda()
    for packed_cap in (int(off[-1]), int(off[-1]) // 2):
        packed = torch.full((max(packed_cap, 1),), SENTINEL, dtype=torch.int32, device="cuda")
        offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        L.check(L.load().vam_rans_pack_device(d_reg.data_ptr(), cap, d_len.data_ptr(), n, packed.data_ptr(), packed_cap,
                                              offsets.data_ptr(), None), "vam_rans_pack_device")
        assert np.array_equal(offsets.cpu().numpy(), off)                     # offsets[n] is the total
        want = np.full(max(packed_cap, 1), SENTINEL, dtype=np.int32)
        fits = np.repeat(off[1:] <= packed_cap, lengths)                      # per word; over-capacity regions are skipped
        want[np.arange(int(off[-1]))[fits]] = tails[fits]
        assert np.array_equal(packed.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------- containers
Q_LIST = [0.5, 0.5, 2.5, 10]                                  # a repeated quality (an empty layer) and the full mask


def _levels(net, x, q_list):
    with torch.no_grad():
        return [net.forward_single_quality(x, 0 if k == 0 else q_list[k - 1]) for k in range(len(q_list) + 1)]


def _assert_levels(dec, fw, ks=None):
    ks = list(range(len(fw))) if ks is None else ks
    for k, o in zip(ks, dec.decode_levels(ks)):
        assert torch.equal(o["x_hat"], fw[k]["x_hat"]), k
        assert torch.equal(o["y_hat"], fw[k]["y_hat"]), k


@pytest.mark.parametrize("case", ["1x64x64", "2x64x128", "single"])
def test_device_containers_are_the_host_containers_and_decode_both_ways(case):
    net = _net(multiple_decoder=False, multiple_hyperprior=False, support_progressive_slices=2) if case == "single" else _net()
    x = _x(2, 64, 128, seed=2) if case == "2x64x128" else _x(1, 64, 64, seed=3)
    cs_h, bits_h = P.encode_batch(net, x, Q_LIST, coder="host")
    cs_d, bits_d = P.encode_batch(net, x, Q_LIST, coder="device")
    assert cs_d == cs_h and bits_d == bits_h and all("lanes" not in c for c in cs_d)
    assert all(set(c) == {"q_list", "shape", "z", "base", "progressive"} for c in cs_d)
    fw = _levels(net, x, Q_LIST)
    _assert_levels(P.ProgressiveDecoder(net, cs_h, coder="device"), fw)       # host-made containers on the device decoder
    _assert_levels(P.ProgressiveDecoder(net, cs_d, coder="host"), fw)         # device-made ones on the host decoder


def test_coder_none_reads_the_model_attribute():
    net = _net()
    x = _x(1, 64, 64, seed=3)
    cs_h, _ = P.encode_batch(net, x, Q_LIST)
    try:
        net.coder = "device"
        cs_d, _ = P.encode_batch(net, x, Q_LIST)
        dec = P.ProgressiveDecoder(net, cs_d)
        assert dec.coder == "device" and dec.dp.coder == "device"
        out = dec.decode(2)
    finally:
        net.coder = "host"
    assert cs_d == cs_h
    ref = P.ProgressiveDecoder(net, cs_h)
    assert ref.coder == "host" and ref.dp is not dec.dp                       # the plan is keyed by coder
    assert torch.equal(out["x_hat"], ref.decode(2)["x_hat"])


def test_incremental_decoding_and_owner_restore():
    net = _net()
    q_list = [0.5, 1, 2.5]
    xa, xb = _x(1, 64, 64, seed=4), _x(1, 64, 64, seed=5)
    ca, _ = P.encode_batch(net, xa, q_list, coder="device")
    cb, _ = P.encode_batch(net, xb, q_list, coder="device")
    d0 = P.ProgressiveDecoder(net, ca, coder="device")
    d0.decode(1)
    assert d0.layers_decoded == 1
    a3 = d0.decode(3)
    assert d0.layers_decoded == 3
    a2 = d0.decode(2)
    assert d0.layers_decoded == 3
    d1, d2 = P.ProgressiveDecoder(net, ca, coder="device"), P.ProgressiveDecoder(net, cb, coder="device")
    hosts = {"a": P.ProgressiveDecoder(net, ca, coder="host"), "b": P.ProgressiveDecoder(net, cb, coder="host")}
    assert d1.dp is d2.dp and d1.dp is not hosts["a"].dp
    same = lambda p, q: all(torch.equal(u["x_hat"], v["x_hat"]) and torch.equal(u["y_hat"], v["y_hat"]) for u, v in zip(p, q))
    for ks in ([0, 2], [1], [0, 2, 3], [3]):                  # the three decoders alternate on the same model
        ra, rb = hosts["a"].decode_levels(ks), hosts["b"].decode_levels(ks)
        assert same(d1.decode_levels(ks), ra), ks
        assert same(d2.decode_levels(ks), rb), ks
        assert same(d1.decode_levels(ks), ra), ks             # d1 again, after d2 used the plans
    assert not torch.equal(hosts["a"].decode(3)["x_hat"], hosts["b"].decode(3)["x_hat"])
    assert same([a3, a2], hosts["a"].decode_levels([3, 2]))
    assert d1.layers_decoded == d2.layers_decoded == 3


def test_truncated_layer_raises_naming_image_level_and_slice():
    """The case of test_gpu_progressive_batch.test_truncated_layer_raises on the device decoder."""
    net = _net()
    x = _x(1, 64, 64, seed=8)
    cs, _ = P.encode_batch(net, x, [0.5, 1, 2.5], coder="device")
    bad = dict(cs[0])
    bad["progressive"] = [list(l_) for l_ in cs[0]["progressive"]]
    bad["progressive"][1][4] = bad["progressive"][1][4][:8]
    dec = P.ProgressiveDecoder(net, [bad], coder="device")
    good = dec.decode(1)
    with pytest.raises(L.VamError, match=r"image 0, level 2, slice 4\): bitstream truncated"):
        dec.decode(2)
    again = dec.decode(1)                                     # the decoder starts over and is usable
    assert torch.equal(again["x_hat"], good["x_hat"])
    assert torch.equal(good["x_hat"], P.ProgressiveDecoder(net, cs, coder="host").decode(1)["x_hat"])


def test_lane_split_containers():
    net = _net()
    x = _x(1, 64, 64, seed=3)
    q_list = [0.5, 2.5, 10]
    c1, _ = P.encode_batch(net, x, q_list, coder="device")
    assert P.encode_batch(net, x, q_list, coder="device", lanes=1)[0] == c1
    try:
        net.coder_lanes = 8                                   # lanes is explicit only: the attribute is not read
        assert P.encode_batch(net, x, q_list, coder="device")[0] == c1
    finally:
        net.coder_lanes = 1
    c8_h, _ = P.encode_batch(net, x, q_list, coder="host", lanes=8)
    c8_d, bits8 = P.encode_batch(net, x, q_list, coder="device", lanes=8)
    assert c8_d == c8_h and c8_d[0]["lanes"] == 8 and c8_d != c1
    assert bits8[0] == P.container_bits(c8_d[0]) and P.bits_up_to(c8_d[0], 3) > P.bits_up_to(c1[0], 3)
    fw = _levels(net, x, q_list)
    _assert_levels(P.ProgressiveDecoder(net, c8_h, coder="device"), fw)
    _assert_levels(P.ProgressiveDecoder(net, c8_d, coder="host"), fw)
    for coder in ("host", "device"):
        with pytest.raises(ValueError, match="same lanes"):
            P.ProgressiveDecoder(net, c1 + c8_d, coder=coder)


def test_device_path_never_calls_the_host_coder(monkeypatch):
    net = _net()
    x = _x(2, 64, 128, seed=2)

    def refuse(*a, **k):
        raise AssertionError("the host coder ran on the device path")
    ref, _ = P.encode_batch(net, x, Q_LIST, coder="host")
    want = P.ProgressiveDecoder(net, ref, coder="host").decode_levels(list(range(len(Q_LIST) + 1)))
    for name in ("encode", "decode", "encode_streams", "decode_streams", "encode_lanes", "decode_lanes"):
        monkeypatch.setattr(bs, name, refuse)
    cs, _ = P.encode_batch(net, x, Q_LIST, coder="device")
    got = P.ProgressiveDecoder(net, cs, coder="device").decode_levels(list(range(len(Q_LIST) + 1)))
    assert cs == ref
    assert all(torch.equal(a["x_hat"], b["x_hat"]) and torch.equal(a["y_hat"], b["y_hat"]) for a, b in zip(got, want))


def test_refusals():
    net = _net()
    x = _x(1, 64, 64)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        P.encode_batch(net, x, [0.5, 1], coder="gpu")
    with pytest.raises(ValueError, match="power of two"):
        P.encode_batch(net, x, [0.5, 1], coder="device", lanes=3)
    cs, _ = P.encode_batch(net, x, [0.5, 1], coder="device")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        P.ProgressiveDecoder(net, cs, coder="gpu")


def test_progressive_rd_passes_the_coder_through():
    net = _net()
    imgs = [vampic.synth.synth_image(1, 50, 100, seed=11).cuda()]
    rows_h = EV.progressive_rd(net, imgs, [0.5, 10])
    rows_d = EV.progressive_rd(net, imgs, [0.5, 10], coder="device")
    rows_8 = EV.progressive_rd(net, imgs, [0.5, 10], coder="device", lanes=8)
    for h_, d_, e_ in zip(rows_h, rows_d, rows_8):
        assert d_["bpp_all"] == h_["bpp_all"] and e_["bpp_all"][0] > h_["bpp_all"][0]
        # compute_psnr's float64 sum is accumulated with atomics (order unspecified): equal to the last few ulps
        assert abs(d_["psnr_all"][0] - h_["psnr_all"][0]) <= 1e-9 and abs(e_["psnr_all"][0] - h_["psnr_all"][0]) <= 1e-9
