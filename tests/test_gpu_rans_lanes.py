"""Lane-split rANS streams on the device (csrc/rans_device.hip): one thread per (stream, lane).  The
kernels give the host exports' strings byte for byte and decode them, from the entry points up to compress / decompress
and their per-image and quality-map siblings with ``model.coder_lanes``.  Everything is bit-exact."""
import argparse
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic                              # noqa: E402
import vampic.synth as synth               # noqa: E402
from vampic import bitstream as bs         # noqa: E402
from vampic import ops                     # noqa: E402
from conftest import README_ARGS           # noqa: E402
from test_gpu_rans_device import _buffers  # noqa: E402

VamError = vampic._lib.VamError


@pytest.fixture(scope="module")
def codec(gpu_model):
    net, sd = gpu_model
    net.update()
    yield net
    net.coder, net.coder_lanes = "host", 1


@pytest.fixture(scope="module")
def pic():
    """A plain (non-REM) model: the batched per-image and quality-map paths."""
    net = vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu").eval()
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
    net = net.cuda()
    net.update()
    return net


@pytest.fixture()
def host_coder_forbidden(monkeypatch):
    """A context in which any call of the host coder fails the test, entered while model.coder == "device": without it
    the byte comparisons would pass with the ``coder`` attribute ignored."""
    @contextlib.contextmanager
    def forbidden():
        def refuse(*a, **k):
            raise AssertionError("the host coder ran while model.coder == 'device'")
        with monkeypatch.context() as mp:
            for name in ("encode", "decode", "encode_streams", "decode_streams", "encode_lanes", "decode_lanes"):
                mp.setattr(bs, name, refuse)
            yield
    return forbidden


@contextlib.contextmanager
def setting(net, coder, lanes):
    net.coder, net.coder_lanes = coder, lanes
    try:
        yield
    finally:
        net.coder, net.coder_lanes = "host", 1


# ----------------------------------------------------------------------------------------------- kernels
def _window(a, b, c0, C, s):
    """Slice s of image b in stream order [C, h, w]."""
    return np.ascontiguousarray(a[b, :, :, c0 + s * C:c0 + (s + 1) * C].transpose(2, 0, 1))


def _check_kernels(t, dt, geometry, K, seed, null_index=False, lane_kernels=None):
    B, h, w, ld, c0, C, n_slices = geometry
    sym, idx = _buffers(t, B, h, w, ld, seed, channel_index=null_index)
    if null_index:                                           # table index = channel within the window
        idx = np.broadcast_to(np.clip(np.arange(ld) - c0, 0, None) % C, (B, h, w, ld)).astype(np.int32)
    want = [[bs.encode_lanes(_window(sym, b, c0, C, s), _window(idx, b, c0, C, s), t, K) for b in range(B)] for s in range(n_slices)]
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    iv = None if null_index else ops.IView(d_idx, c0, C * n_slices)
    got = bs.encode_streams_device(ops.IView(d_sym, c0, C * n_slices), iv, n_slices, C, dt, lanes=K, lane_kernels=lane_kernels)
    assert got == want                                        # device strings == the host export's
    out = torch.full_like(d_sym, -7)                          # the device decodes the host's strings
    up = bs.decode_streams_device(want, iv, ops.IView(out, c0, C * n_slices), n_slices, C, dt, lanes=K, lane_kernels=lane_kernels)
    bs.check_status(up, B)
    ref = np.full_like(sym, -7)                               # nothing outside the window is written
    ref[..., c0:c0 + C * n_slices] = sym[..., c0:c0 + C * n_slices]
    assert np.array_equal(out.cpu().numpy(), ref)
    for s in range(n_slices):                                 # the host decodes the device's strings
        for b in range(B):
            dec = bs.decode_lanes(got[s][b], _window(idx, b, c0, C, s), t, K)
            assert np.array_equal(dec, _window(sym, b, c0, C, s).reshape(-1))
    return d_sym, iv, got


GEOMETRIES = [(2, 4, 4, 64, 0, 32, 2),      # the 64x64 image's slices
              (1, 1, 65, 3, 1, 1, 2),       # n = 65: lanes of 2 and 1 elements at K = 64
              (1, 1, 3, 3, 0, 1, 1),        # n = 3 < K: empty lanes
              (3, 8, 16, 40, 8, 32, 1)]     # a window inside the row, many steps


@pytest.mark.parametrize("K", [2, 8, 64])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_kernels_equal_the_host_exports_on_the_gaussian_tables(codec, geometry, K):
    dt = bs.DeviceCoderTables.of(codec.gaussian_conditional, "cuda")
    assert dt.packed is not None and 0 < dt.lds_bytes <= dt.lds_limit          # the LDS path
    _check_kernels(dt.host, dt, geometry, K, seed=sum(geometry) + K)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_one_lane_through_the_lane_kernels_is_the_existing_stream(codec, geometry):
    dt = bs.DeviceCoderTables.of(codec.gaussian_conditional, "cuda")
    B, h, w, ld, c0, C, n_slices = geometry
    d_sym, iv, got = _check_kernels(dt.host, dt, geometry, 1, seed=sum(geometry), lane_kernels=True)
    assert got == bs.encode_streams_device(ops.IView(d_sym, c0, C * n_slices), iv, n_slices, C, dt)


def test_lane_kernels_code_z_without_an_index_buffer(codec):
    dt = bs.DeviceCoderTables.of(codec.entropy_bottleneck, "cuda")
    assert dt.host.cdf.shape[0] == 192
    _check_kernels(dt.host, dt, (2, 1, 1, 192, 0, 192, 1), 8, seed=3, null_index=True)


def test_lane_kernels_read_tables_too_large_for_lds_from_global_memory():
    n_t, size = 48, 2050                                      # 48 x 2049 x 2 bytes = 196,704: above a CU's 160 KB of LDS
    rng = np.random.default_rng(1)
    cdf = np.zeros((n_t, size), dtype=np.int32)
    for k in range(n_t):
        cdf[k, 1:-1] = np.sort(rng.choice(np.arange(1, 65536), size=size - 2, replace=False))
        cdf[k, -1] = 65536
    t = bs.Tables(cdf, np.full(n_t, size, dtype=np.int32), rng.integers(-1000, 0, n_t).astype(np.int32))
    dt = bs.DeviceCoderTables.build(t, "cuda")
    assert dt.packed is None and dt.lds_bytes > dt.lds_limit
    _check_kernels(t, dt, (2, 4, 4, 64, 0, 32, 2), 8, seed=5)


# ----------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def reference(codec):
    """One 64x64 image per quality: the K = 1 host strings and the x_hat of their round trip, computed once."""
    x = synth.synth_image(1, 64, 64, seed=5).cuda()
    ref = {}
    with torch.no_grad(), setting(codec, "host", 1):
        for q in (0, 2.5, 10):
            enc = codec.compress(x, quality=q)
            ref[q] = (enc, codec.decompress(enc["strings"], enc["shape"], quality=q)["x_hat"].clone())
    return x, ref


@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("q", [0, 2.5, 10])
def test_both_coders_give_the_same_lane_strings_and_the_one_lane_x_hat(codec, reference, host_coder_forbidden, q, K):
    net = codec
    x, ref = reference
    enc_1, x_hat = ref[q]
    with torch.no_grad():
        with setting(net, "host", K):
            enc_h = net.compress(x, quality=q)
            dec_hh = net.decompress(enc_h["strings"], enc_h["shape"], quality=q)["x_hat"]
        with setting(net, "device", K), host_coder_forbidden():
            enc_d = net.compress(x, quality=q)
            dec_dd = net.decompress(enc_d["strings"], enc_d["shape"], quality=q)["x_hat"]
            dec_hd = net.decompress(enc_h["strings"], enc_h["shape"], quality=q)["x_hat"]      # host -> device
        with setting(net, "host", K):
            dec_dh = net.decompress(enc_d["strings"], enc_d["shape"], quality=q)["x_hat"]      # device -> host
    assert len(enc_d["strings"][0]) == (10 if q == 0 else 20) and len(enc_d["strings"][1]) == 1
    assert enc_d["strings"] == enc_h["strings"]
    y1 = [s for row in enc_1["strings"][0] for s in row] + list(enc_1["strings"][1])
    yk = [s for row in enc_h["strings"][0] for s in row] + list(enc_h["strings"][1])
    assert all(len(a) > len(b) and len(a) % 4 == 0 for a, b in zip(yk, y1))    # a header and K - 1 more final states
    for dec in (dec_hh, dec_dd, dec_hd, dec_dh):
        assert torch.equal(dec, x_hat)


def test_per_image_paths(pic, host_coder_forbidden):
    net = pic
    x = synth.synth_image(2, 64, 64, seed=11).cuda()
    qs = [0.5, 5]
    with torch.no_grad():
        with setting(net, "host", 1):
            dec_1 = net.decompress_per_image(net.compress_per_image(x, qs))["x_hat"]
        with setting(net, "host", 8):
            items_h = net.compress_per_image(x, qs)
            dec_h = net.decompress_per_image(items_h)["x_hat"]
        with setting(net, "device", 8), host_coder_forbidden():
            items_d = net.compress_per_image(x, qs)
            dec_d = net.decompress_per_image(items_d)["x_hat"]
    assert [it["strings"] for it in items_d] == [it["strings"] for it in items_h]
    assert torch.equal(dec_d, dec_1) and torch.equal(dec_h, dec_1)


def test_quality_map_paths(pic, host_coder_forbidden):
    net = pic
    x = synth.synth_image(1, 64, 64, seed=12).cuda()
    qmap = torch.full((1, 4, 4), 0.3, dtype=torch.float64)
    qmap[0, :, 2:] = 4.0
    with torch.no_grad():
        with setting(net, "host", 1):
            dec_1 = net.decompress_quality_map(net.compress_quality_map(x, qmap))["x_hat"]
        with setting(net, "host", 8):
            items_h = net.compress_quality_map(x, qmap)
            dec_h = net.decompress_quality_map(items_h)["x_hat"]
        with setting(net, "device", 8), host_coder_forbidden():
            items_d = net.compress_quality_map(x, qmap)
            dec_d = net.decompress_quality_map(items_d)["x_hat"]
    assert [it["strings"] for it in items_d] == [it["strings"] for it in items_h]
    assert torch.equal(dec_d, dec_1) and torch.equal(dec_h, dec_1)


def test_switching_lanes_on_one_model_reuses_nothing_stale(codec, reference):
    net = codec
    x, ref = reference
    enc_1, x_hat = ref[2.5]
    with torch.no_grad(), setting(net, "device", 1):
        seen = {}
        for K in (1, 8, 1):
            net.coder_lanes = K
            enc = net.compress(x, quality=2.5)
            dec = net.decompress(enc["strings"], enc["shape"], quality=2.5)["x_hat"]
            assert torch.equal(dec, x_hat)
            assert seen.setdefault(K, enc["strings"]) == enc["strings"]
        assert seen[1] == enc_1["strings"] and seen[8] != seen[1]


def test_a_string_shorter_than_its_header_raises_and_the_plan_stays_usable(codec, reference):
    """The decoder's contract is a status code: a slice string cut below 4 K bytes is refused whole."""
    net = codec
    x, ref = reference
    K = 8
    with torch.no_grad(), setting(net, "device", K):
        enc = net.compress(x, quality=2.5)
        x_hat = ref[2.5][1]
        strings = [[list(s) for s in enc["strings"][0]], list(enc["strings"][1])]
        strings[0][3][0] = strings[0][3][0][:4 * K - 4]
        with pytest.raises(VamError, match=r"image 0, slice 3\), lane 0: bad stream \(the header of 8 lane lengths"):
            net.decompress(strings, enc["shape"], quality=2.5)
        n_plans = len(net._dec_plans)
        assert torch.equal(net.decompress(enc["strings"], enc["shape"], quality=2.5)["x_hat"], x_hat)
        assert len(net._dec_plans) == n_plans                # the same plan
