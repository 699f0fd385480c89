"""The rANS coder on the device (csrc/rans_device.hip): byte for byte the host coder's streams, from the
kernels up to compress / decompress and their per-image and quality-map siblings.  Everything is bit-exact."""
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

VamError = vampic._lib.VamError


@pytest.fixture(scope="module")
def codec(gpu_model):
    net, sd = gpu_model
    net.update()
    yield net
    net.coder = "host"


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
            for name in ("encode", "decode", "encode_streams", "decode_streams"):
                mp.setattr(bs, name, refuse)
            yield
    return forbidden


# ----------------------------------------------------------------------------------------------- kernels
def _escapes(t, ci):
    """Out-of-range values of table ci: both signs, every n_bypass 1 .. 8, the value at max_value and one beyond."""
    mx, off = int(t.sizes[ci]) - 2, int(t.offsets[ci])
    vals = [mx, mx + 1, -1]
    for nb in range(1, 9):
        vals.append(mx + min(16 ** nb - 2, 2 ** 31 - 2) // 2)
        vals.append(-((min(16 ** nb - 1, 2 ** 31 - 1) if nb > 1 else 1) + 1) // 2)
        vals.append(mx + (16 ** (nb - 1) + 1) // 2)
    return np.array([v for v in vals if abs(v) <= 2 ** 30], dtype=np.int64) + off


def _buffers(t, B, h, w, ld, seed, channel_index=False):
    """int32 [B,h,w,ld] symbols and indexes: in range for their table, with the escapes of three tables injected."""
    rng = np.random.default_rng(seed)
    n_t = t.cdf.shape[0]
    idx = np.broadcast_to(np.arange(ld) % n_t, (B, h, w, ld)).astype(np.int32) if channel_index else \
        rng.integers(0, n_t, (B, h, w, ld)).astype(np.int32)
    mx = t.sizes[idx].astype(np.int64) - 2
    sym = (rng.integers(0, 1 << 30, idx.shape) % np.maximum(mx, 1) + t.offsets[idx]).astype(np.int32)
    flat_s, flat_i = sym.reshape(-1), idx.reshape(-1)
    for ci in {0, n_t // 2, n_t - 1}:
        where = np.flatnonzero(flat_i == ci)
        esc = _escapes(t, ci)
        pos = rng.choice(where, size=min(len(esc), len(where)), replace=False)
        flat_s[pos] = esc[:len(pos)].astype(np.int32)
    return sym, idx


def _host_streams(sym, idx, t, c0, C, n_slices):
    """[slice][image] from the host coder on the transposed host copies."""
    B = sym.shape[0]
    jobs = [(sym[b, :, :, c0 + s * C:c0 + (s + 1) * C].transpose(2, 0, 1), idx[b, :, :, c0 + s * C:c0 + (s + 1) * C].transpose(2, 0, 1))
            for s in range(n_slices) for b in range(B)]
    flat = bs.encode_streams(jobs, t)
    return [flat[s * B:(s + 1) * B] for s in range(n_slices)]


def _check_kernels(t, dt, geometry, seed, null_index=False):
    B, h, w, ld, c0, C, n_slices = geometry
    sym, idx = _buffers(t, B, h, w, ld, seed, channel_index=null_index)
    if null_index:                                           # table index = channel within the window
        idx = np.broadcast_to(np.clip(np.arange(ld) - c0, 0, None) % C, (B, h, w, ld)).astype(np.int32)
    want = _host_streams(sym, idx, t, c0, C, n_slices)
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    iv = None if null_index else ops.IView(d_idx, c0, C * n_slices)
    got = bs.encode_streams_device(ops.IView(d_sym, c0, C * n_slices), iv, n_slices, C, dt)
    assert got == want
    out = torch.full_like(d_sym, -7)
    up = bs.decode_streams_device(want, iv, ops.IView(out, c0, C * n_slices), n_slices, C, dt)
    bs.check_status(up, B)
    ref = np.full_like(sym, -7)                               # nothing outside the window is written
    ref[..., c0:c0 + C * n_slices] = sym[..., c0:c0 + C * n_slices]
    assert np.array_equal(out.cpu().numpy(), ref)


GEOMETRIES = [(2, 4, 4, 64, 0, 32, 2),      # the 64x64 image's slices
              (1, 1, 65, 3, 1, 1, 2),       # one symbol past a 64-symbol chunk, odd strides
              (3, 8, 16, 40, 8, 32, 1)]     # many chunks, a window inside the row


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_kernels_equal_the_host_coder_on_the_gaussian_tables(codec, geometry):
    g = codec.gaussian_conditional
    dt = bs.DeviceCoderTables.of(g, "cuda")
    assert dt.packed is not None and 0 < dt.lds_bytes <= dt.lds_limit          # the LDS path
    assert dt.lds_bytes == 2 * ((int((dt.host.sizes.astype(np.int64) - 1).sum()) + 7) // 8 * 8)
    _check_kernels(dt.host, dt, geometry, seed=sum(geometry))


def test_kernels_code_z_without_an_index_buffer(codec):
    eb = codec.entropy_bottleneck
    dt = bs.DeviceCoderTables.of(eb, "cuda")
    assert dt.host.cdf.shape[0] == 192
    _check_kernels(dt.host, dt, (2, 1, 1, 192, 0, 192, 1), seed=3, null_index=True)


def test_kernels_read_tables_too_large_for_lds_from_global_memory():
    n_t, size = 48, 2050                                      # 48 x 2049 x 2 bytes = 196,704: above a CU's 160 KB of LDS
    rng = np.random.default_rng(1)
    cdf = np.zeros((n_t, size), dtype=np.int32)
    for k in range(n_t):
        cdf[k, 1:-1] = np.sort(rng.choice(np.arange(1, 65536), size=size - 2, replace=False))
        cdf[k, -1] = 65536
    t = bs.Tables(cdf, np.full(n_t, size, dtype=np.int32), rng.integers(-1000, 0, n_t).astype(np.int32))
    dt = bs.DeviceCoderTables.build(t, "cuda")
    assert dt.packed is None and dt.lds_bytes > dt.lds_limit
    _check_kernels(t, dt, (2, 4, 4, 64, 0, 32, 2), seed=5)
    _check_kernels(t, dt, (1, 1, 65, 3, 1, 1, 2), seed=6)


# ----------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def reference(codec):
    """Host-coded strings and the likelihood path's reconstruction of one batch, per quality: computed once."""
    x = synth.synth_image(2, 64, 128, seed=5).cuda()
    ref = {}
    codec.coder = "host"
    with torch.no_grad():
        for q in (0, 2.5, 10):
            ref[q] = (codec.compress(x, quality=q), codec.forward_single_quality(x, q)["x_hat"].clone())
    return x, ref


@pytest.mark.parametrize("q", [0, 2.5, 10])
def test_device_coder_gives_the_host_coders_strings_and_decodes_them(codec, reference, host_coder_forbidden, q):
    net = codec
    x, ref = reference
    enc_h, x_hat = ref[q]
    net.coder = "device"
    try:
        with torch.no_grad(), host_coder_forbidden():
            enc_d = net.compress(x, quality=q)
            assert len(enc_d["strings"][0]) == (10 if q == 0 else 20) and len(enc_d["strings"][1]) == 2
            assert all(isinstance(s, bytes) for row in enc_d["strings"][0] for s in row)
            assert enc_d["strings"] == enc_h["strings"]                   # all 20 B + B of them, byte for byte
            assert torch.equal(net.decompress(enc_d["strings"], enc_d["shape"], quality=q)["x_hat"], x_hat)
            assert torch.equal(net.decompress(enc_h["strings"], enc_h["shape"], quality=q)["x_hat"], x_hat)   # host -> device
    finally:
        net.coder = "host"
    with torch.no_grad():                                                 # device -> host
        assert torch.equal(net.decompress(enc_d["strings"], enc_d["shape"], quality=q)["x_hat"], x_hat)


def test_per_image_paths(pic, host_coder_forbidden):
    net = pic
    x = synth.synth_image(2, 64, 64, seed=11).cuda()
    qs = [0.5, 5]
    with torch.no_grad():
        net.coder = "host"
        items_h = net.compress_per_image(x, qs)
        dec_h = net.decompress_per_image(items_h)["x_hat"]
        net.coder = "device"
        try:
            with host_coder_forbidden():
                items_d = net.compress_per_image(x, qs)
                dec_d = net.decompress_per_image(items_d)["x_hat"]
        finally:
            net.coder = "host"
    assert [it["strings"] for it in items_d] == [it["strings"] for it in items_h]
    assert [(it["shape"], it["quality"]) for it in items_d] == [(it["shape"], it["quality"]) for it in items_h]
    assert torch.equal(dec_d, dec_h)


def test_quality_map_paths(pic, host_coder_forbidden):
    net = pic
    x = synth.synth_image(1, 64, 64, seed=12).cuda()
    qmap = torch.full((1, 4, 4), 0.3, dtype=torch.float64)
    qmap[0, :, 2:] = 4.0
    with torch.no_grad():
        net.coder = "host"
        items_h = net.compress_quality_map(x, qmap)
        dec_h = net.decompress_quality_map(items_h)["x_hat"]
        net.coder = "device"
        try:
            with host_coder_forbidden():
                items_d = net.compress_quality_map(x, qmap)
                dec_d = net.decompress_quality_map(items_d)["x_hat"]
        finally:
            net.coder = "host"
    assert [it["strings"] for it in items_d] == [it["strings"] for it in items_h]
    assert torch.equal(dec_d, dec_h)


def test_truncated_stream_raises_and_the_plan_stays_usable(codec):
    """The device twin of test_corrupt_stream_is_detected_or_changes_output."""
    net = codec
    x = synth.synth_image(1, 64, 64, seed=8).cuda()
    with torch.no_grad():
        net.coder = "host"
        enc = net.compress(x, quality=2.5)
        x_hat = net.forward_single_quality(x, 2.5)["x_hat"].clone()
        strings = [[list(s) for s in enc["strings"][0]], list(enc["strings"][1])]
        strings[0][3][0] = strings[0][3][0][:8]                  # truncate one slice stream
        net.coder = "device"
        try:
            with pytest.raises(VamError, match=r"image 0, slice 3\): bitstream truncated"):
                net.decompress(strings, enc["shape"], quality=2.5)
            n_plans = len(net._dec_plans)
            assert torch.equal(net.decompress(enc["strings"], enc["shape"], quality=2.5)["x_hat"], x_hat)
            assert len(net._dec_plans) == n_plans                # the same plan
        finally:
            net.coder = "host"


def test_bad_coder_setting_is_a_value_error(codec):
    net = codec
    x = synth.synth_image(1, 64, 64, seed=8).cuda()
    with torch.no_grad():
        enc = net.compress(x, quality=0)
        net.coder = "gpu"
        try:
            with pytest.raises(ValueError, match="coder"):
                net.compress(x, quality=0)
            with pytest.raises(ValueError, match="coder"):
                net.decompress(enc["strings"], enc["shape"], quality=0)
        finally:
            net.coder = "host"


def test_plan_reuse_and_table_rebuild(codec):
    """Two images back to back on one cached decode plan each give their own reconstruction; update() rebuilds the device
    tables.  Last in the file: update() drops the model's plans."""
    net = codec
    xa, xb = synth.synth_image(1, 64, 64, seed=21).cuda(), synth.synth_image(1, 64, 64, seed=22).cuda()
    net.coder = "device"
    try:
        with torch.no_grad():
            ea, eb_ = net.compress(xa, quality=2.5), net.compress(xb, quality=2.5)
            assert ea["strings"] != eb_["strings"]
            da = net.decompress(ea["strings"], ea["shape"], quality=2.5)["x_hat"]
            n_plans = len(net._dec_plans)
            db = net.decompress(eb_["strings"], eb_["shape"], quality=2.5)["x_hat"]
            assert len(net._dec_plans) == n_plans
            assert torch.equal(da, net.forward_single_quality(xa, 2.5)["x_hat"])
            assert torch.equal(db, net.forward_single_quality(xb, 2.5)["x_hat"])
            old = bs.DeviceCoderTables.of(net.gaussian_conditional, "cuda")
            assert bs.DeviceCoderTables.of(net.gaussian_conditional, "cuda") is old
            net.update()
            new = bs.DeviceCoderTables.of(net.gaussian_conditional, "cuda")
            assert new is not old and new.key != old.key
            assert net.compress(xa, quality=2.5)["strings"] == ea["strings"]
            assert torch.equal(net.decompress(ea["strings"], ea["shape"], quality=2.5)["x_hat"], da)
    finally:
        net.coder = "host"
