"""Embedded containers with an interleaved base (csrc/rans_device.hip): the two window kernels against
the host exports — strings, the strict decode, guard channels and rows, refused inputs — and embedded.encode_batch /
EmbeddedDecoder with ``base_lanes`` against the host coder and the ``base_lanes=1`` containers.  Everything is bit-exact."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import _lib as L, bitstream as bs, embedded as EB, ops              # noqa: E402
from base_lanes_cases import FILL, GEOMETRIES, window_case, window_jobs          # noqa: E402
from test_gpu_embedded_schedule import _net, _same, _schedule, _x                # noqa: E402

LANES = [1, 8, 64]


# ----------------------------------------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def dt():
    d = bs.DeviceCoderTables.of(_net().gaussian_conditional, "cuda")
    assert d.packed is not None and 0 < d.lds_bytes <= d.lds_limit                # the LDS path
    return d


def _views(sym, idx, geom, null_index):
    B, h, w, ld, c0, C, ns = geom
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    return ops.IView(d_sym, c0, C * ns), None if null_index else ops.IView(d_idx, c0, C * ns)


def _decode(strings, iv, geom, dt, K, up=None):
    """(status, out [B, h, w, ld]) of one decode launch into a FILLed buffer with a guard image on either side."""
    B, h, w, ld, c0, C, ns = geom
    guard = torch.full((B + 2, h, w, ld), FILL, dtype=torch.int32, device="cuda")
    up = bs.upload_streams(strings, "cuda") if up is None else up
    bs.decode_window_interleaved_uploaded(up, 0, iv, ops.IView(guard[1:B + 1], c0, C * ns), ns, C, dt, K)
    g = guard.cpu().numpy()
    assert (g[0] == FILL).all() and (g[-1] == FILL).all()                         # the guard rows
    assert (g[1:-1, ..., :c0] == FILL).all() and (g[1:-1, ..., c0 + ns * C:] == FILL).all()   # the guard channels
    return up.status[:B * ns].cpu().numpy(), g[1:-1]


def _window(out, geom, k):
    """Stream k = slice * B + image of an NHWC buffer, in stream order [C, h, w], flat."""
    B, h, w, ld, c0, C, ns = geom
    s, b = divmod(k, B)
    return out[b, :, :, c0 + s * C:c0 + (s + 1) * C].transpose(2, 0, 1).reshape(-1)


@pytest.mark.parametrize("null_index", [False, True])
@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_kernels_equal_the_host_exports(dt, geom, K, null_index):
    B, h, w, ld, c0, C, ns = geom
    t = dt.host
    sym, idx = window_case(t, geom, seed=sum(geom) + K, channel_index=null_index)
    jobs = window_jobs(sym, idx, geom)
    want = bs.encode_interleaved_streams(jobs, t, lanes=K)
    sv, iv = _views(sym, idx, geom, null_index)
    got = bs.encode_window_interleaved_device(sv, iv, ns, C, dt, K)
    assert [s for row in got for s in row] == want            # [slice][image] == stream order
    if K == 1:
        assert got == bs.encode_streams_device(sv, iv, ns, C, dt)
    status, out = _decode(want, iv, geom, dt, K)
    assert not status.any()
    ref = np.full_like(sym, FILL)
    ref[..., c0:c0 + ns * C] = sym[..., c0:c0 + ns * C]
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("K", LANES)
def test_kernels_refuse_short_strings_bad_indexes_and_offsets(dt, K):
    geom = GEOMETRIES[2]                                      # one image, n = 1000
    B, h, w, ld, c0, C, ns = geom
    t = dt.host
    sym, idx = window_case(t, geom, seed=70 + K)
    (s0, i0), = window_jobs(sym, idx, geom)
    whole, = bs.encode_interleaved_streams([(s0, i0)], t, lanes=K)
    sv, iv = _views(sym, idx, geom, False)
    for cut in (len(whole) - 4, 8 * K - 4):                   # one word short; not even the K states
        status, out = _decode([whole[:cut]], iv, geom, dt, K)
        _, count, st = bs.decode_interleaved_counted(whole[:cut], i0, t, K)
        assert st == 0 and count < 1000 and status.tolist() == [1]
        g0 = count // K * K                                   # the failing group: zeros from there on, symbols before
        got = _window(out, geom, 0)
        assert np.array_equal(got[:g0], s0.reshape(-1)[:g0]) and not got[g0:].any()
    bad = idx.copy()
    bad[0, 5, 3, c0 + 2] = t.cdf.shape[0]                     # element (2 * 10 + 5) * 20 + 3 = 503
    status, out = _decode([whole], ops.IView(torch.from_numpy(bad).cuda(), c0, C * ns), geom, dt, K)
    got = _window(out, geom, 0)
    assert status.tolist() == [2] and np.array_equal(got[:503 // K * K], s0.reshape(-1)[:503 // K * K]) and not got[503 // K * K:].any()
    with pytest.raises(L.VamError, match="index out of range"):
        bs.encode_window_interleaved_device(sv, ops.IView(torch.from_numpy(bad).cuda(), c0, C * ns), ns, C, dt, K)
    for offset, length in ((2, None), (-4, None), (1 << 40, None), (None, 1 << 30), (None, -1)):
        up = bs.upload_streams([whole], "cuda")
        if offset is not None:
            up.buf[:8].view(torch.int64)[0] = offset
        else:
            up.buf[8:12].view(torch.int32)[0] = length
        status, out = _decode([whole], iv, geom, dt, K, up=up)
        assert status.tolist() == [6] and (out == FILL).all(), (offset, length)                # nothing written
    for lanes in (0, 3, 128):
        with pytest.raises(ValueError, match="power of two"):
            bs.encode_window_interleaved_device(sv, iv, ns, C, dt, lanes)


def test_one_failed_stream_leaves_the_others_whole(dt):
    geom = GEOMETRIES[0]                                      # 6 streams of 12 elements share a wave at K = 8
    B, h, w, ld, c0, C, ns = geom
    t = dt.host
    sym, idx = window_case(t, geom, seed=5)
    want = bs.encode_interleaved_streams(window_jobs(sym, idx, geom), t, lanes=8)
    strings = list(want)
    strings[4] = strings[4][:-4]
    status, out = _decode(strings, _views(sym, idx, geom, False)[1], geom, dt, 8)
    assert status.tolist() == [0, 0, 0, 0, 1, 0]
    for k in range(6):
        if k != 4:
            assert np.array_equal(_window(out, geom, k), _window(sym, geom, k)), k
    assert not _window(out, geom, 4)[8:].any()


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
    geom = GEOMETRIES[2]
    B, h, w, ld, c0, C, ns = geom
    sym, idx = window_case(t, geom, seed=9)
    want = bs.encode_interleaved_streams(window_jobs(sym, idx, geom), t, lanes=8)
    sv, iv = _views(sym, idx, geom, False)
    assert bs.encode_window_interleaved_device(sv, iv, ns, C, big, 8) == [want]
    status, out = _decode(want, iv, geom, big, 8)
    assert not status.any() and np.array_equal(_window(out, geom, 0), _window(sym, geom, 0))
    status, out = _decode([want[0][:-4]], iv, geom, big, 8)
    assert status.tolist() == [1]


# ----------------------------------------------------------------------------------------------- model
SHAPES = {"2x64x64": (2, 64, 64, 3), "1x128x192": (1, 128, 192, 4)}
GRID = [(shape, Kb, K) for shape in SHAPES for Kb in (8, 64) for K in (1, 64)]
QS = [0, 0.5, 2.5, 10, 1.0]
_CODED, _OUT = {}, {}


def _input(shape):
    if shape not in _CODED:
        B, H, W, seed = SHAPES[shape]
        _CODED[shape] = _x(B, H, W, seed=seed)
    return _CODED[shape]


def _coded(shape, coder, K, Kb, scheduled=False):
    """The containers of one input per (coder, lanes, base_lanes), encoded once per session."""
    key = (shape, coder, K, Kb, scheduled)
    if key not in _CODED:
        x = _input(shape)
        kw = dict(schedule=_schedule(*SHAPES[shape][:3])) if scheduled else {}
        _CODED[key] = EB.encode_batch(_net(), x, coder=coder, lanes=K, base_lanes=Kb, **kw)
    return _CODED[key]


def _reference(shape, K):
    """decode() and decode_qualities(QS) of the base_lanes = 1 containers on the host coder: the yardstick."""
    if (shape, K) not in _OUT:
        dec = EB.EmbeddedDecoder(_net(), _coded(shape, "host", K, 1), coder="host")
        _OUT[shape, K] = (dec.decode(), dec.decode_qualities(QS), dec.available())
    return _OUT[shape, K]


@contextlib.contextmanager
def host_coder_forbidden(monkeypatch):
    """Any call of a host coder entry point fails the test: without it the comparisons would pass with ``coder`` ignored."""
    def refuse(*a, **k):
        raise AssertionError("the host coder ran in a coder='device' call")
    with monkeypatch.context() as mp:
        for name in ("encode", "decode", "encode_streams", "decode_streams", "encode_lanes", "decode_lanes", "encode_interleaved",
                     "encode_interleaved_streams", "decode_prefix_streams", "prefix_bytes", "decode_interleaved_counted",
                     "decode_interleaved_strict", "resume_prefix_streams"):
            mp.setattr(bs, name, refuse)
        yield


@pytest.mark.parametrize("shape,Kb,K", GRID)
def test_device_containers_equal_the_host_containers(shape, Kb, K):
    host, dev, one = _coded(shape, "host", K, Kb), _coded(shape, "device", K, Kb), _coded(shape, "host", K, 1)
    assert dev == host
    n = 32 * (SHAPES[shape][1] // 16) * (SHAPES[shape][2] // 16)
    for c, o in zip(host, one):
        assert c["format"] == "embedded-4" and c["lanes"] == K and c["base_lanes"] == Kb
        assert set(c) == {"format", "shape", "z", "base", "embedded", "marks", "lanes", "base_lanes"}
        assert c["embedded"] == o["embedded"] and c["marks"] == o["marks"] and c["shape"] == o["shape"]    # those of base_lanes = 1
        assert c["z"] != o["z"] and all(a != b for a, b in zip(c["base"], o["base"]))
        assert all(len(s) == 1 and 8 * Kb <= len(s[0]) <= bs.interleaved_capacity(n, Kb) for s in c["base"])
        assert EB._check_container(c) == K


@pytest.mark.parametrize("K", [1, 64])
def test_one_base_lane_is_todays_container(K):
    net, x = _net(), _input("2x64x64")
    for coder in ("host", "device"):
        got = EB.encode_batch(net, x, coder=coder, lanes=K, base_lanes=1)
        assert got == EB.encode_batch(net, x, coder=coder, lanes=K) == _coded("2x64x64", "host", K, 1)
        keys = {"format", "shape", "z", "base", "embedded", "marks"} | ({"lanes"} if K > 1 else set())
        assert all(set(c) == keys and c["format"] == ("embedded-1" if K == 1 else "embedded-2") for c in got)
    net.coder_lanes = 8                                       # never read: base_lanes is the argument's
    try:
        assert EB.encode_batch(net, x, lanes=K) == _coded("2x64x64", "host", K, 1)
    finally:
        net.coder_lanes = 1
    for bad in (0, 3, 128, "8", None):
        with pytest.raises(ValueError, match="power of two"):
            EB.encode_batch(net, x, base_lanes=bad)


@pytest.mark.parametrize("shape,Kb,K", GRID)
def test_either_coder_reads_the_others_containers(shape, Kb, K):
    net = _net()
    want, want_q, avail = _reference(shape, K)
    dev_dec = EB.EmbeddedDecoder(net, _coded(shape, "host", K, Kb), coder="device")
    host_dec = EB.EmbeddedDecoder(net, _coded(shape, "device", K, Kb), coder="host")
    assert dev_dec.base_lanes == host_dec.base_lanes == Kb and dev_dec.lanes == host_dec.lanes == K
    for dec in (dev_dec, host_dec):
        assert np.array_equal(dec.available(), avail)
        assert _same(dec.decode(), want)
        for q, a, b in zip(QS, dec.decode_qualities(QS), want_q):
            assert _same(a, b), q
    assert dev_dec.bits(2.5) == host_dec.bits(2.5)


@pytest.mark.parametrize("Kb,K", [(64, 64), (8, 1)])
def test_device_session_never_calls_the_host_coder(monkeypatch, Kb, K):
    net, x = _net(), _input("2x64x64")
    want, want_q, _ = _reference("2x64x64", K)
    with host_coder_forbidden(monkeypatch):
        cs = EB.encode_batch(net, x, coder="device", lanes=K, base_lanes=Kb)
        dec = EB.EmbeddedDecoder(net, cs, coder="device")
        assert dec.idx_r is None and (dec.available() == 512).all()
        out, outs = dec.decode(), dec.decode_qualities(QS)
        res = EB.EmbeddedDecoder(net, [EB.truncate(c, q=1) for c in cs], coder="device", resumable=True)
        res.extend([EB.delta(c, h) for c, h in zip(cs, res.containers)])
        out_r = res.decode()
    assert cs == _coded("2x64x64", "host", K, Kb)
    assert _same(out, want) and _same(out_r, want) and all(_same(a, b) for a, b in zip(outs, want_q))


@pytest.mark.parametrize("coder", ["host", "device"])
def test_a_scheduled_container_decodes_stage_by_stage(coder):
    net, shape = _net(), "2x64x64"
    cs, one = _coded(shape, coder, 8, 8, scheduled=True), _coded(shape, "host", 8, 1, scheduled=True)
    assert EB._same(cs, _coded(shape, "host", 8, 8, scheduled=True))              # the schedule's index is an array
    for c, o in zip(cs, one):
        assert c["format"] == "embedded-4" and o["format"] == "embedded-3" and (c["lanes"], c["base_lanes"]) == (8, 8)
        assert set(c) == set(o) | {"base_lanes"}
        for key in set(o) - {"format", "z", "base", "schedule"}:
            assert c[key] == o[key], key
        assert np.array_equal(c["schedule"]["index"], o["schedule"]["index"]) and c["schedule"]["levels"] == o["schedule"]["levels"]
    stages = list(cs[0]["marks"]["stage"])
    want = EB.EmbeddedDecoder(net, one, coder="host").decode_stages(stages)
    dec = EB.EmbeddedDecoder(net, cs, coder=coder)
    assert dec.scheduled and dec.base_lanes == 8
    for k, a, b in zip(stages, dec.decode_stages(stages), want):
        assert _same(a, b), k
    cut = EB.EmbeddedDecoder(net, [EB.truncate(c, stage=1) for c in cs], coder=coder)
    assert _same(cut.decode_stages([1])[0], want[1])
    with pytest.raises(ValueError, match="decode_stages"):
        dec.decode_qualities([2.5])
    with pytest.raises(ValueError, match="scheduled .* or plain containers, not both"):
        EB.EmbeddedDecoder(net, [cs[0], _coded(shape, "host", 8, 8)[1]], coder=coder)


@pytest.mark.parametrize("coder", ["host", "device"])
def test_a_resumable_decoder_fed_through_delta_and_extend_equals_a_fresh_one(coder):
    net, shape = _net(), "1x128x192"
    cs = _coded(shape, "host", 64, 64)
    steps = [[EB.truncate(c, slice_bytes=[0] * net.ns0) for c in cs],
             [EB.truncate(c, slice_bytes=[len(s) // 3 | 1 for s in c["embedded"]]) for c in cs],
             [EB.truncate(c, slice_bytes=[len(s) * 2 // 3 | 1 for s in c["embedded"]]) for c in cs], cs]
    dec = EB.EmbeddedDecoder(net, steps[0], coder=coder, resumable=True)
    for held, now in zip(steps, steps[1:]):
        dec.extend([EB.delta(c, h) for c, h in zip(now, held)])
        fresh = EB.EmbeddedDecoder(net, now, coder=coder)
        assert np.array_equal(dec.available(), fresh.available()) and _same(dec.decode(), fresh.decode())
    assert _same(dec.decode(), _reference(shape, 64)[0])


@pytest.mark.parametrize("coder", ["host", "device"])
@pytest.mark.parametrize("Kb", [8, 64])
def test_a_short_base_slice_is_refused_by_name(coder, Kb):
    net = _net()
    cs = [dict(c) for c in _coded("2x64x64", "host", 1, Kb)]
    cs[1]["base"] = [list(s) for s in cs[1]["base"]]
    cs[1]["base"][3][0] = cs[1]["base"][3][0][:-4]            # slice 3 of image 1 loses its last word
    with pytest.raises(ValueError, match=r"base stream \(image 1, slice 3\): bitstream truncated"):
        EB.EmbeddedDecoder(net, cs, coder=coder)
    cz = [dict(c) for c in _coded("2x64x64", "host", 1, Kb)]
    cz[0]["z"] = [cz[0]["z"][0][:8 * Kb - 4]]                 # not even the states
    with pytest.raises(ValueError, match=r"z stream \(image 0\): bitstream truncated"):
        EB.EmbeddedDecoder(net, cz, coder=coder)
    dec = EB.EmbeddedDecoder(net, _coded("2x64x64", "host", 1, Kb), coder=coder)             # the plans serve the next decoder
    assert _same(dec.decode(), _reference("2x64x64", 1)[0])


def test_mixed_base_lanes_are_refused():
    net = _net()
    c8, c64, c1 = _coded("2x64x64", "host", 1, 8), _coded("2x64x64", "host", 1, 64), _coded("2x64x64", "host", 1, 1)
    for coder in ("host", "device"):
        with pytest.raises(ValueError, match=r"same base_lanes .* got \[8, 64\]"):
            EB.EmbeddedDecoder(net, [c8[0], c64[1]], coder=coder)
        with pytest.raises(ValueError, match=r"same base_lanes .* got \[1, 8\]"):            # without the key: 1
            EB.EmbeddedDecoder(net, [c1[0], c8[1]], coder=coder)
    for bad in (0, 3, 128, None):
        with pytest.raises(ValueError, match="power of two"):
            EB.EmbeddedDecoder(net, [dict(c, base_lanes=bad) for c in c8])
    with pytest.raises(ValueError, match="base_lanes > 1"):
        EB.EmbeddedDecoder(net, [dict(c, base_lanes=1) for c in c8])


def test_evaluate_passes_base_lanes_through():
    from vampic import evaluate as EV
    net, x = _net(), _input("2x64x64")
    rows = EV.embedded_rd(net, [x[0], x[1]], [2.5], coder="device", lanes=8, base_lanes=8)
    ref = EV.embedded_rd(net, [x[0], x[1]], [2.5], coder="host", lanes=8)
    for ra, rb in zip(rows, ref):                             # x_hat is bit-identical; the PSNR's float64 sum is not ordered
        assert ra["psnr_all"] == pytest.approx(rb["psnr_all"], rel=1e-12, abs=0)
    assert all(a > b for ra, rb in zip(rows, ref) for a, b in zip(ra["bpp_all"], rb["bpp_all"]))  # 11 strings of 8 states each
