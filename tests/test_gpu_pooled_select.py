"""The kernels of csrc/pooled_select.hip (vam_pool_keys, vam_pooled_select, vam_threshold_counts) against
the restatement tests/pooled_ref.py, bit for bit, with guard regions around every output.  No model.

"Bit for bit" for a threshold: the same 32 bits, or a NaN on both sides (inf - inf in the lerp is a NaN whose sign the
host and the device choose differently; a NaN threshold keeps nothing either way)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pooled_ref as PR                                            # noqa: E402
from vampic import _lib as L, ops                                 # noqa: E402

NS = 2
QS = [0.05, 0.5, 2.5, 5.0, 9.99, 10.0]
GUARD = 64
SHAPES = [(T, n) for T in (1, 3, 12, 130, 1030) for n in (4, 512)] + [(3, 8192)]


def _weight(q, N):
    """The interpolation weight w of quality q over N elements, in the kernels' fp32 arithmetic."""
    rank = np.float32(np.float32(1.0 - q * 0.1) * np.float32(N - 1))
    return float(rank - np.floor(rank))


def _levels(N):
    """QS plus one quality whose rank over N elements is integral (w = 0), sorted; q = 5 has w >= 0.5 for every even N."""
    m = N - 1
    for k in range(max(1, m // 3), m + 1):
        q = 10.0 * (1.0 - k / m)
        if 0 < q < 10 and q not in QS and _weight(q, N) == 0.0:
            return sorted(QS + [q]), q
    raise AssertionError(f"no quality with an integral rank over {N} elements")


def _sigma(T, n, seed):
    """fp32 [T, NS, n], heavily tied (two decimals), tiles of unlike scale; from n = 512 on with a constant row, +-0,
    denormals and +inf, and with exactly one -0.0 per slice (so that the per-segment kernel, whose keys tell the zeros
    apart, selects the same values at T = 1)."""
    rng = np.random.default_rng(seed)
    s = np.abs(rng.standard_normal((T, NS, n))).astype(np.float32) * np.linspace(0.3, 2.5, T, dtype=np.float32)[:, None, None]
    s = np.round(s, 2).astype(np.float32)
    if T >= 3:
        s[1, 0] = np.float32(0.37)                                              # a constant row
    if n >= 512:
        s[0, :, 3:9] = 0.0
        s[0, :, 5] = -0.0
        s[-1, :, 20:24] = np.float32(1e-45) * np.arange(1, 5, dtype=np.float32)  # denormals
        s[T // 2, 1, 40] = np.inf
    return s


def _same_f32(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def _guarded(shape, dtype, fill):
    """(flat buffer with GUARD elements of ``fill`` on both sides, the view of ``shape`` between them)."""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + size].view(shape)


def _intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _select(sig, qs):
    """(thr fp32 [L, NS], count int32 [L, T, NS]) of the kernels on the ranked keys of ``sig``, guards checked."""
    T, ns, n = sig.shape
    keys = torch.from_numpy(PR.ranked_keys(sig).view(np.int32)).cuda()
    tbuf, thr = _guarded((len(qs), ns), torch.float32, -7.0)
    cbuf, cnt = _guarded((len(qs), T, ns), torch.int32, -7)
    ops.pooled_select(keys, qs, thr)
    ops.threshold_counts(keys, thr, cnt)
    torch.cuda.synchronize()
    assert _intact(tbuf, -7.0) and _intact(cbuf, -7)
    return thr.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("T,n", SHAPES)
def test_thresholds_and_counts_are_the_restatement_s(T, n):
    sig = _sigma(T, n, 7 * T + n)
    qs, q0 = _levels(T * n)
    assert _weight(q0, T * n) == 0.0 and _weight(5.0, T * n) >= 0.5
    want_thr = PR.thresholds(sig, qs)
    want_cnt = PR.counts(sig, want_thr)
    thr, cnt = _select(sig, qs)
    assert _same_f32(thr, want_thr), (thr, want_thr)
    assert np.array_equal(cnt, want_cnt)
    assert (np.diff(cnt.astype(np.int64), axis=0) >= 0).all() and (cnt[-1] == n).all() and np.isneginf(thr[-1]).all()


def test_a_single_nan_makes_its_slice_s_thresholds_nan_and_counts_zero():
    sig = _sigma(12, 512, 5)
    sig[7, 0, 100] = np.nan
    thr, cnt = _select(sig, QS)
    assert np.isnan(thr[:-1, 0]).all() and (cnt[:-1, :, 0] == 0).all() and (cnt[-1] == 512).all()
    want = PR.thresholds(sig, QS)
    assert _same_f32(thr, want) and np.array_equal(cnt, PR.counts(sig, want))
    assert not np.isnan(thr[:, 1]).any() and cnt[2, :, 1].sum() > 0


@pytest.mark.parametrize("n,h,c", [(4, 1, 4), (512, 4, 32)])
def test_one_tile_is_the_per_segment_kernel(n, h, c):
    """T = 1: the pool is the segment, and the thresholds are vam_variance_layers' on the same segment, bit for bit."""
    sig = _sigma(1, n, 11 + n)
    qs, _ = _levels(n)
    thr, cnt = _select(sig, qs)
    nhwc = sig[0].reshape(NS, c, h * h).transpose(2, 0, 1).reshape(1, h, h, NS * c)         # element e = c * n_pix + p
    view = ops.View(torch.from_numpy(np.ascontiguousarray(nhwc)).cuda(), 0, NS * c)
    layer = torch.empty((1, h, h, NS * c), dtype=torch.uint8, device="cuda")
    seg_thr = torch.empty((len(qs), NS), dtype=torch.float32, device="cuda")
    ops.variance_layers(view, qs, layer, n_slice=NS, thr=seg_thr)
    assert _same_f32(thr, seg_thr.cpu().numpy())
    ids = layer.cpu().numpy().reshape(h * h, NS, c)
    for k in range(len(qs)):
        assert [int((ids[:, j] <= k).sum()) for j in range(NS)] == list(cnt[k, 0])


def test_pool_keys_writes_the_rank_order_of_an_nhwc_window():
    B, h, w, c, ld, c0, T, t0 = 3, 3, 5, 8, 24, 4, 6, 2
    n = c * h * w
    rng = np.random.default_rng(2)
    buf = np.round(rng.standard_normal((B, h, w, ld)), 1).astype(np.float32)
    buf[0, 0, :3, c0:c0 + 3] = [[0.0, -0.0, np.nan], [np.inf, -np.inf, 1e-45], [-0.0, np.nan, 0.0]]
    view = ops.View(torch.from_numpy(buf).cuda(), c0, NS * c)
    seg = buf[..., c0:c0 + NS * c].reshape(B, h * w, NS, c).transpose(0, 2, 3, 1).reshape(B, NS, n)   # [C, h, w] order
    order = np.stack([[PR.rank_order(s) for s in row] for row in seg])
    for b in (1, 2):                                                            # no NaN there: the order is argsort(-s, stable)
        for j in range(NS):
            assert np.array_equal(order[b, j], np.argsort(-seg[b, j], kind="stable"))
    perm = torch.empty((B, NS, n), dtype=torch.int32, device="cuda")
    ops.variance_rank(view, perm, n_slice=NS)
    assert np.array_equal(perm.cpu().numpy(), order)
    kbuf, keys = _guarded((T, NS, n), torch.int32, -7)
    ops.pool_keys(view, perm, keys, t0=t0, n_slice=NS)
    torch.cuda.synchronize()
    got = keys.cpu().numpy()
    assert _intact(kbuf, -7) and (got[:t0] == -7).all() and (got[t0 + B:] == -7).all()      # the other tiles' rows are not touched
    assert np.array_equal(got[t0:t0 + B].view(np.uint32), PR.ranked_keys(seg))
    assert np.array_equal(got[t0:t0 + B].view(np.uint32), np.take_along_axis(PR.keys(seg), order, axis=-1))


def test_malformed_calls_are_refused_and_write_nothing():
    lib = L.load()
    T, n = 3, 64
    sig = _sigma(T, n, 1)
    keys = torch.from_numpy(PR.ranked_keys(sig).view(np.int32)).cuda()
    tbuf, thr = _guarded((40, NS), torch.float32, -7.0)
    cbuf, cnt = _guarded((40, T, NS), torch.int32, -7)
    kbuf, kout = _guarded((T, NS, n), torch.int32, -7)
    view = ops.View(torch.from_numpy(np.ascontiguousarray(sig.transpose(0, 2, 1)).reshape(T, 8, 8, NS)).cuda(), 0, NS)   # C = 1 per slice
    perm = torch.zeros((T, NS, n), dtype=torch.int32, device="cuda")
    prs = lambda *q: (C.c_double * len(q))(*q)
    s = ops.stream_ptr()
    k, t, c, o, p = keys.data_ptr(), thr.data_ptr(), cnt.data_ptr(), kout.data_ptr(), perm.data_ptr()
    many = prs(*np.linspace(0.1, 9, 33))
    bad = [
        (lambda: lib.vam_pooled_select(None, T, NS, n, prs(1.0), 1, t, s), "need keys, prs and thr_out"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, prs(1.0), 1, None, s), "need keys, prs and thr_out"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, None, 1, t, s), "need keys, prs and thr_out"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, prs(1.0), 0, t, s), "1..32 levels, got 0"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, many, 33, t, s), "1..32 levels, got 33"),
        (lambda: lib.vam_pooled_select(k, 62, NS, 1 << 18, prs(1.0), 1, t, s), "exceeds torch.quantile's 16M limit"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, prs(2.5, 0.5), 2, t, s), r"non-decreasing (prs[1] < prs[0])"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, prs(0.0, 0.5), 2, t, s), "a mark quality is > 0"),
        (lambda: lib.vam_pooled_select(k, T, NS, n, prs(float("nan")), 1, t, s), "a mark quality is > 0"),
        (lambda: lib.vam_pooled_select(k, 0, NS, n, prs(1.0), 1, t, s), "need T, n_slice, n > 0"),
        (lambda: lib.vam_threshold_counts(None, T, NS, n, t, 1, c, s), "need keys, thr and count_out"),
        (lambda: lib.vam_threshold_counts(k, T, NS, n, None, 1, c, s), "need keys, thr and count_out"),
        (lambda: lib.vam_threshold_counts(k, T, NS, n, t, 1, None, s), "need keys, thr and count_out"),
        (lambda: lib.vam_threshold_counts(k, T, NS, n, t, 0, c, s), "1..32 levels, got 0"),
        (lambda: lib.vam_threshold_counts(k, T, NS, n, t, 33, c, s), "1..32 levels, got 33"),
        (lambda: lib.vam_threshold_counts(k, 62, NS, 1 << 18, t, 1, c, s), "exceeds torch.quantile's 16M limit"),
        (lambda: lib.vam_pool_keys(None, NS, 64 * NS, 1, p, T, NS, 64, 1, o, 0, T, s), "need sigma, perm and keys"),
        (lambda: lib.vam_pool_keys(view.ptr, NS, 64 * NS, 1, None, T, NS, 64, 1, o, 0, T, s), "need sigma, perm and keys"),
        (lambda: lib.vam_pool_keys(view.ptr, NS, 64 * NS, 1, p, T, NS, 64, 1, None, 0, T, s), "need sigma, perm and keys"),
        (lambda: lib.vam_pool_keys(view.ptr, NS, 64 * NS, 1, p, T, NS, 64, 1, o, 1, T, s), "lie outside the 3 tiles"),
        (lambda: lib.vam_pool_keys(view.ptr, NS, 64 * NS, 1, p, T, NS, 64, 1, o, -1, T, s), "lie outside the 3 tiles"),
        (lambda: lib.vam_pool_keys(view.ptr, 0, 64 * NS, 1, p, T, NS, 64, 1, o, 0, T, s), "ld >= C"),
        (lambda: lib.vam_pool_keys(view.ptr, 4, 64 * NS, 1, p, 62, NS, 1 << 16, 4, o, 0, 62, s), "exceeds torch.quantile's 16M limit"),
    ]
    for call, text in bad:
        assert call() != 0
        assert text in lib.vam_last_error().decode(), (text, lib.vam_last_error().decode())
    torch.cuda.synchronize()
    assert bool((tbuf == -7.0).all()) and bool((cbuf == -7).all()) and bool((kbuf == -7).all())
    with pytest.raises(L.VamError, match="vam_pooled_select failed .*non-decreasing"):
        ops.pooled_select(keys, [2.5, 0.5], thr[:2])
    ops.pool_keys(view, perm, kout, t0=0, n_slice=NS)                           # and the well-formed calls go through
    ops.pooled_select(keys, [0.5, 2.5], thr[:2])
    ops.threshold_counts(keys, thr[:2], cnt[:2])
    torch.cuda.synchronize()
    assert _intact(tbuf, -7.0) and _intact(cbuf, -7) and _intact(kbuf, -7) and not bool((thr[:2] == -7.0).any())
