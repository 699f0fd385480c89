"""Lane-split rANS streams on the host (csrc/rans_core.h): a stream of n elements as K independent
lanes behind a header of K lengths.  The lanes strings are the host coder's (csrc/rans.cpp) on every strided subset, K = 1
is its string with no header, a header that does not add up is refused whole, and a lane that fails leaves the others
alone.  Everything is bit-exact; no GPU is needed."""
import argparse
import os
import subprocess

import numpy as np
import pytest
import torch

import vampic
from vampic import _lib as L
from vampic import bitstream as bs
from conftest import README_ARGS
from test_rans_core_cpu import _sanitizer_compiler, _stream_case, _tables, _targs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 63, 64, 65, 512, 4097]
LANES = [1, 2, 8, 64]
BAD_STREAM, TRUNCATED = 6, 1


@pytest.fixture(scope="module")
def gauss_tables():
    """The real 64 x 3133 Gaussian tables."""
    from vampic.entropy_models import GaussianConditional, get_scale_table
    g = GaussianConditional(None)
    g.update_scale_table(get_scale_table())
    t = bs.Tables.of(g)
    assert t.cdf.shape == (64, 3133)
    return t


@pytest.fixture(scope="module", params=["small", "gauss"])
def tables(request, gauss_tables):
    return _tables() if request.param == "small" else gauss_tables


def _header(lanes):
    return np.array([len(s) // 4 for s in lanes], dtype="<u4").tobytes()


def _expected(sym, idx, t, K, layer=None, sel=0):
    """The K-word header plus the host coder's stream of every strided subset."""
    if layer is None:
        lanes = [bs.encode(sym[j::K], idx[j::K], t) for j in range(K)]
    else:
        lanes = bs.encode_streams([(sym[j::K], idx[j::K], layer[j::K], sel) for j in range(K)], t)
    assert all(len(s) % 4 == 0 and len(s) >= 8 for s in lanes)
    return (_header(lanes) if K > 1 else b"") + b"".join(lanes)


def lanes_decode(stream, idx, t, K, layer=None, sel=0, fill=-12345):
    """(status, per-lane status, out): out starts as ``fill`` everywhere."""
    i, ly = bs._i32(idx), bs._layer(layer)
    out = np.full(i.size, fill, dtype=np.int32)
    src = np.frombuffer(stream, dtype=np.uint8)
    lane_st = np.full(K, -1, dtype=np.int32)
    st = L.load().vam_rans_lanes_decode(src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size, *_targs(t),
                                        out.ctypes.data, ly.ctypes.data if ly is not None else None, sel, K, lane_st.ctypes.data)
    return st, lane_st, out


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", LENGTHS)
def test_lanes_string_is_the_header_and_the_host_coders_lanes(tables, n, K):
    t = tables
    sym, idx = _stream_case(t, n, seed=n)
    got = bs.encode_lanes(sym, idx, t, K)
    assert got == _expected(sym, idx, t, K)
    if K == 1:
        assert got == bs.encode(sym, idx, t)                  # no header
    else:
        assert len(got) == 4 * K + 4 * int(np.frombuffer(got[:4 * K], dtype="<u4").sum())
        if n < K:                                             # a lane without elements: the 8 bytes of the initial state
            empty = bs.encode(sym[:0], idx[:0], t)
            assert len(empty) == 8 and got.endswith(empty)
    st, lane_st, out = lanes_decode(got, idx, t, K)
    assert st == 0 and (lane_st == 0).all() and np.array_equal(out, sym)
    assert np.array_equal(bs.decode_lanes(got, idx, t, K), sym)


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", [0, 65, 512])
def test_lanes_layer_selection_behaves_as_in_the_core(tables, n, K):
    t = tables
    sel = 3
    sym, idx = _stream_case(t, n, seed=100 + n)
    layer = np.random.default_rng(n + K).choice(np.array([0, 1, 3, 0xFF], dtype=np.uint8), size=n)
    got = bs.encode_lanes(sym, idx, t, K, layer, sel)
    assert got == _expected(sym, idx, t, K, layer, sel)
    st, lane_st, out = lanes_decode(got, idx, t, K, layer, sel, fill=-7)
    assert st == 0 and (lane_st == 0).all()
    assert np.array_equal(out[layer == sel], sym[layer == sel]) and (out[layer != sel] == -7).all()


@pytest.mark.parametrize("K", LANES)
def test_nhwc_window_variants_equal_the_flat_calls(tables, K):
    t = tables
    lib = L.load()
    B, h, w, ld, c0, Cw = 2, 3, 5, 7, 2, 4                    # a window inside the row: c0 > 0, ld > C
    rng = np.random.default_rng(9 + K)
    n = Cw * h * w
    for image in range(B):
        for with_idx in (True, False):
            sym_f, idx_f = _stream_case(t, n, seed=20 + image)
            if not with_idx:                                 # a null index pointer: table index = channel
                idx_f = np.repeat(np.arange(Cw, dtype=np.int32), h * w)
                sym_f = (t.offsets[idx_f] + rng.integers(-1, 4, n)).astype(np.int32)
            sym = rng.integers(-9, 9, (B, h, w, ld)).astype(np.int32)
            idx = rng.integers(0, t.cdf.shape[0], (B, h, w, ld)).astype(np.int32)
            sym[image, :, :, c0:c0 + Cw] = sym_f.reshape(Cw, h, w).transpose(1, 2, 0)
            idx[image, :, :, c0:c0 + Cw] = idx_f.reshape(Cw, h, w).transpose(1, 2, 0)
            layer = rng.choice(np.array([0, 3], dtype=np.uint8), size=(B, h, w, ld))
            for ly, sel in ((None, 0), (layer, 3)):
                ly_f = None if ly is None else np.ascontiguousarray(ly[image, :, :, c0:c0 + Cw].transpose(2, 0, 1)).reshape(-1)
                ref = bs.encode_lanes(sym_f, idx_f, t, K, ly_f, sel)
                buf = np.empty(bs.lanes_capacity(n, K), dtype=np.uint8)
                nb = lib.vam_rans_lanes_encode_nhwc(sym.ctypes.data, idx.ctypes.data if with_idx else None,
                                                    ly.ctypes.data if ly is not None else None, sel, image, h, w, ld, c0, Cw,
                                                    *_targs(t), buf.ctypes.data, buf.size, K, None)
                assert nb > 0 and buf[:nb].tobytes() == ref
                out = np.full((B, h, w, ld), -7, dtype=np.int32)
                lane_st = np.full(K, -1, dtype=np.int32)
                st = lib.vam_rans_lanes_decode_nhwc(buf.ctypes.data, nb, idx.ctypes.data if with_idx else None,
                                                    ly.ctypes.data if ly is not None else None, sel, image, h, w, ld, c0, Cw,
                                                    *_targs(t), out.ctypes.data, K, lane_st.ctypes.data)
                assert st == 0 and (lane_st == 0).all()
                _, _, flat = lanes_decode(ref, idx_f, t, K, ly_f, sel, fill=-7)
                want = np.full((B, h, w, ld), -7, dtype=np.int32)                # nothing outside the window is written
                want[image, :, :, c0:c0 + Cw] = flat.reshape(Cw, h, w).transpose(1, 2, 0)
                assert np.array_equal(out, want)


def _refused(stream, idx, t, K):
    st, lane_st, out = lanes_decode(stream, idx, t, K)
    assert st == BAD_STREAM and (lane_st == BAD_STREAM).all() and (out == 0).all()
    with pytest.raises(L.VamError, match="lane 0"):
        bs.decode_lanes(stream, idx, t, K)


@pytest.mark.parametrize("K", [2, 8, 64])
def test_headers_that_do_not_add_up_are_refused_whole(tables, K):
    t = tables
    sym, idx = _stream_case(t, 512, seed=7)
    good = bs.encode_lanes(sym, idx, t, K)
    head = np.frombuffer(good[:4 * K], dtype="<u4")
    for cut in (0, 4, 4 * K - 4, 4 * K - 1):                 # shorter than the header
        _refused(good[:cut], idx, t, K)
    for j in (0, K - 1):
        for value in (1, 0, int(head[j]) + 1, int(head[j]) - 1, 0xFFFFFFFF):     # L_j = 1, the sum off by one word either way
            h2 = head.copy()
            h2[j] = value
            _refused(h2.tobytes() + good[4 * K:], idx, t, K)
    _refused(good + b"\0\0\0\0", idx, t, K)                  # the string one word longer / shorter than its header says
    _refused(good[:-4], idx, t, K)
    _refused(np.full(K, 0xFFFFFFFF, dtype="<u4").tobytes() + good[4 * K:], idx, t, K)     # sums that would wrap 32 bits
    st, lane_st, out = lanes_decode(good, idx, t, K)         # and the string itself is fine
    assert st == 0 and np.array_equal(out, sym)


@pytest.mark.parametrize("K", [2, 8])
def test_a_cut_inside_the_last_lane_fails_that_lane_alone(tables, K):
    t = tables
    n = 512
    sym, idx = _stream_case(t, n, seed=11)
    good = bs.encode_lanes(sym, idx, t, K)
    head = np.frombuffer(good[:4 * K], dtype="<u4").copy()
    assert head[K - 1] >= 3
    head[K - 1] -= 1                                          # the header adjusted: the sum still matches
    st, lane_st, out = lanes_decode(head.tobytes() + good[4 * K:-4], idx, t, K)
    assert st == TRUNCATED                                    # the stream's status: that of its lowest failing lane
    assert (lane_st[:K - 1] == 0).all() and lane_st[K - 1] == TRUNCATED
    for j in range(K - 1):
        assert np.array_equal(out[j::K], sym[j::K])           # lower lanes decode
    last, want = out[K - 1::K], sym[K - 1::K]
    good_n = int(np.argmax(last != want)) if (last != want).any() else len(want)
    assert good_n < len(want) and (last[good_n:] == 0).all()  # a right prefix, then zeros from the failure on
    with pytest.raises(L.VamError, match=f"lane {K - 1}: bitstream truncated"):
        bs.decode_lanes(head.tobytes() + good[4 * K:-4], idx, t, K)
    # a failure in lane 0 and one in the last lane: the stream reports lane 0's
    idx_bad = idx.copy()
    idx_bad[0] = t.cdf.shape[0] + 5
    st, lane_st, _ = lanes_decode(head.tobytes() + good[4 * K:-4], idx_bad, t, K)
    assert st == 2 and lane_st[0] == 2 and lane_st[K - 1] == TRUNCATED


@pytest.mark.parametrize("lanes", [0, 3, 6, 128, -2, 2.0, "8", True, None])
def test_lanes_outside_the_powers_of_two_are_value_errors(lanes):
    t = _tables()
    sym, idx = _stream_case(t, 64, seed=1)
    with pytest.raises(ValueError, match="power of two"):
        bs.encode_lanes(sym, idx, t, lanes)
    with pytest.raises(ValueError, match="power of two"):
        bs.decode_lanes(b"\0" * 64, idx, t, lanes)
    buf = np.empty(4096, dtype=np.uint8)                      # the export itself refuses what ctypes lets through
    if isinstance(lanes, int) and not isinstance(lanes, bool):
        rc = L.load().vam_rans_lanes_encode(sym.ctypes.data, idx.ctypes.data, sym.size, *_targs(t), buf.ctypes.data, buf.size,
                                            None, 0, lanes, None)
        assert rc < 0


@pytest.fixture(scope="module")
def cpu_model():
    return vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu").eval()


def test_model_coder_lanes_is_validated_before_any_gpu_use(cpu_model):
    net = cpu_model
    assert net.coder_lanes == 1 and net._coder_lanes() == 1
    x = torch.zeros(1, 3, 64, 64)
    try:
        for bad in (0, 3, 128, "8", 2.0, None):
            net.coder_lanes = bad
            with pytest.raises(ValueError, match="coder_lanes"):
                net.compress(x, quality=2.5)
            with pytest.raises(ValueError, match="coder_lanes"):
                net.decompress([[[b""]], [b""]], (1, 1), quality=2.5)
            with pytest.raises(ValueError, match="coder_lanes"):
                net.compress_per_image(x, [2.5])
            with pytest.raises(ValueError, match="coder_lanes"):
                net.decompress_per_image([{"strings": [[[b""]], [b""]], "shape": (1, 1), "quality": 2.5}])
            with pytest.raises(ValueError, match="coder_lanes"):
                net.compress_quality_map(x, torch.ones(1, 4, 4, dtype=torch.float64))
        for good in (1, 2, 4, 8, 16, 32, 64):
            net.coder_lanes = good
            assert net._coder_lanes() == good
    finally:
        net.coder_lanes = 1


def test_size_control_refuses_lanes_other_than_one(cpu_model):
    """coded_size_curve, qualities_for_bytes and compress_to_bytes bracket the bytes of K = 1 strings."""
    net = cpu_model
    x = torch.zeros(1, 3, 64, 64)
    net.coder_lanes = 8
    try:
        for call in (lambda: net.coded_size_curve(x, [0, 1.0]), lambda: net.qualities_for_bytes(x, 4000.0),
                     lambda: net.compress_to_bytes(x, 4000.0)):
            with pytest.raises(ValueError, match=r"coder_lanes = 1 strings"):
                call()
    finally:
        net.coder_lanes = 1


def test_lanes_under_address_and_undefined_sanitizers(tmp_path):
    """tests/rans_lanes_check.cpp: a stand-alone program over csrc/rans_core.h — round trips over the n x K grid, every
    truncation length of a K = 8 string, every single-word header corruption, strings of random bytes — built with
    -fsanitize=address,undefined and run as a process of its own."""
    src = os.path.join(ROOT, "tests", "rans_lanes_check.cpp")
    inc = os.path.join(ROOT, "efficient-pic-with-variance-aware-masking_amd", "csrc")
    assert os.path.exists(os.path.join(inc, "rans_core.h"))
    exe, errors = str(tmp_path / "rans_lanes_check"), []
    compilers = list(_sanitizer_compiler())
    if not compilers:
        pytest.skip("no host C++ compiler")
    for cxx in compilers:
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", inc, src, "-o", exe]
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, f"{cxx} does not compile the program at all:\n{r.stderr[-3000:]}"
        r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        if r.returncode == 0:
            break
        errors.append(f"{cxx}: {r.stderr[-300:]}")
    else:
        pytest.skip("no host compiler links the sanitizer runtime: " + " | ".join(errors))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rans_lanes_check: ok" in r.stdout
