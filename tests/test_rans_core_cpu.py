"""The coder core shared by host and device (csrc/rans_core.h) against csrc/rans.cpp, its yardstick:
the host exports of the core give the host coder's bytes and symbols on every case, refuse what it refuses, and never
read outside a stream.  Everything is bit-exact; no GPU is needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import vampic
from vampic import _lib as L
from vampic import bitstream as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 63, 64, 65, 512, 4097]


def _tables(widths=(1, 3, 8, 20, 40)):
    """The construction of tests/test_bitstream_cpu.py."""
    cdfs, sizes, offs = [], [], []
    for w in widths:
        k = np.arange(-w, w + 1)
        pmf = np.exp(-0.5 * (k / (0.3 * w + 0.2)) ** 2).astype(np.float32)
        pmf /= pmf.sum()
        prob = torch.from_numpy(np.concatenate([pmf, [np.float32(1e-4)]]).astype(np.float32))
        c = bs.pmf_to_quantized_cdf(prob, 16).numpy()
        cdfs.append(c)
        sizes.append(len(c))
        offs.append(-w)
    tab = np.zeros((len(cdfs), max(sizes)), dtype=np.int32)
    for i, c in enumerate(cdfs):
        tab[i, :len(c)] = c
    return bs.Tables(tab, np.array(sizes, dtype=np.int32), np.array(offs, dtype=np.int32))


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


def _escapes(t, ci):
    """Out-of-range values of table ci: both signs, every n_bypass 1 .. 8, the value at max_value and one beyond."""
    mx, off = int(t.sizes[ci]) - 2, int(t.offsets[ci])
    vals = [mx, mx + 1, -1]                                  # raw 0 (the escape alone), raw 2, raw 1
    for nb in range(1, 9):                                  # raw needs exactly nb nibbles: 16^(nb-1) <= raw < 16^nb
        raw = min(16 ** nb - 2, 2 ** 31 - 2)                # even: above the table
        vals.append(mx + raw // 2)
        raw = min(16 ** nb - 1, 2 ** 31 - 1) if nb > 1 else 1   # odd: below it
        vals.append(-(raw + 1) // 2)
        vals.append(mx + (16 ** (nb - 1) + 1) // 2)         # the smallest raw with nb nibbles (nb = 1: raw 2)
    vals = [v for v in vals if abs(v) <= 2 ** 30]
    return np.array(vals, dtype=np.int64) + off


def _stream_case(t, n, seed):
    """Random in-range symbols with the escapes of every table spread over them."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, t.cdf.shape[0], n).astype(np.int32)
    mx = t.sizes[idx].astype(np.int64) - 2
    sym = (rng.integers(0, 1 << 30, n) % np.maximum(mx, 1) + t.offsets[idx]).astype(np.int32)
    if n >= 63:
        for ci in {0, t.cdf.shape[0] // 2, t.cdf.shape[0] - 1}:
            esc = _escapes(t, ci)
            pos = rng.choice(n, size=min(len(esc), n), replace=False)
            idx[pos], sym[pos] = ci, esc[:len(pos)].astype(np.int32)
    elif n:
        esc = _escapes(t, int(idx[0]))
        sym[0] = esc[seed % len(esc)]
    return sym, idx


def _targs(t):
    return (t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data, t.offsets.ctypes.data, t.cdf.shape[0])


def core_encode(sym, idx, t, layer=None, sel=0):
    s, i = bs._i32(sym), bs._i32(idx)
    ly = bs._layer(layer)
    buf = np.empty(8 * s.size + 64, dtype=np.uint8)
    n = L.load().vam_rans_core_encode(s.ctypes.data, i.ctypes.data, s.size, *_targs(t), buf.ctypes.data, buf.size,
                                      ly.ctypes.data if ly is not None else None, sel)
    if n < 0:
        L.check(int(n), "vam_rans_core_encode")
    return buf[:n].tobytes()


def core_decode(stream, idx, t, layer=None, sel=0, fill=-12345):
    """(status, out): out starts as ``fill`` everywhere."""
    i = bs._i32(idx)
    ly = bs._layer(layer)
    out = np.full(i.size, fill, dtype=np.int32)
    src = np.frombuffer(stream, dtype=np.uint8)
    st = L.load().vam_rans_core_decode(src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size, *_targs(t),
                                       out.ctypes.data, ly.ctypes.data if ly is not None else None, sel)
    return st, out


@pytest.mark.parametrize("n", LENGTHS)
def test_core_encode_bytes_and_decode_symbols_equal_the_host_coder(tables, n):
    t = tables
    sym, idx = _stream_case(t, n, seed=n)
    ref = bs.encode(sym, idx, t)
    got = core_encode(sym, idx, t)
    assert got == ref
    st, out = core_decode(ref, idx, t)
    assert st == 0 and np.array_equal(out, bs.decode(ref, idx, t)) and np.array_equal(out, sym)


@pytest.mark.parametrize("sel", [0, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_core_layer_selection_equals_encode_streams(tables, n, sel):
    t = tables
    sym, idx = _stream_case(t, n, seed=100 + n)
    layer = np.random.default_rng(n + sel).choice(np.array([0, 1, 3, 0xFF], dtype=np.uint8), size=n)
    ref = bs.encode_streams([(sym, idx, layer, sel)], t)[0]
    assert core_encode(sym, idx, t, layer, sel) == ref
    want = np.full(n, -7, dtype=np.int32)
    bs.decode_streams([(ref, idx, want, layer, sel)], t)
    st, out = core_decode(ref, idx, t, layer, sel, fill=-7)
    assert st == 0 and np.array_equal(out, want)
    assert np.array_equal(out[layer == sel], sym[layer == sel]) and (out[layer != sel] == -7).all()


def test_nhwc_window_variants_equal_the_flat_calls(tables):
    t = tables
    lib = L.load()
    B, h, w, ld, c0, Cw = 2, 3, 5, 7, 2, 4
    rng = np.random.default_rng(9)
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
                ref = core_encode(sym_f, idx_f, t, ly_f, sel)
                buf = np.empty(8 * n + 64, dtype=np.uint8)
                nb = lib.vam_rans_core_encode_nhwc(sym.ctypes.data, idx.ctypes.data if with_idx else None,
                                                   ly.ctypes.data if ly is not None else None, sel, image, h, w, ld, c0, Cw,
                                                   *_targs(t), buf.ctypes.data, buf.size)
                assert nb > 0 and buf[:nb].tobytes() == ref
                out = np.full((B, h, w, ld), -7, dtype=np.int32)
                st = lib.vam_rans_core_decode_nhwc(buf.ctypes.data, nb, idx.ctypes.data if with_idx else None,
                                                   ly.ctypes.data if ly is not None else None, sel, image, h, w, ld, c0, Cw,
                                                   *_targs(t), out.ctypes.data)
                assert st == 0
                _, flat = core_decode(ref, idx_f, t, ly_f, sel, fill=-7)
                want = np.full((B, h, w, ld), -7, dtype=np.int32)                # nothing outside the window is written
                want[image, :, :, c0:c0 + Cw] = flat.reshape(Cw, h, w).transpose(1, 2, 0)
                assert np.array_equal(out, want)


def test_truncation_is_a_status_exactly_where_the_host_refuses():
    t = _tables()
    idx = np.zeros(2000, dtype=np.int32) + 4
    sym = np.random.default_rng(0).integers(-30, 30, 2000).astype(np.int32)
    sym[::97] = 500
    stream = bs.encode(sym, idx, t)
    assert core_encode(sym, idx, t) == stream
    n_fail = 0
    for cut in [0, 4, 7] + list(range(8, len(stream) + 1, 4)):
        part = stream[:cut]
        try:
            ref = bs.decode(part, idx, t) if cut else None
            host_ok = cut > 0
        except L.VamError:
            host_ok = False
        st, out = core_decode(part, idx, t)
        assert (st == 0) == host_ok, cut
        if st == 0:
            assert np.array_equal(out, ref)
            continue
        n_fail += 1
        assert st == (6 if cut < 8 or cut % 4 else 1), (cut, st)
        good = int(np.argmax(out != sym)) if (out != sym).any() else len(sym)    # the decoded prefix is right ...
        assert (out[good:] == 0).all(), cut                                    # ... and everything from the failure on is 0
    assert n_fail > len(stream) // 8
    st, out = core_decode(stream, idx + 100, t)              # index 100 with 5 tables: a status, not a read
    assert st == 2 and (out == 0).all()
    with pytest.raises(L.VamError, match="index out of range"):
        core_encode(sym, idx + 100, t)
    bad = bs.Tables(t.cdf, t.sizes.copy(), t.offsets)
    bad.sizes[4] = t.cdf.shape[1] + 1                        # a size the stride cannot hold
    st, out = core_decode(stream, idx, bad)
    assert st == 3 and (out == 0).all()


def _sanitizer_compiler():
    for cxx in (shutil.which("g++"), "/opt/rocm/llvm/bin/clang++", shutil.which("clang++")):
        if cxx and os.path.exists(cxx):
            yield cxx


def test_core_under_address_and_undefined_sanitizers(tmp_path):
    """tests/rans_core_check.cpp: a stand-alone program over csrc/rans_core.h — round trips, every truncation, streams of
    random bytes — built with -fsanitize=address,undefined and run as a process of its own."""
    src = os.path.join(ROOT, "tests", "rans_core_check.cpp")
    inc = os.path.join(ROOT, "efficient-pic-with-variance-aware-masking_amd", "csrc")
    assert os.path.exists(os.path.join(inc, "rans_core.h"))
    exe, errors = str(tmp_path / "rans_core_check"), []
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
    assert "rans_core_check: ok" in r.stdout
