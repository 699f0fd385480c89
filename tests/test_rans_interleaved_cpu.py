"""Interleaved-lanes rANS streams on the host (csrc/rans_core.h): K coder states share one word stream
whose words lie in the decoder's reading order, so a byte prefix decodes a rank prefix.  The library is held to the plain
Python restatement in tests/rans_interleaved_ref.py byte for byte; K = 1 is the existing stream.  No GPU is needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vampic import _lib as L
from vampic import bitstream as bs
from vampic import embedded as EB
import rans_interleaved_ref as ref
from test_rans_core_cpu import _sanitizer_compiler, _stream_case, _tables, _targs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
LANES = [1, 2, 8, 64]
LENGTHS = [0, 1, 12, 63, 64, 65, 1000]
FILL = -12345


@pytest.fixture(scope="module")
def tables():
    """The synthetic tables of the core's tests: five widths, every one with an escape entry."""
    return _tables()


@pytest.fixture(scope="module")
def cases(tables):
    """(n, K) -> (symbols, indexes, the library's string), coded once."""
    out = {}
    for n in LENGTHS:
        sym, idx = _stream_case(tables, n, seed=n + 5)
        for K in LANES:
            out[n, K] = (sym, idx, bs.encode_interleaved(sym, idx, tables, K))
    return out


def prefix_decode(prefix, idx, t, K):
    """(count, status, out) of the single-stream export; out starts as FILL."""
    i = bs._i32(idx)
    out = np.full(i.size, FILL, dtype=np.int32)
    src = np.frombuffer(prefix, dtype=np.uint8)
    st = np.full(1, -1, dtype=np.int32)
    got = L.load().vam_rans_interleaved_decode_prefix(src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size, *_targs(t),
                                                      K, out.ctypes.data, st.ctypes.data)
    return int(got), int(st[0]), out


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", LENGTHS)
def test_strings_equal_the_restatement_and_round_trip(tables, cases, n, K):
    sym, idx, got = cases[n, K]
    assert got == ref.encode(sym, idx, tables, K)
    assert len(got) % 4 == 0 and len(got) >= 8 * K and len(got) <= bs.interleaved_capacity(n, K)
    if n < K:                                                # a lane without elements holds the initial state 2^31
        states = np.frombuffer(got[:8 * K], dtype="<u8")
        assert (states[n:] == 1 << 31).all()
    count, st, out = prefix_decode(got, idx, tables, K)
    assert (count, st) == (n, 0) and np.array_equal(out, sym)
    out2 = np.full(n, FILL, dtype=np.int32)
    assert bs.decode_prefix_streams([(got, idx, out2)], tables, lanes=K) == [n] and np.array_equal(out2, sym)


@pytest.mark.parametrize("n", LENGTHS)
def test_one_lane_is_the_existing_stream(tables, cases, n):
    import rans_oracle
    sym, idx, got = cases[n, 1]
    assert got == bs.encode(sym, idx, tables)
    assert got == rans_oracle.encode(sym, idx, tables.cdf, tables.sizes, tables.offsets)
    counts = sorted({0, min(1, n), n // 3, n})
    buf = np.zeros(len(counts), dtype=np.int64)
    want = np.ascontiguousarray(counts, dtype=np.int64)
    src, i = np.frombuffer(got, dtype=np.uint8), bs._i32(idx)
    L.check(L.load().vam_rans_interleaved_prefix_bytes(src.ctypes.data, src.size, i.ctypes.data, i.size, *_targs(tables), 1,
                                                       want.ctypes.data, want.size, buf.ctypes.data), "prefix_bytes")
    assert buf.tolist() == bs.prefix_bytes(got, idx, counts, tables)          # vam_rans_prefix_bytes
    for cut in {0, 7, 8, len(got) // 2, len(got) - 1, len(got)}:
        a, b = np.full(n, FILL, dtype=np.int32), np.full(n, FILL, dtype=np.int32)
        count, st, a = prefix_decode(got[:cut], idx, tables, 1)
        assert st == 0 and [count] == bs.decode_prefix_streams([(got[:cut], idx, b)], tables) and np.array_equal(a, b)


def test_many_streams_on_the_thread_pool_equal_single_calls(tables, cases):
    for K in LANES:
        jobs = [(cases[n, K][0], cases[n, K][1]) for n in LENGTHS]
        for threads in (1, 4):
            assert bs.encode_interleaved_streams(jobs, tables, threads=threads, lanes=K) == [cases[n, K][2] for n in LENGTHS]
        outs = [np.full(n, FILL, dtype=np.int32) for n in LENGTHS]
        cut = [len(cases[n, K][2]) // 2 for n in LENGTHS]
        got = bs.decode_prefix_streams([(cases[n, K][2][:c], cases[n, K][1], o) for n, c, o in zip(LENGTHS, cut, outs)], tables,
                                       threads=4, lanes=K)
        for n, c, o, g in zip(LENGTHS, cut, outs, got):
            count, st, single = prefix_decode(cases[n, K][2][:c], cases[n, K][1], tables, K)
            assert (g, 0) == (count, st) and np.array_equal(o, single)


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", [12, 65])
def test_every_byte_length_decodes_what_the_restatement_decodes(tables, cases, n, K):
    sym, idx, string = cases[n, K]
    before = 0
    for cut in range(len(string) + 1):
        count, st, out = prefix_decode(string[:cut], idx, tables, K)
        want, _, _ = ref.decode_prefix(string[:cut], idx, tables, K)
        assert st == 0 and count == want, (cut, count, want)
        assert count >= before                                # non-decreasing in the length
        assert cut >= 8 * K or count == 0
        assert np.array_equal(out[:count], sym[:count]) and (out[count:] == FILL).all()
        before = count
    assert before == n


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", [12, 65, 1000])
def test_prefix_bytes_equal_the_restatement_and_are_minimal(tables, cases, n, K):
    sym, idx, string = cases[n, K]
    counts = sorted({0, 1, 2, n // 3, K, K + 1, n - 1, n} & set(range(n + 1)))
    got = bs.prefix_bytes(string, idx, counts, tables, lanes=K)
    assert got == [ref.prefix_bytes(string, idx, tables, K, c) for c in counts]
    assert got == sorted(got)
    for c, b in zip(counts, got):
        assert (b == 0) == (c == 0) and b % 4 == 0 and b <= len(string)
        if c:
            assert b >= 8 * K
            assert prefix_decode(string[:b], idx, tables, K)[0] >= c
            assert prefix_decode(string[:b - 4], idx, tables, K)[0] < c       # four bytes fewer do not reach the count
    assert bs.prefix_bytes(string, idx, [], tables, lanes=K) == []


def test_bad_counts_and_arguments_are_refused_by_message(tables, cases):
    sym, idx, string = cases[65, 8]
    with pytest.raises(L.VamError, match="counts must be >= 0 and sorted"):
        bs.prefix_bytes(string, idx, [5, 3], tables, lanes=8)
    with pytest.raises(L.VamError, match="counts must be >= 0 and sorted"):
        bs.prefix_bytes(string, idx, [-1], tables, lanes=8)
    with pytest.raises(L.VamError, match="66 symbols asked for"):
        bs.prefix_bytes(string, idx, [66], tables, lanes=8)
    with pytest.raises(L.VamError, match=r"30 symbols asked for, the 100 bytes given decode \d+ of 65"):
        bs.prefix_bytes(string[:100], idx, [30], tables, lanes=8)
    for bad in (0, 3, 128, "8", 2.0, True, None):
        with pytest.raises(ValueError, match="power of two"):
            bs.encode_interleaved(sym, idx, tables, bad)
        with pytest.raises(ValueError, match="power of two"):
            bs.decode_prefix_streams([(string, idx, np.zeros(65, dtype=np.int32))], tables, lanes=bad)
        with pytest.raises(ValueError, match="power of two"):
            bs.prefix_bytes(string, idx, [1], tables, lanes=bad)
    buf = np.empty(4096, dtype=np.uint8)                      # the exports refuse what ctypes lets through
    s, i = bs._i32(sym), bs._i32(idx)
    lib = L.load()
    assert lib.vam_rans_interleaved_encode(s.ctypes.data, i.ctypes.data, s.size, *_targs(tables), buf.ctypes.data, buf.size, 3) < 0
    assert lib.vam_rans_interleaved_encode(s.ctypes.data, i.ctypes.data, s.size, *_targs(tables), buf.ctypes.data, 16, 8) < 0
    assert lib.vam_rans_interleaved_encode(None, i.ctypes.data, s.size, *_targs(tables), buf.ctypes.data, buf.size, 8) < 0
    assert lib.vam_rans_interleaved_decode_prefix(None, 16, i.ctypes.data, i.size, *_targs(tables), 8, None, None) < 0
    far = sym.copy()
    far[3] = 0
    bad_idx = idx.copy()
    bad_idx[3] = tables.cdf.shape[0]
    with pytest.raises(L.VamError, match="index out of range"):
        bs.encode_interleaved(far, bad_idx, tables, 8)


@pytest.mark.parametrize("K", LANES)
def test_corrupted_indexes_and_states_end_with_a_status_not_a_crash(tables, cases, K):
    sym, idx, string = cases[1000, K]
    for where, bad in ((0, -1), (500, tables.cdf.shape[0]), (999, 1 << 30)):
        idx2 = idx.copy()
        idx2[where] = bad
        count, st, out = prefix_decode(string, idx2, tables, K)
        assert st == 2 and where // K * K <= count <= where
        assert np.array_equal(out[:count], sym[:count]) and (out[count:] == FILL).all()
        with pytest.raises(L.VamError, match="out of range"):
            bs.decode_prefix_streams([(string, idx2, np.zeros(1000, dtype=np.int32))], tables, lanes=K)
    t2 = bs.Tables(tables.cdf, tables.sizes.copy(), tables.offsets)
    t2.sizes[int(idx[0])] = tables.cdf.shape[1] + 1
    assert prefix_decode(string, idx, t2, K)[:2] == (0, 3)
    rng = np.random.default_rng(K)
    words = np.frombuffer(string, dtype="<u4")
    for _ in range(50):                                       # a corrupted state or word: some count, some symbols, no crash
        w2 = words.copy()
        w2[rng.integers(0, min(len(w2), 4 * K))] = rng.integers(0, 1 << 32)
        count, st, out = prefix_decode(w2.tobytes(), idx, tables, K)
        assert st in (0, 3) and 0 <= count <= 1000 and (out[count:] == FILL).all()


def _container(tables, K, n=65, ns=3):
    """A hand-made container of ns slices with marks at the counts 0, n // 3 and n."""
    emb, cnt, byt = [], [], []
    for j in range(ns):
        sym, idx = _stream_case(tables, n, seed=40 + j)
        s = bs.encode_interleaved(sym, idx, tables, K)
        emb.append(s)
        cnt.append([0, n // 3, n])
        byt.append(bs.prefix_bytes(s, idx, cnt[-1], tables, lanes=K))
    c = {"format": EB.FORMAT if K == 1 else EB.FORMAT_LANES, "shape": (1, 1), "z": [b"z" * 12], "base": [[b"b" * 20]] * ns,
         "embedded": emb, "marks": {"q": [0.0, 1.0, 10.0], "count": [list(r) for r in zip(*cnt)], "bytes": [list(r) for r in zip(*byt)]}}
    if K > 1:
        c["lanes"] = K
    return c


@pytest.mark.parametrize("K", [1, 8])
def test_truncate_reads_the_marks_of_both_formats(tables, K):
    c = _container(tables, K)
    ns, fixed = 3, 12 + 3 * 20
    cut = EB.truncate(c, q=1.0)
    assert [len(s) for s in cut["embedded"]] == c["marks"]["bytes"][1]
    assert all(s == full[:len(s)] for s, full in zip(cut["embedded"], c["embedded"]))
    assert cut["format"] == c["format"] and cut.get("lanes") == c.get("lanes")
    for j in range(ns):                                       # the cut decodes the mark's count, as the marks promise
        _, idx = _stream_case(tables, 65, seed=40 + j)
        assert prefix_decode(cut["embedded"][j], idx, tables, K)[0] >= 65 // 3
    assert all(len(s) == 0 for s in EB.truncate(c, q=0.0)["embedded"])
    budget = fixed + sum(c["marks"]["bytes"][1])
    assert [len(s) for s in EB.truncate(c, max_bytes=budget)["embedded"]] == c["marks"]["bytes"][1]
    assert [len(s) for s in EB.truncate(c, max_bytes=budget - 1)["embedded"]] == [0] * ns
    assert [len(s) for s in EB.truncate(c, slice_bytes=[0, 7, 10 ** 6])["embedded"]] == [0, 7, len(c["embedded"][2])]
    with pytest.raises(ValueError, match="is not marked"):
        EB.truncate(c, q=2.0)
    with pytest.raises(ValueError, match="already cut below it"):
        EB.truncate(EB.truncate(c, q=1.0), q=10.0)


def test_container_formats_and_lanes_are_checked(tables):
    c8 = _container(tables, 8)
    assert c8["format"] == "embedded-2" and c8["lanes"] == 8 and "lanes" not in _container(tables, 1)
    assert EB._check_container(c8) == 8 and EB._check_container(_container(tables, 1)) == 1
    for bad in (3, 0, 128, None, "8"):
        with pytest.raises(ValueError, match="power of two"):
            EB.truncate(dict(c8, lanes=bad), q=1.0)
    with pytest.raises(ValueError, match="lanes > 1"):
        EB.truncate(dict(c8, lanes=1), q=1.0)
    with pytest.raises(ValueError, match="not an embedded container"):
        EB.truncate(dict(c8, format="embedded-3"), q=1.0)


def test_interleaved_under_address_and_undefined_sanitizers(tmp_path):
    """tests/rans_interleaved_check.cpp: a stand-alone program over csrc/rans_core.h — encode, tolerant decode and marks
    over the n x K grid, K = 1 against encode_stream, every byte length, corrupted indexes, states and strings of random
    bytes — built with -fsanitize=address,undefined and run as a process of its own."""
    src = os.path.join(ROOT, "tests", "rans_interleaved_check.cpp")
    inc = os.path.join(ROOT, "efficient-pic-with-variance-aware-masking_amd", "csrc")
    assert os.path.exists(os.path.join(inc, "rans_core.h"))
    exe, errors = str(tmp_path / "rans_interleaved_check"), []
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
    assert "rans_interleaved_check: ok" in r.stdout
