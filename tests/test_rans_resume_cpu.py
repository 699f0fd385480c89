"""Resumable decode of the interleaved-lanes streams on the host (csrc/rans_core.h): a checkpoint at a
group boundary and a tolerant decode that starts from it and sees only the bytes from the checkpoint's word on.  The one
rule is equivalence: after the call for a longer prefix, count, symbols and status are those of the one-shot decode of that
prefix — the plain Python restatement in tests/rans_interleaved_ref.py and the existing export.  No GPU is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vampic import _lib as L
from vampic import bitstream as bs
from vampic import embedded as EB
import rans_interleaved_ref as ref
from test_rans_core_cpu import _sanitizer_compiler, _stream_case, _tables, _targs
from test_rans_interleaved_cpu import prefix_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [1, 2, 8, 64]
LENGTHS = [1, 50, 130]                     # n < K, n no multiple of K and n a multiple of K all occur
FILL = -12345


@pytest.fixture(scope="module")
def tables():
    return _tables()


@pytest.fixture(scope="module")
def cases(tables):
    """(n, K) -> (symbols, indexes, string); the streams hold escapes, so elements take several rounds."""
    out = {}
    for n in LENGTHS + [1000]:
        sym, idx = _stream_case(tables, n, seed=n + 11)
        for K in LANES:
            out[n, K] = (sym, idx, bs.encode_interleaved(sym, idx, tables, K))
    return out


class Receiver:
    """A checkpoint and a sentinel-filled output.  :meth:`feed` hands the export ONLY the bytes of ``prefix`` from byte
    4 * pos on — nothing earlier is ever supplied — and checks that no element outside [done_in, count) changed."""

    def __init__(self, idx, t, K):
        self.idx, self.t, self.K = bs._i32(idx), t, K
        self.done, self.pos = 0, 0
        self.states = np.zeros(K, dtype=np.uint64)
        self.out = np.full(self.idx.size, FILL, dtype=np.int32)

    def snapshot(self):
        return self.done, self.pos, self.states.copy(), self.out.copy()

    def restore(self, snap):
        self.done, self.pos = snap[0], snap[1]
        self.states, self.out = snap[2].copy(), snap[3].copy()

    def call(self, tail: bytes, done=None, pos=None, n=None, lanes=None, n_bytes=None, states_ptr=None):
        src = np.frombuffer(tail, dtype=np.uint8)
        ck = L.VamRansCheckpoint(self.done if done is None else done, self.pos if pos is None else pos,
                                 self.states.ctypes.data if states_ptr is None else states_ptr)
        st = np.full(1, -1, dtype=np.int32)
        got = L.load().vam_rans_interleaved_resume(src.ctypes.data if src.size else None, src.size if n_bytes is None else n_bytes,
                                                   self.idx.ctypes.data, self.idx.size if n is None else n, *_targs(self.t),
                                                   self.K if lanes is None else lanes, self.out.ctypes.data, C.byref(ck),
                                                   st.ctypes.data)
        return int(got), int(st[0]), ck

    def feed(self, prefix: bytes):
        before, done_in = self.out.copy(), self.done
        got, st, ck = self.call(prefix[4 * self.pos:])
        assert got >= 0, L.load().vam_last_error().decode()
        self.done, self.pos = ck.done, ck.pos
        keep = np.ones(self.out.size, dtype=bool)
        keep[done_in:got] = False
        assert np.array_equal(self.out[keep], before[keep])       # nothing outside [done_in, count) is touched
        return got, st


def expect(prefix, idx, t, K):
    """(count, symbols, done, pos) of a prefix from the restatement."""
    n = np.asarray(idx).size
    count, symbols, reach = ref.decode_prefix(prefix, idx, t, K)
    done = n if count == n else K * (count // K)
    fresh = len(prefix) // 4 < 2 * K and n > 0
    return count, symbols, done, 0 if fresh else max([2 * K] + reach[:done])


def check(r, prefix, want, one_shot):
    got, st = r.feed(prefix)
    count, symbols, done, pos = want
    assert (got, st) == (count, 0) == one_shot[:2]
    assert r.out[:got].tolist() == symbols and np.array_equal(r.out[:got], one_shot[2][:got])
    assert (r.done, r.pos) == (done, pos)


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", LENGTHS)
def test_every_pair_of_byte_lengths_equals_the_one_shot_decode(tables, cases, n, K):
    """Every pair L1 <= L2.  The second call is a function of the checkpoint the first one left and of the bytes from
    4 * pos to L2, so pairs whose first call left the same checkpoint make the same second call: it is made once."""
    sym, idx, string = cases[n, K]
    total = len(string)
    want = [expect(string[:cut], idx, tables, K) for cut in range(total + 1)]
    shot = [prefix_decode(string[:cut], idx, tables, K) for cut in range(total + 1)]
    seen, snaps = set(), {}
    for l1 in range(total + 1):
        r = Receiver(idx, tables, K)
        check(r, string[:l1], want[l1], shot[l1])
        key = (r.done, r.pos, r.states.tobytes() if r.pos else b"")
        snaps.setdefault(key, r.snapshot())
        for l2 in range(l1, total + 1):
            if (key, l2) in seen:
                continue
            seen.add((key, l2))
            r.restore(snaps[key])
            r.out[want[l1][0]:] = FILL                            # what this l1 holds beyond its own count
            check(r, string[:l2], want[l2], shot[l2])
    assert want[total][0] == n and want[total][2] == n and np.array_equal(shot[total][2], sym)


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", LENGTHS)
def test_a_chain_through_lengths_not_divisible_by_four(tables, cases, n, K):
    sym, idx, string = cases[n, K]
    total = len(string)
    cuts = sorted({min(total, c) for c in (8 * K + 1, 8 * K + (total - 8 * K) // 3 | 1, 8 * K + 2 * (total - 8 * K) // 3 | 3)})
    r = Receiver(idx, tables, K)
    for cut in [3] + cuts + [total, total]:                       # and one more call after the end
        check(r, string[:cut], expect(string[:cut], idx, tables, K), prefix_decode(string[:cut], idx, tables, K))
    assert r.done == n and np.array_equal(r.out, sym)
    states = r.states.copy()
    assert r.call(b"")[:2] == (n, 0) and np.array_equal(r.states, states)      # a finished stream reads and writes nothing


@pytest.mark.parametrize("K", LANES)
def test_corrupt_indexes_give_the_one_shot_status_and_count(tables, cases, K):
    """A corrupt index in the checkpointed group, in an earlier group and in a later one: the same status and count as
    one-shot at every step, recomputed on every call, never a crash."""
    sym, idx, string = cases[1000, K]
    total = len(string)
    mid = (8 * K + total) // 2 | 1
    at = ref.decode_prefix(string[:mid], idx, tables, K)[0]       # the element the middle cut stops at
    for where in (at, max(at - 3 * K - 1, 0), min(at + 3 * K + 1, 999)):
        for bad in (-1, tables.cdf.shape[0], 1 << 30):
            idx2 = idx.copy()
            idx2[where] = bad
            r = Receiver(idx2, tables, K)
            for cut in (0, mid, total - 2, total, total):
                got, st = r.feed(string[:cut])
                count, status, out = prefix_decode(string[:cut], idx2, tables, K)
                assert (got, st) == (count, status) and np.array_equal(r.out[:got], out[:got])
                assert r.done == K * (got // K)
            assert st == 2 and where // K * K <= got <= where and (r.out[got:] == FILL).all()
    jobs_idx = idx.copy()
    jobs_idx[5] = -1
    with pytest.raises(L.VamError, match="stream 0.*out of range"):
        bs.resume_prefix_streams([(string, jobs_idx, np.zeros(1000, dtype=np.int32))], tables, bs.Checkpoints.fresh(1, K), lanes=K)


def test_impossible_checkpoints_and_bad_arguments_are_refused_by_message(tables, cases):
    sym, idx, string = cases[50, 8]
    r = Receiver(idx, tables, 8)
    r.states[:] = 0x5555555555555555
    untouched = lambda: (r.out == FILL).all() and (r.states == 0x5555555555555555).all()
    for done, pos in ((3, 16), (51, 16), (56, 16), (8, 15), (8, 0), (-8, 16), (0, -1)):
        got, st, ck = r.call(string, done=done, pos=pos)
        assert got < 0 and st == -1 and (ck.done, ck.pos) == (done, pos) and untouched()
        assert "impossible checkpoint" in L.load().vam_last_error().decode()
    for kw, msg in ((dict(lanes=3), "power of two"), (dict(lanes=128), "power of two"), (dict(n=-1), "bad arguments"),
                    (dict(n_bytes=-4), "bad arguments"), (dict(states_ptr=r.states.ctypes.data + 4), "misaligned")):
        got, st, ck = r.call(string, **kw)
        assert got < 0 and st == -1 and untouched()
        assert msg in L.load().vam_last_error().decode()
    assert L.load().vam_rans_interleaved_resume(None, 16, r.idx.ctypes.data, 50, *_targs(tables), 8, None, None, None) < 0
    for bad in (0, 3, 128, "8", None):
        with pytest.raises(ValueError, match="power of two"):
            bs.resume_prefix_streams([], tables, bs.Checkpoints.fresh(0, 1), lanes=bad)
    with pytest.raises(ValueError, match="host checkpoints of 1 streams on 8 lanes"):
        bs.resume_prefix_streams([(string, idx, np.zeros(50, dtype=np.int32))], tables, bs.Checkpoints.fresh(1, 2), lanes=8)
    ck = bs.Checkpoints.fresh(1, 8)
    ck.done[0] = 3
    with pytest.raises(L.VamError, match="stream 0.*impossible checkpoint"):
        bs.resume_prefix_streams([(string, idx, np.zeros(50, dtype=np.int32))], tables, ck, lanes=8)


def test_many_streams_on_the_thread_pool_equal_single_calls(tables, cases):
    for K in LANES:
        keys = [(n, K) for n in LENGTHS + [1000]]
        for threads in (1, 4):
            ck = bs.Checkpoints.fresh(len(keys), K)
            outs = [np.full(n, FILL, dtype=np.int32) for n, _ in keys]
            singles = [Receiver(cases[k][1], tables, K) for k in keys]
            for frac in (0.0, 0.4, 0.77, 1.0, 1.0):
                cuts = [int(len(cases[k][2]) * frac) | (1 if frac < 1 else 0) for k in keys]
                cuts = [min(c, len(cases[k][2])) for c, k in zip(cuts, keys)]
                status = np.full(len(keys), -1, dtype=np.int32)
                got = bs.resume_prefix_streams([(cases[k][2][4 * int(ck.pos[j]):c], cases[k][1], outs[j])
                                                for j, (k, c) in enumerate(zip(keys, cuts))], tables, ck, threads=threads, lanes=K,
                                               status=status)
                assert (status == 0).all()
                for j, (k, c) in enumerate(zip(keys, cuts)):
                    count, st = singles[j].feed(cases[k][2][:c])
                    assert (got[j], 0) == (count, st) and np.array_equal(outs[j], singles[j].out)
                    assert (int(ck.done[j]), int(ck.pos[j])) == (singles[j].done, singles[j].pos)
                    assert np.array_equal(ck.states[j], singles[j].states)
            assert all(np.array_equal(o, cases[k][0]) for o, k in zip(outs, keys))


def _container(tables, fmt, K, n=65, ns=3):
    """A hand-made container of ns slices in one of the three formats."""
    emb = []
    for j in range(ns):
        sym, idx = _stream_case(tables, n, seed=60 + j)
        emb.append(bs.encode_interleaved(sym, idx, tables, K))
    c = {"format": fmt, "shape": (1, 1), "z": [b"z" * 12], "base": [[b"b" * 20], [b"c" * 8], [b"d" * 4]], "embedded": emb,
         "marks": {"q": [10.0], "count": [[n] * ns], "bytes": [[len(s) for s in emb]]}}
    if fmt != EB.FORMAT:
        c["lanes"] = K
    if fmt == EB.FORMAT_SCHEDULED:
        c["marks"]["stage"] = c["marks"].pop("q")
        c["schedule"] = {"levels": [1.0, 10.0], "index": np.zeros((1, 4, 4), dtype=np.uint8)}
        c["side_bytes"] = 32
    return c


@pytest.mark.parametrize("fmt,K", [(EB.FORMAT, 1), (EB.FORMAT_LANES, 8), (EB.FORMAT_SCHEDULED, 1), (EB.FORMAT_SCHEDULED, 64)])
def test_delta_gives_the_bytes_that_follow_and_refuses_what_is_no_cut(tables, fmt, K):
    c = _container(tables, fmt, K)
    lens = [len(s) for s in c["embedded"]]
    cut = EB.truncate(c, slice_bytes=[0, 7, lens[2]])
    d = EB.delta(c, cut)
    assert [type(s) for s in d] == [bytes] * 3 and d == [c["embedded"][0], c["embedded"][1][7:], b""]
    assert [a + b for a, b in zip(cut["embedded"], d)] == c["embedded"]
    assert EB.delta(c, c) == [b""] * 3
    mid = EB.truncate(c, slice_bytes=[5, 9, lens[2]])
    assert EB.delta(mid, cut)[:2] == [c["embedded"][0][:5], c["embedded"][1][7:9]]
    with pytest.raises(ValueError, match=r"slice 0: .* no prefix"):          # longer than the "longer" one
        EB.delta(cut, mid)
    other = dict(cut, embedded=[cut["embedded"][0], b"\x00" * 7, cut["embedded"][2]])
    assert other["embedded"][1] != cut["embedded"][1]
    with pytest.raises(ValueError, match=r"slice 1: .* no prefix"):
        EB.delta(c, other)
    with pytest.raises(ValueError, match="differ in their shape"):
        EB.delta(c, dict(cut, shape=(1, 2)))
    with pytest.raises(ValueError, match="differ in their z stream"):
        EB.delta(c, dict(cut, z=[b"y" * 12]))
    with pytest.raises(ValueError, match="base stream of slice 2 differs"):
        EB.delta(c, dict(cut, base=[[b"b" * 20], [b"c" * 8], [b"e" * 4]]))
    with pytest.raises(ValueError, match="hold 2 and 3 slices"):
        EB.delta(c, dict(cut, embedded=cut["embedded"][:2]))
    with pytest.raises(ValueError, match="not an embedded container"):
        EB.delta(c, dict(cut, format="layered"))
    if fmt == EB.FORMAT:
        with pytest.raises(ValueError, match="differ in their format"):
            EB.delta(c, dict(cut, format=EB.FORMAT_LANES, lanes=8))
    else:
        with pytest.raises(ValueError, match="differ in their lanes"):
            EB.delta(c, dict(cut, lanes=2))
    if fmt == EB.FORMAT_SCHEDULED:
        sc = {"levels": [1.0, 10.0], "index": np.ones((1, 4, 4), dtype=np.uint8)}
        with pytest.raises(ValueError, match="differ in their schedule"):
            EB.delta(c, dict(cut, schedule=sc))
        with pytest.raises(ValueError, match="differ in their format"):
            EB.delta(c, dict(cut, format=EB.FORMAT_LANES, lanes=max(K, 2)))


def test_resume_under_address_and_undefined_sanitizers(tmp_path):
    """tests/rans_resume_check.cpp: a stand-alone program over csrc/rans_core.h — the split pairs of a few streams at
    K = 1, 8, 64, a chain through every length, corrupted indexes and impossible checkpoints — built with
    -fsanitize=address,undefined and run as a process of its own.  Nothing loaded into Python is sanitised."""
    src = os.path.join(ROOT, "tests", "rans_resume_check.cpp")
    inc = os.path.join(ROOT, "efficient-pic-with-variance-aware-masking_amd", "csrc")
    assert os.path.exists(os.path.join(inc, "rans_core.h"))
    exe, errors = str(tmp_path / "rans_resume_check"), []
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
    assert "rans_resume_check: ok" in r.stdout
