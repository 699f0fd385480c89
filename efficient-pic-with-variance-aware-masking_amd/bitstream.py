"""Host-side bitstream helpers over the C ABI (`vam_pmf_to_quantized_cdf`, `vam_rans_encode`,
`vam_rans_decode`): the role compressai's C++ extension plays for the reference
(entropy_models.py:61-64,175-183,231-239,280-290).  Streams are per (image, slice) byte strings."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L


def pmf_to_quantized_cdf(pmf: torch.Tensor, precision: int = 16) -> torch.Tensor:
    p = np.ascontiguousarray(pmf.detach().cpu().numpy(), dtype=np.float32)
    out = np.zeros(p.size + 1, dtype=np.int32)
    L.check(L.load().vam_pmf_to_quantized_cdf(p.ctypes.data, p.size, precision, out.ctypes.data), "vam_pmf_to_quantized_cdf")
    return torch.from_numpy(out)


@dataclass
class Tables:
    """CDF tables of one entropy model, host side, in the layout the coder wants."""
    cdf: np.ndarray       # [n, stride] int32
    sizes: np.ndarray     # [n] int32
    offsets: np.ndarray   # [n] int32

    @staticmethod
    def of(model) -> "Tables":
        if model._quantized_cdf.numel() == 0:
            raise ValueError("Uninitialized CDFs. Run update() first")
        # _tables_generation is bumped by update() / load_state_dict(): a re-built table can land at the address (and
        # version) of the one it replaced, so pointers alone do not identify it
        key = (getattr(model, "_tables_generation", 0), model._quantized_cdf.data_ptr(), model._quantized_cdf._version,
               model._offset._version, tuple(model._quantized_cdf.shape))
        if getattr(model, "_tables_key", None) != key:
            t = Tables(np.ascontiguousarray(model._quantized_cdf.detach().cpu().numpy(), dtype=np.int32),
                       np.ascontiguousarray(model._cdf_length.detach().cpu().reshape(-1).numpy(), dtype=np.int32),
                       np.ascontiguousarray(model._offset.detach().cpu().reshape(-1).numpy(), dtype=np.int32))
            object.__setattr__(model, "_tables", t)
            object.__setattr__(model, "_tables_key", key)
        return model._tables


def encode(symbols: np.ndarray, indexes: np.ndarray, t: Tables) -> bytes:
    s = np.ascontiguousarray(symbols, dtype=np.int32).reshape(-1)
    i = np.ascontiguousarray(indexes, dtype=np.int32).reshape(-1)
    assert s.size == i.size
    buf = np.empty(8 * s.size + 64, dtype=np.uint8)
    n = L.load().vam_rans_encode(s.ctypes.data, i.ctypes.data, s.size, t.cdf.ctypes.data, t.cdf.shape[1],
                                 t.sizes.ctypes.data, t.offsets.ctypes.data, t.cdf.shape[0], buf.ctypes.data, buf.size)
    if n < 0:
        L.check(int(n), "vam_rans_encode")
    return buf[:n].tobytes()


def decode(stream: bytes, indexes: np.ndarray, t: Tables) -> np.ndarray:
    i = np.ascontiguousarray(indexes, dtype=np.int32).reshape(-1)
    out = np.empty(i.size, dtype=np.int32)
    src = np.frombuffer(stream, dtype=np.uint8)
    L.check(L.load().vam_rans_decode(src.ctypes.data, src.size, i.ctypes.data, i.size, t.cdf.ctypes.data, t.cdf.shape[1],
                                     t.sizes.ctypes.data, t.offsets.ctypes.data, t.cdf.shape[0], out.ctypes.data),
            "vam_rans_decode")
    return out


# ---------------------------------------------------------------- lane-split streams
def check_lanes(lanes) -> int:
    """``lanes`` as an int: a power of two in 1 .. 64, anything else is a ValueError."""
    if isinstance(lanes, bool) or not isinstance(lanes, (int, np.integer)) or not 1 <= lanes <= L.VAM_RANS_MAX_LANES \
            or lanes & (lanes - 1):
        raise ValueError(f"lanes is a power of two in 1 .. {L.VAM_RANS_MAX_LANES}, got {lanes!r}")
    return int(lanes)


def lanes_capacity(n: int, lanes: int) -> int:
    """Bytes that hold any lane-split string of n elements: the header and 8 m + 64 bytes per lane of m = ceil(n / K)."""
    return 4 * lanes + lanes * (8 * (-(-n // lanes)) + 64)


def encode_lanes(symbols: np.ndarray, indexes: np.ndarray, t: Tables, lanes: int, layer=None, sel: int = 0) -> bytes:
    """One stream as ``lanes`` = K independent lanes (vam_rans_lanes_encode): K uint32 lane lengths in words, then lane j =
    :func:`encode` of the elements j, j + K, ...  K = 1 is :func:`encode`'s string, with no header.  K is not stored in
    the string: the decoder must be given the same value, like the quality and the shape."""
    K = check_lanes(lanes)
    s, i, ly = _i32(symbols), _i32(indexes), _layer(layer)
    assert s.size == i.size and (ly is None or ly.size == s.size)
    buf = np.empty(lanes_capacity(s.size, K), dtype=np.uint8)
    n = L.load().vam_rans_lanes_encode(s.ctypes.data, i.ctypes.data, s.size, t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                       t.offsets.ctypes.data, t.cdf.shape[0], buf.ctypes.data, buf.size,
                                       ly.ctypes.data if ly is not None else None, int(sel), K, None)
    if n < 0:
        L.check(int(n), "vam_rans_lanes_encode")
    return buf[:n].tobytes()


def decode_lanes(stream: bytes, indexes: np.ndarray, t: Tables, lanes: int, layer=None, sel: int = 0, out=None) -> np.ndarray:
    """The symbols of a string of :func:`encode_lanes` with the same ``lanes`` (a wrong value gives a VamError or wrong
    symbols: it is not stored).  VamError names the lowest-numbered failing lane.  With a layer array only
    out[layer == sel] is written (``out``: an int32 array of the indexes' size, zeros when not given)."""
    K = check_lanes(lanes)
    i, ly = _i32(indexes), _layer(layer)
    out = np.zeros(i.size, dtype=np.int32) if out is None else out
    assert out.dtype == np.int32 and out.flags.c_contiguous and out.size == i.size and (ly is None or ly.size == i.size)
    src = np.frombuffer(stream, dtype=np.uint8)
    status = np.zeros(K, dtype=np.int32)
    st = L.load().vam_rans_lanes_decode(src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size, t.cdf.ctypes.data,
                                        t.cdf.shape[1], t.sizes.ctypes.data, t.offsets.ctypes.data, t.cdf.shape[0], out.ctypes.data,
                                        ly.ctypes.data if ly is not None else None, int(sel), K, status.ctypes.data)
    if st < 0:
        L.check(int(st), "vam_rans_lanes_decode")
    if st:
        raise L.VamError(f"vam_rans_lanes_decode: lane {int(np.flatnonzero(status)[0])}: {status_text(int(st), K)}")
    return out


def coder_threads(requested: Optional[int] = None) -> int:
    """Host threads for the stream coder: at most L.VAM_RANS_MAX_THREADS and the CPUs this process may run on."""
    n = min(L.VAM_RANS_MAX_THREADS, len(os.sched_getaffinity(0)))
    return max(1, n if requested is None else min(int(requested), n))


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _layer(a) -> Optional[np.ndarray]:
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def _lane_jobs(fn, jobs, threads: Optional[int]):
    """``fn(job)`` for every job on :func:`coder_threads` host threads (the library calls release the GIL), in job order."""
    from concurrent.futures import ThreadPoolExecutor
    n = coder_threads(threads)
    if n == 1 or len(jobs) <= 1:
        return [fn(j) for j in jobs]
    with ThreadPoolExecutor(max_workers=n) as pool:
        return list(pool.map(fn, jobs))


def encode_streams(jobs: Sequence[Tuple], t: Tables, threads: Optional[int] = None, lanes: int = 1) -> List[bytes]:
    """Many independent streams in one vam_rans_encode_streams call.  ``jobs``: (symbols, indexes) or (symbols, indexes,
    layer, sel) per stream; with a layer array only the elements with layer == sel are coded (the others as 0 / table 0).
    Each stream's bytes equal :func:`encode`'s on the same (masked) inputs.  ``threads`` is passed on as given (the library
    clamps it to L.VAM_RANS_MAX_THREADS); None = :func:`coder_threads`.  ``lanes`` = K > 1: every job
    is :func:`encode_lanes`'s string, the jobs spread over the same number of host threads."""
    K = check_lanes(lanes)
    if K > 1:
        return _lane_jobs(lambda j: encode_lanes(j[0], j[1], t, K, j[2] if len(j) > 2 else None, int(j[3]) if len(j) > 2 else 0),
                          list(jobs), threads)
    keep, arr = [], (L.VamRansStream * max(len(jobs), 1))()
    caps = []
    for j in jobs:
        s, i = _i32(j[0]), _i32(j[1])
        ly = _layer(j[2]) if len(j) > 2 else None
        assert s.size == i.size and (ly is None or ly.size == s.size)
        caps.append(8 * s.size + 64)
        keep.append((s, i, ly))
    out = np.empty(sum(caps), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    for k, (j, (s, i, ly)) in enumerate(zip(jobs, keep)):
        arr[k] = L.VamRansStream(s.ctypes.data, None, i.ctypes.data, ly.ctypes.data if ly is not None else None, s.size,
                                 int(j[3]) if ly is not None else 0, 0, out.ctypes.data + int(off[k]), caps[k], 0)
    L.check(L.load().vam_rans_encode_streams(arr, len(jobs), t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                             t.offsets.ctypes.data, t.cdf.shape[0],
                                             coder_threads() if threads is None else int(threads)), "vam_rans_encode_streams")
    return [out[int(off[k]):int(off[k]) + arr[k].n_bytes].tobytes() for k in range(len(jobs))]


def decode_streams(jobs: Sequence[Tuple], t: Tables, threads: Optional[int] = None, lanes: int = 1) -> None:
    """Decode many streams in one vam_rans_decode_streams call.  ``jobs``: (stream bytes, indexes, out) or (stream bytes,
    indexes, out, layer, sel); ``out`` is a writable C-contiguous int32 array of the indexes' size.  With a layer array only
    out[layer == sel] is written, so the layers of a container can fill one array.  ``lanes`` = K > 1: every job is a
    string of :func:`encode_lanes`, decoded by :func:`decode_lanes` on the same number of host threads."""
    K = check_lanes(lanes)
    if K > 1:
        _lane_jobs(lambda j: decode_lanes(j[0], j[1], t, K, j[3] if len(j) > 3 else None, int(j[4]) if len(j) > 3 else 0, out=j[2]),
                   list(jobs), threads)
        return
    keep, arr = [], (L.VamRansStream * max(len(jobs), 1))()
    for k, j in enumerate(jobs):
        src = np.frombuffer(j[0], dtype=np.uint8)
        i, o = _i32(j[1]), j[2]
        ly = _layer(j[3]) if len(j) > 3 else None
        assert o.dtype == np.int32 and o.flags.c_contiguous and o.size == i.size and (ly is None or ly.size == i.size)
        keep.append((src, i, ly))
        arr[k] = L.VamRansStream(None, o.ctypes.data, i.ctypes.data, ly.ctypes.data if ly is not None else None, i.size,
                                 int(j[4]) if ly is not None else 0, 0, src.ctypes.data, src.size, src.size)
    L.check(L.load().vam_rans_decode_streams(arr, len(jobs), t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                             t.offsets.ctypes.data, t.cdf.shape[0],
                                             coder_threads() if threads is None else int(threads)), "vam_rans_decode_streams")


# ---------------------------------------------------------------- byte prefixes of a stream
def interleaved_capacity(n: int, lanes: int) -> int:
    """Bytes that hold any interleaved string of n elements: the K states and two words per element, with the host's slack."""
    return 8 * n + 8 * lanes + 64


def encode_interleaved(symbols: np.ndarray, indexes: np.ndarray, t: Tables, lanes: int) -> bytes:
    """One stream on ``lanes`` = K INTERLEAVED lanes (vam_rans_interleaved_encode): element i belongs to
    lane i % K, the K coder states share one word stream whose words lie in the order the decoder reads them, and the K
    final states stand in front.  Any byte prefix decodes a prefix of the elements (:func:`decode_prefix_streams`);
    K = 1 is :func:`encode`'s string.  K is not stored in the string."""
    return encode_interleaved_streams([(symbols, indexes)], t, lanes=lanes)[0]


def encode_interleaved_streams(jobs: Sequence[Tuple], t: Tables, threads: Optional[int] = None, lanes: int = 1) -> List[bytes]:
    """Many (symbols, indexes) streams as :func:`encode_interleaved` strings in one vam_rans_interleaved_encode_streams call,
    threaded as :func:`encode_streams`."""
    K = check_lanes(lanes)
    keep, arr, caps = [], (L.VamRansStream * max(len(jobs), 1))(), []
    for j in jobs:
        s, i = _i32(j[0]), _i32(j[1])
        assert s.size == i.size
        caps.append(interleaved_capacity(s.size, K))
        keep.append((s, i))
    out = np.empty(sum(caps), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    for k, (s, i) in enumerate(keep):
        arr[k] = L.VamRansStream(s.ctypes.data, None, i.ctypes.data, None, s.size, 0, 0, out.ctypes.data + int(off[k]), caps[k], 0)
    L.check(L.load().vam_rans_interleaved_encode_streams(arr, len(jobs), t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                                         t.offsets.ctypes.data, t.cdf.shape[0], K,
                                                         coder_threads() if threads is None else int(threads)),
            "vam_rans_interleaved_encode_streams")
    return [out[int(off[k]):int(off[k]) + arr[k].n_bytes].tobytes() for k in range(len(jobs))]


def decode_prefix_streams(jobs: Sequence[Tuple], t: Tables, threads: Optional[int] = None, lanes: int = 1) -> List[int]:
    """Tolerant decode of many stream PREFIXES in one vam_rans_decode_prefix_streams call.  ``jobs``: (the first L >= 0
    bytes of a stream, the indexes of the whole stream, out); ``out`` is a writable C-contiguous int32 array of the indexes'
    size.  Per job the number of leading symbols the bytes decode (written to out[:count]; the rest of ``out`` is left
    untouched): L < 8 gives 0, a symbol whose renormalisation word or bypass nibbles are incomplete is not counted.
    ``lanes`` = K > 1: the strings are :func:`encode_interleaved`'s (vam_rans_interleaved_decode_prefix_streams): fewer than
    8 K bytes give 0, and the count is g K + the lowest lane of the last group whose element is incomplete."""
    K = check_lanes(lanes)
    keep, arr = [], (L.VamRansStream * max(len(jobs), 1))()
    for k, j in enumerate(jobs):
        src = np.frombuffer(j[0], dtype=np.uint8)
        i, o = _i32(j[1]), j[2]
        assert o.dtype == np.int32 and o.flags.c_contiguous and o.flags.writeable and o.size == i.size
        keep.append((src, i))
        arr[k] = L.VamRansStream(None, o.ctypes.data, i.ctypes.data, None, i.size, 0, 0, src.ctypes.data if src.size else None,
                                 src.size, src.size)
    counts = np.zeros(max(len(jobs), 1), dtype=np.int64)
    n_threads = coder_threads() if threads is None else int(threads)
    if K > 1:
        L.check(L.load().vam_rans_interleaved_decode_prefix_streams(arr, len(jobs), t.cdf.ctypes.data, t.cdf.shape[1],
                                                                    t.sizes.ctypes.data, t.offsets.ctypes.data, t.cdf.shape[0], K,
                                                                    n_threads, counts.ctypes.data),
                "vam_rans_interleaved_decode_prefix_streams")
        return [int(c) for c in counts[:len(jobs)]]
    L.check(L.load().vam_rans_decode_prefix_streams(arr, len(jobs), t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                                    t.offsets.ctypes.data, t.cdf.shape[0], n_threads, counts.ctypes.data),
            "vam_rans_decode_prefix_streams")
    return [int(c) for c in counts[:len(jobs)]]


def decode_interleaved_counted(stream: bytes, indexes, t: Tables, lanes: int) -> Tuple[np.ndarray, int, int]:
    """The tolerant decode of one :func:`encode_interleaved` string with its verdict (vam_rans_interleaved_decode_prefix):
    (symbols, count, status) — ``symbols[:count]`` are decoded, the rest is 0, and ``status`` is 0 or the code (2 index out
    of range, 3 cdf size invalid) that ended the stream.  Running out of bytes is no status: the count says it."""
    K = check_lanes(lanes)
    src = np.frombuffer(stream, dtype=np.uint8)
    i = _i32(indexes)
    out = np.zeros(i.size, dtype=np.int32)
    st = C.c_int32(0)
    n = L.load().vam_rans_interleaved_decode_prefix(src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size,
                                                    t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data, t.offsets.ctypes.data,
                                                    t.cdf.shape[0], K, out.ctypes.data, C.byref(st))
    if n < 0:
        L.check(int(n), "vam_rans_interleaved_decode_prefix")
    return out, int(n), int(st.value)


def decode_interleaved_strict(stream: bytes, indexes, t: Tables, lanes: int, what: str = "stream") -> np.ndarray:
    """The symbols of an :func:`encode_interleaved` string that is needed WHOLE (z and the base slices of an ``"embedded-4"``
    container): :func:`decode_interleaved_counted` with count == n required.  ValueError names ``what``
    and gives :func:`status_text`: the status that ended the stream, or 1 (truncated) for a string that ends early."""
    out, count, st = decode_interleaved_counted(stream, indexes, t, lanes)
    if st or count != out.size:
        raise ValueError(f"{what}: {status_text(st if st else 1)} ({count} of {out.size} elements decode from {len(stream)} bytes "
                         f"on {lanes} lanes)")
    return out


@dataclass
class Checkpoints:
    """The checkpoints of ``n`` resumable streams on K lanes: per stream the decoder at the start of a
    group — ``done`` elements before it, ``pos`` the next word of the whole string, ``states`` [n, K] the lane states.  On the
    host numpy arrays (uint64, int64, int64), on the device tensors (int64 holding the uint64 bits, int32, int32)."""
    states: object
    done: object
    pos: object

    @staticmethod
    def fresh(n_streams: int, lanes: int, device=None) -> "Checkpoints":
        K = check_lanes(lanes)
        if device is None:
            return Checkpoints(np.zeros((n_streams, K), dtype=np.uint64), np.zeros(n_streams, dtype=np.int64),
                               np.zeros(n_streams, dtype=np.int64))
        return Checkpoints(torch.zeros((n_streams, K), dtype=torch.int64, device=device),
                           torch.zeros(n_streams, dtype=torch.int32, device=device),
                           torch.zeros(n_streams, dtype=torch.int32, device=device))


def resume_prefix_streams(jobs: Sequence[Tuple], t: Tables, checkpoints: Checkpoints, threads: Optional[int] = None, lanes: int = 1,
                          status: Optional[np.ndarray] = None) -> List[int]:
    """:func:`decode_prefix_streams` continued from ``checkpoints`` (host arrays, one row per job, updated in place) in one
    vam_rans_interleaved_resume_streams call.  ``jobs``: (the bytes of the string FROM BYTE 4 * pos ON, the indexes of the
    whole stream, out); out[done_in:count] is written, nothing else.  Per job the count :func:`decode_prefix_streams` gives
    on everything received so far.  The bytes beyond the last whole word are not consumed: send them again, in front of what
    follows.  ``status`` (int32, one per job) receives the status codes; a non-zero one raises VamError all the same."""
    K = check_lanes(lanes)
    ck = checkpoints
    nj = len(jobs)
    if not (isinstance(ck.states, np.ndarray) and ck.states.dtype == np.uint64 and ck.states.shape == (nj, K)
            and ck.states.flags.c_contiguous and all(isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == (nj,)
                                                     for a in (ck.done, ck.pos))):
        raise ValueError(f"resume_prefix_streams: host checkpoints of {nj} streams on {K} lanes (Checkpoints.fresh)")
    keep, arr, cks = [], (L.VamRansStream * max(nj, 1))(), (L.VamRansCheckpoint * max(nj, 1))()
    for k, j in enumerate(jobs):
        src = np.frombuffer(j[0], dtype=np.uint8)
        i, o = _i32(j[1]), j[2]
        assert o.dtype == np.int32 and o.flags.c_contiguous and o.flags.writeable and o.size == i.size
        keep.append((src, i))
        arr[k] = L.VamRansStream(None, o.ctypes.data, i.ctypes.data, None, i.size, 0, 0, src.ctypes.data if src.size else None,
                                 src.size, src.size)
        cks[k] = L.VamRansCheckpoint(int(ck.done[k]), int(ck.pos[k]), ck.states.ctypes.data + 8 * K * k)
    counts = np.zeros(max(nj, 1), dtype=np.int64)
    st = np.zeros(max(nj, 1), dtype=np.int32)
    rc = L.load().vam_rans_interleaved_resume_streams(arr, cks, nj, t.cdf.ctypes.data, t.cdf.shape[1], t.sizes.ctypes.data,
                                                      t.offsets.ctypes.data, t.cdf.shape[0], K,
                                                      coder_threads() if threads is None else int(threads), counts.ctypes.data,
                                                      st.ctypes.data)
    for k in range(nj):
        ck.done[k], ck.pos[k] = cks[k].done, cks[k].pos
    if status is not None:
        status[:nj] = st[:nj]
    L.check(rc, "vam_rans_interleaved_resume_streams")
    return [int(c) for c in counts[:nj]]


def prefix_bytes(stream: bytes, indexes, counts: Sequence[int], t: Tables, lanes: int = 1) -> List[int]:
    """Per element count of the sorted list ``counts``: the smallest byte length (a multiple of 4) from which
    :func:`decode_prefix_streams` yields at least that many symbols of ``stream`` (0 for a count of 0).  One decoding pass.
    ``lanes`` = K > 1: of an :func:`encode_interleaved` string — 4 x the read position after the last word that any of the
    first ``count`` elements reads, 8 K when they read none."""
    return [int(b) for b in _prefix_bytes(stream, indexes, np.ascontiguousarray([int(c) for c in counts], dtype=np.int64), t, lanes)]


def _prefix_bytes(stream: bytes, indexes, want: np.ndarray, t: Tables, lanes: int) -> np.ndarray:
    """:func:`prefix_bytes` on arrays: ``want`` contiguous int64 counts, the result int64 of the same length."""
    K = check_lanes(lanes)
    src = np.frombuffer(stream, dtype=np.uint8)
    i = _i32(indexes)
    out = np.zeros(max(want.size, 1), dtype=np.int64)
    head = (src.ctypes.data if src.size else None, src.size, i.ctypes.data, i.size, t.cdf.ctypes.data, t.cdf.shape[1],
            t.sizes.ctypes.data, t.offsets.ctypes.data, t.cdf.shape[0])
    tail = (want.ctypes.data if want.size else None, want.size, out.ctypes.data)
    if K > 1:
        L.check(L.load().vam_rans_interleaved_prefix_bytes(*head, K, *tail), "vam_rans_interleaved_prefix_bytes")
    else:
        L.check(L.load().vam_rans_prefix_bytes(*head, *tail), "vam_rans_prefix_bytes")
    return out[:want.size]


def cut_table(stream: bytes, indexes, t: Tables, lanes: int = 1) -> np.ndarray:
    """The cut table of one embedded string: int32 [n + 1], entry c = :func:`prefix_bytes` of count c,
    for every count 0 .. n, from ONE prefix_bytes pass over the string (one decoding pass).  The row never decreases, entry 0 is 0 and
    entry n is at most ``len(stream)``."""
    n = _i32(indexes).size
    return _prefix_bytes(stream, indexes, np.arange(n + 1, dtype=np.int64), t, lanes).astype(np.int32)


# ---------------------------------------------------------------- coded-size pricing
LOG2E = 1.4426950408889634
MAX_BYPASS = 8            # raw nibbles of one out-of-range value (a 32-bit raw value; csrc/rans.cpp)


def cost_table(t: Tables) -> np.ndarray:
    """float64 [n, stride]: what the coder charges for entry v of table i, 16 - log2(cdf[i][v+1] - cdf[i][v]) bits, for
    v <= sizes[i] - 2 (entry sizes[i] - 2 is the escape); 0 beyond.  Tables the coder itself would refuse are refused."""
    cdf = t.cdf.astype(np.int64)
    n, stride = cdf.shape
    mx = t.sizes.astype(np.int64) - 2
    if (mx < 0).any() or (mx + 1 >= stride).any():
        raise ValueError(f"cdf sizes {t.sizes.tolist()} invalid for tables of stride {stride}")
    used = np.arange(stride - 1)[None, :] <= mx[:, None]
    freq = np.where(used, cdf[:, 1:] - cdf[:, :-1], 1)
    if (freq <= 0).any():
        raise ValueError("zero-frequency symbol (cdf table not normalised)")
    out = np.zeros((n, stride), dtype=np.float64)
    out[:, :-1] = np.where(used, 16.0 - np.log2(freq.astype(np.float64)), 0.0)
    return out


def price(symbols, indexes, t: Tables, layer=None, sel: int = 0, cost: Optional[np.ndarray] = None) -> np.ndarray:
    """The exact price in bits of every element of a stream as :func:`encode` / :func:`encode_streams` code it (with a
    ``layer`` array: symbol 0 in table 0 where layer != sel), float64 of the symbols' shape: the table entry's
    16 - log2(freq), and for a value outside the table the escape entry plus 4 * (1 + n_bypass) bits (one count nibble and
    n_bypass <= 8 raw nibbles).  The host statement of what vam_coded_layer_bits computes on the device."""
    s = np.asarray(symbols).astype(np.int64)
    i = np.broadcast_to(np.asarray(indexes), s.shape).astype(np.int64)
    if layer is not None:
        keep = np.asarray(layer) == sel
        s, i = np.where(keep, s, 0), np.where(keep, i, 0)
    if i.size and (i.min() < 0 or i.max() >= t.cdf.shape[0]):
        raise ValueError("index out of range")
    cost = cost_table(t) if cost is None else cost
    mx = t.sizes.astype(np.int64)[i] - 2
    v = s - t.offsets.astype(np.int64)[i]
    inside = (v >= 0) & (v < mx)
    raw = np.where(v < 0, -2 * v - 1, 2 * (v - mx)) & 0xFFFFFFFF
    nb = np.zeros(s.shape, dtype=np.int64)
    for k in range(MAX_BYPASS):
        nb += (raw >> (4 * k)) != 0
    return np.where(inside, cost[i, np.where(inside, v, 0)], cost[i, mx] + 4.0 * (1 + nb))


def stream_words(bits, n_symbols):
    """(lo, hi) bounds of the number W of 32-bit words a stream flushes before its final state, from its exact table cost
    ``bits`` (S) and its number of symbols n.  The coder's state obeys 32 W + log2(x_final) = 31 + S + e with log2(x_final)
    in [31, 63), so W = floor((S + e) / 32).  Every symbol put maps x to floor(x / f) * 2^16 + x % f + start with
    floor(x / f) >= 2^15 (renormalisation included: floor(floor(u) / f) = floor(u / f)), so it moves log2 x by
    16 - log2 f up to log2(1 + 2^-15); a bypass nibble shifts a state >= 2^27 by four bits: up to log2(1 + 2^-27), at most
    9 nibbles per symbol.  Hence |e| <= n * log2(e) * (2^-15 + 9 * 2^-27); the float64 rounding of S itself gets
    S * 2^-36 + 2^-30 on top.  lo == hi unless S is that close to a multiple of 32."""
    S = np.asarray(bits, dtype=np.float64)
    n = np.asarray(n_symbols, dtype=np.float64)
    e = n * LOG2E * (2.0 ** -15 + 9.0 * 2.0 ** -27) + S * 2.0 ** -36 + 2.0 ** -30
    lo = np.floor((S - e) / 32.0).astype(np.int64)
    hi = np.floor((S + e) / 32.0).astype(np.int64)
    return np.maximum(lo, 0), np.maximum(hi, 0)


def stream_bytes(bits, n_symbols):
    """(lo, hi) bounds of a stream's length in bytes: 8 (the final 64-bit state) + 4 W (:func:`stream_words`).  The two
    are equal or 4 apart for streams of up to about 3e5 symbols."""
    lo, hi = stream_words(bits, n_symbols)
    return 8 + 4 * lo, 8 + 4 * hi


@dataclass
class DeviceTables:
    """The device-side companion of :class:`Tables` for the pricing kernels: the float64 cost table (16 - log2(freq), built
    once on the host from the int32 CDFs), sizes and offsets, and the constants an element outside the variance mask costs:
    ``zero_cost[i]`` = the price of symbol 0 under table i (a container layer codes 0 in table 0, compress(x, q) codes 0
    at the index build_indexes gives sigma = 0)."""
    host: Tables
    cost: torch.Tensor        # float64 [n, stride]
    sizes: torch.Tensor       # int32 [n]
    offsets: torch.Tensor     # int32 [n]
    zero_cost: np.ndarray     # float64 [n]
    struct: "L.VamCoderTables"
    key: tuple = ()           # the generation key of ``host`` and the device

    def __deepcopy__(self, memo):
        return None           # device pointers of THIS model: a copied model builds its own at its first use

    @staticmethod
    def of(model, device) -> "DeviceTables":
        t = Tables.of(model)
        key = (model._tables_key, str(torch.device(device)))
        d = getattr(model, "_device_tables", None)
        if d is None or d.key != key:
            c = cost_table(t)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            d = DeviceTables(t, dev(c), dev(t.sizes), dev(t.offsets),
                             price(np.zeros(t.cdf.shape[0], dtype=np.int64), np.arange(t.cdf.shape[0]), t, cost=c), None, key)
            d.struct = L.VamCoderTables(d.cost.data_ptr(), d.sizes.data_ptr(), d.offsets.data_ptr(), t.cdf.shape[0], t.cdf.shape[1])
            object.__setattr__(model, "_device_tables", d)
        return d


# ---------------------------------------------------------------- the coder on the device
STATUS_TEXT = {1: "bitstream truncated", 2: "index out of range", 3: "cdf size invalid for its table",
               4: "output buffer too small", 5: "zero-frequency symbol (cdf table not normalised)",
               6: "bad arguments (a stream is at least 8 bytes, in whole words)"}


def status_text(st: int, lanes: int = 1) -> str:
    """The words for a status code; for a lane-split string code 6 is the header check's refusal."""
    if st == 6 and lanes > 1:
        return f"bad stream (the header of {lanes} lane lengths does not match the string)"
    return STATUS_TEXT.get(st, f"status {st}")


def pack_tables(t: Tables):
    """The tables ragged as 16-bit values for the decoder's LDS copy: table k is its entries 0 .. sizes[k]-2 at starts[k],
    the terminal 65536 implied; the total is padded to a multiple of 8 entries (16-byte loads).  None when a table does
    not start at 0, increase strictly and end at 65536 within its row: the decoder then reads the int32 tables."""
    sizes = t.sizes.astype(np.int64)
    if (sizes < 2).any() or (sizes > t.cdf.shape[1]).any():
        return None
    rows = [t.cdf[k, :sizes[k]].astype(np.int64) for k in range(t.cdf.shape[0])]
    if any(r[0] != 0 or r[-1] != 65536 or (np.diff(r) <= 0).any() for r in rows):
        return None
    starts = np.concatenate([[0], np.cumsum(sizes - 1)]).astype(np.int64)
    packed = np.zeros((int(starts[-1]) + 7) // 8 * 8, dtype=np.uint16)
    for k, r in enumerate(rows):
        packed[starts[k]:starts[k + 1]] = r[:-1]
    return packed, starts[:-1].astype(np.int32)


@dataclass
class DeviceCoderTables:
    """The device coder's companion of :class:`Tables`, next to :class:`DeviceTables` and keyed like it: the int32 CDFs,
    sizes and offsets on the device (the encoder's look-ups, the decoder's fallback) and the packed 16-bit form with
    per-table start offsets, kept when it fits the LDS a workgroup may use (``lds_bytes`` of ``lds_limit``)."""
    host: Tables
    cdf: torch.Tensor
    sizes: torch.Tensor
    offsets: torch.Tensor
    packed: Optional[torch.Tensor]     # int16 storage of the uint16 values
    starts: Optional[torch.Tensor]
    lds_bytes: int                     # the packed tables' size (0: not packable)
    lds_limit: int
    struct: "L.VamRansTables"
    key: tuple = ()

    def __deepcopy__(self, memo):
        return None           # device pointers of THIS model: a copied model builds its own at its first use

    @staticmethod
    def build(t: Tables, device, key=()) -> "DeviceCoderTables":
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        with torch.cuda.device(device):
            limit = L.load().vam_rans_lds_table_bytes()
        if limit < 0:
            L.check(limit, "vam_rans_lds_table_bytes")
        pk = pack_tables(t)
        lds = 2 * pk[0].size if pk is not None else 0
        fits = pk is not None and lds <= limit
        d = DeviceCoderTables(t, dev(t.cdf), dev(t.sizes), dev(t.offsets), dev(pk[0].view(np.int16)) if fits else None,
                              dev(pk[1]) if fits else None, lds, limit, None, key)
        d.struct = L.VamRansTables(d.cdf.data_ptr(), d.sizes.data_ptr(), d.offsets.data_ptr(), t.cdf.shape[0], t.cdf.shape[1],
                                   d.packed.data_ptr() if fits else None, d.starts.data_ptr() if fits else None,
                                   pk[0].size if fits else 0, 0)
        return d

    @staticmethod
    def of(model, device) -> "DeviceCoderTables":
        t = Tables.of(model)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (model._tables_key, str(device))
        d = getattr(model, "_device_coder_tables", None)
        if d is None or d.key != key:
            d = DeviceCoderTables.build(t, device, key)
            object.__setattr__(model, "_device_coder_tables", d)
        return d


def _geometry(sym_view, idx_view, n_slices: int, C_: int, layer):
    buf = sym_view.buf
    B, h, w, ld = (int(v) for v in buf.shape)
    if buf.dtype != torch.int32 or not buf.is_contiguous() or sym_view.c0 + n_slices * C_ > ld:
        raise ValueError(f"device coder: symbols are a contiguous int32 [B,h,w,ld] buffer holding {n_slices} x {C_} channels from {sym_view.c0}")
    if idx_view is not None and (idx_view.buf.dtype != torch.int32 or tuple(idx_view.buf.shape) != tuple(buf.shape)
                                 or idx_view.c0 != sym_view.c0 or not idx_view.buf.is_contiguous()):
        raise ValueError("device coder: the index window must have the geometry of the symbol window")
    if layer is not None and (layer.dtype != torch.uint8 or tuple(layer.shape) != tuple(buf.shape) or not layer.is_contiguous()):
        raise ValueError("device coder: the layer ids must be a uint8 buffer of the symbols' shape")
    return B, h, w, ld


def raise_status(status: np.ndarray, B: int, what: str, lanes: int = 1):
    """VamError for the first stream with a non-zero status; stream id = slice * B + image.  ``lanes`` > 1: one code per
    (stream, lane), and the message names the stream's lowest-numbered failing lane too."""
    bad = np.flatnonzero(status)
    if bad.size:
        k, st = int(bad[0]) // lanes, int(status[bad[0]])
        n_bad = np.unique(bad // lanes).size
        raise L.VamError(f"{what}: stream (image {k % B}, slice {k // B})" + (f", lane {int(bad[0]) % lanes}" if lanes > 1 else "")
                         + f": {status_text(st, lanes)}" + (f" ({n_bad} streams failed)" if n_bad > 1 else ""))


def encode_streams_device(sym_view, idx_view, n_slices: int, C_: int, tables: DeviceCoderTables, layer=None,
                          sel: int = 0, lanes: int = 1, lane_kernels: Optional[bool] = None) -> List[List[bytes]]:
    """All B * n_slices streams of an int32 NHWC window in one vam_rans_encode_device launch on the current stream, packed by
    vam_rans_pack_device, then two device-to-host copies: the lengths with the status codes, and the coded bytes.
    ``idx_view`` None: table index = channel (the z streams).  Returns ``[slice][image]``; each stream's bytes equal
    :func:`encode`'s on the window's [C, h, w] transpose.

    ``lanes`` = K > 1: one vam_rans_lanes_encode_device launch, one thread per (stream, lane), packed
    over the K * B * n_slices lane regions; each string equals :func:`encode_lanes`'s.  K is not stored in the strings.
    ``lane_kernels``: run the per-lane kernel also at K = 1 (the same bytes; None: only for K > 1)."""
    from . import ops
    K = check_lanes(lanes)
    B, h, w, ld = _geometry(sym_view, idx_view, n_slices, C_, layer)
    if K > 1 if lane_kernels is None else lane_kernels:
        return _encode_lanes_device(sym_view, idx_view, n_slices, C_, tables, layer, sel, K, B, h, w, ld)
    ns, cap = B * n_slices, 2 * C_ * h * w + 16            # 8 n + 64 bytes per stream, the host coder's budget
    dev = sym_view.buf.device
    regions = torch.empty(ns * cap, dtype=torch.int32, device=dev)
    packed = torch.empty(ns * cap, dtype=torch.int32, device=dev)
    meta = torch.empty((2, ns), dtype=torch.int32, device=dev)          # lengths in words, status
    offs = torch.empty(ns + 1, dtype=torch.int64, device=dev)
    lib, st = L.load(), ops.stream_ptr()
    L.check(lib.vam_rans_encode_device(sym_view.buf.data_ptr(), idx_view.buf.data_ptr() if idx_view is not None else None,
                                       layer.data_ptr() if layer is not None else None, int(sel), B, h, w, ld, sym_view.c0, C_,
                                       n_slices, C.byref(tables.struct), regions.data_ptr(), cap, meta[0].data_ptr(),
                                       meta[1].data_ptr(), st), "vam_rans_encode_device")
    L.check(lib.vam_rans_pack_device(regions.data_ptr(), cap, meta[0].data_ptr(), ns, packed.data_ptr(), ns * cap,
                                     offs.data_ptr(), st), "vam_rans_pack_device")
    m = meta.cpu().numpy()
    raise_status(m[1], B, "vam_rans_encode_device")
    off = np.concatenate([[0], np.cumsum(m[0].astype(np.int64))]) * 4
    data = packed[:int(off[-1]) // 4].cpu().numpy().view(np.uint8)
    return [[data[off[s * B + b]:off[s * B + b + 1]].tobytes() for b in range(B)] for s in range(n_slices)]


def _encode_lanes_device(sym_view, idx_view, n_slices, C_, tables, layer, sel, K, B, h, w, ld) -> List[List[bytes]]:
    """encode_streams_device with one thread per (stream, lane): the pack over the lane regions leaves every stream's lanes
    back to back, and the lengths it scanned are the headers."""
    from . import ops
    n = C_ * h * w
    ns, cap = B * n_slices, 2 * (-(-n // K)) + 16          # 8 m + 64 bytes per lane of m = ceil(n / K) elements
    dev = sym_view.buf.device
    regions = torch.empty(ns * K * cap, dtype=torch.int32, device=dev)
    packed = torch.empty(ns * K * cap, dtype=torch.int32, device=dev)
    meta = torch.empty((2, ns * K), dtype=torch.int32, device=dev)      # per (stream, lane): length in words, status
    offs = torch.empty(ns * K + 1, dtype=torch.int64, device=dev)
    lib, st = L.load(), ops.stream_ptr()
    L.check(lib.vam_rans_lanes_encode_device(sym_view.buf.data_ptr(), idx_view.buf.data_ptr() if idx_view is not None else None,
                                             layer.data_ptr() if layer is not None else None, int(sel), B, h, w, ld, sym_view.c0,
                                             C_, n_slices, K, C.byref(tables.struct), regions.data_ptr(), cap, meta[0].data_ptr(),
                                             meta[1].data_ptr(), st), "vam_rans_lanes_encode_device")
    L.check(lib.vam_rans_pack_device(regions.data_ptr(), cap, meta[0].data_ptr(), ns * K, packed.data_ptr(), ns * K * cap,
                                     offs.data_ptr(), st), "vam_rans_pack_device")
    m = meta.cpu().numpy()
    raise_status(m[1], B, "vam_rans_lanes_encode_device", K)
    lens = m[0].reshape(ns, K)
    off = np.concatenate([[0], np.cumsum(lens.sum(1).astype(np.int64))]) * 4      # the streams' bodies, back to back
    data = packed[:int(off[-1]) // 4].cpu().numpy().view(np.uint8)
    head = (lambda k: b"") if K == 1 else (lambda k: lens[k].astype("<u4").tobytes())
    return [[head(s * B + b) + data[off[s * B + b]:off[s * B + b + 1]].tobytes() for b in range(B)] for s in range(n_slices)]


@dataclass
class DeviceStreams:
    """Byte strings on the device: one uint8 buffer [offsets int64 | lengths int32 | the strings, each at a multiple of 4],
    uploaded in one host-to-device copy; ``status`` receives one code per (string, lane)."""
    buf: torch.Tensor
    n: int
    status: torch.Tensor       # int32 [n * lanes]
    lanes: int = 1

    @property
    def offsets_ptr(self): return self.buf.data_ptr()
    @property
    def lengths_ptr(self): return self.buf.data_ptr() + 8 * self.n
    @property
    def bytes_ptr(self): return self.buf.data_ptr() + 8 * self.n + 4 * (self.n + self.n % 2)


def upload_streams(strings: Sequence[bytes], device, lanes: int = 1) -> DeviceStreams:
    lanes = check_lanes(lanes)
    n = len(strings)
    lens = np.array([len(s_) for s_ in strings], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
    head = 8 * n + 4 * (n + n % 2)
    host = np.zeros(head + int(off[-1]) + 4, dtype=np.uint8)
    host[:8 * n].view(np.int64)[:] = off[:-1]
    host[8 * n:8 * n + 4 * n].view(np.int32)[:] = lens
    for k, s_ in enumerate(strings):
        host[head + off[k]:head + off[k] + lens[k]] = np.frombuffer(s_, dtype=np.uint8)
    return DeviceStreams(torch.from_numpy(host).to(device), n, torch.zeros(max(n, 1) * lanes, dtype=torch.int32, device=device), lanes)


def decode_uploaded(up: DeviceStreams, first: int, idx_view, sym_view, n_slices: int, C_: int, tables: DeviceCoderTables,
                    layer=None, sel: int = 0, lanes: int = 1, lane_kernels: Optional[bool] = None):
    """One vam_rans_decode_device launch on the current stream: the B * n_slices strings of ``up`` from ``first`` on
    (string first + slice * B + image) into the window of ``sym_view``.  No synchronisation.  ``lanes`` = K > 1: the
    strings are lane-split (:func:`encode_lanes`) and ``up`` was uploaded with the same K; one
    vam_rans_lanes_decode_device launch, one thread and one status code per (string, lane).  ``lane_kernels``: run the
    per-lane kernel also at K = 1 (None: only for K > 1)."""
    from . import ops
    K = check_lanes(lanes)
    B, h, w, ld = _geometry(sym_view, idx_view, n_slices, C_, layer)
    if first < 0 or first + B * n_slices > up.n:
        raise ValueError(f"device coder: strings {first} .. {first + B * n_slices} of {up.n} uploaded")
    if K != up.lanes:
        raise ValueError(f"device coder: strings uploaded for {up.lanes} lanes, decode asked for {K}")
    if K > 1 if lane_kernels is None else lane_kernels:
        L.check(L.load().vam_rans_lanes_decode_device(up.bytes_ptr, up.offsets_ptr + 8 * first, up.lengths_ptr + 4 * first,
                                                      idx_view.buf.data_ptr() if idx_view is not None else None,
                                                      layer.data_ptr() if layer is not None else None, int(sel), B, h, w, ld,
                                                      sym_view.c0, C_, n_slices, K, C.byref(tables.struct), sym_view.buf.data_ptr(),
                                                      up.status.data_ptr() + 4 * first * K, ops.stream_ptr()),
                "vam_rans_lanes_decode_device")
        return
    L.check(L.load().vam_rans_decode_device(up.bytes_ptr, up.offsets_ptr + 8 * first, up.lengths_ptr + 4 * first,
                                            idx_view.buf.data_ptr() if idx_view is not None else None,
                                            layer.data_ptr() if layer is not None else None, int(sel), B, h, w, ld, sym_view.c0, C_,
                                            n_slices, C.byref(tables.struct), sym_view.buf.data_ptr(),
                                            up.status.data_ptr() + 4 * first, ops.stream_ptr()), "vam_rans_decode_device")


def decode_streams_device(strings: Sequence[Sequence[bytes]], idx_view, sym_view, n_slices: int, C_: int,
                          tables: DeviceCoderTables, layer=None, sel: int = 0, lanes: int = 1,
                          lane_kernels: Optional[bool] = None) -> DeviceStreams:
    """``strings[slice][image]`` uploaded in one host-to-device copy and decoded by one launch into the window of
    ``sym_view``, on the current stream.  Returns without synchronising; :func:`check_status` reads the codes later.
    ``lanes`` / ``lane_kernels``: as in :func:`decode_uploaded`."""
    B = int(sym_view.buf.shape[0])
    if len(strings) != n_slices or any(len(row) != B for row in strings):
        raise ValueError(f"device coder: expected {n_slices} slices x {B} images of strings")
    up = upload_streams([s_ for row in strings for s_ in row], sym_view.buf.device, lanes)
    decode_uploaded(up, 0, idx_view, sym_view, n_slices, C_, tables, layer, sel, lanes, lane_kernels)
    return up


def check_status(up: DeviceStreams, B: int, what: str = "vam_rans_decode_device", name=None, lanes: Optional[int] = None):
    """Reads the status codes of ``up`` (synchronises) and raises VamError naming the first failed stream, and with
    ``lanes`` > 1 (None: what ``up`` was uploaded for) its lowest-numbered failing lane.  ``name(k)`` words string k; the
    default is stream id = slice * B + image."""
    K = up.lanes if lanes is None else check_lanes(lanes)
    if K != up.lanes:
        raise ValueError(f"device coder: strings uploaded for {up.lanes} lanes, status asked for {K}")
    st = up.status[:up.n * K].cpu().numpy()
    if name is None:
        return raise_status(st, B, what, K)
    bad = np.flatnonzero(st)
    if bad.size:
        k = int(bad[0])
        raise L.VamError(f"{what}: {name(k // K)}" + (f", lane {k % K}" if K > 1 else "")
                         + f": {status_text(int(st[k]), K)}")


# ---------------------------------------------------------------- layered launches: a container's layers
LAYER_SCRATCH_BYTES = 1 << 30     # default bound of encode_layers_device's device scratch: regions plus packed buffer


def layer_groups(n_levels: int, level_bytes: int, max_scratch_bytes: Optional[int] = None) -> List[Tuple[int, int]]:
    """The consecutive level ranges [k0, k1) that :func:`encode_layers_device` codes per launch: as many levels as keep
    ``(k1 - k0) * level_bytes`` (one level's regions plus its share of the packed buffer) within ``max_scratch_bytes``
    (None: LAYER_SCRATCH_BYTES), at least one level per group whatever the bound.  Covers 0 .. n_levels in order."""
    if n_levels < 1 or level_bytes < 1:
        raise ValueError(f"layer_groups: n_levels and level_bytes must be >= 1, got {n_levels} and {level_bytes}")
    budget = LAYER_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
    per = max(1, budget // int(level_bytes))
    return [(k0, min(k0 + per, n_levels)) for k0 in range(0, n_levels, per)]


def layer_status_message(status: np.ndarray, B: int, n_slices: int, what: str, lanes: int = 1, first_level: int = 0) -> Optional[str]:
    """The words for the first non-zero code of a layered launch, None when every stream is fine.  One code per (stream,
    lane), stream id = (k * n_slices + slice) * B + image; the level is printed as ``first_level`` + k."""
    bad = np.flatnonzero(status)
    if not bad.size:
        return None
    k, st = int(bad[0]) // lanes, int(status[bad[0]])
    n_bad = np.unique(bad // lanes).size
    return (f"{what}: stream (image {k % B}, level {first_level + k // (B * n_slices)}, slice {k // B % n_slices})"
            + (f", lane {int(bad[0]) % lanes}" if lanes > 1 else "") + f": {status_text(st, lanes)}"
            + (f" ({n_bad} streams failed)" if n_bad > 1 else ""))


def _check_layers(layer, sel0: int, n_sel: int):
    if layer is None:
        raise ValueError("device coder: a layered launch needs the layer ids")
    if sel0 < 0 or n_sel < 1 or sel0 + n_sel > 256:
        raise ValueError(f"device coder: selectors [{sel0}, {sel0 + n_sel}) outside the layer ids 0 .. 255")


def encode_layers_device(sym_view, idx_view, layer, n_levels: int, n_slices: int, C_: int, tables: DeviceCoderTables,
                         lanes: int = 1, sel0: int = 0, max_scratch_bytes: Optional[int] = None,
                         first_level: Optional[int] = None) -> List[List[List[bytes]]]:
    """The layers ``sel0 .. sel0 + n_levels - 1`` of an int32 NHWC window, all n_levels * n_slices * B streams of a group
    of levels in ONE vam_rans_layers_encode_device launch on the current stream.  Returns ``[level][slice][image]``; string
    (k, s, b) is what :func:`encode_streams_device` gives with ``sel = sel0 + k``: the elements with layer == sel0 + k, every
    other one as symbol 0 in table 0.  ``lanes`` = K > 1: lane-split strings, one thread per (stream, lane).

    A stream's region is the host budget, 8 n + 64 bytes (per lane 8 ceil(n / K) + 64), and the packed buffer is as large
    again, so n_levels levels need n_levels times the scratch of one :func:`encode_streams_device` call.  It is bounded:
    the levels are coded in the groups of :func:`layer_groups` under ``max_scratch_bytes`` (None: LAYER_SCRATCH_BYTES), each
    group one encode launch, one pack, one read of lengths + status and one read of the bytes.  ``first_level``: the number
    an error message prints for level 0 (None: sel0)."""
    from . import ops
    K = check_lanes(lanes)
    n_levels, sel0 = int(n_levels), int(sel0)
    _check_layers(layer, sel0, n_levels)
    B, h, w, ld = _geometry(sym_view, idx_view, n_slices, C_, layer)
    n = C_ * h * w
    per, cap = B * n_slices, 2 * (-(-n // K)) + 16
    dev = sym_view.buf.device
    lib, st = L.load(), ops.stream_ptr()
    out: List[List[List[bytes]]] = []
    for k0, k1 in layer_groups(n_levels, 2 * 4 * per * K * cap, max_scratch_bytes):
        ns = (k1 - k0) * per
        regions = torch.empty(ns * K * cap, dtype=torch.int32, device=dev)
        packed = torch.empty(ns * K * cap, dtype=torch.int32, device=dev)
        meta = torch.empty((2, ns * K), dtype=torch.int32, device=dev)      # per (stream, lane): length in words, status
        offs = torch.empty(ns * K + 1, dtype=torch.int64, device=dev)
        L.check(lib.vam_rans_layers_encode_device(sym_view.buf.data_ptr(), idx_view.buf.data_ptr() if idx_view is not None else None,
                                                  layer.data_ptr(), sel0 + k0, k1 - k0, B, h, w, ld, sym_view.c0, C_, n_slices, K,
                                                  C.byref(tables.struct), regions.data_ptr(), cap, meta[0].data_ptr(),
                                                  meta[1].data_ptr(), st), "vam_rans_layers_encode_device")
        L.check(lib.vam_rans_pack_device(regions.data_ptr(), cap, meta[0].data_ptr(), ns * K, packed.data_ptr(), ns * K * cap,
                                         offs.data_ptr(), st), "vam_rans_pack_device")
        m = meta.cpu().numpy()
        msg = layer_status_message(m[1], B, n_slices, "vam_rans_layers_encode_device", K,
                                   (sel0 if first_level is None else first_level) + k0)
        if msg:
            raise L.VamError(msg)
        lens = m[0].reshape(ns, K)
        off = np.concatenate([[0], np.cumsum(lens.sum(1).astype(np.int64))]) * 4      # the streams' bodies, back to back
        data = packed[:int(off[-1]) // 4].cpu().numpy().view(np.uint8)
        head = (lambda i: b"") if K == 1 else (lambda i: lens[i].astype("<u4").tobytes())
        for k in range(k1 - k0):
            out.append([[head(i) + data[off[i]:off[i + 1]].tobytes() for i in range((k * n_slices + s) * B, (k * n_slices + s + 1) * B)]
                        for s in range(n_slices)])
    return out


def decode_layers_uploaded(up: DeviceStreams, first: int, idx_view, sym_view, layer, sel0: int, n_sel: int, n_slices: int, C_: int,
                           tables: DeviceCoderTables, lanes: int = 1):
    """One vam_rans_layers_decode_device launch on the current stream, no synchronisation: the n_sel * n_slices * B strings
    of ``up`` from ``first`` on (string first + (k * n_slices + slice) * B + image is layer sel0 + k) into the ONE window of
    ``sym_view``.  Every level writes only the elements of its own layer; elements of other layers keep what they hold.
    The status codes go to ``up.status`` (one per (string, lane)); :func:`check_layer_status` reads them later."""
    from . import ops
    K = check_lanes(lanes)
    sel0, n_sel = int(sel0), int(n_sel)
    _check_layers(layer, sel0, n_sel)
    B, h, w, ld = _geometry(sym_view, idx_view, n_slices, C_, layer)
    count = n_sel * n_slices * B
    if first < 0 or first + count > up.n:
        raise ValueError(f"device coder: strings {first} .. {first + count} of {up.n} uploaded")
    if K != up.lanes:
        raise ValueError(f"device coder: strings uploaded for {up.lanes} lanes, decode asked for {K}")
    L.check(L.load().vam_rans_layers_decode_device(up.bytes_ptr, up.offsets_ptr + 8 * first, up.lengths_ptr + 4 * first,
                                                   idx_view.buf.data_ptr() if idx_view is not None else None, layer.data_ptr(),
                                                   sel0, n_sel, B, h, w, ld, sym_view.c0, C_, n_slices, K, C.byref(tables.struct),
                                                   sym_view.buf.data_ptr(), up.status.data_ptr() + 4 * first * K, ops.stream_ptr()),
            "vam_rans_layers_decode_device")


def check_layer_status(up: DeviceStreams, B: int, n_slices: int, what: str = "vam_rans_layers_decode_device", first_level: int = 0):
    """Reads the status codes of an upload that holds only the strings of one layered launch (synchronises) and raises
    VamError naming image, level, slice and, for lane-split strings, the lowest-numbered failing lane."""
    msg = layer_status_message(up.status[:up.n * up.lanes].cpu().numpy(), B, n_slices, what, up.lanes, first_level)
    if msg:
        raise L.VamError(msg)


# ---------------------------------------------------------------- embedded streams on the device coder
def encode_embedded_device(r_sym: torch.Tensor, r_idx: torch.Tensor, tables: DeviceCoderTables, lanes: int = 1,
                           count: Optional[torch.Tensor] = None) -> Tuple[List[bytes], np.ndarray]:
    """The flat ranked buffers ``r_sym`` / ``r_idx`` (contiguous int32 [..., n] on the device, every leading index one
    stream) as :func:`encode_interleaved` strings (K = 1: :func:`encode`'s) in ONE vam_rans_interleaved_encode_device launch
    on the current stream, packed by vam_rans_pack_device; then one copy of lengths, status codes and marks and one of the
    coded bytes.  ``count``: int32 [L, ...streams] on the device, non-decreasing in L; the second result is then
    :func:`prefix_bytes` of every count, int64 [L, n_streams], taken from the encoder's own word positions (None: [0, n_streams])."""
    from . import ops
    K = check_lanes(lanes)
    for a in (r_sym, r_idx):
        if a.dtype != torch.int32 or not a.is_contiguous() or a.dim() < 1 or tuple(a.shape) != tuple(r_sym.shape) or not a.is_cuda:
            raise ValueError("device coder: the ranked symbols and indexes are contiguous int32 device buffers of one shape")
    n = int(r_sym.shape[-1])
    ns = int(np.prod(r_sym.shape[:-1]))
    n_marks = 0 if count is None else int(count.shape[0])
    if count is not None and (count.dtype != torch.int32 or not count.is_contiguous() or count.numel() != n_marks * ns):
        raise ValueError(f"device coder: count is a contiguous int32 [L, {ns}] buffer")
    cap = 2 * n + 2 * K + 16
    dev = r_sym.device
    regions = torch.empty(ns * cap, dtype=torch.int32, device=dev)
    packed = torch.empty(ns * cap, dtype=torch.int32, device=dev)
    meta = torch.empty((2 + n_marks, ns), dtype=torch.int32, device=dev)          # lengths in words, status, the marks' bytes
    offs = torch.empty(ns + 1, dtype=torch.int64, device=dev)
    lib, st = L.load(), ops.stream_ptr()
    L.check(lib.vam_rans_interleaved_encode_device(r_sym.data_ptr(), r_idx.data_ptr(), ns, n, K, C.byref(tables.struct),
                                                   regions.data_ptr(), cap, meta[0].data_ptr(), meta[1].data_ptr(),
                                                   count.data_ptr() if n_marks else None, n_marks,
                                                   meta[2].data_ptr() if n_marks else None, st), "vam_rans_interleaved_encode_device")
    L.check(lib.vam_rans_pack_device(regions.data_ptr(), cap, meta[0].data_ptr(), ns, packed.data_ptr(), ns * cap,
                                     offs.data_ptr(), st), "vam_rans_pack_device")
    m = meta.cpu().numpy()
    bad = np.flatnonzero(m[1])
    if bad.size:
        raise L.VamError(f"vam_rans_interleaved_encode_device: embedded stream {int(bad[0])}: {status_text(int(m[1][bad[0]]))}"
                         + (f" ({bad.size} streams failed)" if bad.size > 1 else ""))
    off = np.concatenate([[0], np.cumsum(m[0].astype(np.int64))]) * 4
    data = packed[:int(off[-1]) // 4].cpu().numpy().view(np.uint8)
    return [data[off[k]:off[k + 1]].tobytes() for k in range(ns)], m[2:].astype(np.int64)


def cut_table_launch(r_sym: torch.Tensor, r_idx: torch.Tensor, tables: DeviceCoderTables, lanes: int, cut: torch.Tensor,
                     status: torch.Tensor):
    """ONE vam_rans_interleaved_cut_table_device launch on the current stream, no synchronisation and no allocation: the
    cut tables of the streams of ``r_sym`` / ``r_idx`` (as :func:`encode_embedded_device` takes them) into ``cut``
    (contiguous int32 [n_streams, n + 1] on the device) and their status codes into ``status`` (int32 [n_streams])."""
    from . import ops
    K = check_lanes(lanes)
    for a in (r_sym, r_idx):
        if a.dtype != torch.int32 or not a.is_contiguous() or a.dim() < 1 or tuple(a.shape) != tuple(r_sym.shape) or not a.is_cuda:
            raise ValueError("device coder: the ranked symbols and indexes are contiguous int32 device buffers of one shape")
    n = int(r_sym.shape[-1])
    ns = int(np.prod(r_sym.shape[:-1]))
    if cut.dtype != torch.int32 or not cut.is_contiguous() or cut.numel() != ns * (n + 1) or cut.device != r_sym.device:
        raise ValueError(f"device coder: cut is a contiguous int32 [{ns}, {n + 1}] device buffer")
    if status.dtype != torch.int32 or not status.is_contiguous() or status.numel() != ns or status.device != r_sym.device:
        raise ValueError(f"device coder: status is a contiguous int32 [{ns}] device buffer")
    L.check(L.load().vam_rans_interleaved_cut_table_device(r_sym.data_ptr(), r_idx.data_ptr(), ns, n, K, C.byref(tables.struct),
                                                           cut.data_ptr(), status.data_ptr(), ops.stream_ptr()),
            "vam_rans_interleaved_cut_table_device")


def cut_table_device(r_sym: torch.Tensor, r_idx: torch.Tensor, tables: DeviceCoderTables, lanes: int = 1) -> torch.Tensor:
    """The cut tables of the streams of the flat ranked buffers ``r_sym`` / ``r_idx`` (contiguous int32 [..., n] on the
    device, every leading index one stream): int32 [n_streams, n + 1] ON THE DEVICE, entry (s, c) =
    :func:`prefix_bytes` of count c on the string :func:`encode_embedded_device` writes for stream s, from one dry walk of
    the encoder (:func:`cut_table_launch`) and one read of the status codes.  A stream the encode launch would refuse is
    raised as that wrapper raises it."""
    n = int(r_sym.shape[-1]) if r_sym.dim() else 0
    ns = int(np.prod(r_sym.shape[:-1])) if r_sym.dim() else 0
    cut = torch.empty((ns, n + 1), dtype=torch.int32, device=r_sym.device)
    status = torch.empty(ns, dtype=torch.int32, device=r_sym.device)
    cut_table_launch(r_sym, r_idx, tables, lanes, cut, status)
    raise_cut_status(status)
    return cut


def raise_cut_status(status: torch.Tensor):
    """Reads the status codes of :func:`cut_table_launch` (synchronises) and raises VamError naming the first failed stream."""
    m = status.cpu().numpy().reshape(-1)
    bad = np.flatnonzero(m)
    if bad.size:
        raise L.VamError(f"vam_rans_interleaved_cut_table_device: embedded stream {int(bad[0])}: {status_text(int(m[bad[0]]))}"
                         + (f" ({bad.size} streams failed)" if bad.size > 1 else ""))


def decode_embedded_uploaded(up: DeviceStreams, first: int, r_idx: torch.Tensor, ranked: torch.Tensor, tables: DeviceCoderTables,
                             lanes: int, meta: torch.Tensor):
    """One vam_rans_interleaved_decode_device launch on the current stream, no synchronisation: the strings of ``up`` from
    ``first`` on, one per stream of the flat buffers ``r_idx`` / ``ranked`` (contiguous int32 [..., n]), each the first bytes
    of an :func:`encode_interleaved` string of ``lanes`` = K, decoded tolerantly.  ``ranked`` receives the decoded elements
    and 0 beyond them; ``meta`` (int32 [2, n_streams] on the device) the available counts and the status codes."""
    from . import ops
    K = check_lanes(lanes)
    for a in (r_idx, ranked):
        if a.dtype != torch.int32 or not a.is_contiguous() or tuple(a.shape) != tuple(r_idx.shape):
            raise ValueError("device coder: the ranked symbols and indexes are contiguous int32 device buffers of one shape")
    n = int(r_idx.shape[-1])
    ns = int(np.prod(r_idx.shape[:-1]))
    if first < 0 or first + ns > up.n:
        raise ValueError(f"device coder: strings {first} .. {first + ns} of {up.n} uploaded")
    if meta.dtype != torch.int32 or tuple(meta.shape) != (2, ns) or not meta.is_contiguous():
        raise ValueError(f"device coder: meta is a contiguous int32 [2, {ns}] buffer")
    total = up.buf.numel() - (up.bytes_ptr - up.buf.data_ptr())
    L.check(L.load().vam_rans_interleaved_decode_device(up.bytes_ptr, total, up.offsets_ptr + 8 * first, up.lengths_ptr + 4 * first,
                                                        r_idx.data_ptr(), ns, n, K, C.byref(tables.struct), ranked.data_ptr(),
                                                        meta[0].data_ptr(), meta[1].data_ptr(), ops.stream_ptr()),
            "vam_rans_interleaved_decode_device")


def resume_embedded_uploaded(up: DeviceStreams, first: int, r_idx: torch.Tensor, ranked: torch.Tensor, tables: DeviceCoderTables,
                             lanes: int, checkpoints: Checkpoints, meta: torch.Tensor):
    """:func:`decode_embedded_uploaded` continued from ``checkpoints`` (device tensors, updated by the kernel): ONE
    vam_rans_interleaved_resume_device launch on the current stream, no synchronisation.  String k of ``up`` (from ``first``
    on) holds stream k FROM BYTE 4 * pos[k] ON.  ``ranked`` receives the elements done_in <= i < available of every stream and
    keeps what it holds elsewhere; ``meta`` (int32 [3, n_streams] on the device) the available counts, the status codes and
    the new ``pos``, which is all the host needs to cut the next upload."""
    from . import ops
    K = check_lanes(lanes)
    for a in (r_idx, ranked):
        if a.dtype != torch.int32 or not a.is_contiguous() or tuple(a.shape) != tuple(r_idx.shape):
            raise ValueError("device coder: the ranked symbols and indexes are contiguous int32 device buffers of one shape")
    n = int(r_idx.shape[-1])
    ns = int(np.prod(r_idx.shape[:-1]))
    if first < 0 or first + ns > up.n:
        raise ValueError(f"device coder: strings {first} .. {first + ns} of {up.n} uploaded")
    if meta.dtype != torch.int32 or tuple(meta.shape) != (3, ns) or not meta.is_contiguous():
        raise ValueError(f"device coder: meta is a contiguous int32 [3, {ns}] buffer")
    ck = checkpoints
    if not (torch.is_tensor(ck.states) and ck.states.dtype == torch.int64 and tuple(ck.states.shape) == (ns, K)
            and ck.states.is_contiguous() and all(torch.is_tensor(a) and a.dtype == torch.int32 and tuple(a.shape) == (ns,)
                                                  and a.is_contiguous() for a in (ck.done, ck.pos))):
        raise ValueError(f"device coder: device checkpoints of {ns} streams on {K} lanes (Checkpoints.fresh)")
    total = up.buf.numel() - (up.bytes_ptr - up.buf.data_ptr())
    L.check(L.load().vam_rans_interleaved_resume_device(up.bytes_ptr, total, up.offsets_ptr + 8 * first, up.lengths_ptr + 4 * first,
                                                        r_idx.data_ptr(), ns, n, K, C.byref(tables.struct), ranked.data_ptr(),
                                                        ck.states.data_ptr(), ck.done.data_ptr(), ck.pos.data_ptr(),
                                                        meta[0].data_ptr(), meta[1].data_ptr(), ops.stream_ptr()),
            "vam_rans_interleaved_resume_device")
    if ck.pos.data_ptr() != meta[2].data_ptr():               # a decoder keeps pos in meta itself
        meta[2].copy_(ck.pos)


# ---------------------------------------------------------------- an interleaved base
def encode_window_interleaved_device(sym_view, idx_view, n_slices: int, C_: int, tables: DeviceCoderTables, lanes: int) -> List[List[bytes]]:
    """:func:`encode_streams_device` with every string an :func:`encode_interleaved` string of ``lanes`` = K: all
    B * n_slices streams of an int32 NHWC window in ONE vam_rans_interleaved_encode_nhwc_device launch on the current stream,
    one thread per (stream, lane), packed by vam_rans_pack_device; then the two device-to-host copies.  ``idx_view`` None:
    table index = channel (the z streams).  Returns ``[slice][image]``; at K = 1 the bytes are encode_streams_device's."""
    from . import ops
    K = check_lanes(lanes)
    B, h, w, ld = _geometry(sym_view, idx_view, n_slices, C_, None)
    ns, cap = B * n_slices, 2 * C_ * h * w + 2 * K + 16
    dev = sym_view.buf.device
    regions = torch.empty(ns * cap, dtype=torch.int32, device=dev)
    packed = torch.empty(ns * cap, dtype=torch.int32, device=dev)
    meta = torch.empty((2, ns), dtype=torch.int32, device=dev)          # lengths in words, status
    offs = torch.empty(ns + 1, dtype=torch.int64, device=dev)
    lib, st = L.load(), ops.stream_ptr()
    L.check(lib.vam_rans_interleaved_encode_nhwc_device(sym_view.buf.data_ptr(), idx_view.buf.data_ptr() if idx_view is not None else None,
                                                        B, h, w, ld, sym_view.c0, C_, n_slices, K, C.byref(tables.struct),
                                                        regions.data_ptr(), cap, meta[0].data_ptr(), meta[1].data_ptr(), st),
            "vam_rans_interleaved_encode_nhwc_device")
    L.check(lib.vam_rans_pack_device(regions.data_ptr(), cap, meta[0].data_ptr(), ns, packed.data_ptr(), ns * cap,
                                     offs.data_ptr(), st), "vam_rans_pack_device")
    m = meta.cpu().numpy()
    raise_status(m[1], B, "vam_rans_interleaved_encode_nhwc_device")
    off = np.concatenate([[0], np.cumsum(m[0].astype(np.int64))]) * 4
    data = packed[:int(off[-1]) // 4].cpu().numpy().view(np.uint8)
    return [[data[off[s * B + b]:off[s * B + b + 1]].tobytes() for b in range(B)] for s in range(n_slices)]


def decode_window_interleaved_uploaded(up: DeviceStreams, first: int, idx_view, sym_view, n_slices: int, C_: int,
                                       tables: DeviceCoderTables, lanes: int):
    """:func:`decode_uploaded` for :func:`encode_interleaved` strings of ``lanes`` = K: one
    vam_rans_interleaved_decode_nhwc_device launch on the current stream, no synchronisation.  The decode is STRICT: a string
    that ends before its stream does gets status 1.  ``up`` is an upload for one lane: one status code per string."""
    from . import ops
    K = check_lanes(lanes)
    B, h, w, ld = _geometry(sym_view, idx_view, n_slices, C_, None)
    if first < 0 or first + B * n_slices > up.n:
        raise ValueError(f"device coder: strings {first} .. {first + B * n_slices} of {up.n} uploaded")
    if up.lanes != 1:
        raise ValueError(f"device coder: interleaved strings have one status code each, these were uploaded for {up.lanes} lanes")
    total = up.buf.numel() - (up.bytes_ptr - up.buf.data_ptr())
    L.check(L.load().vam_rans_interleaved_decode_nhwc_device(up.bytes_ptr, total, up.offsets_ptr + 8 * first, up.lengths_ptr + 4 * first,
                                                             idx_view.buf.data_ptr() if idx_view is not None else None, B, h, w, ld,
                                                             sym_view.c0, C_, n_slices, K, C.byref(tables.struct),
                                                             sym_view.buf.data_ptr(), up.status.data_ptr() + 4 * first,
                                                             ops.stream_ptr()), "vam_rans_interleaved_decode_nhwc_device")


def sigma0_index(scale_table) -> int:
    """The table index build_indexes gives sigma = 0 (the 0.11 bound applies), in float32 as the kernel compares."""
    tb = np.asarray(torch.as_tensor(scale_table).detach().cpu().numpy(), dtype=np.float32)
    return int(tb.size - 1 - np.count_nonzero(np.float32(0.11) <= tb[:-1]))
