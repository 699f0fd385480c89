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


def coder_threads(requested: Optional[int] = None) -> int:
    """Host threads for the stream coder: at most L.VAM_RANS_MAX_THREADS and the CPUs this process may run on."""
    n = min(L.VAM_RANS_MAX_THREADS, len(os.sched_getaffinity(0)))
    return max(1, n if requested is None else min(int(requested), n))


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _layer(a) -> Optional[np.ndarray]:
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def encode_streams(jobs: Sequence[Tuple], t: Tables, threads: Optional[int] = None) -> List[bytes]:
    """Many independent streams in one vam_rans_encode_streams call.  ``jobs``: (symbols, indexes) or (symbols, indexes,
    layer, sel) per stream; with a layer array only the elements with layer == sel are coded (the others as 0 / table 0).
    Each stream's bytes equal :func:`encode`'s on the same (masked) inputs.  ``threads`` is passed on as given (the library
    clamps it to L.VAM_RANS_MAX_THREADS); None = :func:`coder_threads`."""
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


def decode_streams(jobs: Sequence[Tuple], t: Tables, threads: Optional[int] = None) -> None:
    """Decode many streams in one vam_rans_decode_streams call.  ``jobs``: (stream bytes, indexes, out) or (stream bytes,
    indexes, out, layer, sel); ``out`` is a writable C-contiguous int32 array of the indexes' size.  With a layer array only
    out[layer == sel] is written, so the layers of a container can fill one array."""
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
