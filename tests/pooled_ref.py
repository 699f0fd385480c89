"""Picture-wide quality marks restated with NumPy and ``torch.quantile``: keys, pool, thresholds, counts.

One rule.  A picture has T tiles; slice j of tile t is a segment of n sigmas.  The pool of slice j is the multiset of the
T * n sigmas of slice j of all tiles.  For a mark quality q the picture's threshold is
``torch.quantile(pool_j, float32(1 - 0.1 q))`` (linear interpolation; -inf for q >= 10; NaN when the pool holds a NaN), and
tile t keeps ``#{sigma >= thr}`` of its slice j (every element for q >= 10).  The pool is canonicalised as the rank order
canonicalises (-0.0 == +0.0), so the threshold does not depend on which zero a sort happens to put first.
"""
import numpy as np
import torch


def keys(s: np.ndarray) -> np.ndarray:
    """uint32 keys of fp32 ``s`` that ascend as s descends: -0.0 == +0.0, every NaN the key 0xFFFFFFFF (csrc/quantile.h)."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    u = s.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    asc = np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), ~asc).astype(np.uint32)


def rank_order(s: np.ndarray) -> np.ndarray:
    """The rank order of one flat segment: ``argsort(-s, kind="stable")`` with -0.0 == +0.0 and NaNs last (ties by index)."""
    return np.argsort(keys(s), kind="stable")


def ranked_keys(sig: np.ndarray) -> np.ndarray:
    """uint32 [T, ns, n]: every segment of ``sig`` fp32 [T, ns, n] in rank order, as keys (each row ascends)."""
    return np.sort(keys(sig), axis=-1)


def thresholds(sig: np.ndarray, qs) -> np.ndarray:
    """fp32 [len(qs), ns] from ``sig`` fp32 [T, ns, n]."""
    sig = np.ascontiguousarray(sig, dtype=np.float32)
    T, ns, n = sig.shape
    out = np.empty((len(qs), ns), dtype=np.float32)
    for k, q in enumerate(qs):
        for j in range(ns):
            if q >= 10:
                out[k, j] = -np.inf
                continue
            pool = torch.from_numpy(sig[:, j].reshape(-1).copy()) + 0.0           # -0.0 + 0.0 == +0.0
            out[k, j] = torch.quantile(pool, torch.tensor(1.0 - 0.1 * float(q), dtype=torch.float32)).item()
    return out


def counts(sig: np.ndarray, thr: np.ndarray) -> np.ndarray:
    """int32 [L, T, ns]: the elements of every segment with sigma >= thr[k, j]; the whole segment where thr is -inf."""
    sig = np.ascontiguousarray(sig, dtype=np.float32)
    T, ns, n = sig.shape
    with np.errstate(invalid="ignore"):
        c = (sig[None] >= thr[:, None, :, None]).sum(-1)
    return np.where(np.isneginf(thr)[:, None, :], n, c).astype(np.int32)
