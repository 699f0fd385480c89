"""The streams the cut-table tests share: synthetic tables and three kinds of content, for the host
table (tests/test_cut_table_cpu.py) and the kernel (tests/test_gpu_cut_table.py)."""
import numpy as np
import torch

from vampic import bitstream as bs

LANES = [1, 8, 64]
LENGTHS = [1, 63, 64, 65, 512, 1000]
CONTENTS = ["mixed", "zeros", "bypass"]
PEAKED = 5                  # the index of the peaked table


def tables(zero_freq: bool = False) -> bs.Tables:
    """Five Gaussian-like tables of widths 1 .. 40 and, as table PEAKED, one whose centre holds all but a sliver of the mass:
    its symbol 0 costs about 0.001 bits, so hundreds of elements pass without a renormalisation word.  Every table ends in an
    escape entry.  ``zero_freq``: table 0's first entry is given frequency 0 (a table that is not normalised)."""
    cdfs, offs = [], []
    for w in (1, 3, 8, 20, 40):
        k = np.arange(-w, w + 1)
        pmf = np.exp(-0.5 * (k / (0.3 * w + 0.2)) ** 2).astype(np.float32)
        pmf /= pmf.sum()
        cdfs.append(bs.pmf_to_quantized_cdf(torch.from_numpy(np.concatenate([pmf, [np.float32(1e-4)]]).astype(np.float32)), 16).numpy())
        offs.append(-w)
    cdfs.append(np.array([0, 8, 65520, 65528, 65536], dtype=np.int32))       # values -1, 0, 1 and the escape
    offs.append(-1)
    if zero_freq:
        cdfs[0] = cdfs[0].copy()
        cdfs[0][1] = 0
    tab = np.zeros((len(cdfs), max(len(c) for c in cdfs)), dtype=np.int32)
    for i, c in enumerate(cdfs):
        tab[i, :len(c)] = c
    return bs.Tables(tab, np.array([len(c) for c in cdfs], dtype=np.int32), np.array(offs, dtype=np.int32))


def content(t: bs.Tables, kind: str, n: int, seed: int):
    """(symbols, indexes) int32 [n].  "mixed": every table, in-range values.  "zeros": symbol 0 on the peaked table
    throughout.  "bypass": mixed, with a quarter of the elements outside their table on either side, by up to 2^20: escapes
    of one to six raw nibbles."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, dtype=np.int32), np.full(n, PEAKED, dtype=np.int32)
    idx = rng.integers(0, t.cdf.shape[0], n).astype(np.int32)
    mx = t.sizes[idx].astype(np.int64) - 2
    sym = rng.integers(0, 1 << 30, n) % np.maximum(mx, 1) + t.offsets[idx]
    if kind == "bypass":
        out = rng.random(n) < 0.25
        far = (1 << rng.integers(0, 21, n)) + rng.integers(0, 16, n)
        sym = np.where(out, np.where(rng.random(n) < 0.5, t.offsets[idx] - far, t.offsets[idx] + mx + far), sym)
    else:
        assert kind == "mixed", kind
    return sym.astype(np.int32), idx
