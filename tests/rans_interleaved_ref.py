"""A plain-Python restatement of the interleaved-lanes wire format, written from its description and
not from csrc/rans_core.h: a stream of n elements on K lanes (element i: lane i % K, group i // K), the K final states in
front, then the renormalisation words in the decoder's order.  Slow and obvious on purpose; the tests hold the library
to it byte for byte."""
import numpy as np

PRECISION, NIB, RANS_L = 16, 4, 1 << 31
MASK64 = (1 << 64) - 1


def _puts(symbol, ci, t):
    """The gets of one element in decoder order: ("sym", start, freq) then ("bits", value) per nibble."""
    cdf, mx, off = t.cdf[ci], int(t.sizes[ci]) - 2, int(t.offsets[ci])
    v = int(symbol) - off
    raw = None
    if v < 0:
        raw, v = -2 * v - 1, mx
    elif v >= mx:
        raw, v = 2 * (v - mx), mx
    out = [("sym", int(cdf[v]), int(cdf[v + 1]) - int(cdf[v]))]
    if raw is not None:
        nb = 0
        while nb < 8 and (raw >> (4 * nb)) != 0:
            nb += 1
        out += [("bits", 15)] * (nb // 15) + [("bits", nb % 15)]
        out += [("bits", (raw >> (4 * j)) & 15) for j in range(nb)]
    return out


def encode(symbols, indexes, t, K):
    """The exact mirror of the decoder: groups, rounds and lanes descending; a put flushes first when its bound says so."""
    sym, idx = np.asarray(symbols).reshape(-1), np.asarray(indexes).reshape(-1)
    n = sym.size
    x = [RANS_L] * K
    rev = []                                       # words in reverse decoder order
    for g in range(-(-n // K) - 1, -1, -1):
        lanes = range(min(K, n - g * K))
        puts = [_puts(sym[g * K + l], int(idx[g * K + l]), t) for l in lanes]
        for r in range(max(len(p) for p in puts) - 1, -1, -1):
            for l in reversed(lanes):
                if r >= len(puts[l]):
                    continue
                p = puts[l][r]
                freq = p[2] if p[0] == "sym" else 1 << (PRECISION - NIB)
                if x[l] >= ((RANS_L >> PRECISION) << 32) * freq:
                    rev.append(x[l] & 0xFFFFFFFF)
                    x[l] >>= 32
                if p[0] == "sym":
                    x[l] = ((x[l] // freq) << PRECISION) + x[l] % freq + p[1]
                else:
                    x[l] = (x[l] << NIB) | p[1]
    words = []
    for l in range(K):
        words += [x[l] & 0xFFFFFFFF, x[l] >> 32]
    return np.array(words + rev[::-1], dtype="<u4").tobytes()


def decode_prefix(prefix, indexes, t, K):
    """(available, symbols[:available], reach): the tolerant decode of a byte prefix.  reach[i] = the read position (in
    words) after the last word element i reads, 0 when it reads none; it covers the elements below ``available``."""
    idx = np.asarray(indexes).reshape(-1)
    n = idx.size
    W = len(prefix) // 4
    words = np.frombuffer(prefix[:4 * W], dtype="<u4")
    if W < 2 * K:
        return 0, [], []
    x = [int(words[2 * l]) | (int(words[2 * l + 1]) << 32) for l in range(K)]
    pos, out, reach = 2 * K, [], []
    for g in range(-(-n // K)):
        m = min(K, n - g * K)
        # per lane: the state machine of one element
        phase, nb, raw, j, val, failed, last = ["sym"] * m, [0] * m, [0] * m, [0] * m, [0] * m, [False] * m, [0] * m
        done = [False] * m
        while not all(d or f for d, f in zip(done, failed)):
            need = []
            for l in range(m):
                if done[l] or failed[l]:
                    continue
                ci = int(idx[g * K + l])
                cdf, sz = t.cdf[ci], int(t.sizes[ci])
                if phase[l] == "sym":
                    cum = x[l] & 0xFFFF
                    s = 0
                    while s + 1 < sz and int(cdf[s + 1]) <= cum:
                        s += 1
                    start, freq = int(cdf[s]), int(cdf[s + 1]) - int(cdf[s])
                    x[l] = freq * (x[l] >> 16) + cum - start
                    val[l] = s
                    if s == sz - 2:
                        phase[l] = "count"
                    else:
                        done[l] = True
                else:
                    nib = x[l] & 15
                    x[l] >>= 4
                    if phase[l] == "count":
                        nb[l] += nib
                        if nib != 15:
                            phase[l] = "raw"
                            done[l] = nb[l] == 0
                    else:
                        if j[l] < 8:
                            raw[l] |= nib << (4 * j[l])
                        j[l] += 1
                        done[l] = j[l] == nb[l]
                    if done[l]:
                        val[l] = -(raw[l] >> 1) - 1 if raw[l] & 1 else (raw[l] >> 1) + sz - 2
                if x[l] < RANS_L:
                    need.append(l)
            for l in need:                         # ascending lane order
                if pos < W:
                    x[l] = ((x[l] << 32) | int(words[pos])) & MASK64
                    pos += 1
                    last[l] = pos
                else:
                    failed[l] = True
        first = failed.index(True) if any(failed) else m
        for l in range(first):
            out.append(val[l] + int(t.offsets[int(idx[g * K + l])]))
            reach.append(last[l])
        if first < m:
            break
    return len(out), out, reach


def prefix_bytes(stream, indexes, t, K, count):
    if count == 0:
        return 0
    got, _, reach = decode_prefix(stream, indexes, t, K)
    assert got >= count
    return 4 * max([2 * K] + reach[:count])
