"""The cut table of an embedded string on the host, and the budget solver of tiled pictures:
``bitstream.cut_table`` gives, for EVERY element count, the bytes ``prefix_bytes`` gives for that count, and each entry is the
smallest whole-word prefix that decodes that many symbols; ``tiled.solve_budgets`` places rounds at byte budgets on any
non-decreasing size curve.  No GPU, no model."""
import numpy as np
import pytest

from vampic import bitstream as bs, tiled
from cut_table_cases import CONTENTS, LANES, LENGTHS, content, tables


@pytest.fixture(scope="module")
def t():
    return tables()


def _decoded(prefix, idx, t, K):
    return bs.decode_prefix_streams([(prefix, idx, np.zeros(idx.size, dtype=np.int32))], t, lanes=K)[0]


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("n", LENGTHS)
def test_host_table_is_prefix_bytes_of_every_count(t, n, K, kind):
    sym, idx = content(t, kind, n, seed=n + K)
    string = bs.encode_interleaved(sym, idx, t, K)
    cut = bs.cut_table(string, idx, t, K)
    assert cut.dtype == np.int32 and cut.shape == (n + 1,)
    assert cut.tolist() == [bs.prefix_bytes(string, idx, [c], t, lanes=K)[0] for c in range(n + 1)]      # count by count
    assert cut[0] == 0 and (np.diff(cut) >= 0).all() and 8 * K <= cut[1] and cut[n] <= len(string) and not (cut % 4).any()
    for c in range(0, n + 1, 7):                              # the smallest multiple of 4 that decodes at least c symbols
        b = int(cut[c])
        assert _decoded(string[:b], idx, t, K) >= c, c
        assert b == 0 or _decoded(string[:b - 4], idx, t, K) < c, c
    if kind == "zeros" and n >= 63:                           # the peaked table: long runs that read no word at all
        assert cut[min(n, 8 * K)] == 8 * K and (cut == 8 * K).sum() >= 63
    if kind == "bypass" and n >= 63:
        mx = t.sizes[idx].astype(np.int64) - 2
        v = sym.astype(np.int64) - t.offsets[idx]
        assert 0.1 < ((v < 0) | (v >= mx)).mean() < 0.4       # about a quarter of the elements take the bypass


# ------------------------------------------------------------------------------------------------ the solver
HEADS = 1000


def _steps(seed=0, n=200):
    """A fabricated size curve: n steps at random qualities in (0, 10), each of 4 .. 4000 bytes, on top of HEADS."""
    rng = np.random.default_rng(seed)
    at, w = np.sort(rng.uniform(0, 10, n)), rng.integers(1, 1000, n) * 4
    asked = []

    def sizes(rows):
        asked.append([len(r) for r in rows])
        assert all(0 < len(r) <= 32 and all(0 < q <= 10 for q in r) and list(r) == sorted(r) for r in rows)
        return [[HEADS + int(w[at <= q].sum()) for q in r] for r in rows]
    return sizes, asked, HEADS + int(w.sum())


@pytest.mark.parametrize("q_tol", [1e-3, 0.05])
def test_solver_meets_every_budget_and_is_maximal_at_q_tol(q_tol):
    sizes, asked, total = _steps()
    budgets = [5000, 100000, 300000]
    qs = tiled.solve_budgets(sizes, HEADS, budgets, q_tol)
    passes = len(asked)
    from vampic.control import rate_search_passes
    assert passes == rate_search_passes(q_tol) and all(len(a) == 3 for a in asked)        # every pass asks every open budget once
    assert qs == sorted(qs) and len(set(qs)) == 3
    for q, N in zip(qs, budgets):
        assert 0 < q < 10
        assert sizes([[q]])[0][0] <= N < sizes([[min(q + q_tol, 10.0)]])[0][0]
    assert tiled.solve_budgets(sizes, HEADS, [100000], q_tol) == [qs[1]]                  # every budget is solved on its own


def test_solver_gives_ten_to_a_budget_that_holds_everything():
    sizes, _, total = _steps()
    assert tiled.solve_budgets(sizes, HEADS, [total]) == [10.0]
    assert tiled.solve_budgets(sizes, HEADS, [total + 12345]) == [10.0]
    q = tiled.solve_budgets(sizes, HEADS, [total - 1])[0]
    assert q < 10 and sizes([[q]])[0][0] < total


def test_solver_refuses_by_message():
    sizes, _, total = _steps()
    with pytest.raises(ValueError, match=r"budget 2, 7000 bytes, does not exceed budget 1, 7000 bytes: budgets are strictly increasing"):
        tiled.solve_budgets(sizes, HEADS, [5000, 7000, 7000])
    with pytest.raises(ValueError, match=r"budget 1, 4000 bytes, does not exceed budget 0, 5000"):
        tiled.solve_budgets(sizes, HEADS, [5000, 4000])
    with pytest.raises(ValueError, match=rf"budget 0, {HEADS - 1} bytes, is below heads_end = {HEADS} bytes"):
        tiled.solve_budgets(sizes, HEADS, [HEADS - 1, 5000])
    # a curve whose smallest quality already costs more than the heads: the budget holds the heads, but no round
    floor = lambda rows: [[HEADS + 640 + int(100 * q) for q in r] for r in rows]
    with pytest.raises(ValueError, match=rf"budget 0, {HEADS + 600} bytes, holds the heads \({HEADS} bytes\) but no round: the smallest "
                                         rf"quality tried, [0-9.e-]+, needs {HEADS + 640} bytes"):
        tiled.solve_budgets(floor, HEADS, [HEADS + 600, 5000])
    with pytest.raises(ValueError, match=rf"budgets 0 and 1, {total} and {total + 1} bytes, solve to the same quality 10"):
        tiled.solve_budgets(sizes, HEADS, [total, total + 1])
    flat = lambda rows: [[HEADS + (0 if q < 5 else 4000) for q in r] for r in rows]       # one step: two budgets below it coincide
    with pytest.raises(ValueError, match=r"budgets 0 and 1, 2000 and 3000 bytes, solve to the same quality"):
        tiled.solve_budgets(flat, HEADS, [2000, 3000, 9000])
    for bad, text in (([], "1 .. 32 budgets, got 0"), (list(range(2000, 2033)), "1 .. 32 budgets, got 33")):
        with pytest.raises(ValueError, match=text):
            tiled.solve_budgets(sizes, HEADS, bad)
    with pytest.raises(ValueError, match="q_tol must be > 0"):
        tiled.solve_budgets(sizes, HEADS, [5000], q_tol=0)
    assert len(tiled.solve_budgets(sizes, HEADS, [5000, 100000, 300000])) == 3            # and a correct call
