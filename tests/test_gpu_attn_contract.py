"""``vam_win_attention`` / ``vam_win_attention_bwd`` against the float64 statement of their contract (tests/attn_contract.py):
every kernel the two dispatchers name, on the matrix pipe and on the FMA path, at the smallest shapes where the roll, the
region mask, the table index or the head grouping can still go wrong; what a launch owns and what it must leave alone;
determinism, locality and the refusals.  This file is what a rewrite of the attention kernels has to keep."""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import vampic.synth                 # noqa: E402
from vampic import ops, _lib as L   # noqa: E402
import attn_contract as AC          # noqa: E402

MODE = {"mfma": 1, "fma": 0}


def _paths(case):
    """8 x 8 windows of 24-wide heads have a matrix-pipe kernel and an FMA kernel; everything else is FMA only."""
    return ("mfma", "fma") if (case.ws, case.hd) == (8, 24) else ("fma",)


RUNS = [(cid, path) for cid, case in AC.CASES.items() for path in _paths(case)]
BWD_RUNS = [(cid, path) for cid, path in RUNS if AC.CASES[cid].backward]


@contextlib.contextmanager
def _path(path):
    lib = L.load()
    lib.vam_attn_set_mfma(MODE[path])
    try:
        yield
    finally:
        lib.vam_attn_set_mfma(-1)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _ref(cid):
    case = AC.CASES[cid]
    t = AC.tensors(case)
    ref = AC.reference(case, t)
    return case, t, ref, AC.bounds(case, ref)


def _run(built, path, dtable_fill=AC.SENTINEL):
    case = built.case
    r = SimpleNamespace(dqkv=None, dtable=None, s_dq=0, s_dt=0, s_ws=0)
    with _path(path):
        r.out, r.s_out = built.forward()
        if case.backward:
            r.dqkv, r.dtable, r.s_dq, r.s_dt, r.s_ws = built.backward(dtable_fill)
    return r


@functools.lru_cache(maxsize=None)
def _launch(cid, path):
    """One forward and one backward launch of a case on a path, shared by the tests."""
    case, t, _, _ = _ref(cid)
    built = AC.build(case, "cuda", t)
    return built, _run(built, path)


@pytest.mark.parametrize("cid,path", RUNS)
def test_contract_against_float64(cid, path):
    """out, dq, dk, dv and dtable within the elementwise bounds of attn_contract.bounds, which an fp32 ATen evaluation of
    the same formulas meets with a factor 13 or more to spare (tests/test_attn_contract_cpu.py) and which a roll, index,
    region, mask, scale or table-layout mistake misses by a factor 1e4 or more.  The largest error / bound of each quantity
    is printed and handed to conftest.record_measurement."""
    from conftest import record_measurement
    case, _, ref, bnd = _ref(cid)
    _, r = _launch(cid, path)
    got = AC.split(case, r.out, r.dqkv, r.dtable)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{cid} {path}: {k} is not finite: something outside an input window, or a workspace row never written, was read"
    measured = AC.ratios(case, ref, got, bnd)
    print(f"{cid} {path}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in measured.items()))
    record_measurement(f"attention contract {cid} ({path})", **{k: f"{v:.3g}" for k, v in measured.items()})
    assert set(measured) == (set(AC.QUANTITIES) if case.backward else {"out"})
    AC.check(case, ref, got, path, bnd)


@pytest.mark.parametrize("cid,path", RUNS)
def test_launch_writes_only_what_it_owns(cid, path):
    """After the launches every element outside the written windows still holds the sentinel's bits: the 4 + 4 guard
    channels beside out and dqkv, their spare image, the rows around dtable, the workspace beyond
    vam_win_attention_bwd_workspace bytes.  Every owned element was written (none holds the sentinel) and is finite
    although everything around the input windows, and the workspace, was NaN."""
    case = AC.CASES[cid]
    _, r = _launch(cid, path)
    assert r.s_out == 0, f"{cid} {path}: {r.s_out} elements outside out's window were written"
    assert r.s_dq == 0, f"{cid} {path}: {r.s_dq} elements outside dqkv's window were written"
    assert r.s_dt == 0, f"{cid} {path}: {r.s_dt} elements in the rows around dtable were written"
    assert r.s_ws == 0, f"{cid} {path}: {r.s_ws} elements beyond the workspace size were written"
    for k, v in AC.split(case, r.out, r.dqkv, r.dtable).items():
        assert bool(torch.isfinite(v).all()), (cid, path, k)
        assert not bool((v == AC.SENTINEL).any()), f"{cid} {path}: part of {k} was not written"


@pytest.mark.parametrize("cid,path", RUNS)
def test_second_launch_gives_the_same_bits(cid, path):
    """Deterministic, and dtable is written, not accumulated: a second launch into fresh buffers (other addresses, dtable
    pre-filled with zeros instead of the sentinel) gives the bits of the first for out, dqkv and dtable."""
    case = AC.CASES[cid]
    built, first = _launch(cid, path)
    again = _run(built, path, dtable_fill=0.0)
    for (k, a), b in zip(AC.split(case, first.out, first.dqkv, first.dtable).items(), AC.split(case, again.out, again.dqkv, again.dtable).values()):
        assert torch.equal(_bits(a), _bits(b)), f"{cid} {path}: {(_bits(a) != _bits(b)).sum().item()} elements of {k} differ between two launches"


def _changed(case, t, b, window, head):
    """The inputs with q, k, v and dO of one (image, window, head) redrawn, and the maps of what may then change."""
    C, hd = case.C, case.hd
    pix = AC.window_pixels(case, window)
    y, x = pix[:, 0], pix[:, 1]
    t2 = {k: v.clone() for k, v in t.items()}
    may_out = torch.zeros((case.B, case.H, case.W, C), dtype=torch.bool)
    may_dq = torch.zeros((case.B, case.H, case.W, 3 * C), dtype=torch.bool)
    for part in range(3):
        c0 = part * C + head * hd
        t2["qkv"][b, y, x, c0:c0 + hd] = vampic.synth.normal((case.N, hd), 900 + part) * (case.qk if part < 2 else 1.0)
        may_dq[b, y, x, c0:c0 + hd] = True
    t2["dout"][b, y, x, head * hd:(head + 1) * hd] = vampic.synth.normal((case.N, hd), 903)
    may_out[b, y, x, head * hd:(head + 1) * hd] = True
    assert int(may_out.sum()) == case.N * hd and int(may_dq.sum()) == 3 * case.N * hd
    return t2, may_out, may_dq


@pytest.mark.parametrize("cid,path", [(c, p) for c, p in RUNS if c in ("a", "g")])
def test_one_window_head_changes_only_its_own_pixels(cid, path):
    """Redraw q, k, v and dO of one (image, window, head) — the last window, the one that holds all four regions of the
    shifted image: exactly that window's pixels (by the reference's roll arithmetic) x that head's channels change in out
    and dqkv, everything else is bit-identical, and so are the other heads' columns of dtable."""
    case, t, _, _ = _ref(cid)
    b, window, head = case.B - 1, case.nW - 1, 5
    _, first = _launch(cid, path)
    t2, may_out, may_dq = _changed(case, t, b, window, head)
    second = _run(AC.build(case, "cuda", t2), path)
    for k, a, c, may in (("out", first.out, second.out, may_out), ("dqkv", first.dqkv, second.dqkv, may_dq)):
        diff = _bits(a) != _bits(c)
        assert not bool(diff[~may].any()), f"{cid} {path}: {int(diff[~may].sum())} elements of {k} outside the window-head changed"
        assert int(diff[may].sum()) > 0.9 * int(may.sum()), f"{cid} {path}: the window-head's own {k} did not change"
    others = [h for h in range(case.heads) if h != head]
    assert torch.equal(_bits(first.dtable[:, others]), _bits(second.dtable[:, others]))
    assert not torch.equal(first.dtable[:, head], second.dtable[:, head])


@pytest.mark.parametrize("cid,path", [(c, p) for c, p in RUNS if c in ("a", "g")])
def test_image_alone_equals_image_in_the_batch(cid, path):
    case, t, _, _ = _ref(cid)
    _, batch = _launch(cid, path)
    case0, t0 = AC.image0(case, t)
    alone = _run(AC.build(case0, "cuda", t0), path)
    assert alone.s_out == 0 and alone.s_dq == 0 and alone.s_dt == 0 and alone.s_ws == 0
    assert torch.equal(_bits(alone.out[0]), _bits(batch.out[0]))
    assert torch.equal(_bits(alone.dqkv[0]), _bits(batch.dqkv[0]))


@pytest.mark.parametrize("cid,path", BWD_RUNS)
def test_zero_output_gradient_gives_zero_gradients(cid, path):
    case, t, _, _ = _ref(cid)
    t0 = dict(t, dout=torch.zeros_like(t["dout"]))
    r = _run(AC.build(case, "cuda", t0), path)
    assert bool((r.dqkv == 0).all()) and bool((r.dtable == 0).all())
    assert r.s_dq == 0 and r.s_dt == 0 and r.s_ws == 0


# (name, ws, heads, hd, H, W, shift, what is wrong, does the forward refuse too)
REFUSALS = [
    ("backward at (8, 40)", 8, 8, 40, 8, 8, 1, {}, False),
    ("backward at (4, 24)", 4, 12, 24, 8, 8, 3, {}, False),
    ("H not a multiple of ws", 8, 8, 24, 12, 8, 4, {}, True),
    ("shift = ws", 8, 8, 24, 8, 8, 8, {}, True),
    ("ld_qkv not a multiple of 4", 8, 8, 24, 8, 8, 4, {"ld_qkv": 10}, True),
    ("ld_out / ld_dq not a multiple of 4", 4, 8, 40, 8, 8, 2, {"ld_out": 10, "ld_dq": 10}, True),
    ("ld_do not a multiple of 4", 4, 8, 40, 8, 8, 2, {"ld_do": 10}, False),
    ("ld_qkv < 3C", 8, 8, 24, 8, 8, 4, {"ld_qkv": -4}, True),
    ("heads = 2 with ws = 4", 4, 2, 40, 8, 8, 2, {}, True),
    ("hd = 32", 8, 8, 32, 8, 8, 4, {}, True),
]


@pytest.mark.parametrize("name,ws,heads,hd,H,W,shift,bad,fwd", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_arguments_are_refused(name, ws, heads, hd, H, W, shift, bad, fwd):
    """Each call raises L.VamError and leaves every output at the sentinel.  Only the arguments are bad: every buffer is
    finite, aligned and, with its spare image, larger than anything a launch of these extents could touch."""
    C, NT, B = heads * hd, (2 * ws - 1) ** 2, 1

    def buf(chans, delta, fill):
        delta = delta or 0
        ld = chans + delta if delta < 0 else chans + 8 + delta                          # a negative delta: ld below the window
        return torch.full((B + 1, H, W, ld), fill, dtype=torch.float32, device="cuda")

    def view(b, chans):
        narrow = b.shape[3] < chans + 4
        return ops.View(b[:B], 0 if narrow else 4, chans)

    qkv = buf(3 * C, bad.get("ld_qkv"), 0.25)
    dout = buf(C, bad.get("ld_do"), 0.5)
    out = buf(C, bad.get("ld_out"), AC.SENTINEL)
    dqkv = buf(3 * C, bad.get("ld_dq"), AC.SENTINEL)
    table = torch.zeros((NT, heads), device="cuda")
    dtable = torch.full((NT, heads), AC.SENTINEL, device="cuda")
    wsp = torch.full(((B + 1) * (H // ws + 1) * (W // ws + 1) * heads * NT,), AC.SENTINEL, device="cuda")
    if fwd:
        with pytest.raises(L.VamError):
            ops.win_attention(view(qkv, 3 * C), view(out, C), table, C, heads, ws, shift)
    with pytest.raises(L.VamError):
        ops.win_attention_bwd(view(qkv, 3 * C), view(dout, C), view(dqkv, 3 * C), table, dtable, C, heads, ws, shift, workspace=wsp)
    torch.cuda.synchronize()
    none = torch.zeros(1, dtype=torch.bool)
    for what, b in (("out", out), ("dqkv", dqkv), ("dtable", dtable), ("workspace", wsp)):
        b = b.cpu()
        assert AC.stray(b, none.expand(b.shape)) == 0, f"{name}: {what} was written"
