"""The float64 reference of tests/attn_contract.py checked without a GPU: against the oracle's window attention and float64
autograd, its bounds against an fp32 ATen evaluation of the same formulas, and against seven wrong formulas."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import vampic.synth
import vampic_oracle as O

import attn_contract as AC


@functools.lru_cache(maxsize=None)
def _ref(cid):
    case = AC.CASES[cid]
    t = AC.tensors(case)
    ref = AC.reference(case, t)
    return case, t, ref, AC.bounds(case, ref)


@pytest.mark.parametrize("cid", ["a", "c", "d", "e", "g", "h", "l"])
def test_reference_equals_the_oracle_core(cid, monkeypatch):
    """O.win_attention is shortcut + proj(attention(qkv(x))).  With proj the identity, qkv of the reference taken as the
    oracle's own linear layer of x, and float64 throughout, ``oracle - x`` is the core: the two formulations of the
    relative-position index, the region mask, the partition and the roll must agree to rounding."""
    case = AC.CASES[cid]
    C = case.C
    monkeypatch.setattr(O, "NUM_HEADS", case.heads)
    x = vampic.synth.normal((case.B, C, case.H, case.W), 5).double()
    sd = {"p.attn.qkv.weight": vampic.synth.normal((3 * C, C), 6, C ** -0.5).double(),
          "p.attn.qkv.bias": vampic.synth.normal((3 * C,), 7, 0.5).double(),
          "p.attn.relative_position_bias_table": vampic.synth.normal((case.NT, case.heads), 8, 0.5).double(),
          "p.attn.proj.weight": torch.eye(C, dtype=torch.float64), "p.attn.proj.bias": torch.zeros(C, dtype=torch.float64)}
    want = (O.win_attention(sd, "p.", x, case.ws, case.shift) - x).permute(0, 2, 3, 1)
    qkv = F.linear(x.permute(0, 2, 3, 1), sd["p.attn.qkv.weight"], sd["p.attn.qkv.bias"])
    t = {"qkv": qkv, "dout": torch.zeros((case.B, case.H, case.W, C), dtype=torch.float64), "table": sd["p.attn.relative_position_bias_table"]}
    got = AC.evaluate(case, t, backward=False).out
    assert got.shape == want.shape and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("cid", [c for c, v in AC.CASES.items() if v.backward])
def test_closed_form_backward_equals_float64_autograd(cid):
    case, t, ref, _ = _ref(cid)
    qkv = t["qkv"].double().requires_grad_(True)
    table = t["table"].double().requires_grad_(True)
    out = AC.evaluate(case, t, backward=False, qkv=qkv, table=table).out
    out.backward(t["dout"].double())
    assert torch.equal(out.detach(), ref.out)
    for name, got, want in (("dqkv", ref.dqkv, qkv.grad), ("dtable", ref.dtable, table.grad)):
        err = (got - want).abs().max().item()
        assert err <= 1e-12 * max(1.0, want.abs().max().item()), (cid, name, err)


def _dispatched(source, pattern):
    csrc = os.path.join(os.path.dirname(os.path.abspath(vampic._lib.__file__)), "csrc")
    with open(os.path.join(csrc, source)) as f:
        return {(int(a), int(b)) for a, b in re.findall(pattern, f.read())}


def test_table_covers_every_kernel_the_dispatchers_name():
    """The (ws, hd) pairs are read from the dispatchers' own text, so a new instantiation without a case fails here."""
    assert _dispatched("win_attn.hip", r"ws == (\d+) && hd == (\d+)") == set(AC.FORWARD_PAIRS)
    assert _dispatched("train_gs.hip", r"VAM_ATT_BWD\((\d+), (\d+)\)") == set(AC.BACKWARD_PAIRS)
    assert _dispatched("train_gs.hip", r"ws == (\d+) && hd == (\d+) && vam_attn_mfma") <= set(AC.BACKWARD_PAIRS)
    fwd = {(c.ws, c.hd) for c in AC.CASES.values()}
    bwd = {(c.ws, c.hd) for c in AC.CASES.values() if c.backward}
    assert fwd == set(AC.FORWARD_PAIRS) and bwd == set(AC.BACKWARD_PAIRS)
    c = AC.CASES
    assert {v.shift for v in c.values() if v.ws == 8} >= {0, 1, 4, 7} and {v.shift for v in c.values() if v.ws == 4} >= {0, 2, 3}
    assert any(v.H == v.ws and v.shift > 0 for v in c.values()) and any(v.heads not in (8,) for v in c.values())
    assert any(v.nW == 1 and v.B == 1 for v in c.values())


def test_shapes_and_masks():
    for cid in AC.CASES:
        case, t, ref, bnd = _ref(cid)
        assert ref.out.shape == (case.B, case.H, case.W, case.C)
        assert ref.p.shape == (case.B, case.nW, case.heads, case.N, case.N)
        assert bool(torch.isfinite(ref.out).all()) and bool((bnd["out"] > 0).all())
        assert (ref.mask != 0).any().item() == (case.shift > 0), cid
        assert bool((ref.mask.diagonal(dim1=-2, dim2=-1) == 0).all())
        if case.backward:
            assert ref.dqkv.shape == (case.B, case.H, case.W, 3 * case.C) and ref.dtable.shape == (case.NT, case.heads)
            for k in ("dq", "dk", "dv", "dtable"):
                assert bool((bnd[k] > 0).all()) and bool(torch.isfinite(bnd[k]).all()), (cid, k)
    # the strong-logit cases are what tells the additive -100 from a hard mask: a masked key keeps visible weight there
    for cid in ("b", "d", "f"):
        case, t, ref, _ = _ref(cid)
        masked = ref.p * (ref.mask != 0)[None, :, None]
        assert masked.sum(-1).max().item() > 0.5, cid


@pytest.mark.parametrize("cid", list(AC.CASES))
def test_fp32_aten_meets_every_bound(cid):
    """The bounds asserted on the GPU are ones a plain fp32 evaluation meets: ATen's fp32 evaluation of the same formulas
    (fp32 matmul, softmax, index_add) passes every one of them on every case, with room — which is the justification of
    the constants in ``bounds``; they move only on this evidence.  Measured on an x86 host, error / bound over the cases:
    out 0.0092 ... 0.060, dq 0.0007 ... 0.0065, dk 0.0010 ... 0.017, dv 0.013 ... 0.075, dtable 0.0004 ... 0.017 (the largest
    on the strong-logit cases b and d)."""
    case, t, ref, bnd = _ref(cid)
    got = AC.evaluate(case, t, torch.float32, backward=case.backward)
    assert got.out.dtype == torch.float32
    r = AC.check(case, ref, AC.split(case, got.out, got.dqkv, got.dtable), "fp32 ATen", bnd)
    print(f"{cid}: fp32 ATen error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert set(r) == (set(AC.QUANTITIES) if case.backward else {"out"})
    assert max(r.values()) <= 0.5, (cid, r)


FACTOR = 100.0      # "outside the bound by a wide factor"


@pytest.mark.parametrize("wrong", AC.WRONG)
def test_the_bounds_reject_a_wrong_formula(wrong):
    """Each wrong formula, evaluated in float64 (no rounding to hide behind), is outside the bounds by at least a factor 100
    on some case — on the forward and on a gradient, except dk <-> dq, which has no forward.  Measured: the largest forward
    ratio is roll+1 3e8, ridx^T 2e5, region-1 5e7, hard mask 2e6, no scale 3e8, table[head][ridx] 3e5; per case the largest
    ratio of any quantity is 1e4 or more on every case a variant can touch (region-1 needs a shift, dk <-> dq a backward).
    The hard mask is told from the additive -100 by the strong-logit cases alone: b 1e9, d 9e22, f 2e35, j 3.8, at most
    2e-7 on the eight cases with unscaled q and k.  (Backward ratios run to 1e30 and beyond where the float64 gradient
    element, and with it its bound, is next to nothing.)"""
    worst_f, worst_b, per_case = 0.0, 0.0, {}
    for cid in AC.CASES:
        case, t, ref, bnd = _ref(cid)
        bad = AC.evaluate(case, t, torch.float64, wrong=wrong, backward=case.backward)
        r = AC.ratios(case, ref, AC.split(case, bad.out, bad.dqkv, bad.dtable), bnd)
        per_case[cid] = r
        worst_f = max(worst_f, r["out"])
        worst_b = max([worst_b] + [v for k, v in r.items() if k != "out"])
    print(f"{wrong}: forward {worst_f:.3g}, backward {worst_b:.3g} x the bound; "
          + ", ".join(f"{c} {max(v.values()):.2g}" for c, v in per_case.items()))
    if wrong != "dk<->dq":
        assert worst_f >= FACTOR, (wrong, worst_f)
    else:
        assert worst_f == 0.0
    assert worst_b >= FACTOR, (wrong, worst_b)
    if wrong == "hard mask":            # separated by the strong-logit cases only: that is why they are in the table
        weak = max(max(per_case[c].values()) for c in AC.CASES if AC.CASES[c].qk == 1.0)
        assert weak <= 1.0, weak
