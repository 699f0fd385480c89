"""The float64 contract of the inference likelihood and rate kernels (tests/entropy_contract.py), checked WITHOUT a GPU: its
float32 body against the oracle's own functions, its float32 statement against its bound (K_cpu), the placement of its
ties, bounds and table points, and that wrong formulas fall outside the judgement the GPU test uses — so that the GPU test
compares the kernels with something this module did not merely assert."""
import numpy as np
import torch

import vampic_oracle as O
import entropy_contract as EC
from entropy_contract import Tape
from conftest import record_measurement

F32 = np.float32


def _t32(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32)


def _same_bits(a, b, what):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    diff = EC.bits(a) != EC.bits(b)
    assert not diff.any(), (what, int(diff.sum()), a[diff][:4], b[diff][:4])


# ------------------------------------------------------------------------------------------------ ref against the oracle
def test_tail_body_in_float32_is_the_oracle_s_likelihood():
    """Where their domains meet the float32 body IS oracle gaussian_likelihood, bit for bit: unmasked against ``means``, masked
    with m = 1 against ``means=None`` on d, and masked with any m against ``means=None`` on (d m, sigma m)."""
    for cid in ("t-ragged", "t-opt", "t-mixed"):
        I = EC.inputs(cid)[0]
        r = _t32(I["y"]) - _t32(I["y2"])
        mu, sg = _t32(I["mu"]), _t32(I["sigma"])
        o = EC.tail_body(Tape("f32"), I, False)
        _same_bits(o["lik"], O.gaussian_likelihood(r, sg, mu), (cid, "unmasked lik"))
        _same_bits(o["yhat"], torch.round(r - mu) + mu, (cid, "unmasked yhat"))
        d = r - mu
        o = EC.tail_body(Tape("f32"), {**I, "mask": np.ones_like(I["sigma"])}, True)
        _same_bits(o["lik"], O.gaussian_likelihood(d, sg, None), (cid, "m = 1"))
        m = _t32(I["mask"])
        o = EC.tail_body(Tape("f32"), I, True)
        _same_bits(o["lik"], O.gaussian_likelihood(d * m, sg * m, None), (cid, "masked lik"))     # pic.py:625-629
        _same_bits(o["yhat"], torch.round(d) * m + mu, (cid, "masked yhat"))
        # the emulated chain states the exact outputs, and this host's float32 agrees with it
        e = EC.tail_body(Tape("f32e"), I, True)
        _same_bits(o["yhat"], e["yhat"], (cid, "f32e yhat"))
        assert np.array_equal(o["sym"].numpy(), e["sym"].numpy())


def test_index_body_is_the_oracle_s_build_indexes():
    tb = EC.scale_table()
    for cid in ("t-ragged", "t-mixed"):
        I = EC.inputs(cid)[0]
        for mask in (None, I["mask"][0]):
            s = _t32(I["sigma"]) * (1 if mask is None else _t32(mask))
            got = EC.index_body(Tape("f32e"), I["sigma"], mask, tb).numpy()
            assert np.array_equal(got, O.build_indexes(s, torch.from_numpy(tb)).numpy()), cid


def test_eb_eval_body_in_float32_against_the_oracle():
    """zhat and the symbols are the oracle's in bits.  The likelihood is not, and the residue has two named causes: the oracle
    multiplies its 3x3 matrices with ``torch.matmul`` (another order of the three products' sum) and calls ``torch.sigmoid``
    where the kernel and the body write 1 / (1 + exp(-x)).  Bounded: the oracle's float32 likelihood meets the same judgement
    the GPU must meet, at the floor K = 8."""
    for cid in ("e-small", "e-odd", "e-wide"):
        case = EC.CASES[cid]
        I = EC.inputs(cid)[0]
        C, N = I["z"].shape
        P = EC.eb_split(I["params"], C)
        sd = {"eb." + n: _t32(a.reshape((C,) + shp)) for n, shp, a in zip(EC.TC.EB_NAMES, EC.TC.EB_SHAPES, P)}
        zh, lik = O.eb_forward(sd, _t32(I["z"])[None, :, None, :], "eb.")
        o = EC.eb_eval_body(Tape("f32"), P, I["z"])
        _same_bits(o["zhat"], zh.reshape(C, N), (cid, "zhat"))
        ref = EC.eb_reference(cid)
        _same_bits(ref["zhat"].ref32, zh.reshape(C, N), (cid, "zhat f32e"))
        assert np.array_equal(ref["sym"], torch.round(_t32(I["z"]) - sd["eb.quantiles"][:, 0, 1:2]).int().numpy())
        differ = int((EC.bits(o["lik"].numpy()) != EC.bits(lik.reshape(C, N).numpy())).sum())
        rat, berr = EC.judge_lik((cid, "oracle"), lik.reshape(C, N).numpy(), ref["lik"], EC.K_FLOOR)
        print(f"{cid}: oracle eb_forward differs from the float32 body in {differ} of {C * N} likelihoods; its ratio {rat:.3f}, {berr:.3g} bits")
        record_measurement(f"entropy_contract oracle eb_forward vs float64 {cid}", differing=differ, ratio=round(rat, 3))


# ------------------------------------------------------------------------------------------------ ref32 inside the bound
def test_ref32_is_inside_every_bound_and_k_cpu():
    for fam in ("gauss", "eb"):
        k = EC.k_cpu(fam)
        print(f"K_cpu {fam} lik = {k:.3f}, K = {EC.k_of(fam):.1f}")
        record_measurement(f"entropy_contract K_cpu {fam}", lik=round(k, 3), K=EC.k_of(fam))
        assert k <= 4.0, (fam, k, "the budget is missing a term")
    worst_bits = {}
    for cid, vs in EC.GAUSS_VARIANTS.items():
        for v in vs:
            ref = EC.tail_reference(cid, v)
            assert np.isfinite(ref["lik"].A).all() and (ref["lik"].A >= 0).all(), (cid, v)
            rat, berr = EC.judge_lik((cid, v), ref["lik"].ref32, ref["lik"], EC.k_of("gauss"))
            worst_bits["gauss"] = max(worst_bits.get("gauss", 0.0), berr)
            I = dict(EC.inputs(cid)[0])                              # this host's float32 states the exact outputs as the emulation does
            if v.endswith("-noy2"):
                del I["y2"]
            kind = v.split("-")[0]
            if kind == "masked":
                I["mask"] = I["mask"][0]
            elif kind == "ones":
                I["mask"] = np.ones_like(I["sigma"])
            o = EC.tail_body(Tape("f32"), I, kind != "unmasked")
            EC.judge_exact((cid, v, "yhat"), EC.expand(EC.CASES[cid], o["yhat"].numpy()), ref["yhat"].ref32)
            EC.judge_exact((cid, v, "sym"), EC.expand(EC.CASES[cid], o["sym"].numpy().astype(np.int32)), ref["sym"])
    for cid, case in EC.CASES.items():
        if case.fam == "eb":
            ref = EC.eb_reference(cid)
            rat, berr = EC.judge_lik(cid, ref["lik"].ref32, ref["lik"], EC.k_of("eb"))
            worst_bits["eb"] = max(worst_bits.get("eb", 0.0), berr)
    out = EC.outside_ref()
    EC.judge_lik("outside", out.ref32, out, EC.k_of("gauss"))
    print("worst float32 error in bits:", worst_bits)
    record_measurement("entropy_contract float32 body, worst error in bits", **{k: float(f"{v:.3g}") for k, v in worst_bits.items()})


# ------------------------------------------------------------------------------------------------ placement
def test_points_are_placed_and_every_other_element_is_clear():
    tb = EC.scale_table()
    b = F32(0.11)
    for cid, case in EC.CASES.items():
        if case.fam != "tail":
            continue
        I, placed = EC.inputs(cid)
        q = EC.n_unique(case)
        e = EC.tail_body(Tape("f32e"), I, True)
        d, rq, s = e["d"].numpy(), e["rq"].numpy(), e["s"].numpy()
        d_in = (e["d"][None, :] * torch.tensor(I["mask"], dtype=torch.float64)).numpy()
        at = lambda name: placed.get(name, [])
        # ties really tie in fp32 (both signs, both parities), and round to even
        want = [sg * (k + 0.5) for k in (0, 1, 2, 7, 1022) for sg in (1.0, -1.0)][:len(at("tie"))]
        assert list(d[at("tie")]) == want, (cid, d[at("tie")])
        assert all(rq[0, i] == 2 * np.round(d[i] / 2) for i in at("tie"))
        assert all(np.signbit(e["q"].numpy()[i]) == (d[i] < 0) for i in at("tie"))                # +-0.5 gives +-0: symbol 0
        if at("tie_ulp"):
            assert list(d[at("tie_ulp")]) == [np.nextafter(F32(sg * 2.5), F32(side)) for sg in (1.0, -1.0) for side in (np.inf, -np.inf)]
            assert sorted(rq[0, at("tie_ulp")]) == [-3, -2, 2, 3]
            assert list(d_in[0, at("half_mask")]) == [2.5, -2.5, 1.5, -1.5] and list(rq[0, at("half_mask")]) == [2, -2, 2, -2]
            assert (I["mask"][:, at("m0") + at("s_m0")] == 0).all() and (rq[:, at("m0")] == 0).all()
            assert (s[:, at("s_at")] == b).all() and (s[:, at("s_below")] == np.nextafter(b, F32(0))).all()
            assert (I["sigma"][at("s_half")] > b).all() and (s[:, at("s_half")] < b).all() and (I["mask"][:, at("s_half")] == 0.5).all()
            assert np.signbit(I["y"][at("neg_zero")]).all()
            u = EC.tail_body(Tape("f32e"), I, False)
            assert (u["absv"].numpy()[at("big_mu")] != np.abs(u["q"].numpy()[at("big_mu")])).all(), "fl(fl(q + mu) - mu) == q at the big-mu points"
            assert (np.abs(u["q"].numpy()[at("big_mu")]) == 1).all()
            sig = I["sigma"][at("table")].reshape(4, 3)               # (entry, one ulp above, one ulp below) of entries 0, 1, 31, 62
            for row, t in zip(sig, (0, 1, 31, 62)):
                assert row[0] == tb[t] and row[1] == np.nextafter(tb[t], F32(np.inf)) and row[2] == np.nextafter(tb[t], F32(-np.inf))
            idx = EC.index_body(Tape("f32e"), I["sigma"], None, tb).numpy()[at("table")].reshape(4, 3)
            assert (idx[1:, 1] == idx[1:, 0] + 1).all() and (idx[1:, 2] == idx[1:, 0]).all(), idx     # `<=`: the entry itself counts
            assert list(idx[0]) == [0, 1, 0]                                                  # entry 0 is the 0.11 bound itself
            assert list(EC.index_body(Tape("f32e"), I["sigma"], None, tb).numpy()[at("table_edge")]) == [len(tb) - 1, 0]
        assert set(np.unique(I["mask"])) <= {0.0, 0.5, 1.0}
        assert np.abs(d).max() < 2.0 ** 24 and all(np.isfinite(v).all() for v in I.values())
        # the likelihood bound
        fixed = np.zeros(q, dtype=bool)
        fixed[[i for k, v in placed.items() if not k.startswith("table") for i in v]] = True
        n_odd = 0
        for v in EC.GAUSS_VARIANTS[cid]:
            ref = EC.tail_reference(cid, v)["lik"]
            flat = lambda a: a.reshape(-1, case.n_pix * case.C)[:, :q]
            band, below = flat(ref.band), flat(ref.ref64) <= EC.BOUND_L
            assert not band[:, ~fixed].any() and not below[:, ~fixed].any(), (cid, v, "an unplaced element in or below the band")
            if not case.o("band"):
                assert not ref.band.any(), (cid, v, "a case that checks its sums against float64 has no in-band element")
            elif not v.endswith("noy2"):
                assert band[:, at("band")].all(), (cid, v, flat(ref.ref64)[:, at("band")])
            if at("below") and not v.endswith("noy2"):
                assert below[:, at("below") + at("far_below")].all(), (cid, v)
            frac = (ref.band.sum() + (ref.ref64 <= EC.BOUND_L).sum()) / ref.ref64.size
            assert frac <= 0.01, (cid, v, frac)
            n_odd = max(n_odd, frac)
        print(f"{cid}: at most {100 * n_odd:.2f} % of the elements in the band or below it")
        if at("bits"):
            r = EC.tail_reference(cid, EC.GAUSS_VARIANTS[cid][0])["lik"].ref64.reshape(-1)[at("bits")]
            assert ((r > 0.9e-4) & (r < 1e-4)).all(), r
        if cid in EC.LAYER_LEVELS_OF and q >= 200:
            for nl in EC.LAYER_LEVELS_OF[cid]:
                assert {0, nl - 1, nl, EC.LAYER_NONE} <= set(I["layer"].tolist()), (cid, nl)


def test_eb_points_are_placed():
    for cid, case in EC.CASES.items():
        if case.fam != "eb":
            continue
        I, placed = EC.inputs(cid)
        C, N = I["z"].shape
        med = EC.eb_split(I["params"], C)[14][:, 1]
        assert (med * EC.GRID == np.round(med * EC.GRID)).all()
        e = EC.eb_eval_body(Tape("f32e"), EC.eb_split(I["params"], C), I["z"])
        ref = EC.eb_reference(cid)
        dz = (I["z"].astype(np.float64) - med[:, None].astype(np.float64)).astype(F32)
        for p, k, sy in zip(placed["tie"], (0.5, 1.5, -0.5, -2.5), (0, 2, 0, -2)):     # (a channel that would sit in the band there ties at 0.5)
            assert set(np.unique(dz[:, p])) <= {k, 0.5} and (dz[:, p] == k).sum() >= 0.9 * C, (cid, p, np.unique(dz[:, p]))
            assert (ref["sym"][:, p][dz[:, p] == k] == sy).all() and (ref["sym"][:, p][dz[:, p] != k] == 0).all()
        for c, p in placed["saturated"]:
            assert ref["lik"].ref64[c, p] == EC.BOUND_L and not ref["lik"].band[c, p]
        if N >= 7:
            assert len(placed["saturated"]) == 2
            s = e["sum"].numpy()
            assert (s > 0).any() and (s < 0).any()
            c, p, k0 = placed["sign"][0]
            print(f"{cid}: lower + upper closest to zero at z - med = {k0}: {s[c, p]:.3g}")
        frac = (ref["lik"].band.sum() + (ref["lik"].ref64 <= EC.BOUND_L).sum()) / ref["lik"].ref64.size
        assert frac <= 0.01 or case.n_pix * case.C < 200, (cid, frac)
        assert not ref["lik"].band.any(), cid                           # the bottleneck cases check their sums against float64
    assert EC.eb_reference("e-wide")["lik"].ref64.min() == EC.BOUND_L
    tails = EC.eb_reference("e-wide")["lik"].ref64
    assert ((tails > 2e-9) & (tails < 1e-4)).sum() >= 100               # likelihoods where an absolute 3e-7 says nothing


# ------------------------------------------------------------------------------------------------ wrong formulas
def _fails(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)[:160]
    return None


def _tail_mutant(cid, variant, mut):
    """the mutant's exact outputs from its emulated float32 chain and its likelihood in float64, through the GPU test's judgement"""
    case = EC.CASES[cid]
    I = dict(EC.inputs(cid)[0])
    masked = variant != "unmasked"
    if variant == "masked":
        I["mask"] = I["mask"][0]
    ref = EC.tail_reference(cid, variant)
    e = EC.tail_body(Tape("f32e"), I, masked, mut)
    o = EC.tail_body(Tape("f64"), I, masked, mut)
    ex = lambda a: EC.expand(case, a)

    def run():
        EC.judge_exact("yhat", ex(e["yhat"].numpy().astype(F32)), ref["yhat"].ref32)
        EC.judge_exact("sym", ex(e["sym"].numpy().astype(np.int32)), ref["sym"])
        EC.judge_lik("lik", ex(o["lik"].numpy()), ref["lik"], EC.k_of("gauss"))
    return _fails(run)


def _eb_mutant(cid, mut, mode):
    I = EC.inputs(cid)[0]
    P = EC.eb_split(I["params"], I["z"].shape[0])
    ref = EC.eb_reference(cid)
    e = EC.eb_eval_body(Tape("f32e"), P, I["z"], mut)
    o = EC.eb_eval_body(Tape(mode), P, I["z"], mut)

    def run():
        EC.judge_exact("zhat", e["zhat"].numpy().astype(F32), ref["zhat"].ref32)
        EC.judge_exact("sym", e["sym"].numpy().astype(np.int32), ref["sym"])
        EC.judge_lik("lik", o["lik"].numpy(), ref["lik"], EC.k_of("eb"))
    return _fails(run)


def test_wrong_formulas_fall_outside():
    """Each mutant must fail the judgement of the GPU test on the named case.  They are run in float64 (their decisions from
    their own emulated float32 chain) — but for the bottleneck's sign rule, which is an identity in exact arithmetic
    (sigmoid(-a) - sigmoid(-b) = -(sigmoid(a) - sigmoid(b))) and exists for float32 alone: that mutant is run in float32."""
    found = {
        "rint replaced by round-half-away": _tail_mutant("t-ragged", "masked", ("half_away",)),
        "rint replaced by round-half-away (the smallest case)": _tail_mutant("t-min", "masked", ("half_away",)),
        "|v| taken before the mask": _tail_mutant("t-ragged", "masked", ("absv_before_mask",)),
        "s = sigma in the masked branch": _tail_mutant("t-ragged", "masked", ("s_sigma",)),
        "the scale bound dropped": _tail_mutant("t-ragged", "masked", ("no_scale_bound",)),
        "the scale bound applied before the mask": _tail_mutant("t-ragged", "masked", ("scale_bound_before_mask",)),
        "|q| for |fl(fl(q + mu) - mu)| in the unmasked branch": _tail_mutant("t-ragged", "unmasked", ("absq",)),
        "the likelihood bound 1e-8": _tail_mutant("t-opt", "unmasked", ("lik_bound_1e-8",)),
        "0.7071f for the erfc constant": _tail_mutant("t-opt", "unmasked", ("erfc_const",)),
        "relative error 3e-5 on likelihoods below 1e-4": _tail_mutant("t-opt", "unmasked", ("bits_scale",)),
        "the EB median taken from quantile 0": _eb_mutant("e-wide", ("median_q0",), "f64"),
        "the EB rounding half away": _eb_mutant("e-small", ("half_away",), "f64"),
        "the EB sign rule dropped (float32)": _eb_mutant("e-wide", ("no_sign_rule",), "f32"),
    }
    tb = EC.scale_table()
    I = EC.inputs("t-ragged")[0]
    wrong = EC.expand(EC.CASES["t-ragged"], EC.index_body(Tape("f32e"), I["sigma"], None, tb, mut=("index_lt",)).numpy().astype(np.int32))
    found["`<` for `<=` in the index count"] = _fails(lambda: EC.judge_exact("idx", wrong, EC.index_reference("t-ragged", False)))
    # the bits-scale mutant passes the bar the suite had: 3e-7 absolute
    ref = EC.tail_reference("t-opt", "unmasked")["lik"]
    o = EC.tail_body(Tape("f64"), dict(EC.inputs("t-opt")[0]), False, ("bits_scale",))["lik"].numpy()
    assert np.abs(EC.expand(EC.CASES["t-opt"], o) - ref.ref64).max() < 3e-7
    for name, why in found.items():
        print(f"wrong formula: {name}: {why}")
        record_measurement("entropy_contract wrong formula", formula=name, fails=why is not None)
    missed = [n for n, why in found.items() if why is None]
    assert not missed, missed
