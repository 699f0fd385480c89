"""The float64 contract of the training element-wise and likelihood kernels (tests/train_ew_contract.py), checked WITHOUT a GPU:
its reference against autograd over the oracle's own functions, its float32 statement against its bound, the placement of
its decision points, and that wrong formulas fall outside the bound — so that the GPU test compares the kernels with
something this module did not merely assert."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vampic_oracle as O
import train_ew_contract as TC
from conftest import record_measurement

F64 = torch.float64
ULP64 = 2.0 ** -53


def _t(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=F64, requires_grad=grad)


def _close(got, want, A=None, what=""):
    """1e-12 relative, plus the float64 rounding of the two evaluations where the result is a cancellation: 64 ulp64 of the budget"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = 1e-12 * np.abs(want) + (64 * ULP64 * np.asarray(A) if A is not None else 0.0) + 1e-300
    bad = np.abs(got - want) > tol
    assert not bad.any(), (what, int(bad.sum()), got[bad][:3], want[bad][:3])


def _ew64(name, ins, coef=0.0, flag=0, budget=False):
    T = TC.Tape("budget" if budget else "f64")
    outs = TC.ew_body(T, TC.EW_OPS[name][0], [T.inp(a) for a in ins], coef, flag)
    if budget:
        return [T.budget_of(o) for o in outs]
    return [o.numpy() for o in outs]


def _pat(cid):
    return TC.inputs(cid)[0]


# ------------------------------------------------------------------------------------------------ ref64 against autograd
def test_elementwise_ref64_is_autograd_of_the_layers():
    I = _pat("ew-GELU_BWD-f0-C36")
    v, g = _t(I["in0"], True), _t(I["in1"])
    y = F.gelu(v)
    y.backward(g)
    _close(_ew64("GELU_FWD", [I["in0"]])[0], y.detach(), _ew64("GELU_FWD", [I["in0"]], budget=True)[0], "gelu")
    _close(_ew64("GELU_BWD", [I["in0"], I["in1"]])[0], v.grad, _ew64("GELU_BWD", [I["in0"], I["in1"]], budget=True)[0], "gelu'")

    I = _pat("ew-GATE_BWD-f0-C36")
    a, b, x = _t(I["in0"], True), _t(I["in1"], True), _t(I["in2"])
    y = a * torch.sigmoid(b) + x                                       # layers.py:72-74
    _close(_ew64("GATE_FWD", [I["in0"], I["in1"], I["in2"]])[0], y.detach(), _ew64("GATE_FWD", [I["in0"], I["in1"], I["in2"]], budget=True)[0], "gate")
    y.backward(x)                                                      # in2 of the backward = dout
    got, A = _ew64("GATE_BWD", [I["in0"], I["in1"], I["in2"]]), _ew64("GATE_BWD", [I["in0"], I["in1"], I["in2"]], budget=True)
    _close(got[0], a.grad, A[0], "gate da")
    _close(got[1], b.grad, A[1], "gate db")

    I = _pat("ew-HTANH_FWD-f0-C36")
    z = _t(I["in0"], True)
    y = 0.5 * torch.tanh(z) + _t(I["in1"]) + _t(I["in2"])               # pic.py:635-641
    _close(_ew64("HTANH_FWD", [I["in0"], I["in1"], I["in2"]])[0], y.detach(), _ew64("HTANH_FWD", [I["in0"], I["in1"], I["in2"]], budget=True)[0], "htanh")
    y.backward(_t(I["in1"]))
    _close(_ew64("HTANH_BWD", [I["in0"], I["in1"]])[0], z.grad, _ew64("HTANH_BWD", [I["in0"], I["in1"]], budget=True)[0], "htanh'")

    I = _pat("ew-MASK_SPLIT-f0-C36")
    g, m = _t(I["in0"]), _t(I["in1"])
    got = _ew64("MASK_SPLIT", [I["in0"], I["in1"]])
    _close(got[0], g * m)
    _close(got[1], g * (1 - m))
    I = _pat("ew-AXPY-f0-C36")
    _close(_ew64("AXPY", [I["in0"], I["in1"]], coef=TC.AXPY_COEF)[0], _t(I["in0"]) + TC.AXPY_COEF * _t(I["in1"]))

    I = _pat("ew-CLAMP_BWD-f0-C36")                                    # away from the two edges torch.clamp passes the same elements
    v = _t(np.where((I["in0"] == 0) | (I["in0"] == 1), 0.5, I["in0"]) + np.where(I["in1"] > 1.0, 2.0, 0.0) - np.where(I["in1"] < -1.0, 2.0, 0.0), True)
    c = torch.clamp(v, 0, 1)
    c.backward(_t(I["in1"]))
    _close(_ew64("CLAMP_BWD", [c.detach().numpy().astype(np.float32), I["in1"]])[0], v.grad)

    I = _pat("leaky-C36")
    pre = _t(np.where(I["in0"] == 0, 0.25, I["in0"]), True)
    act = F.leaky_relu(pre, 0.01)
    act.backward(_t(I["in1"]))
    T = TC.Tape("f64")
    _close(TC.leaky_body(T, [act.detach(), T.inp(I["in1"])])[0], pre.grad)


def test_gdn_and_reparam_ref64_are_autograd_of_the_oracle():
    """APPLY, BWD_PREP, gamma^T, BWD_FIN chained = autograd through oracle gdn(), both directions; REPARAM_BWD = autograd through
    oracle nonneg() (LowerBound's rule at p == bound, one ulp below, both signs)."""
    rng = np.random.RandomState(5)
    C, H, W = 8, 5, 7
    for inverse in (False, True):
        x = rng.standard_normal((1, C, H, W)) * 2
        sd = {"g.beta": _t(rng.uniform(0.5, 2.0, C)), "g.gamma": _t(rng.uniform(0.0, 0.3, (C, C)))}
        dy = rng.standard_normal((1, C, H, W))
        xt = _t(x, True)
        y = O.gdn(sd, "g.", xt, inverse)
        y.backward(_t(dy))
        gamma = O.nonneg(sd["g.gamma"], 0.0)
        norm = F.conv2d(_t(x) ** 2, gamma.reshape(C, C, 1, 1), O.nonneg(sd["g.beta"], 1e-6)).numpy()
        flat = lambda a: np.asarray(a).transpose(0, 2, 3, 1).reshape(-1, C)          # [pixels, C]
        fl = int(inverse)
        T = TC.Tape("f64")
        ins = [torch.tensor(flat(a)) for a in (x, norm, dy)]
        _close(TC.ew_body(T, TC.EW_GDN_APPLY, ins[:2], flag=fl)[0], flat(y.detach()), None, "gdn apply")
        dnorm, part, xsq = TC.ew_body(T, TC.EW_GDN_BWD_PREP, ins, flag=fl)
        _close(xsq, flat(x) ** 2)
        u = dnorm @ gamma                                              # gamma^T dL/dnorm: norm_i = beta_i + sum_j gamma_ij x_j^2
        dx = TC.ew_body(T, TC.EW_GDN_BWD_FIN, [part, ins[0], u])[0]
        scale = (part.abs() + 2 * (ins[0].abs() * (dnorm.abs() @ gamma))).numpy()
        _close(dx, flat(xt.grad), scale, f"gdn dx inverse={inverse}")

    I = _pat("ew-REPARAM_BWD-f0-C36")
    p = _t(I["in0"], True)
    O.nonneg(p, 1e-6).backward(_t(I["in1"]))
    got = _ew64("REPARAM_BWD", [I["in0"], I["in1"]], coef=TC.REPARAM_BOUND)[0]
    _close(got, p.grad, None, "reparam")
    b = np.float32(TC.REPARAM_BOUND)
    e = TC.inputs("ew-REPARAM_BWD-f0-C36")[1]["edges"]
    assert list(I["in0"][e]) == [b, b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(0))]
    assert got[e[0]] > 0 and got[e[1]] < 0 and got[e[2]] == 0 and got[e[3]] < 0      # at the bound both pass; below it only g < 0


def _oracle_gauss(I, k=None):
    """(lik, dmu, dsigma) by autograd over oracle gaussian_likelihood_noise on the kernel's operands"""
    lv = lambda n: I[n][k] if k is not None else I[n]
    y, mu, sg = _t(I["y"]), _t(I["mu"], True), _t(I["sigma"], True)
    d = (y - _t(I["y2"]) if "y2" in I else y) - mu
    if "mask" in I:
        m = _t(lv("mask"))
        lik = O.gaussian_likelihood_noise(d * m, sg * m, None, _t(lv("noise")))
    else:
        lik = O.gaussian_likelihood_noise(d, sg, None, _t(lv("noise")))
    lik.backward(_t(lv("g")))
    return lik.detach().numpy(), mu.grad.numpy(), sg.grad.numpy()


@pytest.mark.parametrize("cid", ["gauss-y20-m0-C36", "gauss-y21-m0-C36", "gauss-y20-m1-C36", "gauss-y21-m1-C36"])
def test_gauss_ref64_is_autograd_of_the_oracle(cid):
    I = _pat(cid)
    ref = TC.reference(cid)
    lik, dmu, dsg = _oracle_gauss(I)
    for name, want in (("lik", lik), ("dmu", dmu), ("dsigma", dsg)):
        _close(ref[name].ref64.reshape(-1), want, ref[name].A.reshape(-1), f"{cid} {name}")


@pytest.mark.parametrize("cid", ["levels-L1-y20-C36", "levels-L3-y21-C36"])
def test_levels_ref64_is_the_sum_of_the_oracle_levels(cid):
    """rq = round(r - mu) m + mu and the likelihood per level; gmu = sum (drq (1 - m) + dmu), dsigma = sum dsigma_l,
    dyt += sum d_r, dys -= sum d_r with d_r = drq m - dmu (straight-through rounding under the mask)."""
    I = _pat(cid)
    ref = TC.reference(cid)
    L = TC.CASES[cid].o("levels")
    gmu, dsig, dr = 0, 0, 0
    for k in range(L):
        lik, dmu, dsg = _oracle_gauss(I, k)
        _close(ref["lik"].ref64[k].reshape(-1), lik, ref["lik"].A[k].reshape(-1), f"lik {k}")
        d = I["y"].astype(np.float64) - (I["y2"] if "y2" in I else 0) - I["mu"]
        _close(ref["rq"].ref64[k].reshape(-1), np.round(d) * I["mask"][k] + I["mu"], np.abs(d) + np.abs(I["mu"]) + 1, f"rq {k}")
        q, m = I["drq"][k].astype(np.float64), I["mask"][k].astype(np.float64)
        gmu, dsig, dr = gmu + q * (1 - m) + dmu, dsig + dsg, dr + q * m - dmu
    for name, want in (("gmu", gmu), ("dsigma", dsig), ("dyt", I["dyt"] + dr)) + ((("dys", I["dys"] - dr),) if "dys" in I else ()):
        _close(ref[name].ref64.reshape(-1), want, ref[name].A.reshape(-1), f"{cid} {name}")


@pytest.mark.parametrize("cid", ["eb-C5-N129-ld5", "eb-C1-N100-ld4"])
def test_eb_ref64_is_autograd_of_the_oracle(cid):
    case = TC.CASES[cid]
    I = _pat(cid)
    C, N = case.C, case.n_pix
    P = TC.eb_split(I["params"], C)
    sd = {}
    for name, shp, a in zip(TC.EB_NAMES, TC.EB_SHAPES, P):
        sd["eb." + name] = _t(a.reshape((C,) + shp), name != "quantiles")
    z = _t(I["z"].reshape(1, C, 1, N), True)
    lik = O.eb_likelihood_noise_bounded(sd, z, _t(I["noise"].reshape(1, C, 1, N)), "eb.")
    lik.backward(_t(I["g"].reshape(1, C, 1, N)))
    ref = TC.reference(cid)
    _close(ref["lik"].ref64, lik.detach().reshape(C, N), ref["lik"].A, "eb lik")
    _close(ref["dz"].ref64, z.grad.reshape(C, N), ref["dz"].A, "eb dz")
    want = np.concatenate([sd["eb." + n].grad.reshape(-1).numpy() for n in TC.EB_NAMES[:14]] + [np.zeros(3 * C)])
    # a stored matrix entry above softplus' threshold: F.softplus differentiates the identity there (1), the kernel and the
    # contract keep sigmoid(21) = 1 - 7.6e-10 — the same fp32 number, and the one place where the two float64 values part
    big = np.concatenate([I["params"][:-3 * C] > 20, np.zeros(3 * C, dtype=bool)])
    _close(ref["dparams"].ref64[~big], want[~big], ref["dparams"].A[~big], "eb dparams")
    assert np.all(np.abs(ref["dparams"].ref64[big] - want[big]) <= 1e-9 * np.abs(want[big]))
    assert np.all(ref["dparams"].ref64[-3 * C:] == 0)


def test_layout_refs_are_the_adjoints_of_the_layers():
    """ps2_unshuffle = the gradient of PixelShuffle(2) w.r.t. its input (NHWC); upsample2_zero = the data gradient of a
    stride-2 convolution whose taps are a unit (a 1x1 identity: where the samples land)."""
    src = TC.inputs("ps2-Cq3")[0]["src"]                               # [B, 2H, 2W, Cq] = dL/d(shuffled)
    B, H2, W2, Cq = src.shape
    x = torch.zeros(B, 4 * Cq, H2 // 2, W2 // 2, dtype=F64, requires_grad=True)
    F.pixel_shuffle(x, 2).backward(_t(src).permute(0, 3, 1, 2))
    assert np.array_equal(TC.ps2_unshuffle_ref(src.astype(np.float64)), x.grad.permute(0, 2, 3, 1).numpy())
    src = TC.inputs("up2-C8")[0]["src"]                                # [B, H, W, C] = dL/d(conv output)
    B, H, W, C = src.shape
    x = torch.zeros(B, C, 2 * H, 2 * W, dtype=F64, requires_grad=True)
    F.conv2d(x, torch.eye(C, dtype=F64).reshape(C, C, 1, 1), stride=2).backward(_t(src).permute(0, 3, 1, 2))
    assert np.array_equal(TC.upsample2_zero_ref(src.astype(np.float64)), x.grad.permute(0, 2, 3, 1).numpy())


# ------------------------------------------------------------------------------------------------ ref32 inside the bound
def test_ref32_is_inside_every_bound_and_k_cpu():
    """The float32 statement of every operation lies inside |ref32 - ref64| <= 8 * 2^-24 A + 2^-126 on the contract's own inputs
    (an honest budget gives K_cpu well below 4), exact operations have a float32 statement that is finite, and every budget is
    finite and non-negative."""
    for op in TC.ops_of_cases():
        k = TC.k_cpu(op)
        print(f"K_cpu {op}: " + (", ".join(f"{n} = {v:.3f}" for n, v in k.items()) or "exact"))
        record_measurement(f"train_ew_contract K_cpu {op}", **{n: round(v, 3) for n, v in k.items()} or {"exact": True})
        for n, v in k.items():
            assert v <= 4.0, (op, n, v, "the budget is missing a term")
    # informational: does this host's ATen float32 agree with the correctly rounded (emulated) chain of the exact operations?
    host = {}
    for cid, case in TC.CASES.items():
        if case.fam == "ew" and case.op in TC.EXACT_EW and not case.o("tile"):
            outs = TC._ew_like_body(case, TC.inputs(cid)[0])(TC.Tape("f32"), None)
            for name, ref in TC.reference(cid).items():
                host[case.op] = host.get(case.op, 0) + int((TC.bits(TC.expand(case, outs[name].numpy())) != TC.bits(ref.ref32)).sum())
    print("host ATen float32 vs emulated fp32, differing elements:", host)
    record_measurement("train_ew_contract host float32 vs emulated fp32 (differing elements)", **host)
    for cid in TC.CASES:
        for name, ref in TC.reference(cid).items():
            assert np.isfinite(ref.ref32).all() and np.isfinite(ref.ref64).all(), (cid, name)
            if not ref.exact:
                assert np.isfinite(ref.A).all() and (ref.A >= 0).all(), (cid, name)
                assert ref.ratio(ref.ref32)[0] <= TC.K_FLOOR, (cid, name)


def test_exact_inputs_have_no_subnormal_intermediate():
    """Bit-equality is asked only where no intermediate of the float32 statement is subnormal (a GPU may flush those)."""
    tiny = np.finfo(np.float32).tiny
    for cid, case in TC.CASES.items():
        if case.fam in ("ew", "mul", "axpy") and (case.fam != "ew" or case.op in TC.EXACT_EW) and case.op not in ("CLAMP_BWD",):
            for name, ref in TC.reference(cid).items():
                v = np.abs(ref.ref32[ref.ref32 != 0])
                assert v.size == 0 or v.min() >= tiny * 2 ** 24, (cid, name, v.min())
        if case.fam == "ew" and case.op.startswith("GDN") and case.op != "GDN_BWD_FIN":
            n = TC.inputs(cid)[0]["in1"]
            assert n.min() >= 1e-3 * (1 - 1e-6) and n.max() <= 1e3 * (1 + 1e-6)


# ------------------------------------------------------------------------------------------------ decision points
def test_decision_points_are_placed_and_every_other_element_is_clear():
    for cid, case in TC.CASES.items():
        I, placed = TC.inputs(cid)
        if case.fam in ("gauss", "levels"):
            q = TC._n_unique(case)
            L = case.o("levels") or 1
            band = np.zeros(q, dtype=bool)
            band[placed["band"]] = True
            assert 0 < band.sum() <= 0.01 * q or q < 200, (cid, band.sum())
            for k in range(L):
                J = {n: (v[k] if case.fam == "levels" and n in ("mask", "noise") else v) for n, v in I.items() if n in ("y", "y2", "mu", "sigma", "mask", "noise")}
                lr = TC._lik_raw64(J)
                clear = (lr > TC.BAND[1]) | (lr < TC.BAND[0])
                assert clear[~band].all(), (cid, k, np.flatnonzero(~clear & ~band))
                assert ((lr >= TC.BAND[0]) & (lr <= TC.BAND[1]))[band].all(), (cid, k, lr[band])
                below = lr < TC.BAND[0]
                g = I["g"][k] if case.fam == "levels" else I["g"]
                assert (below & (g > 0)).any() and (below & (g < 0)).any(), cid
            masked = "mask" in I
            m = (I["mask"] if masked else np.ones_like(I["sigma"])).reshape(L, q)
            sm = (I["sigma"] * m).astype(np.float32)
            b = np.float32(0.11)
            assert (sm[:, placed["s_at"]] == b).all() and (sm[:, placed["s_below"]] == np.nextafter(b, np.float32(0))).all()
            if masked:
                assert (m[:, placed["s_m0"]] == 0).all() and (m[:, placed["v0_m0"]] == 0).all() and (I["noise"].reshape(L, q)[:, placed["v0_m0"]] == 0).all()
                assert (m[:, placed["s_half"]] == 0.5).all() and (sm[:, placed["s_half"]] < b).all() and (I["sigma"][placed["s_half"]] > b).all()
                assert set(np.unique(m)) <= {0.0, 0.5, 1.0}             # d * m and sigma * m are exact: no decision depends on a rounding
            d = (I["y"].astype(np.float64) - (I["y2"] if "y2" in I else 0) - I["mu"])[placed["v0_m1"]]
            assert (d.astype(np.float32) == d).all() and (I["noise"].reshape(L, q)[:, placed["v0_m1"]] == -d).all()
            # what the reference does at these points
            ref = TC.reference(cid)
            flat = lambda a: a.reshape(L, -1)[:, :q] if a.shape[0] == L and case.fam == "levels" and a.ndim == 3 else a.reshape(1, -1)[:, :q]
            if case.fam == "gauss":
                for r in (ref["dmu"].ref64, ref["dmu"].ref32):
                    assert (flat(r)[:, placed["v0_m1"] + placed.get("v0_m0", [])] == 0).all(), cid
                dsg, g = flat(ref["dsigma"].ref64), I["g"].reshape(1, q)
                # near the mode dlik/ds < 0: a negative g gives gs > 0, which the scale bound stops one ulp below 0.11f and not at it
                stop = [i for i in placed["s_below"] if g[0, i] < 0]
                go = [i for i in placed["s_below"] if g[0, i] > 0]
                assert stop and go and (dsg[:, stop] == 0).all() and (dsg[:, go] != 0).all() and (dsg[:, placed["s_at"]] != 0).all(), cid
                far = [i for i in placed["far_below"] + placed["below"] if g[0, i] >= 0]
                assert far and (flat(ref["dmu"].ref64)[:, far] == 0).all() and (dsg[:, far] == 0).all(), cid
                thru = [i for i in placed["below"] if g[0, i] < 0]
                assert thru and (flat(ref["dmu"].ref64)[:, thru] != 0).all(), cid
        if case.fam == "eb":
            ref = TC.reference(cid)
            lr = TC.eb_body(TC.Tape("f64"), TC.eb_split(I["params"], case.C), I["z"], I["noise"])["lik_raw"].numpy()
            band = ref["lik"].band
            assert band.sum() <= max(1, 0.01 * band.size), cid
            assert ((lr > TC.BAND[1]) | (lr < TC.BAND[0]))[~band].all(), cid
            if case.n_pix >= 100:
                below = lr < TC.BAND[0]
                assert (below & (I["g"] > 0)).any() and (below & (I["g"] < 0)).any(), cid
            if case.n_pix >= 100 and case.C >= 5:
                assert band.sum() >= 1 and (I["params"] > 20).sum() == 1, cid
            for p in placed["zero_pix"]:
                c = placed["odd_channel"]
                assert I["z"][c, p] + I["noise"][c, p] == 0
                assert ref["dz"].ref64[c, p] == 0 and ref["dz"].ref32[c, p] == 0 and ref["lik"].ref32[c, p] == np.float32(1e-9)
        if case.fam == "leaky":
            e = placed["edges"]
            assert list(np.signbit(I["in0"][e])) == [False, True, False, True] and list(np.abs(I["in0"][e])) == [0, 0, TC.TINY, TC.TINY]
            r, g = TC.reference(cid)["out0"].ref32.reshape(-1), I["in1"]
            assert [r[i] == g[i] for i in e] == [False, False, True, False]              # only act > 0 passes whole
            assert all(r[i] == np.float32(0.01) * g[i] for i in (e[0], e[1], e[3]))
        if case.fam == "ew" and case.op == "CLAMP_BWD":
            e = placed["edges"]
            r, g = TC.reference(cid)["out0"].ref32.reshape(-1), I["in1"]
            assert [r[i] == g[i] for i in e] == [False, False, True, True, False, True] and r[e[0]] == 0 and r[e[1]] == 0


def test_eb_zero_pixels_contribute_nothing():
    """The channel with zero biases is an odd function in fp32 and in float64: at z + noise == 0 the two logits cancel exactly,
    sign = 0, and the pixel adds exactly 0 to every parameter gradient — in the kernel's summation order dparams with and without
    those pixels are bit-equal (that dz is exactly 0 there, in both precisions, is asserted with the decision points)."""
    cid = "eb-C5-N129-ld5"
    I, placed = TC.inputs(cid)
    C, N, nz = 5, 129, TC.EB_ZERO_PIX
    assert placed["zero_pix"] == list(range(N - nz, N))
    P = TC.eb_split(I["params"], C)
    for mode in ("f32",):                                         # the kernel's summation order (float64 sums pairwise: another tree per length)
        full = TC.eb_body(TC.Tape(mode), P, I["z"], I["noise"], I["g"])["dparams"]
        cut = TC.eb_body(TC.Tape(mode), P, I["z"][:, :N - nz], I["noise"][:, :N - nz], I["g"][:, :N - nz])["dparams"]
        c = placed["odd_channel"]
        for key in TC.eb_keys():
            a, b = full[key].numpy()[c], cut[key].numpy()[c]
            assert a == b and np.signbit(a) == np.signbit(b), (mode, key, a, b)


# ------------------------------------------------------------------------------------------------ wrong formulas
def _factor(ref, wrong, K):
    return ref.ratio(np.asarray(wrong, dtype=np.float64).reshape(ref.ref64.shape))[0] / K


def test_wrong_formulas_fall_outside_the_bound():
    """Each mutant is evaluated in float64 on the contract's inputs; its worst element must miss the GPU's acceptance bound
    (K = max(4 K_cpu, 8)) by the printed factor.  For exact operations the float32 mutant must differ in bits."""
    found = {}
    g64 = lambda cid, bwd, **kw: {k: TC.expand(TC.CASES[cid], v.numpy()) for k, v in
                                  TC.gauss_body(TC.Tape("f64"), TC._gauss_in(TC.Tape("f64"), _pat(cid), ("y", "y2", "mu", "sigma", "mask", "noise", "g")), bwd, **kw).items()}
    cid = "gauss-y21-m1-C36"
    ref = TC.reference(cid)
    found["dsigma without the mask factor"] = _factor(ref["dsigma"], g64(cid, True, mut=("no_mask_dsigma",))["dsigma"], TC.k_of("gauss_train", "dsigma"))
    found["scale rule on sigma instead of sigma * m"] = _factor(ref["dsigma"], g64(cid, True, mut=("scale_on_sigma",))["dsigma"], TC.k_of("gauss_train", "dsigma"))
    I = _pat(cid)
    found["dmu without the mask factor"] = _factor(ref["dmu"], np.where(TC.expand(TC.CASES[cid], I["mask"]) == 0.5, 2, 1) * ref["dmu"].ref64, TC.k_of("gauss_train", "dmu"))
    found["likelihood clamped without LowerBound's pass-through (g < 0 dropped)"] = _factor(
        ref["dmu"], np.where(TC.reference(cid)["lik"].ref64 <= TC.BOUND_L, 0.0, ref["dmu"].ref64), TC.k_of("gauss_train", "dmu"))
    equiv = g64(cid, True, mut=("lb_le",))
    # `g <= 0` for `g < 0` in LowerBound's rule changes no value: the rule multiplies by g, and g = 0 gives 0 either way
    assert np.array_equal(equiv["dmu"], ref["dmu"].ref64) and np.array_equal(equiv["dsigma"], ref["dsigma"].ref64)

    def ew_mut(cid, wrong_outs, exact=False):
        ref = TC.reference(cid)
        out = 0.0
        for k, w in wrong_outs.items():
            r = ref[f"out{k}"]
            w = TC.expand(TC.CASES[cid], np.asarray(w))
            if exact:
                out = max(out, float((TC.bits(w) != TC.bits(r.ref32)).sum()))
            else:
                out = max(out, _factor(r, w, TC.k_of(TC.CASES[cid].op, f"out{k}")))
        return out

    I = _pat("ew-HTANH_BWD-f0-C36")
    found["HTANH_BWD without the 0.5"] = ew_mut("ew-HTANH_BWD-f0-C36", {0: 2 * _ew64("HTANH_BWD", [I["in0"], I["in1"]])[0]})
    I = _pat("ew-GATE_BWD-f0-C36")
    s = 1 / (1 + np.exp(-I["in1"].astype(np.float64)))
    found["GATE_BWD with s for s (1 - s)"] = ew_mut("ew-GATE_BWD-f0-C36", {1: I["in2"].astype(np.float64) * I["in0"] * s})
    I = _pat("ew-GDN_BWD_PREP-f0-C36")
    T = TC.Tape("f32")
    swapped = TC.ew_body(T, TC.EW_GDN_BWD_PREP, [T.inp(I[f"in{k}"]) for k in range(3)], flag=1)
    found["GDN_BWD_PREP with the flag branches swapped (elements that differ in bits)"] = ew_mut(
        "ew-GDN_BWD_PREP-f0-C36", {0: swapped[0].numpy(), 1: swapped[1].numpy()}, exact=True)
    I = _pat("ew-REPARAM_BWD-f0-C36")
    T = TC.Tape("f32")
    p, g = T.inp(I["in0"]), T.inp(I["in1"])
    go = (g * 2.0) * torch.clamp_min(p, TC.REPARAM_BOUND)
    found["LowerBound with p > bound for p >= bound (elements that differ in bits)"] = ew_mut(
        "ew-REPARAM_BWD-f0-C36", {0: torch.where((p > TC.REPARAM_BOUND) | (go < 0), go, torch.zeros_like(go)).numpy()}, exact=True)
    I = _pat("ew-CLAMP_BWD-f0-C36")
    found["CLAMP_BWD passing at the edges (elements that differ in bits)"] = ew_mut(
        "ew-CLAMP_BWD-f0-C36", {0: np.where((I["in0"] >= 0) & (I["in0"] <= 1), I["in1"], 0)}, exact=True)
    src = TC.inputs("ps2-Cq3")[0]["src"]
    found["ps2 channel order c*4 + j*2 + i (elements that differ in bits)"] = float(
        (TC.bits(TC.ps2_unshuffle_ref(src, mut=("ji",))) != TC.bits(TC.reference("ps2-Cq3")["dst"].ref32)).sum())
    src = TC.inputs("up2-C8")[0]["src"]
    found["upsample2_zero sampling at odd positions (elements that differ in bits)"] = float(
        (TC.bits(TC.upsample2_zero_ref(src, mut=("odd",))) != TC.bits(TC.reference("up2-C8")["dst"].ref32)).sum())
    cid = "eb-C5-N129-ld5"
    I, ref = _pat(cid), TC.reference(cid)
    for name, mut in (("eb sign not detached (straight-through)", "sign_attached"), ("eb tanh' of the factor from the raw value", "tanh_raw")):
        o = TC.eb_body(TC.Tape("f64"), TC.eb_split(I["params"], 5), I["z"], I["noise"], I["g"], mut=(mut,))
        f = _factor(ref["dparams"], TC.eb_flat({k: v.numpy() for k, v in o["dparams"].items()}, 5, np.float64), TC.k_of("eb_train_bwd", "dparams"))
        found[name] = max(f, _factor(ref["dz"], o["dz"].numpy(), TC.k_of("eb_train_bwd", "dz")))
    for name, f in found.items():
        print(f"wrong formula: {name}: outside by {f:.3g}")
        record_measurement("train_ew_contract wrong formula", formula=name, outside_by=float(f"{f:.3g}"))
    assert len(found) >= 10
    for name, f in found.items():
        assert f >= 1.0 if "differ in bits" in name else f > 1.0, (name, f)      # a count of elements, or a factor over the bound
