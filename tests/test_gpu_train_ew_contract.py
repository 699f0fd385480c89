"""The training element-wise and likelihood kernels (``vam_train_elementwise``, ``vam_train_axpy_group``, ``vam_leaky_bwd``,
``vam_mul``, ``vam_gauss_train``, ``vam_gauss_levels_fwd`` / ``_bwd``, ``vam_eb_forward_noise``, ``vam_eb_train_bwd``,
``vam_ps2_unshuffle``, ``vam_upsample2_zero``) against the float64 statement of their contract (tests/train_ew_contract.py).

Every case runs on channel windows [c0, c0 + C) of buffers with another pitch per operand; everything outside an input
window is NaN, everything outside an output window (one guard pixel row before and after included) is a sentinel that must
survive bit for bit.  Budgeted operations must meet |got - ref64| <= K 2^-24 A + 2^-126 with K = max(4 K_cpu, 8), exact
operations must equal the float32 statement in bits, and a second launch must repeat the first in bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import ops, _lib as L        # noqa: E402
import train_ew_contract as TC            # noqa: E402
from conftest import record_measurement   # noqa: E402

NAN_BITS = 0x7FC00000
WORST = {}                                # (operation, output) -> worst GPU ratio; "exact" for bit-equal operations


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A launch that faulted leaves a context in which nothing that follows means anything: end the session there."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


class Slot:
    """One operand: a [B, H, W, ld] buffer with a guard pixel row on either side, the window [c0, c0 + C) of it as a View."""

    def __init__(self, shape, C, ld, c0, data=None, levels=1):
        B, H, W = shape
        self.n, self.G, self.ld, self.c0, self.C = levels * B * H * W, W, ld, c0, C
        fill = NAN_BITS if data is not None else TC.SENTINEL_BITS
        host = np.full((self.n + 2 * self.G, ld), fill, dtype=np.int32)
        if data is not None:
            host[self.G:self.G + self.n, c0:c0 + C] = TC.bits(np.asarray(data, dtype=np.float32).reshape(self.n, C))
        self.before = host
        self.dev = torch.from_numpy(host.copy()).cuda().view(torch.float32)
        self.view = ops.View(self.dev[self.G:self.G + self.n].view(levels * B, H, W, ld), c0, C)

    def window(self, c0, C):
        return ops.View(self.view.buf, self.c0 + c0, C)

    def read(self, c0=None, C=None):
        """the window as float32 [n, C], after checking that nothing outside [c0, c0 + C) of this buffer changed"""
        c0 = self.c0 if c0 is None else c0
        C = self.C if C is None else C
        after = self.dev.cpu().view(torch.int32).numpy()
        mask = np.ones(after.shape, dtype=bool)
        mask[self.G:self.G + self.n, c0:c0 + C] = False
        assert np.array_equal(after[mask], self.before[mask]), "a launch wrote outside its output window"
        return after[self.G:self.G + self.n, c0:c0 + C].copy().view(np.float32)

    def untouched(self):
        assert np.array_equal(self.dev.cpu().view(torch.int32).numpy(), self.before), "a launch wrote to an input buffer"


def _judge(case, name, got, ref, what=None):
    """the bound or bit-equality for one output; got in the reference's shape"""
    key = (case.op, what or name)
    got = np.asarray(got).reshape(ref.ref64.shape)
    assert np.isfinite(got).all(), (case.id, name, "not finite inside the window")
    if ref.exact:
        diff = TC.bits(got) != TC.bits(ref.ref32)
        WORST[key] = "exact" if not diff.any() and WORST.get(key, "exact") == "exact" else "differs"
        assert not diff.any(), (case.id, name, int(diff.sum()), got[diff][:4], ref.ref32[diff][:4])
        return
    kname = what or name
    if case.fam == "ew" and case.op.startswith("GDN"):
        kname = f"{name}/flag{case.o('flag')}"
    K = TC.k_of(case.op, kname)
    rat, i = ref.ratio(got)
    print(f"{case.id} {name}: GPU ratio {rat:.3f} (K_cpu {TC.k_cpu(case.op).get(kname, 0.0):.3f}, K {K:.1f})")
    WORST[key] = max(WORST.get(key, 0.0), rat)
    assert rat <= K, (case.id, name, rat, K, i, got.reshape(-1)[i], ref.ref64.reshape(-1)[i], ref.A.reshape(-1)[i])


def _slots(case, arrays, outs, levels=None):
    """inputs and outputs of an element-wise case as Slots, pitches and offsets by TC.layout"""
    S = {}
    for k, (name, a) in enumerate(arrays.items()):
        ld, c0 = TC.layout(case, k)
        S[name] = Slot(case.shape, case.C, ld, c0, a, levels=(levels or {}).get(name, 1))
    for k, name in enumerate(outs):
        ld, c0 = TC.layout(case, len(arrays) + k)
        S[name] = Slot(case.shape, case.C, ld, c0, None, levels=(levels or {}).get(name, 1))
    return S


def _twice(run):
    """run() -> dict of float32 arrays; the second launch (fresh buffers) must repeat the first bit for bit"""
    a, b = run(), run()
    for k in a:
        assert np.array_equal(TC.bits(a[k]), TC.bits(b[k])), (k, "a second launch differs")
    return a


# ---------------------------------------------------------------------------------------------------------------- ew family
def _run_ew(case, flag=None):
    I = TC.inputs(case.id)[0]
    code, n_in, n_out = TC.EW_OPS[case.op]
    coef = TC.AXPY_COEF if case.op == "AXPY" else (TC.REPARAM_BOUND if case.op == "REPARAM_BWD" else 0.0)
    arrays = {f"in{k}": TC.expand(case, I[f"in{k}"]) for k in range(n_in)}
    inplace = case.op == "AXPY"                                  # the plans accumulate with out == in0
    S = _slots(case, arrays, [] if inplace else [f"out{k}" for k in range(n_out)])
    ins = [S[f"in{k}"].view for k in range(n_in)]
    outs = [S["in0"].view] if inplace else [S[f"out{k}"].view for k in range(n_out)]
    ops.ew(code, ins, outs, coef=coef, flag=case.o("flag") if flag is None else flag)
    torch.cuda.synchronize()
    res = {f"out{k}": (S["in0"] if inplace else S[f"out{k}"]).read() for k in range(n_out)}
    for k in range(1 if inplace else 0, n_in):
        S[f"in{k}"].untouched()
    return res


@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam == "ew"])
def test_elementwise(cid):
    case = TC.CASES[cid]
    got = _twice(lambda: _run_ew(case))
    ref = TC.reference(cid)
    for name in ref:
        _judge(case, name, got[name], ref[name])
    if case.op == "GDN_BWD_FIN":                                 # the op does not read the flag
        other = _run_ew(case, flag=1 - case.o("flag"))
        assert np.array_equal(TC.bits(other["out0"]), TC.bits(got["out0"]))


# ---------------------------------------------------------------------------------------------------------------- axpy group
def _run_axpy(case):
    I = TC.inputs(case.id)[0]
    n = case.o("jobs")
    S, updates = {}, []
    for j in range(n):
        sub = case if j == 0 else TC.Case("-", "axpy", "axpy_group", TC.BASE, 8)
        for k, nm in enumerate((f"a{j}", f"b{j}")):
            ld, c0 = TC.layout(sub, 2 * j + k)
            S[nm] = Slot(sub.shape, sub.C, ld, c0, TC.expand(sub, I[nm]))
        updates.append((S[f"a{j}"].view, S[f"b{j}"].view, float(np.float32(0.5 * (j + 1) * (-1) ** j))))
    ops.axpy_group(ops.axpy_jobs(updates))
    torch.cuda.synchronize()
    for j in range(n):
        S[f"b{j}"].untouched()
    return {f"a{j}": S[f"a{j}"].read() for j in range(n)}


@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam == "axpy"])
def test_axpy_group(cid):
    case = TC.CASES[cid]
    got = _twice(lambda: _run_axpy(case))
    for name, ref in TC.reference(cid).items():
        _judge(case, name, got[name], ref, what="out")


# ---------------------------------------------------------------------------------------------------------------- leaky, mul
@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam in ("leaky", "mul")])
def test_leaky_bwd_and_mul(cid):
    case = TC.CASES[cid]
    I = TC.inputs(cid)[0]

    def run():
        S = _slots(case, {k: TC.expand(case, I[k]) for k in ("in0", "in1")}, ["out0"])
        (ops.leaky_bwd if case.fam == "leaky" else ops.mul)(S["in0"].view, S["in1"].view, S["out0"].view)
        torch.cuda.synchronize()
        S["in0"].untouched(), S["in1"].untouched()
        return {"out0": S["out0"].read()}
    got = _twice(run)
    _judge(case, "out0", got["out0"], TC.reference(cid)["out0"])


# ---------------------------------------------------------------------------------------------------------------- likelihood
def _check_gauss_decisions(case, got):
    """decisions taken on input values, exactly: dmu = 0 at v == 0; below the likelihood bound a non-negative gradient gives
    exactly 0 for both; the scale bound stops at one ulp below 0.11f and not at 0.11f"""
    I, placed = TC.inputs(case.id)
    q = TC._n_unique(case)
    at = lambda a, idx: np.asarray(a).reshape(-1)[:q][idx]
    g = I["g"].reshape(-1)[:q]
    v0 = placed["v0_m1"] + placed.get("v0_m0", [])
    assert (at(got["dmu"], v0) == 0).all(), (case.id, "dmu at v == 0", at(got["dmu"], v0))
    far = [i for i in placed["far_below"] + placed["below"] if g[i] >= 0]
    assert (at(got["dmu"], far) == 0).all() and (at(got["dsigma"], far) == 0).all(), (case.id, "below the likelihood bound, g >= 0")
    thru = [i for i in placed["below"] if g[i] < 0]
    assert (at(got["dmu"], thru) != 0).all(), (case.id, "below the likelihood bound, g < 0 passes")
    stop = [i for i in placed["s_below"] if g[i] < 0]
    go = [i for i in placed["s_below"] if g[i] > 0] + placed["s_at"]
    assert (at(got["dsigma"], stop) == 0).all() and (at(got["dsigma"], go) != 0).all(), (case.id, "scale bound")
    if "s_half" in placed:
        stop = [i for i in placed["s_half"] + placed["s_m0"] if g[i] < 0]
        assert (at(got["dsigma"], stop) == 0).all(), (case.id, "scale bound on sigma * m")


def _run_gauss(case):
    I = TC.inputs(case.id)[0]
    names = [n for n in ("y", "y2", "mu", "sigma", "mask", "noise", "g") if n in I]
    S = _slots(case, {n: TC.expand(case, I[n]) for n in names}, ["lik", "dmu", "dsigma"])
    kw = {k: S[k].view for k in ("y2", "mask") if k in S}
    ops.gauss_train(S["y"].view, S["mu"].view, S["sigma"].view, S["noise"].view, lik=S["lik"].view, **kw)
    ops.gauss_train(S["y"].view, S["mu"].view, S["sigma"].view, S["noise"].view, grad_lik=S["g"].view, dmu=S["dmu"].view,
                    dsigma=S["dsigma"].view, **kw)
    torch.cuda.synchronize()
    for n in names:
        S[n].untouched()
    return {k: S[k].read() for k in ("lik", "dmu", "dsigma")}


@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam == "gauss"])
def test_gauss_train(cid):
    case = TC.CASES[cid]
    got = _twice(lambda: _run_gauss(case))
    ref = TC.reference(cid)
    for name in ("lik", "dmu", "dsigma"):
        _judge(case, name, got[name], ref[name])
    _check_gauss_decisions(case, got)


def _run_levels(case, fused=True):
    """the fused launches, or — fused=False — the per-level gauss_tail / gauss_train / MASK_SPLIT / AXPY sequence on the same
    windowed layout (what the plans ran before the fusion, and what the fused kernel must repeat bit for bit)"""
    I = TC.inputs(case.id)[0]
    Lv, C = case.o("levels"), case.C
    chan = bool(case.o("y2"))                 # noise / lik / grad_lik: consecutive channel blocks (y2 cases) or image blocks
    ex = lambda n: TC.expand(case, I[n])
    shared = {n: ex(n) for n in ("y", "y2", "mu", "sigma", "dyt", "dys") if n in I}
    per = {n: ex(n) for n in ("mask", "noise", "g", "drq")}
    S, k = {}, 0
    for n, a in shared.items():
        ld, c0 = TC.layout(case, k)
        S[n] = Slot(case.shape, C, ld, c0, a)
        k += 1
    for n in ("mask", "noise", "g", "drq", "rq", "lik"):
        ld, c0 = TC.layout(case, k)
        k += 1
        a = per.get(n)
        if chan and n in ("noise", "g", "lik"):
            data = None if a is None else a.transpose(1, 0, 2).reshape(case.n_pix, Lv * C)
            S[n] = Slot(case.shape, Lv * C, ld + (Lv - 1) * C, c0, data)
        else:
            S[n] = Slot(case.shape, C, ld, c0, a, levels=Lv)
    for n in ("gmu", "dsigma"):
        ld, c0 = TC.layout(case, k)
        k += 1
        S[n] = Slot(case.shape, C, ld, c0, None)
    V = lambda n: S[n].view if n in S else None
    lvl = lambda n, l: S[n].window(l * C, C) if chan and n in ("noise", "g", "lik") else \
        ops.View(S[n].view.buf[l * case.shape[0]:(l + 1) * case.shape[0]], S[n].c0, C)
    first = lambda n: S[n].window(0, C) if chan and n in ("noise", "g", "lik") else S[n].view
    ls = dict(noise_ls=C) if chan else {}
    if fused:
        ops.gauss_levels_fwd(V("y"), V("mu"), V("sigma"), V("mask"), first("noise"), V("rq"), first("lik"), Lv, y2=V("y2"),
                             **ls, **(dict(lik_ls=C) if chan else {}))
        ops.gauss_levels_bwd(V("y"), V("mu"), V("sigma"), V("mask"), first("noise"), first("g"), V("drq"), V("gmu"), V("dsigma"),
                             V("dyt"), Lv, y2=V("y2"), dy_sub=V("dys"), **ls, **(dict(glik_ls=C) if chan else {}))
    else:
        B, H, W = case.shape
        tmp = lambda zero=False: ops.new_view(B, H, W, C, zero=zero)
        G_t, S_t = tmp(True), tmp(True)
        for l in range(Lv):
            m, junk, dmu_l, dsg_l, d_r, G = lvl("mask", l), tmp(), tmp(), tmp(), tmp(), tmp()
            ops.gauss_tail(V("y"), V("mu"), V("sigma"), y2=V("y2"), mask=m, yhat=lvl("rq", l), lik=junk)
            ops.gauss_train(V("y"), V("mu"), V("sigma"), lvl("noise", l), y2=V("y2"), mask=m, lik=lvl("lik", l))
            ops.gauss_train(V("y"), V("mu"), V("sigma"), lvl("noise", l), y2=V("y2"), mask=m, grad_lik=lvl("g", l), dmu=dmu_l, dsigma=dsg_l)
            ops.ew(L.EW_MASK_SPLIT, [lvl("drq", l), m], [d_r, G])
            ops.ew(L.EW_AXPY, [G, dmu_l], [G], coef=1.0)
            ops.ew(L.EW_AXPY, [d_r, dmu_l], [d_r], coef=-1.0)
            ops.ew(L.EW_AXPY, [V("dyt"), d_r], [V("dyt")], coef=1.0)
            if "dys" in S:
                ops.ew(L.EW_AXPY, [V("dys"), d_r], [V("dys")], coef=-1.0)
            ops.ew(L.EW_AXPY, [G_t, G], [G_t], coef=1.0)
            ops.ew(L.EW_AXPY, [S_t, dsg_l], [S_t], coef=1.0)
        ops.ew(L.EW_AXPY, [G_t, G_t], [V("gmu")], coef=0.0)
        ops.ew(L.EW_AXPY, [S_t, S_t], [V("dsigma")], coef=0.0)
    torch.cuda.synchronize()
    for n in ("y", "y2", "mu", "sigma", "mask", "noise", "g", "drq"):
        if n in S:
            S[n].untouched()
    out = {n: S[n].read() for n in ("gmu", "dsigma", "dyt", "dys") if n in S}
    for n in ("rq", "lik"):
        a = S[n].read()
        out[n] = a.reshape(case.n_pix, Lv, C).transpose(1, 0, 2) if (chan and n == "lik") else a.reshape(Lv, case.n_pix, C)
    return out


@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam == "levels"])
def test_gauss_levels(cid):
    case = TC.CASES[cid]
    got = _twice(lambda: _run_levels(case))
    ref = TC.reference(cid)
    for name in ref:
        _judge(case, name, got[name], ref[name])
    unfused = _run_levels(case, fused=False)
    for name in got:
        assert np.array_equal(TC.bits(unfused[name]), TC.bits(got[name])), (cid, name, "the fused launch differs from the per-level sequence")


# ---------------------------------------------------------------------------------------------------------------- bottleneck
def _run_eb(case, n_pix=None):
    I = TC.inputs(case.id)[0]
    C, N = case.C, n_pix or case.n_pix
    shape = (1, 1, N)
    params = torch.from_numpy(I["params"].copy()).cuda()
    arrays = {n: np.ascontiguousarray(I[n][:, :N].T) for n in ("z", "noise", "g")}     # [N, C]
    S = {}
    for k, n in enumerate(("z", "noise", "g", "lik", "dz")):
        ld, c0 = TC.layout(case, k)
        S[n] = Slot(shape, C, ld, c0, arrays.get(n))
    dpar = torch.from_numpy(np.full(params.numel(), TC.SENTINEL_BITS, dtype=np.int32)).cuda().view(torch.float32)
    ops.eb_forward(S["z"].view, params, None, S["lik"].view, noise=S["noise"].view)
    ops.eb_train_bwd(S["z"].view, S["noise"].view, params, S["g"].view, S["dz"].view, dpar)
    torch.cuda.synchronize()
    for n in ("z", "noise", "g"):
        S[n].untouched()
    assert np.array_equal(params.cpu().numpy(), I["params"])
    return {"lik": S["lik"].read().T, "dz": S["dz"].read().T, "dparams": dpar.cpu().numpy()}


@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam == "eb"])
def test_entropy_bottleneck(cid):
    case = TC.CASES[cid]
    I, placed = TC.inputs(cid)
    got = _twice(lambda: _run_eb(case))
    ref = TC.reference(cid)
    for name in ("lik", "dz", "dparams"):
        _judge(case, name, got[name], ref[name])
    C = case.C
    assert np.all(TC.bits(got["dparams"][-3 * C:]) == 0), "the quantile gradient is zeroed"
    for c, p in placed.get("far_below", []):                      # clear-below: g >= 0 gives exactly 0, g < 0 passes
        if I["g"][c, p] >= 0:
            assert got["dz"][c, p] == 0 and got["lik"][c, p] == np.float32(1e-9)
    if placed["zero_pix"]:                                        # sign == 0: dz exactly 0, and exactly nothing added to any sum
        c = placed["odd_channel"]
        assert (got["dz"][c, placed["zero_pix"]] == 0).all() and (got["lik"][c, placed["zero_pix"]] == np.float32(1e-9)).all()
        cut = _run_eb(case, n_pix=case.n_pix - TC.EB_ZERO_PIX)
        idx = np.concatenate([o + np.arange(c * n, (c + 1) * n) for o, n in _eb_offsets(C)])
        assert np.array_equal(TC.bits(cut["dparams"][idx]), TC.bits(got["dparams"][idx])), "pixels with sign == 0 changed a parameter gradient"


def _eb_offsets(C):
    out, o = [], 0
    for shp in TC.EB_SHAPES[:14]:
        n = shp[0] * shp[1]
        out.append((o, n))
        o += C * n
    return out


# ---------------------------------------------------------------------------------------------------------------- layout kernels
@pytest.mark.parametrize("cid", [c for c, v in TC.CASES.items() if v.fam in ("ps2", "up2")])
def test_layout_kernels(cid):
    case = TC.CASES[cid]
    src = TC.inputs(cid)[0]["src"]
    B, H, W = case.shape

    def run():
        if case.fam == "ps2":
            s = Slot((B, 2 * H, 2 * W), case.C, case.C + 5, 3, src)               # scalar loads: no alignment asked
            d = Slot((B, H, W), 4 * case.C, 4 * case.C + 7, 2, None)
            ops.ps2_unshuffle(s.view, d.view)
        else:
            s = Slot((B, H, W), case.C, case.C + 12, 4, src)
            d = Slot((B, 2 * H, 2 * W), case.C, case.C + 8, 8, None)
            ops.upsample2_zero(s.view, d.view)
        torch.cuda.synchronize()
        s.untouched()
        return {"dst": d.read()}
    got = _twice(run)
    _judge(case, "dst", got["dst"], TC.reference(cid)["dst"])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_message():
    def buf(C, ld=None, c0=0):
        return ops.View(torch.zeros(1, 2, 2, ld or C + c0, device="cuda"), c0, C)
    ok = buf(8)
    with pytest.raises(L.VamError, match="vam_train_elementwise: bad arguments"):
        ops.ew(L.EW_AXPY, [buf(6, 8), buf(6, 8)], [buf(6, 8)])                   # C % 4 != 0
    with pytest.raises(L.VamError, match="vam_train_elementwise: input 1 alignment"):
        ops.ew(L.EW_AXPY, [ok, buf(8, 12, 1)], [ok])                             # a pointer off the 16-byte grid
    with pytest.raises(L.VamError, match="vam_train_elementwise: output 0 alignment"):
        ops.ew(L.EW_AXPY, [ok, ok], [buf(8, 10)])                                # ld % 4 != 0
    with pytest.raises(L.VamError, match="vam_train_elementwise: op 2 needs 3 inputs"):
        ops.ew(L.EW_GATE_BWD, [ok, ok], [ok, ok])
    with pytest.raises(L.VamError, match="vam_train_elementwise: op 4 needs 3 outputs"):
        ops.ew(L.EW_GDN_BWD_PREP, [ok, ok, ok], [ok, ok])
    with pytest.raises(L.VamError, match="vam_train_elementwise: op 13"):
        ops.ew(13, [ok, ok], [ok])
    with pytest.raises(L.VamError, match="vam_train_elementwise: op -1"):
        ops.ew(-1, [ok, ok], [ok])
    arr = (L.VamEw * 9)()
    for e in arr:
        e.inp[0].ptr, e.inp[0].ld, e.inp[1].ptr, e.inp[1].ld, e.out[0].ptr, e.out[0].ld = ok.ptr, ok.ld, ok.ptr, ok.ld, ok.ptr, ok.ld
        e.n_pix, e.C = ok.n_pix, ok.C
    with pytest.raises(L.VamError, match=r"vam_train_axpy_group: 1 \.\. 8 jobs"):
        L.check(L.load().vam_train_axpy_group(arr, 9, ops.stream_ptr()), "vam_train_axpy_group")
    with pytest.raises(L.VamError, match="vam_train_axpy_group: job 0 alignment"):
        ops.axpy_group(ops.axpy_jobs([(buf(8, 12, 1), buf(8, 12, 1), 1.0)]))
    with pytest.raises(L.VamError, match="vam_train_axpy_group: job 0 row pitches"):
        ops.axpy_group(ops.axpy_jobs([(buf(8, 10), buf(8, 10), 1.0)]))
    for fn, name in ((ops.leaky_bwd, "vam_leaky_bwd"), (ops.mul, "vam_mul")):
        for bad in (buf(6, 8), buf(8, 12, 1), buf(8, 10)):
            with pytest.raises(L.VamError, match=f"{name}: bad arguments"):
                fn(bad, bad, bad)
    with pytest.raises(L.VamError, match="vam_gauss_train: bad arguments"):
        ops.gauss_train(buf(6, 8), buf(6, 8), buf(6, 8), buf(6, 8), lik=buf(6, 8))
    with pytest.raises(L.VamError, match="vam_gauss_train: alignment"):
        ops.gauss_train(ok, ok, buf(8, 12, 1), ok, lik=ok)
    with pytest.raises(L.VamError, match="vam_gauss_train: strides"):
        ops.gauss_train(ok, ok, ok, buf(8, 10), lik=ok)
    with pytest.raises(L.VamError, match="vam_gauss_train: forward needs lik, backward needs dmu and dsigma"):
        ops.gauss_train(ok, ok, ok, ok, grad_lik=ok, dmu=ok)
    with pytest.raises(L.VamError, match="vam_upsample2_zero: alignment"):
        ops.upsample2_zero(buf(8, 12, 1), ops.View(torch.zeros(1, 4, 4, 8, device="cuda"), 0, 8))
    torch.cuda.synchronize()


def test_zz_report_measured_ratios():
    """The worst GPU ratio per operation and output next to K_cpu (what DESIGN.md quotes), and which exact operations were bit-equal."""
    assert WORST, "run after the cases of this file"
    for (op, name), v in sorted(WORST.items()):
        k = TC.k_cpu(op).get(name)
        record_measurement(f"train_ew_contract GPU {op} {name}", gpu=v if isinstance(v, str) else round(v, 3),
                           k_cpu=None if k is None else round(k, 3))
