"""The inference likelihood and rate kernels (``vam_gauss_tail``, ``vam_gauss_levels_eval``, ``vam_gauss_levels_decode``,
``vam_gauss_layer_bits``, ``vam_build_indexes``, the evaluation path of ``vam_eb_forward``) against the float64 statement of
their contract (tests/entropy_contract.py), through the ``ops`` wrappers only.

Every operand is a channel window [c0, c0 + C) of its own wider buffer with its own pitch; everything outside an input
window is NaN (0xEE for layer ids), everything outside an output window (one guard pixel row before and after included) is
a sentinel that must survive bit for bit.  Exact outputs (yhat, zhat, symbols, indexes, decoded yhat, counts) equal the
emulated float32 chain in bits; likelihoods meet |got - ref64| <= K 2^-24 A + 2^-126 and the same bound in bits, with
K = max(4 K_cpu, 8); a second launch repeats the first in bits.

The float64 sums (``log2sum`` of gauss_tail, gauss_levels_eval and eb_forward, ``bits`` of gauss_layer_bits) are the one
exception to that repetition: they are accumulated with float64 atomics (wave partial sums, LDS bins, one atomic per
element in eb_forward) whose order is not fixed, so two launches may differ in the last bits.  They are held to 1e-12 of
the sum of |term| against the float64 sum of log2 of the launch's own fp32 likelihoods instead, and — in the cases without
an in-band element — to the float64 reference within the summed per-element bounds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import ops, _lib as L         # noqa: E402
import entropy_contract as EC             # noqa: E402
from conftest import record_measurement   # noqa: E402

NAN_BITS = 0x7FC00000
WORST = {}                                # (kernel, output) -> worst ratio / "exact"; (kernel, output, "bits") -> worst error in bits


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A launch that faulted leaves a context in which nothing that follows means anything: end the session there."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


class Slot:
    """One operand: a [levels * B, H, W, ld] buffer of 32-bit words with a guard pixel row on either side, the window
    [c0, c0 + C) of it as a View (kind "f32") or an IView (kind "i32")."""

    def __init__(self, shape, C, ld, c0, data=None, levels=1, kind="f32"):
        B, H, W = shape
        self.n, self.G, self.ld, self.c0, self.C, self.kind = levels * B * H * W, W, ld, c0, C, kind
        host = np.full((self.n + 2 * self.G, ld), NAN_BITS if data is not None else EC.SENTINEL_BITS, dtype=np.int32)
        if data is not None:
            a = np.asarray(data)
            host[self.G:self.G + self.n, c0:c0 + C] = (EC.bits(a) if kind == "f32" else a.astype(np.int32)).reshape(self.n, C)
        self.before = host
        self.dev = torch.from_numpy(host.copy()).cuda()
        typed = self.dev.view(torch.float32) if kind == "f32" else self.dev
        body = typed[self.G:self.G + self.n].view(levels * B, H, W, ld)
        self.view = ops.View(body, c0, C) if kind == "f32" else ops.IView(body, c0, C)

    def level(self, l, B):
        """level l's image block as a window of its own (what a per-level launch is handed)"""
        cls = ops.View if self.kind == "f32" else ops.IView
        return cls(self.view.buf[l * B:(l + 1) * B], self.c0, self.C)

    def read(self):
        """the window [n, C], after checking that nothing outside it changed"""
        after = self.dev.cpu().numpy()
        mask = np.ones(after.shape, dtype=bool)
        mask[self.G:self.G + self.n, self.c0:self.c0 + self.C] = False
        assert np.array_equal(after[mask], self.before[mask]), "a launch wrote outside its output window"
        w = after[self.G:self.G + self.n, self.c0:self.c0 + self.C].copy()
        return w.view(np.float32) if self.kind == "f32" else w

    def untouched(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.before), "a launch wrote to an input buffer"


class Sums:
    """a float64 (or int64) accumulator row, zeroed, with sentinels behind it"""

    def __init__(self, n, dtype=torch.float64):
        self.n = n
        self.full = torch.zeros(n + 4, dtype=dtype)
        self.full[n:] = -12345
        self.full = self.full.cuda()
        self.t = self.full[:n]

    def read(self):
        a = self.full.cpu().numpy()
        assert (a[self.n:] == -12345).all(), "a launch wrote behind its sums"
        return a[:self.n].copy()


class Layer:
    """uint8 layer ids [B, H, W, ld] with guard rows; 0xEE outside the window"""

    def __init__(self, case, data, ld=None, c0=0):
        B, H, W = case.shape
        C = case.C
        ld = C if ld is None else ld
        self.n, self.G = case.n_pix, W
        host = np.full((self.n + 2 * self.G, ld), 0xEE, dtype=np.uint8)
        host[self.G:self.G + self.n, c0:c0 + C] = np.asarray(data, dtype=np.uint8).reshape(self.n, C)
        self.before = host
        self.dev = torch.from_numpy(host.copy()).cuda()
        body = self.dev[self.G:self.G + self.n]
        self.ld = ld
        self.t = body.view(B, H, W, ld) if ld == C else body[:, c0:c0 + C]     # contiguous, or the window's first element with a pitch

    def untouched(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.before), "a launch wrote to the layer ids"


def _twice(run):
    """run() -> dict of arrays; the second launch (fresh buffers) must repeat the first bit for bit, but for the float64 sums
    (keys "sum:...": atomics in no fixed order, see the module docstring)"""
    a, b = run(), run()
    for k in a:
        if k.startswith("sum:"):
            continue
        w = (lambda x: EC.bits(x)) if np.asarray(a[k]).dtype == np.float32 else (lambda x: np.asarray(x))
        assert np.array_equal(w(a[k]), w(b[k])), (k, "a second launch differs")
    return a


def _lik(kernel, what, got, ref):
    K = EC.k_of("eb" if kernel == "eb_forward" else "gauss")
    rat, berr = EC.judge_lik((kernel, what), got, ref, K)
    print(f"{kernel} {what}: GPU ratio {rat:.3f} (K {K:.1f}), worst {berr:.3g} bits")
    WORST[(kernel, "lik")] = max(WORST.get((kernel, "lik"), 0.0), rat)
    WORST[(kernel, "lik", "bits")] = max(WORST.get((kernel, "lik", "bits"), 0.0), berr)
    return K


def _exact(kernel, name, what, got, want):
    try:
        EC.judge_exact((kernel, name, what), got, want)
    except AssertionError:
        WORST[(kernel, name)] = "differs"
        raise
    WORST.setdefault((kernel, name), "exact")


def _sum(kernel, name, what, got, own, ref, K, groups, n_groups=None):
    w = EC.judge_sum((kernel, name, what), got, own, ref if ref is not None and not ref.band.any() else None, K, groups, n_groups)
    WORST[(kernel, name, "rel")] = max(WORST.get((kernel, name, "rel"), 0.0), w)


def _inputs(case, names, variant):
    I = EC.inputs(case.id)[0]
    S = {}
    for k, n in enumerate(names):
        a = I[n][0] if n == "mask" else I[n]
        if n == "mask" and variant == "ones":
            a = np.ones_like(I["sigma"])
        ld, c0 = EC.layout(case, k)
        S[n] = Slot(case.shape, case.C, ld, c0, EC.expand(case, a))
    return S


def _item_of(case, pix_per_item=None):
    """[n_pix, C]: the item of each element"""
    ppi = case.shape[1] * case.shape[2] if pix_per_item is None else pix_per_item
    return np.repeat(np.arange(case.n_pix) // ppi, case.C).reshape(case.n_pix, case.C)


# ---------------------------------------------------------------------------------------------------------------- gauss_tail
def _run_tail(case, variant, outs):
    masked, y2 = not variant.startswith("unmasked"), not variant.endswith("-noy2")
    names = ["y", "mu", "sigma"] + (["y2"] if y2 else []) + (["mask"] if masked else [])
    S = _inputs(case, names, variant.split("-")[0])
    k0 = len(names)
    O = {}
    for k, n in enumerate(n for n in ("yhat", "lik", "sym") if n in outs):
        ld, c0 = EC.layout(case, k0 + k)
        O[n] = Slot(case.shape, case.C, ld, c0, None, kind="i32" if n == "sym" else "f32")
    ls = Sums(case.shape[0]) if "log2sum" in outs else None
    ops.gauss_tail(S["y"].view, S["mu"].view, S["sigma"].view, y2=S["y2"].view if y2 else None,
                   mask=S["mask"].view if masked else None, yhat=O["yhat"].view if "yhat" in O else None,
                   lik=O["lik"].view if "lik" in O else None, sym=O["sym"].view if "sym" in O else None,
                   log2sum=ls.t if ls is not None else None)
    torch.cuda.synchronize()
    for s in S.values():
        s.untouched()
    res = {n: O[n].read() for n in O}
    if ls is not None:
        res["sum:log2sum"] = ls.read()
    return res


def _check_tail(case, variant, outs, got, own_lik=None):
    ref = EC.tail_reference(case.id, variant)
    what = f"{case.id} {variant} {'+'.join(outs)}"
    K = EC.k_of("gauss")
    if "yhat" in got:
        _exact("gauss_tail", "yhat", what, got["yhat"], ref["yhat"].ref32)
    if "sym" in got:
        _exact("gauss_tail", "sym", what, got["sym"], ref["sym"])
    if "lik" in got:
        _lik("gauss_tail", what, got["lik"], ref["lik"])
    if "sum:log2sum" in got:
        own = got["lik"] if "lik" in got else own_lik
        _sum("gauss_tail", "log2sum", what, got["sum:log2sum"], own, ref["lik"], K, _item_of(case))


TAIL_RUNS = [("t-min", "unmasked", ("yhat", "lik", "sym", "log2sum")), ("t-min", "masked", ("yhat", "lik", "sym", "log2sum")),
             ("t-mixed", "unmasked", ("lik", "log2sum")), ("t-mixed", "masked", ("yhat", "lik", "sym", "log2sum")),
             ("t-ragged", "unmasked", ("yhat", "lik", "sym", "log2sum")), ("t-ragged", "masked", ("yhat", "lik", "sym", "log2sum")),
             ("t-stride", "masked", ("yhat", "lik", "sym", "log2sum")),
             # t-opt: the argument sets of the plans (entropy_models.py, plans.py, full_train.py) and each output alone
             ("t-opt", "unmasked-noy2", ("yhat", "lik", "sym", "log2sum")), ("t-opt", "unmasked-noy2", ("yhat",)),
             ("t-opt", "unmasked-noy2", ("sym",)), ("t-opt", "unmasked-noy2", ("yhat", "lik")),
             ("t-opt", "masked", ("yhat", "lik")), ("t-opt", "masked", ("yhat", "lik", "sym", "log2sum")),
             ("t-opt", "unmasked", ("lik",)), ("t-opt", "masked-noy2", ("log2sum",))]


@pytest.mark.parametrize("cid,variant,outs", TAIL_RUNS, ids=[f"{c}-{v}-{'+'.join(o)}" for c, v, o in TAIL_RUNS])
def test_gauss_tail(cid, variant, outs):
    case = EC.CASES[cid]
    assert variant in EC.GAUSS_VARIANTS[cid]                       # K_cpu was measured on this chain
    got = _twice(lambda: _run_tail(case, variant, outs))
    own = None
    if "log2sum" in outs and "lik" not in outs:                     # the sum alone: its terms from a launch that writes them
        own = _run_tail(case, variant, ("lik",))["lik"]
    _check_tail(case, variant, outs, got, own)


# ---------------------------------------------------------------------------------------------------------------- gauss_levels_eval
def _run_eval(case, n_levels, outs=("yhat", "lik", "sym", "log2sum")):
    I = EC.inputs(case.id)[0]
    B = case.shape[0]
    S = _inputs(case, ["y", "mu", "sigma", "y2"], "levels")
    ld, c0 = EC.layout(case, 4)
    S["mask"] = Slot(case.shape, case.C, ld, c0, EC.expand(case, I["mask"][:n_levels]), levels=n_levels)
    O = {}
    for k, n in enumerate(n for n in ("yhat", "lik", "sym") if n in outs):
        ld, c0 = EC.layout(case, 5 + k)
        O[n] = Slot(case.shape, case.C, ld, c0, None, levels=n_levels, kind="i32" if n == "sym" else "f32")
    ls = Sums(n_levels * B) if "log2sum" in outs else None
    ops.gauss_levels_eval(S["y"].view, S["mu"].view, S["sigma"].view, S["mask"].view, n_levels, y2=S["y2"].view,
                          yhat=O["yhat"].view if "yhat" in O else None, lik=O["lik"].view if "lik" in O else None,
                          sym=O["sym"].view if "sym" in O else None, log2sum=ls.t.view(n_levels, B) if ls is not None else None)
    torch.cuda.synchronize()
    for s in S.values():
        s.untouched()
    res = {n: O[n].read().reshape(n_levels, case.n_pix, case.C) for n in O}
    if ls is not None:
        res["sum:log2sum"] = ls.read()
    return res


@pytest.mark.parametrize("cid", list(EC.LEVELS_OF))
def test_gauss_levels_eval(cid):
    case = EC.CASES[cid]
    ref = EC.tail_reference(cid, "levels")
    B = case.shape[0]
    for nl in EC.LEVELS_OF[cid]:
        got = _twice(lambda: _run_eval(case, nl))
        what = f"{cid} {nl} levels"
        sub = lambda r: EC.Ref(r.ref64[:nl], r.ref32[:nl], None if r.A is None else r.A[:nl], r.exact,
                               None if r.alt64 is None else r.alt64[:nl], None if r.band is None else r.band[:nl])
        _exact("gauss_levels_eval", "yhat", what, got["yhat"], ref["yhat"].ref32[:nl])
        _exact("gauss_levels_eval", "sym", what, got["sym"], ref["sym"][:nl])
        K = _lik("gauss_levels_eval", what, got["lik"], sub(ref["lik"]))
        groups = np.stack([l * B + _item_of(case) for l in range(nl)])
        _sum("gauss_levels_eval", "log2sum", what, got["sum:log2sum"], got["lik"], sub(ref["lik"]), K, groups)
    if cid == "t-ragged":                                             # the sum alone
        alone = _run_eval(case, nl, outs=("log2sum",))
        _sum("gauss_levels_eval", "log2sum", what + " alone", alone["sum:log2sum"], got["lik"], sub(ref["lik"]), K, groups)


# ---------------------------------------------------------------------------------------------------------------- gauss_levels_decode
@pytest.mark.parametrize("cid", ["t-min", "t-ragged", "t-levels"])
def test_gauss_levels_decode(cid):
    case = EC.CASES[cid]
    I = EC.inputs(cid)[0]
    for nl in EC.LEVELS_OF[cid]:
        sym, want = EC.decode_reference(cid, nl)

        def run():
            ld, c0 = EC.layout(case, 0)
            s = Slot(case.shape, case.C, ld, c0, EC.expand(case, sym), kind="i32")
            ld, c0 = EC.layout(case, 1)
            mu = Slot(case.shape, case.C, ld, c0, EC.expand(case, I["mu"]))
            ld, c0 = EC.layout(case, 2)
            out = Slot(case.shape, case.C, ld, c0, None, levels=nl)
            lay = Layer(case, EC.expand(case, I["layer"]))
            ops.gauss_levels_decode(s.view, lay.t, mu.view, EC.decode_ks(nl), out.view)
            torch.cuda.synchronize()
            s.untouched(), mu.untouched(), lay.untouched()
            return {"yhat": out.read().reshape(nl, case.n_pix, case.C)}
        got = _twice(run)
        _exact("gauss_levels_decode", "yhat", f"{cid} {nl} levels", got["yhat"], want)


# ---------------------------------------------------------------------------------------------------------------- gauss_layer_bits
def _run_layer_bits(case, n_levels, pix_per_item):
    I = EC.inputs(case.id)[0]
    S = _inputs(case, ["y", "mu", "sigma", "y2"], "ones")
    lay = Layer(case, EC.expand(case, I["layer"]), ld=case.C + 8, c0=4)
    n_items = case.shape[0] if pix_per_item is None else case.n_pix // pix_per_item
    nb = n_levels + 1
    bits, count = Sums(n_items * nb), Sums(n_items * nb, torch.int64)
    ops.gauss_layer_bits(S["y"].view, S["mu"].view, S["sigma"].view, lay.t, n_levels, bits.t.view(n_items, nb), count.t.view(n_items, nb),
                         y2=S["y2"].view, ld_layer=lay.ld, pix_per_item=pix_per_item)
    torch.cuda.synchronize()
    for s in S.values():
        s.untouched()
    lay.untouched()
    return {"sum:bits": bits.read(), "count": count.read()}


@pytest.mark.parametrize("cid", list(EC.LAYER_LEVELS_OF))
def test_gauss_layer_bits(cid):
    case = EC.CASES[cid]
    I = EC.inputs(cid)[0]
    ref = EC.tail_reference(cid, "ones")["lik"]
    K = EC.k_of("gauss")
    # the terms: the launch's own fp32 likelihoods, from gauss_tail under a mask of ones (the float the kernel is documented to bin)
    S = _inputs(case, ["y", "mu", "sigma", "y2", "mask"], "ones")
    ld, c0 = EC.layout(case, 5)
    lk = Slot(case.shape, case.C, ld, c0, None)
    ops.gauss_tail(S["y"].view, S["mu"].view, S["sigma"].view, y2=S["y2"].view, mask=S["mask"].view, lik=lk.view)
    torch.cuda.synchronize()
    own = lk.read()
    _lik("gauss_layer_bits", f"{cid} terms", own, ref)
    layer = EC.expand(case, I["layer"]).astype(np.int64)
    for nl in EC.LAYER_LEVELS_OF[cid]:
        for ppi in ((None, 1, 7) if cid == "t-blocks" else (None,)):
            got = _twice(lambda: _run_layer_bits(case, nl, ppi))
            nb = nl + 1
            groups = _item_of(case, ppi) * nb + np.minimum(layer, nl)
            n_groups = got["count"].size
            what = f"{cid} {nl} levels, pix_per_item {ppi}"
            _exact("gauss_layer_bits", "count", what, got["count"], np.bincount(groups.reshape(-1), minlength=n_groups))
            _sum("gauss_layer_bits", "bits", what, got["sum:bits"], own, ref, K, groups, n_groups)


def test_log2_lik_outside():
    ref = EC.outside_ref()
    K = EC.k_of("gauss")
    got = ops.log2_lik_outside("cuda")
    want = float(np.log2(ref.ref64[0]))
    tol = float(EC.bits_bound(ref, K)[0])
    print(f"log2_lik_outside: {got!r}, float64 {want!r}, off by {abs(got - want):.3g} bits (bound {tol:.3g})")
    WORST[("log2_lik_outside", "value", "bits")] = abs(got - want)
    assert abs(got - want) <= tol, (got, want, tol)


# ---------------------------------------------------------------------------------------------------------------- build_indexes
@pytest.mark.parametrize("cid", ["t-min", "t-ragged", "t-stride"])
def test_build_indexes(cid):
    case = EC.CASES[cid]
    table = torch.from_numpy(EC.scale_table()).cuda()
    for masked in (False, True):
        def run():
            S = _inputs(case, ["sigma"] + (["mask"] if masked else []), "masked")
            ld, c0 = EC.layout(case, 2)
            out = Slot(case.shape, case.C, ld, c0, None, kind="i32")
            ops.build_indexes(S["sigma"].view, table, mask=S["mask"].view if masked else None, out=out.view)
            torch.cuda.synchronize()
            for s in S.values():
                s.untouched()
            return {"idx": out.read()}
        got = _twice(run)
        _exact("build_indexes", "idx", f"{cid} masked={masked}", got["idx"], EC.index_reference(cid, masked))


# ---------------------------------------------------------------------------------------------------------------- bottleneck
def _run_eb(case, outs=("zhat", "lik", "sym", "log2sum")):
    I = EC.inputs(case.id)[0]
    params = torch.from_numpy(I["params"].copy()).cuda()
    ld, c0 = EC.layout(case, 0)
    z = Slot(case.shape, case.C, ld, c0, np.ascontiguousarray(I["z"].T))
    O = {}
    for k, n in enumerate(n for n in ("zhat", "lik", "sym") if n in outs):
        ld, c0 = EC.layout(case, 1 + k)
        O[n] = Slot(case.shape, case.C, ld, c0, None, kind="i32" if n == "sym" else "f32")
    ls = Sums(case.shape[0]) if "log2sum" in outs else None
    ops.eb_forward(z.view, params, O["zhat"].view if "zhat" in O else None, O["lik"].view if "lik" in O else None,
                   log2sum=ls.t if ls is not None else None, sym=O["sym"].view if "sym" in O else None)
    torch.cuda.synchronize()
    z.untouched()
    assert np.array_equal(params.cpu().numpy(), I["params"])
    res = {n: O[n].read().T for n in O}                               # [C, N]
    if ls is not None:
        res["sum:log2sum"] = ls.read()
    return res


@pytest.mark.parametrize("cid", [c for c, v in EC.CASES.items() if v.fam == "eb"])
def test_eb_forward_eval(cid):
    case = EC.CASES[cid]
    ref = EC.eb_reference(cid)
    got = _twice(lambda: _run_eb(case))
    _exact("eb_forward", "zhat", cid, got["zhat"], ref["zhat"].ref32)
    _exact("eb_forward", "sym", cid, got["sym"], ref["sym"])
    K = _lik("eb_forward", cid, got["lik"], ref["lik"])
    groups = _item_of(case).T                                        # [C, N]
    _sum("eb_forward", "log2sum", cid, got["sum:log2sum"], got["lik"], ref["lik"], K, groups)
    alone = _run_eb(case, outs=("lik",))                              # the likelihood alone (what the plans ask for with a sum)
    assert np.array_equal(EC.bits(alone["lik"]), EC.bits(got["lik"]))


def test_constants_are_the_library_s():
    assert (EC.MAX_MASK_LEVELS, EC.MAX_LAYER_LEVELS, EC.LAYER_NONE) == (L.VAM_MAX_MASK_LEVELS, L.VAM_MAX_LAYER_LEVELS, L.LAYER_NONE)


def test_zz_report_measured_ratios():
    """The worst GPU ratio and the worst error in bits per kernel and output next to K_cpu and K (what DESIGN.md quotes), and
    which exact outputs were bit-equal."""
    assert WORST, "run after the cases of this file"
    for fam in ("gauss", "eb"):
        record_measurement(f"entropy_contract K {fam}", k_cpu=round(EC.k_cpu(fam), 3), K=EC.k_of(fam))
    for key, v in sorted(WORST.items(), key=lambda kv: tuple(map(str, kv[0]))):
        record_measurement("entropy_contract GPU " + " ".join(key), gpu=v if isinstance(v, str) else float(f"{v:.4g}"))
