"""The float64 reference of tests/wgrad_contract.py checked without a GPU: against float64 autograd of F.conv2d, its bounds
against fp32 ATen autograd and against seven wrong formulas, and its case table against the instantiations the weight-
gradient dispatchers can launch (vam_conv_wgrad_route: host arithmetic, the functions the launch itself asks)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import wgrad_contract as WC

SMALL = [k for k in WC.CASES if k not in WC.BIG_CASES]


def _autograd(case, t, dtype):
    x = torch.cat(t["segs"], 1).to(dtype)
    w = torch.zeros((case.n, case.cin, case.k, case.k), dtype=dtype, requires_grad=True)
    b = torch.zeros((case.n,), dtype=dtype, requires_grad=True)
    F.conv2d(x, w, b, stride=case.stride, padding=case.k // 2).backward(t["dy"].to(dtype))
    return w.grad, b.grad


@pytest.mark.parametrize("cid", SMALL)
def test_reference_equals_float64_autograd(cid):
    """The tap loop of pixel GEMMs is the weight / bias gradient of F.conv2d(cat(segments), stride s, padding k/2)."""
    case = WC.CASES[cid]
    t = WC.tensors(case)
    ref = WC.reference(case, t)
    gw, gb = _autograd(case, t, torch.float64)
    assert gw.shape == ref.dw.shape == ref.abs_sum.shape and gb.shape == ref.db.shape
    assert bool(((ref.dw - gw).abs() <= 1e-12 * (1.0 + ref.abs_sum)).all())          # elementwise, against each element's own scale
    assert bool(((ref.db - gb).abs() <= 1e-12 * (1.0 + ref.abs_db)).all())
    assert bool((ref.abs_sum >= ref.dw.abs() * (1 - 1e-12)).all())     # (0 = 0 on the taps an H = 1 grid never reaches)


@pytest.mark.parametrize("cid", list(WC.CASES))
def test_fp32_aten_autograd_meets_every_bound(cid):
    """The bounds asserted on the GPU are ones a correct fp32 implementation meets: ATen's fp32 autograd of F.conv2d passes
    check_dw, check_db and (on the RMS cases) check_rms.  Measured on an x86 host: dw within 1.2e-5 ... 0.062 x
    (K + 4) 2^-24 abs_sum (smallest on the 65536-pixel cases), db within 5.3e-6 ... 0.022 x its bound, rms 0.38 (w32),
    0.42 (l3b16), 0.21 (l5s2big32) x its bound."""
    case = WC.CASES[cid]
    t = WC.tensors(case)
    ref = WC.reference(case, t)
    gw, gb = _autograd(case, t, torch.float32)
    assert gw.dtype == torch.float32
    r = {"dw": WC.check_dw(case, ref, gw, "fp32 ATen"), "db": WC.check_db(case, ref, gb, "fp32 ATen")}
    if cid in WC.RMS_CASES:
        r["rms"] = WC.check_rms(case, ref, gw, "fp32 ATen")
    print(f"{cid}: fp32 ATen error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) < 1.0


def _bounds_ratio(case, ref, dw, db):
    """(dw error / bound, db error / bound) without asserting."""
    return (WC._ratio((dw.double() - ref.dw).abs(), (case.K + 4) * WC.U * ref.abs_sum),
            WC._ratio((db.double() - ref.db).abs(), (case.K + 4) * WC.U * ref.abs_db))


WRONG = ("ty<->tx", "taps flipped", "pad off by one", "stride-2 parity", "c_off ignored", "last pixel dropped", "a split counted twice")


@pytest.mark.parametrize("wrong", WRONG)
def test_the_bounds_reject_a_wrong_formula(wrong):
    """Seven wrong formulas, evaluated in float64 (so the only error is the formula's), miss the elementwise dw bound by
    orders of magnitude (measured: 5.2e3 ... 9.1e4 x the bound; db 1.0e3 / 2.1e3 x for the two that change it); check_dw raises on each."""
    cid = {"stride-2 parity": "l3s2b16", "c_off ignored": "lseg", "a split counted twice": "ls4"}.get(wrong, "l5a16")
    case = WC.CASES[cid]
    t = WC.tensors(case)
    ref = WC.reference(case, t)
    db = ref.db
    if wrong == "ty<->tx":
        dw = ref.dw.transpose(2, 3)
    elif wrong == "taps flipped":
        dw = ref.dw.flip(2, 3)
    elif wrong == "pad off by one":
        dw = WC.evaluate(case, t, shift=(-1, -1)).dw
    elif wrong == "stride-2 parity":
        dw = WC.evaluate(case, t, shift=(1, 1)).dw                     # s oy + ty - pad + 1
    elif wrong == "c_off ignored":
        dw = torch.zeros_like(ref.dw)
        for off, c in zip(case.c_offs, case.segs):                     # every segment's problem writes from column 0
            dw[:, 0:c] = ref.dw[:, off:off + c]
    elif wrong == "last pixel dropped":
        dy = t["dy"].clone()
        dy[-1, :, -1, -1] = 0.0
        bad = WC.evaluate(case, dict(t, dy=dy))
        dw, db = bad.dw, bad.db
    else:                                                              # chunks 5 .. 9 of 18 (split 1 of 4) twice
        dy = t["dy"].permute(0, 2, 3, 1).reshape(-1, case.n).clone()
        dy[:5 * 32] = 0.0
        dy[10 * 32:] = 0.0
        part = WC.evaluate(case, dict(t, dy=dy.reshape(case.B, case.H, case.W, case.n).permute(0, 3, 1, 2)))
        dw, db = ref.dw + part.dw, ref.db + part.db
    rw, rb = _bounds_ratio(case, ref, dw, db)
    print(f"{wrong} on {cid}: dw error / bound {rw:.3g}, db error / bound {rb:.3g}")
    assert rw > 100.0
    with pytest.raises(AssertionError):
        WC.check_dw(case, ref, dw.float())
    if wrong in ("last pixel dropped", "a split counted twice"):
        assert rb > 100.0
        with pytest.raises(AssertionError):
            WC.check_db(case, ref, db.float())


def test_one_hot_reference_is_the_patch_of_x():
    """dy = 1.0 at one pixel: the reference's row is the k x k patch of x around s * pixel, zero outside the image — exactly
    (what test_gpu_wgrad_contract's placement test compares bits with)."""
    case = WC.CASES["l3s2b16"]
    P = case.K
    pixels = [0, P - 1, case.H * case.W + case.W - 1, 31, 32]
    t = WC.one_hot(case, pixels)
    ref = WC.reference(case, t)
    x = torch.cat(t["segs"], 1)
    for i, p in enumerate(pixels):
        b, r = divmod(p, case.H * case.W)
        oy, ox = divmod(r, case.W)
        for ty in range(case.k):
            for tx in range(case.k):
                iy, ix = 2 * oy + ty - 1, 2 * ox + tx - 1
                want = x[b, :, iy, ix].double() if 0 <= iy < case.Hx and 0 <= ix < case.Wx else torch.zeros(case.cin, dtype=torch.float64)
                assert torch.equal(ref.dw[3 * i + 1, :, ty, tx], want)
    rows = [3 * i + 1 for i in range(len(pixels))]
    rest = torch.ones(case.n, dtype=torch.bool)
    rest[rows] = False
    assert bool((ref.dw[rest] == 0).all()) and bool((ref.db[rest] == 0).all()) and bool((ref.db[rows] == 1).all())


def test_plane_layout_decodes_to_the_fp32_values():
    """to_planes is the exact split the kernels make: the three bf16 planes add up to every fp32 value, and ops.View3
    decodes the windowed buffer of a plane case to its fp32 input."""
    case = WC.CASES["lpa"]
    built = WC.build(case, "cpu")
    x = built.t["segs"][0].permute(0, 2, 3, 1).contiguous()
    assert torch.equal(built.x3[0].to_float(), x)
    from vampic import ops
    assert bool(torch.isnan(ops.View3(built.x3[0].buf, 0, 8).to_float()).all())          # the guard group beside the window


def test_case_table_reaches_every_instantiation():
    """Every kernel instantiation the dispatchers launch without the measurement switches VAMPIC_WGRAD_TILE /
    VAMPIC_WGRAD_KP is reached by a case: the six (TN, TC) tiles of the register-gather kernel (which the fp32 pipe of
    VAMPIC_WGRAD=f32 and VAMPIC_WGRAD_LDS=0 reuse with the same cases), and for the LDS kernel the wave grids 4 x 1 / 3 x 2 /
    2 x 2 with 32-pixel chunks for each of k3 / k5 x stride 1 / 2, 4 x 2 with 64-pixel chunks for k5 stride 2, the three
    plane-input grids and the three 1x1 block shapes."""
    from vampic import _lib as L
    lib = L.load()
    seen = {}
    for cid, case in WC.CASES.items():
        built = WC.build(case, "cpu")
        for s in range(len(case.segs)):
            r = built.route(s)
            key = r + ((case.k, case.stride) if r[0] == "lds" else (None, None))
            seen.setdefault(key, []).append(cid)
    if os.environ.get("VAMPIC_WGRAD", "")[:1] in ("f", "F") or os.environ.get("VAMPIC_WGRAD_LDS", "")[:1] == "0":
        pytest.skip("VAMPIC_WGRAD / VAMPIC_WGRAD_LDS in the environment: the table is stated for the default mode")
    assert WC.build(WC.CASES[WC.PROBE], "cpu").route(0)[:2] == ("lds", 1), "the default mode takes the LDS kernel on the bf16x3 pipe"
    for cid in WC.PLANE_CASES:
        assert WC.build(WC.CASES[cid], "cpu").route(0)[0] == "lds", cid
    want = WC.reachable_default()
    for key in sorted(seen, key=str):
        print(key, "<-", ", ".join(seen[key]))
    assert set(seen) == want, (sorted(want - set(seen), key=str), sorted(set(seen) - want, key=str))
    # the gather tiles come from cases the LDS kernel declines in every mode (so f32 / LDS-off runs reach them too)
    gather = {k[4:6] for k in seen if k[0] == "gather"}
    assert gather == {(1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (3, 2)}
    # the planner itself returns more than one split on the PLAN cases, on both kernels
    kernels = set()
    for cid in WC.PLAN_CASES:
        case = WC.CASES[cid]
        built = WC.build(case, "cpu")
        p = built.problem(0, *built.outputs())
        nbytes = ctypes.c_size_t(0)
        s = lib.vam_conv_wgrad_plan(ctypes.byref(p), ctypes.byref(nbytes))
        assert s > 1 and p.splits == s, cid
        assert nbytes.value == 4 * s * (case.n * case.segs[0] * case.taps + case.n)      # the workspace formula the cases use
        kernels.add(built.route(0)[0])
    assert kernels == {"gather", "lds"}


def test_route_rejects_bad_arguments():
    from vampic import _lib as L
    out = (ctypes.c_int * 8)()
    p = L.VamWgrad()
    assert L.load().vam_conv_wgrad_route(ctypes.byref(p), out) == 1
    assert L.load().vam_conv_wgrad_route(None, out) == 1
