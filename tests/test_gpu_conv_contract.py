"""``vam_conv_group`` against the float64 statement of its contract (tests/conv_contract.py): every corner of the problem
struct at the smallest shape where it can still go wrong, every tile shape and both epilogues, what a launch owns and
what it must leave alone.  This file is what a rewrite of the convolution kernel has to keep."""
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import ops, _lib as L  # noqa: E402
import conv_contract as CC          # noqa: E402

# (name, forced tile, forced epilogue): the automatic choice, then the three tile families (two-wave 64-row, the direct
# epilogue's 128x64, the wide 128x192), and the 128x64 tile with the epilogue left automatic (0) and LDS-staged (1)
VARIANTS = (("auto", (0, 0, 0), -1), ("64x64", (64, 64, 0), -1), ("128x64", (128, 64, 0), -1), ("128x192", (128, 192, 0), -1),
            ("128x64 epilogue 0", (128, 64, 0), 0), ("128x64 epilogue 1", (128, 64, 0), 1))


def _launch(prob):
    ops.conv_group([prob])
    torch.cuda.synchronize()


AUTO_TILE = {}      # case -> ((BM, BN, BK) vam_conv_last_tile reported after the automatic-tile launch, vam_conv_plan's for the same problem)


def _last_and_planned_tile(prob):
    lib = L.load()
    bm, bn, bk = (ctypes.c_int() for _ in range(3))
    lib.vam_conv_last_tile(ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(bk))
    ch = L.VamConvChoice()
    L.check(lib.vam_conv_plan((L.VamConv * 1)(prob), 1, ctypes.byref(ch)), "vam_conv_plan")
    return (bm.value, bn.value, bk.value), (ch.bm, ch.bn, ch.bk)


@functools.lru_cache(maxsize=None)
def _launches(cid):
    """Every variant of one case, launched once and shared by the tests: (built, reference, [(name, out, stray elements of
    the out buffer, preact, stray elements of the preact buffer)])."""
    lib = L.load()
    case = CC.CASES[cid]
    built = CC.build(case, "cuda")
    ref = CC.reference(case, built.t)
    res = []
    for name, tile, epi in VARIANTS:
        lib.vam_conv_force_tile(*tile)
        lib.vam_conv_force_epilogue(epi)
        try:
            prob, obuf, pbuf = built.problem()
            _launch(prob)
            if name == "auto":
                AUTO_TILE[cid] = _last_and_planned_tile(prob)
        finally:
            lib.vam_conv_force_tile(0, 0, 0)
            lib.vam_conv_force_epilogue(-1)
        out, stray = built.read(obuf, ref.written, case.nchw)
        pre, pstray = built.read(pbuf, ref.written) if pbuf is not None else (None, 0)
        res.append((name, out, stray, pre, pstray))
    return built, ref, res


@pytest.mark.parametrize("cid", list(CC.CASES))
def test_contract_against_float64(cid):
    """out = post2 + post + mul * act(conv(cat(seg...)) + bias + pre) against float64, elementwise.

    * the tile of the automatic launch (``vam_conv_last_tile``) is the one ``vam_conv_plan`` names for the same problem;
    * every tile shape and both epilogues give the same bits, ``out`` and ``preact`` alike;
    * z (ACT_NONE cases without mul / post / post2, and the preact output) within (K + 4) 2^-24 abs_sum, the worst case of
      an fp32 accumulation of exact products in any order: a correct kernel cannot fail it, a wrong tap, segment, pad,
      stride or placement cannot pass it;
    * on g4, g11 and e-preact also rms(z - z64) <= (0.5 sqrt(K) + 2) 2^-24 rms(z64), the bound of
      test_conv_accuracy_against_float64: what a lost low-order term of the operand split breaks;
    * out of the epilogue cases within Lip(act) |mul| E_z + 16 2^-24 (1 + |act(z) mul| + |post| + |post2|).

    The largest error / bound of every case is printed and handed to conftest.record_measurement, so a run lists it
    with the other measured parity quantities (conftest's parity_measured.json).  Measured on an MI355X, error / bound
    (bf16x3 default | f32 | f16x2): z 0.0015 ... 0.022 | 0.0018 ... 0.024 | 0.0009 ... 0.013 (largest on g8, the thin 1x1);
    rms g4 0.38 | 0.44 | 0.28, g11 0.36 | 0.42 | 0.28, e-preact 0.23 | 0.26 | 0.17; out at most 0.060 | 0.058 | 0.060
    (e-gdn-RSQRT / e-gdn-SQRT; e-CLAMP01 0.051, every other case below 0.03).  The elementwise bounds are worst-case bounds
    and are met with a factor 17 or more to spare; the rms bound is the tight one."""
    from conftest import record_measurement
    case = CC.CASES[cid]
    built, ref, res = _launches(cid)
    launched, planned = AUTO_TILE[cid]
    assert planned == launched, f"{cid}: vam_conv_plan says {planned}, the automatic-tile launch took {launched}"
    name0, out0, _, pre0, _ = res[0]
    for name, out, _, pre, _ in res[1:]:
        assert torch.equal(out, out0), f"{cid}: {name} differs from {name0} in {(out != out0).sum().item()} elements of out"
        if pre0 is not None:
            assert torch.equal(pre, pre0), f"{cid}: {name} differs from {name0} in preact"
    w = ref.written
    assert bool(torch.isfinite(out0[w]).all()), f"{cid}: a channel outside an input or operand window reached the output"
    measured = {}
    if cid in CC.Z_CASES:
        measured["z"] = CC.check_z(case, ref, out0)
    if case.preact:
        assert bool(torch.isfinite(pre0[w]).all())
        measured["z"] = CC.check_z(case, ref, pre0, "preact")
    if cid in CC.RMS_CASES:
        measured["rms"] = CC.check_rms(case, ref, pre0 if case.preact else out0)
    if cid in CC.OUT_CASES:
        measured["out"] = CC.check_out(case, ref, out0)
    assert measured
    print(f"{cid}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in measured.items()))
    record_measurement(f"conv contract {cid} (mode {L.load().vam_conv_get_mode()})", **{k: f"{v:.3g}" for k, v in measured.items()})


@pytest.mark.parametrize("cid", list(CC.CASES))
def test_launch_writes_only_what_it_owns(cid):
    """After each launch every element outside ``written`` still holds the sentinel's bits: the 4 + 4 guard channels beside
    the output window, the spare image after the last one, the three other phases of a strided placement — in ``out`` and in
    ``preact``.  Every owned element is finite although every channel outside an input or operand window is NaN."""
    _, ref, res = _launches(cid)
    for name, out, stray, pre, pstray in res:
        assert stray == 0, f"{cid} {name}: {stray} elements outside the problem's own were written"
        assert pstray == 0, f"{cid} {name}: {pstray} preact elements outside the problem's own were written"
        assert bool(torch.isfinite(out[ref.written]).all()), f"{cid} {name}"
        assert not bool((out[ref.written] == CC.SENTINEL).all()), f"{cid} {name}: nothing was written"
        if pre is not None:
            assert bool(torch.isfinite(pre[ref.written]).all()), f"{cid} {name}"


@pytest.mark.parametrize("cid", ["g3", "g4", "g8"])
def test_segments_equal_materialised_concat(cid):
    """Virtual concatenation: two to four windows of unrelated buffers give the bits of one contiguous tensor."""
    built, ref, res = _launches(cid)
    prob, obuf, _ = built.problem(concat=True)
    assert prob.n_seg == 1
    _launch(prob)
    out, stray = built.read(obuf, ref.written)
    assert stray == 0
    assert torch.equal(out, res[0][1]), f"{cid}: {(out != res[0][1]).sum().item()} elements differ"


GROUP = ("g5", "g6", "g7a", "g7b", "g8", "g9a", "g11", "e-phase")


def test_group_of_unlike_problems_equals_single_launches():
    """One grid for eight problems that share nothing (taps, stride, placement, segments, epilogue; all with Cin % 32 == 0,
    so every arithmetic mode takes the group): each output equals the problem launched alone, and the guards hold."""
    singles = [_launches(cid) for cid in GROUP]
    probs = [b.problem() for b, _, _ in singles]
    ops.conv_group([p for p, _, _ in probs])
    torch.cuda.synchronize()
    for cid, (built, ref, res), (_, obuf, _) in zip(GROUP, singles, probs):
        out, stray = built.read(obuf, ref.written)
        assert stray == 0, f"{cid} in the group: {stray} elements outside the problem's own were written"
        assert torch.equal(out, res[0][1]), f"{cid} in the group: {(out != res[0][1]).sum().item()} elements differ from the single launch"


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_contract_in_the_other_arithmetic_modes(mode):
    """VAMPIC_CONV=f32 (fp32 operands on the fp32 matrix pipe) and VAMPIC_CONV=f16x2 fix the packed-weight layout for the
    life of a process: the tests above run again in a fresh child process for each, with the bounds unchanged."""
    env = dict(os.environ, VAMPIC_CONV=mode)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not other_arithmetic"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "passed" in r.stdout
