"""The float64 reference of tests/conv_contract.py checked without a GPU: against torch's own float64 operators where they
exist, and its tolerances against an fp32 ATen evaluation of the same formula."""
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

import vampic.synth

import conv_contract as CC


def _x64(t):
    return torch.cat(t["segs"], 1).double()


@pytest.mark.parametrize("cid", ["g3", "g5", "g6", "g11"])
def test_reference_equals_conv2d_with_symmetric_padding(cid):
    case = CC.CASES[cid]
    t = CC.tensors(case)
    ref = CC.reference(case, t)
    want = F.conv2d(_x64(t), t["w"].double(), t["b"].double(), stride=case.stride, padding=(case.pad_y, case.pad_x))
    assert want.shape == ref.z.shape and bool(ref.written.all())
    assert (ref.z - want).abs().max().item() <= 1e-13
    assert torch.equal(ref.out, ref.z)


@pytest.mark.parametrize("cid", ["g9a", "g9b"])
def test_reference_equals_pixel_shuffle_of_conv2d(cid):
    case = CC.CASES[cid]
    t = CC.tensors(case)
    ref = CC.reference(case, t)
    want = F.pixel_shuffle(F.conv2d(_x64(t), t["w"].double(), t["b"].double(), padding=1), 2)
    assert want.shape == ref.z.shape == (case.B, case.cout, 2 * case.H, 2 * case.W) and bool(ref.written.all())
    assert (ref.z - want).abs().max().item() <= 1e-13


def test_phase_geometries_rebuild_conv_transpose2d():
    """ConvTranspose2d(k5, stride 2, padding 2, output_padding 1) is four correlations, one per output phase (py, px): taps
    [4, 2, 0] (padding 1) on an even axis, [3, 1] (padding 0) on an odd one, written at (2 oy + py, 2 ox + px).  The
    geometries of g7a / g7b / g7c and the 3x3 phase, fed phase weights gathered by hand from one IOHW tensor, must sum to
    torch's float64 operator, and their ``written`` maps must tile the output exactly once."""
    g = CC.CASES["g7a"]
    phases = [replace(g, id="phase00", kh=3, kw=3, pad_y=1, pad_x=1, ooy=0, oox=0), g, CC.CASES["g7b"], CC.CASES["g7c"]]
    cin, cout = g.cin, g.n
    wt = vampic.synth.normal((cin, cout, 5, 5), 5, 1.0 / 20.0)
    t0 = CC.tensors(g)
    total = torch.zeros((g.B, cout, g.Hf, g.Wf), dtype=torch.float64)
    cover = torch.zeros((g.B, cout, g.Hf, g.Wf), dtype=torch.int32)
    for ph in phases:
        assert (ph.kh, ph.pad_y) == ((2, 0) if ph.ooy else (3, 1)) and (ph.kw, ph.pad_x) == ((2, 0) if ph.oox else (3, 1))
        ty = [3, 1] if ph.ooy else [4, 2, 0]
        tx = [3, 1] if ph.oox else [4, 2, 0]
        w = wt[:, :, ty][:, :, :, tx].permute(1, 0, 2, 3).contiguous()           # OIHW of this phase's correlation
        ref = CC.reference(ph, dict(t0, w=w))
        total += torch.where(ref.written, ref.z, torch.zeros_like(ref.z))
        cover += ref.written.int()
    assert bool((cover == 1).all()), "the four phases own every output element exactly once"
    want = F.conv_transpose2d(_x64(t0), wt.double(), t0["b"].double(), stride=2, padding=2, output_padding=1)
    assert want.shape == total.shape
    assert (total - want).abs().max().item() <= 1e-13


def test_written_maps_and_shapes():
    for case in CC.CASES.values():
        ref = CC.reference(case)
        shape = (case.B, case.cout, case.Hf, case.Wf)
        for k in ("out", "z", "written", "abs_sum"):
            assert getattr(ref, k).shape == shape, (case.id, k)
        assert int(ref.written.sum()) == case.B * case.n * case.Ho * case.Wo, case.id
        assert bool(torch.isfinite(ref.out).all()) and bool((ref.abs_sum[ref.written] > 0).all()), case.id
        if case.gdn:
            assert float(ref.z.min()) >= 0.5, case.id


@pytest.mark.parametrize("cid", list(CC.CASES))
def test_fp32_aten_meets_every_tolerance(cid):
    """The bounds asserted on the GPU are ones a correct fp32 implementation meets: ATen's fp32 evaluation of the same
    formula (fp32 F.conv2d, fp32 epilogue in the contract's order) passes check_z and check_out on every case — with the
    epilogue constant 16 as written, which therefore stays (it would be raised, to the next power of two, only if ATen came
    within a factor 2 of it).  Measured on an x86 host: z within 0.081 x (K + 4) 2^-24 abs_sum (e-gdn-SQRT; the geometry cases
    0.0008 ... 0.024), out within 0.060 x its bound (e-gdn-RSQRT; e-CLAMP01 0.051, the others below 0.03)."""
    case = CC.CASES[cid]
    t = CC.tensors(case)
    ref = CC.reference(case, t)
    got = CC.evaluate(case, t, torch.float32)
    assert got.out.dtype == torch.float32
    rz = CC.check_z(case, ref, got.z, "fp32 ATen")
    ro = CC.check_out(case, ref, got.out, "fp32 ATen")
    print(f"{cid}: fp32 ATen z error / bound {rz:.3g}, out error / bound {ro:.3g}")
    assert ro <= 0.5, (cid, ro)


@pytest.mark.parametrize("wrong", ["tap", "pre<->post"])
def test_the_bounds_reject_a_wrong_formula(wrong):
    """A reference with one tap column shifted, or with pre and post exchanged, is outside the bounds by orders of
    magnitude (fp32 ATen stands in for a kernel here)."""
    case = CC.CASES["e-GELU"]
    t = CC.tensors(case)
    got = CC.evaluate(case, t, torch.float32)
    if wrong == "tap":
        bad = dict(t, w=torch.roll(t["w"], 1, 3))
    else:
        bad = dict(t, pre=t["post"], post=t["pre"])
    ref = CC.reference(case, bad)
    with pytest.raises(AssertionError):
        CC.check_out(case, ref, got.out)
    with pytest.raises(AssertionError):
        CC.check_z(case, ref, got.z)
