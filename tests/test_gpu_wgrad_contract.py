"""``vam_conv_wgrad_group`` (wgrad_kernel of csrc/train.hip, wgrad2_kernel of csrc/wgrad_lds.hip) and ``vam_colsum`` against
the float64 statement of their contract (tests/wgrad_contract.py): every tile of both kernels at the smallest shape that
reaches it, the grids where the LDS kernel's chunking has an edge, forced and planned pixel splits, what a launch owns
and what it must leave alone.  This file is what a rewrite of either weight-gradient kernel has to keep."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from vampic import ops, _lib as L  # noqa: E402
import wgrad_contract as WC         # noqa: E402

# the two switches as the library reads them (once per process), taken from the environment and never from its answers
F32_PIPE = os.environ.get("VAMPIC_WGRAD", "")[:1] in ("f", "F")
LDS_OFF = os.environ.get("VAMPIC_WGRAD_LDS", "")[:1] == "0"
MODE = ("f32" if F32_PIPE else "bf16x3") + (", LDS kernel off" if LDS_OFF else "")
LDS_RUNS = not (F32_PIPE or LDS_OFF)


def _group(probs):
    arr = (L.VamWgrad * len(probs))(*probs)
    return L.load().vam_conv_wgrad_group(arr, len(probs), ops.stream_ptr())


def _run(probs):
    L.check(_group(probs), "vam_conv_wgrad_group")
    torch.cuda.synchronize()


def _needs_lds(case):
    return case.plane


def _skip_unless_launchable(built):
    """Plane inputs exist for the LDS kernel only: with VAMPIC_WGRAD=f32 or VAMPIC_WGRAD_LDS=0 in the environment the
    library refuses them and the case skips.  Without those switches the case must take the LDS kernel
    (vam_conv_wgrad_route): a library that stops choosing it fails here, it does not skip."""
    if not _needs_lds(built.case):
        return
    kernel = built.route(0)[0]
    if not LDS_RUNS:
        assert kernel == "gather", f"{built.case.id}: {MODE} in the environment, yet vam_conv_wgrad_route names the LDS kernel"
        pytest.skip("a plane input needs the LDS kernel, which VAMPIC_WGRAD / VAMPIC_WGRAD_LDS switch off")
    assert kernel == "lds", f"{built.case.id}: the default mode must take the LDS kernel for a plane input"


def test_route_follows_the_environment():
    """Which kernel and pipe run is what the environment says, as vam_conv_wgrad_route reports it: the LDS kernel on the
    bf16x3 pipe for the probe case by default, the gather kernel on the fp32 pipe under VAMPIC_WGRAD=f32, the gather kernel
    on the bf16x3 pipe under VAMPIC_WGRAD_LDS=0 — so the runs of this file in the three modes are runs of three code paths."""
    r = _built(WC.PROBE)[0].route(0)
    assert r[:2] == (("lds", 1) if LDS_RUNS else ("gather", 0 if F32_PIPE else 1)), (MODE, r)
    assert _built("w11")[0].route(0)[:2] == ("gather", 0 if F32_PIPE else 1)


@functools.lru_cache(maxsize=None)
def _built(cid):
    case = WC.CASES[cid]
    built = WC.build(case, "cuda")
    return built, WC.reference(case, built.t)


@functools.lru_cache(maxsize=None)
def _launches(cid):
    """Every segment of one case launched ALONE, once, into fresh sentinel-filled buffers, then again into buffers filled
    with 3.5: (built, reference, [(segment, dw, db, stray elements, dw of the second launch, db of the second launch)])."""
    built, ref = _built(cid)
    case = built.case
    res = []
    for s in range(len(case.segs)):
        out = []
        for fill in (WC.SENTINEL, 3.5):
            dwbuf, dbbuf = built.outputs(fill)
            p = built.problem(s, dwbuf, dbbuf if case.db else None)
            _run([p])
            assert WC.ws_stray(p) == 0, f"{cid} segment {s}: the launch wrote behind its workspace"
            out.append((dwbuf, dbbuf))
        owns_db = case.db and case.c_offs[s] == 0
        dw, db, stray = built.read(*out[0], [s], owns_db)
        dwbuf2, dbbuf2 = out[1][0].cpu(), out[1][1].cpu()
        dw2 = dwbuf2[WC.GUARD:WC.GUARD + dw.numel()].reshape(dw.shape)
        res.append((s, dw, db, stray, dw2, dbbuf2[WC.GUARD:WC.GUARD + case.n]))
    return built, ref, res


def _merged(cid):
    """dw of the whole case from its segments' own columns, db from the c_off == 0 problem."""
    built, ref, res = _launches(cid)
    case = built.case
    dw = torch.full(ref.dw.shape, float("nan"))
    for s, dws, _, _, _, _ in res:
        o, c = case.c_offs[s], case.segs[s]
        dw[:, o:o + c] = dws[:, o:o + c]
    return dw, res[0][2]


@pytest.mark.parametrize("cid", list(WC.CASES))
def test_contract_against_float64(cid):
    """dW / db of every case against the float64 tap loop, elementwise:

    * |dw - dw64| <= (K + 4) 2^-24 sum |dY| |X| and |db - db64| <= (K + 4) 2^-24 sum |dY| with K = B H W, the worst case of
      an fp32 accumulation of K exact products in any order (the + 4 holds the mid x lo, lo x mid and lo x lo products the
      bf16x3 pipe drops, about 2 x 2^-24 per product): a correct kernel cannot fail it, a wrong tap, row, channel block,
      pad, stride, c_off or split cannot pass it (tests/test_wgrad_contract_cpu.py: seven wrong formulas miss it 5e3 ... 9e4 x);
    * on w32, l3b16 and l5s2big32 also rms(dw - dw64) <= (0.5 sqrt(K) + 2) 2^-24 rms(dw64): what a lost low-order term of
      the operand split breaks;
    * every owned element is finite although every channel beside an input window and the image behind the last are NaN.

    The largest error / bound of every case is printed and handed to conftest.record_measurement.  Measured on an MI355X,
    error / bound (bf16x3 default | VAMPIC_WGRAD=f32 | VAMPIC_WGRAD_LDS=0):
    dw 4.9e-6 ... 0.041 | 2.1e-6 ... 0.043 | 2.3e-6 ... 0.041 (largest on wk5s2, smallest on the 65536-pixel cases, whose
    worst-case bound grows with K); db 5.8e-7 ... 0.0090 | 5.9e-7 ... 0.010 | 6.0e-7 ... 0.0090; rms w32 0.23 | 0.26 | 0.23,
    l3b16 0.37 | 0.20 | 0.19, l5s2big32 0.10 | 0.037 | 0.045.  The elementwise bounds are worst-case bounds and are met
    with a factor 23 or more to spare (fp32 ATen autograd: 0.062 at most); the rms bound is the tight one.  A dropped
    low-order product of the operand split (the (lo, hi) MFMA, tried on a scratch build) is caught by the elementwise
    bound where K is small (the gather cases at K = 70 ... 105, l3b32 at K = 128) and by the rms bound at larger K
    (l3b16, l5s2big32)."""
    from conftest import record_measurement
    built, ref = _built(cid)
    _skip_unless_launchable(built)
    case = built.case
    dw, db = _merged(cid)
    assert bool(torch.isfinite(dw).all()), f"{cid}: something outside an input window or the pixel range reached dw"
    measured = {"dw": WC.check_dw(case, ref, dw)}
    if case.db:
        assert bool(torch.isfinite(db).all()), f"{cid}: something outside the dy window reached db"
        measured["db"] = WC.check_db(case, ref, db)
    if cid in WC.RMS_CASES:
        measured["rms"] = WC.check_rms(case, ref, dw)
    print(f"{cid}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in measured.items()))
    record_measurement(f"wgrad contract {cid} ({MODE})", **{k: f"{v:.3g}" for k, v in measured.items()})


@pytest.mark.parametrize("cid", list(WC.CASES))
def test_launch_writes_only_what_it_owns(cid):
    """A segment's problem launched alone writes the columns [c_off, c_off + C) of dw and, when c_off == 0 and db was
    asked for, db — every guard element, every other segment's column and the db of a c_off > 0 problem keep the
    sentinel's bits, and nothing lands behind the workspace.  A second launch into buffers holding 3.5 instead gives the
    same bits: written, not accumulated, and deterministic."""
    built, ref = _built(cid)
    _skip_unless_launchable(built)
    case = built.case
    _, _, res = _launches(cid)
    for s, dw, db, stray, dw2, db2 in res:
        o, c = case.c_offs[s], case.segs[s]
        assert stray == 0, f"{cid} segment {s}: {stray} elements outside the problem's own were written"
        assert not bool((dw[:, o:o + c] == WC.SENTINEL).all()), f"{cid} segment {s}: nothing was written"
        assert torch.equal(dw[:, o:o + c], dw2[:, o:o + c]), f"{cid} segment {s}: a second launch gives other bits"
        if o + c < case.cin or o > 0:
            rest = torch.ones(case.cin, dtype=torch.bool)
            rest[o:o + c] = False
            assert bool((dw2[:, rest] == 3.5).all())
        if case.db and o == 0:
            assert torch.equal(db, db2) and not bool((db == WC.SENTINEL).all())
        else:
            assert bool((db2 == 3.5).all()), f"{cid} segment {s}: db belongs to the c_off == 0 problem that asked for it"


@pytest.mark.parametrize("cid", WC.PLANE_CASES)
def test_plane_input_gives_the_bits_of_the_fp32_input(cid):
    """The same values handed over as bf16x3 planes (a window of a NaN-filled plane buffer, made on the host by
    wgrad_contract.to_planes) and as an fp32 window: the staged tile holds the three bf16 terms the in-kernel split makes,
    so dw and db are bit-identical on each of the three tiles — and the plane launch wrote only what it owns."""
    built, ref = _built(cid)
    _skip_unless_launchable(built)
    case = built.case
    got = []
    for plane in (True, False):
        dwbuf, dbbuf = built.outputs()
        p = built.problem(0, dwbuf, dbbuf, plane=plane)
        assert bool(p.flags & L.WGRAD_X_P3) == plane
        _run([p])
        dw, db, stray = built.read(dwbuf, dbbuf, [0], True)
        assert stray == 0
        got.append((dw, db))
    assert torch.equal(got[0][0], got[1][0]), f"{cid}: {(got[0][0] != got[1][0]).sum().item()} elements of dw differ between plane and fp32 input"
    assert torch.equal(got[0][1], got[1][1])
    assert torch.equal(got[0][0], _merged(cid)[0])           # ... and are the bits test_contract_against_float64 holds to the bounds
    WC.check_dw(case, ref, got[1][0], "fp32 input")


PLACEMENT = ("w11", "l3b16", "l3s2b16")        # the gather kernel, the LDS kernel at stride 1 and at stride 2


def _placement_pixels(case):
    return [0, case.K - 1, case.H * case.W + case.W - 1, 31, 32]     # first, last, a corner of image 1, a chunk edge


@pytest.mark.parametrize("cid", PLACEMENT)
def test_exact_placement_of_single_pixels(cid):
    """dy = 0 except 1.0 at five (pixel_i, n_i): row n_i of dw is, bit for bit, the k x k patch of x around s * pixel_i
    with zeros outside the image; every other row is exactly 0, db exactly one-hot.  (A product with 1.0 and a sum with
    zeros is exact on the fp32 pipe and on the bf16x3 pipe, whose three planes add up to x.)"""
    case = WC.CASES[cid]
    pixels = _placement_pixels(case)
    t = WC.one_hot(case, pixels)
    built = WC.build(case, "cuda", t)
    dwbuf, dbbuf = built.outputs()
    _run([built.problem(0, dwbuf, dbbuf)])
    dw, db, stray = built.read(dwbuf, dbbuf, [0], True)
    assert stray == 0
    x = t["segs"][0]
    s, k, pad = case.stride, case.k, case.k // 2
    want = torch.zeros_like(dw)
    for i, p in enumerate(pixels):
        b, r = divmod(p, case.H * case.W)
        oy, ox = divmod(r, case.W)
        for ty in range(k):
            for tx in range(k):
                iy, ix = s * oy + ty - pad, s * ox + tx - pad
                if 0 <= iy < case.Hx and 0 <= ix < case.Wx:
                    want[3 * i + 1, :, ty, tx] = x[b, :, iy, ix]
    assert torch.equal(dw, want), f"{cid}: {(dw != want).sum().item()} elements of dw are not the patch of x"
    want_db = torch.zeros(case.n)
    want_db[[3 * i + 1 for i in range(len(pixels))]] = 1.0
    assert torch.equal(db, want_db)
    assert torch.equal(want.double(), WC.reference(case, t).dw)


@pytest.mark.parametrize("cid", PLACEMENT)
def test_zero_dy_gives_exact_zeros(cid):
    case = WC.CASES[cid]
    t = WC.one_hot(case, [])
    built = WC.build(case, "cuda", t)
    dwbuf, dbbuf = built.outputs()
    _run([built.problem(0, dwbuf, dbbuf)])
    dw, db, stray = built.read(dwbuf, dbbuf, [0], True)
    assert stray == 0 and bool((dw == 0).all()) and bool((db == 0).all())


GROUP = ("w11", "w32", "wk1seg", "wk5s2", "l3b16", "l5a16", "l3s2c64", "l5s2b16", "lk1a", "lseg", "ls4", "gs3")    # 16 problems


def _group_members():
    ids = [c for c in GROUP if not (_needs_lds(WC.CASES[c]))]
    return [(cid,) + _launches(cid) for cid in ids]


def test_group_of_unlike_problems():
    """Sixteen problems of twelve cases in one ``ops.wgrad_group`` (both kernels, every kernel size and stride, several
    tiles, split and unsplit; the three-segment 1x1 case through ``ops.wgrad_problems`` with dw as a 2-D tensor), which
    plans the splits anew against each problem's share: bounds and guards hold.  Then ``vam_conv_wgrad_group`` directly
    with every problem's single-launch splits: the bits of the single launches."""
    members = _group_members()
    for planned in (True, False):
        probs, outs = [], []
        for cid, built, ref, res in members:
            case = built.case
            dwbuf, dbbuf = built.outputs()
            if case.dw2d and planned:
                ps = ops.wgrad_problems(built.x, built.dy, built.dw_view(dwbuf), dbbuf[WC.GUARD:WC.GUARD + case.n])
            else:
                ps = [built.problem(s, dwbuf, dbbuf if (case.db and s == 0) else None) for s in range(len(case.segs))]
            probs += ps
            outs.append((dwbuf, dbbuf))
        assert len(probs) == L.VAM_MAX_WGRAD_GROUP
        if planned:
            ops.wgrad_group(probs)
            torch.cuda.synchronize()
        else:
            _run(probs)
        for (cid, built, ref, res), (dwbuf, dbbuf) in zip(members, outs):
            case = built.case
            dw, db, stray = built.read(dwbuf, dbbuf, range(len(case.segs)), True)
            assert stray == 0, f"{cid} in the group: {stray} elements outside the problem's own were written"
            if planned:
                WC.check_dw(case, ref, dw, "in the group")
                WC.check_db(case, ref, db, "in the group")
            else:
                single, single_db = _merged(cid)
                assert torch.equal(dw, single), f"{cid} in the group: {(dw != single).sum().item()} elements differ from the single launches"
                assert torch.equal(db, single_db)
        for p in probs:
            if getattr(p, "_ws", None) is not None and not planned:
                assert WC.ws_stray(p) == 0


def _refusal_problem(**change):
    built, _ = _built("w11")
    dwbuf, dbbuf = built.outputs()
    p = built.problem(0, dwbuf, dbbuf)
    for k, v in change.items():
        setattr(p, k, v)
    return p, dwbuf, dbbuf, built


@pytest.mark.parametrize("what,why,change", [
    ("a non-square kernel", "square odd kernels", dict(kh=3, kw=1)),
    ("an even kernel", "square odd kernels", dict(kh=2, kw=2)),
    ("stride 2 with a 1x1 kernel", "stride 2 (1, or 2 with k3 / k5", dict(kh=1, kw=1, stride=2, Hx=10, Wx=14)),
    ("stride 2 with Hx != 2 H", "stride 2 (1, or 2 with k3 / k5", dict(stride=2, Hx=9, Wx=14)),
    ("c_off + C > cin_total", "channel window", dict(c_off=4)),
    ("splits without a workspace", "2 pixel splits need a workspace", dict(splits=2)),
    ("a plane input on an ineligible grid", "a plane (P3) input needs the LDS-tiled kernel", dict(flags=L.WGRAD_X_P3)),
])
def test_group_refuses(what, why, change):
    """The refusals of vam_conv_wgrad_group: an error code, the message of the check that is meant, and nothing written."""
    p, dwbuf, dbbuf, built = _refusal_problem(**change)
    assert _group([p]) != 0, what
    msg = L.load().vam_last_error().decode(errors="replace")
    assert why in msg, f"{what}: refused with {msg!r}"
    torch.cuda.synchronize()
    assert built.read(dwbuf, dbbuf, [], False)[2] == 0, f"{what}: refused, yet something was written"


def test_group_refuses_bad_problem_counts():
    p, dwbuf, dbbuf, built = _refusal_problem()
    arr = (L.VamWgrad * (L.VAM_MAX_WGRAD_GROUP + 1))(*([p] * (L.VAM_MAX_WGRAD_GROUP + 1)))
    lib = L.load()
    for count in (0, L.VAM_MAX_WGRAD_GROUP + 1):
        assert lib.vam_conv_wgrad_group(arr, count, ops.stream_ptr()) != 0
        assert f"1..{L.VAM_MAX_WGRAD_GROUP} problems" in lib.vam_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert built.read(dwbuf, dbbuf, [], False)[2] == 0


@pytest.mark.parametrize("n_pix", [1, 4095, 8195])
@pytest.mark.parametrize("n", [4, 36])
def test_colsum_against_float64(n_pix, n):
    """``vam_colsum`` (one and two pixel ranges; 8195 = 2 x 4097 + 1) on a window of a wider NaN-filled buffer with a
    NaN-filled workspace: |out - sum64| <= (K + 4) 2^-24 sum |dy|, the db bound; the guards beside ``out`` hold."""
    import vampic.synth as synth
    lib = L.load()
    dy = synth.normal((n_pix, n), 31 + n)
    buf = torch.full((1, 1, n_pix + 1, n + 12), float("nan"), device="cuda")
    buf[0, 0, :n_pix, 8:8 + n] = dy.cuda()
    view = ops.View(buf[:, :, :n_pix], 8, n)
    assert view.n_pix == n_pix and view.ld == n + 12
    ws = torch.full((lib.vam_colsum_workspace(n_pix, n) // 4 + WC.GUARD,), float("nan"), device="cuda")
    ws[-WC.GUARD:] = WC.SENTINEL
    out = torch.full((WC.GUARD + n + WC.GUARD,), WC.SENTINEL, device="cuda")
    L.check(lib.vam_colsum(view.ptr, view.ld, n_pix, n, out.data_ptr() + 4 * WC.GUARD, ws.data_ptr(), ops.stream_ptr()), "vam_colsum")
    torch.cuda.synchronize()
    out, ws = out.cpu(), ws.cpu()
    assert bool((out[:WC.GUARD] == WC.SENTINEL).all()) and bool((out[-WC.GUARD:] == WC.SENTINEL).all())
    assert bool((ws[-WC.GUARD:] == WC.SENTINEL).all())
    got = out[WC.GUARD:WC.GUARD + n]
    assert bool(torch.isfinite(got).all())
    want, scale = dy.double().sum(0), dy.double().abs().sum(0)
    r = float(((got.double() - want).abs() / ((n_pix + 4) * WC.U * scale)).max())
    print(f"colsum n_pix {n_pix} N {n}: error / bound {r:.3g}")
    from conftest import record_measurement
    record_measurement(f"colsum contract n_pix {n_pix} N {n}", out=f"{r:.3g}")
    assert r <= 1.0


@pytest.mark.parametrize("env", [{"VAMPIC_WGRAD": "f32"}, {"VAMPIC_WGRAD_LDS": "0"}], ids=["f32", "lds0"])
def test_contract_in_the_other_modes(env):
    """VAMPIC_WGRAD=f32 (the fp32-pipe loop of the register-gather kernel, also the automatic path of tensors of 2 GiB and
    more) and VAMPIC_WGRAD_LDS=0 (every grid through the register-gather kernel's larger tiles) are read once per process:
    the tests above run again in a fresh child process for each, case table and bounds unchanged.  The plane-input cases
    skip themselves there (vam_conv_wgrad_route: no LDS kernel)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not other_modes"],
                       env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "passed" in r.stdout
