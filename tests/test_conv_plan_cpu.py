"""The host half of the convolution launch path, without a GPU: ``vam_conv_plan`` runs the contract checks and the tile
heuristic of ``vam_conv_group`` and launches nothing.

* tests/golden/conv_tile_choice.json pins every tile decision: the problems of each ``vam_conv_group`` call of inference
  (32x3x256x256, 1x3x256x256, 1x3x64x64), a quality sweep, a bf16-storage forward, one step of the three training plans
  and a forward in the fp32 and fp16x2 modes, with the tile the call took — recorded on an MI355X at the commit before
  ``vam_conv_plan`` existed, so a slip in a factor, a candidate list or a fallback shows here although every tile
  computes the same bits.
* every rule the launch path refuses a problem by, and every rule of the weight-pack entry points, with its message.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from vampic import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "conv_tile_choice.json")
ADDR = 0x10000          # a 16-byte aligned address that is never dereferenced
VAM_EINVAL = -1
AUX = ("pre", "mul", "post", "post2", "preact")
PTRS = ("wpack", "bias", "out", "out_amax")


def _problem(fields, values):
    """A vam_conv from a row of the golden table; non-null pointers become ADDR."""
    c = L.VamConv()
    for name, v in zip(fields, values):
        if name.startswith("seg"):
            s, k = int(name[3]), name[5:]
            setattr(c.seg[s], k, (ADDR if v else None) if k == "ptr" else v)
        elif name.startswith("in_amax"):
            c.in_amax[int(name[7:])] = ADDR if v else None
        elif "." in name:
            a, k = name.split(".")
            setattr(getattr(c, a), k, (ADDR if v else None) if k == "ptr" else v)
        elif name in PTRS:
            setattr(c, name, ADDR if v else None)
        else:
            setattr(c, name, v)
    return c


def _plan(lib, probs):
    ch = L.VamConvChoice()
    rc = lib.vam_conv_plan((L.VamConv * max(len(probs), 1))(*probs), len(probs), C.byref(ch))
    return rc, ch


def check_entries(spec_env=None):
    """Plan every entry of the table recorded with VAMPIC_SPEC = spec_env (None: unset) and compare all it holds."""
    lib = L.load()
    doc = json.load(open(GOLD))
    fields, table = doc["fields"], doc["problems"]
    entries = [e for e in doc["entries"] if e.get("spec_env") == spec_env]
    assert entries
    mode0 = lib.vam_conv_get_mode()
    wrong = []
    try:
        for k, e in enumerate(entries):
            assert lib.vam_conv_set_mode(e["mode"]) == 0
            lib.vam_conv_force_tile(*e.get("force", (0, 0, 0)))
            rc, ch = _plan(lib, [_problem(fields, table[i]) for i in e["problems"]])
            assert rc == 0, (e["from"], lib.vam_last_error())
            n = len(e["problems"])
            got = ([ch.bm, ch.bn, ch.bk], ch.spec, ch.blocks, list(ch.dual)[:n], list(ch.staged)[:n])
            want = (e["tile"], e["spec"], e["blocks"], e["dual"], e["staged"])
            if got != want:
                wrong.append((k, e["from"], e.get("force"), got, want))
            assert not any(list(ch.dual)[n:]) and not any(list(ch.staged)[n:])
    finally:
        lib.vam_conv_force_tile(0, 0, 0)
        lib.vam_conv_set_mode(mode0)
    assert not wrong, f"{len(wrong)} of {len(entries)} entries differ from the recording, first: {wrong[:3]}"
    return len(entries)


def _check_in_child(spec_env):
    """VAMPIC_SPEC is read once per process: plan the entries recorded under a value of it in a fresh child."""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_conv_plan_cpu as T; print('PLANNED', T.check_entries({spec_env!r}))"
    env = {k: v for k, v in os.environ.items() if k != "VAMPIC_SPEC"}
    if spec_env is not None:
        env["VAMPIC_SPEC"] = spec_env
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PLANNED" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return int(r.stdout.split("PLANNED")[1].split()[0])


def test_tile_choice_equals_the_recording():
    n = check_entries(None) if "VAMPIC_SPEC" not in os.environ else _check_in_child(None)
    assert n >= 900


def test_table_holds_the_decision_boundaries():
    """What the table must contain to be worth its name (counted from the file, not from the code under test)."""
    doc = json.load(open(GOLD))
    f = {n: i for i, n in enumerate(doc["fields"])}
    P = doc["problems"]

    def cin(p):
        return sum(p[f[f"seg{s}.C"]] for s in range(p[f["n_seg"]]))

    def chunks(e):
        return min(P[i][f["kh"]] * P[i][f["kw"]] * ((cin(P[i]) + 31) // 32) for i in e["problems"])

    E = doc["entries"]
    auto = [e for e in E if "force" not in e and "spec_env" not in e]
    assert any(len(set(e["problems"])) > 1 for e in auto), "a group of unlike problems"
    assert any(any(e["dual"]) and all(cin(P[i]) == 16 and P[i][f["kh"]] * P[i][f["kw"]] > 1 for i in e["problems"]) for e in auto), "a dual problem"
    assert any(all(P[i][f["kh"]] == 1 and P[i][f["kw"]] == 1 for i in e["problems"]) and
               max(cin(P[i]) for i in e["problems"]) <= 256 for e in auto), "a 1x1 thin-K layer"
    assert any(e["tile"][:2] == [128, 224] and e["spec"] == 1 for e in auto), "a layer on 128x224"
    assert any(e["mode"] == 1 and all(P[i][f["N"]] == 224 for i in e["problems"]) and len(e["problems"]) == 8 and
               e["tile"][1] != 224 and chunks(e) < 16 for e in auto), "a 224-channel group kept off 128x224 by min_chunks < 16"
    forced = {(tuple(e["force"][:2]), tuple(e["tile"][:2])) for e in E if "force" in e}
    assert {((128, 224), (128, 128)), ((128, 160), (128, 96)), ((64, 160), (64, 64)), ((64, 96), (64, 64))} <= forced
    assert {e["spec_env"] for e in E if "spec_env" in e} == {"0", "1"}
    assert {e["mode"] for e in E} == {0, 1, 3} and any(P[i][f["flags"]] & L.CONV_W_BF16 for e in E for i in e["problems"])


@pytest.mark.parametrize("spec_env", ["0", "1"])
def test_vampic_spec_in_a_child_process(spec_env):
    assert _check_in_child(spec_env) == 1


# ---------------------------------------------------------------------------------------------------------- refusals
def _base(kind="f32"):
    """A valid 32-channel 3x3 problem on 1x8x8.  kind: fp32 tensors; "bf16": bf16 weights and input; "p3": bf16x3-plane
    input; "2seg": two 32-channel input segments."""
    c = L.VamConv()
    c.n_seg = 2 if kind == "2seg" else 1
    for s in range(c.n_seg):
        c.seg[s].ptr, c.seg[s].C, c.seg[s].ld = ADDR, 32, 32
    c.B, c.H, c.W, c.kh, c.kw, c.stride, c.pad_y, c.pad_x, c.Ho, c.Wo, c.N = 1, 8, 8, 3, 3, 1, 1, 1, 8, 8, 32
    c.wpack, c.bias, c.out = ADDR, ADDR, ADDR
    c.ldo, c.Hf, c.Wf, c.osy, c.osx = 32, 8, 8, 1, 1
    c.flags = {"bf16": L.CONV_W_BF16 | L.CONV_IN_BF16, "p3": L.CONV_IN_BF3}.get(kind, 0)
    return c


def _edit(c, path, value):
    obj = c
    parts = path.split(".")
    for p in parts[:-1]:
        obj = obj[int(p)] if p.isdigit() else getattr(obj, p)
    setattr(obj, parts[-1], value)


BIG = 1 << 15
# (what, base kind, arithmetic mode, {field: value}, in a group behind an unedited base, message).  One field per row, but
# for "too many pixels", which no single field reaches before an earlier rule does, and the two fields of preact.
REFUSALS = [
    ("n_seg", "f32", 1, {"n_seg": 0}, False, "conv[0]: n_seg 0"),
    ("extent", "f32", 1, {"B": 0}, False, "conv[0]: bad extent"),
    ("taps", "f32", 1, {"kh": 6}, False, "conv[0]: kernel 6x3 stride 1"),
    ("stride", "f32", 1, {"stride": 3}, False, "conv[0]: kernel 3x3 stride 3"),
    ("null weights", "f32", 1, {"wpack": None}, False, "conv[0]: null weights/output"),
    ("mixed storage", "f32", 1, {"flags": L.CONV_W_BF16}, True, "conv group mixes bf16-storage and fp32 problems"),
    ("bf16 input, fp32 weights", "f32", 1, {"flags": L.CONV_IN_BF16}, False, "conv[0]: bf16 input needs bf16-packed weights (VAM_CONV_W_BF16)"),
    ("bf16 and planes", "f32", 1, {"flags": L.CONV_W_BF16 | L.CONV_OUT_BF3}, False, "conv[0]: bf16 storage and bf16x3 planes do not combine"),
    ("bf16 output placement", "f32", 1, {"flags": L.CONV_OUT_BF16 | L.CONV_OUT_NCHW}, False, "conv[0]: bf16 output needs plain NHWC placement, ldo % 4 == 0"),
    ("bf16 operands", "f32", 1, {"flags": L.CONV_AUX_BF16 | L.CONV_OUT_NCHW}, False, "conv[0]: bf16 epilogue operands need the vector epilogue"),
    ("mixed planes", "f32", 1, {"flags": L.CONV_IN_BF3}, True, "conv group mixes fp32 and bf16x3-plane inputs"),
    ("fp16x2 without amax", "f32", 3, {}, False, "conv[0]: the fp16x2 mode needs in_amax[0] (max |x| of that input segment: vam_absmax, or its producer's out_amax)"),
    ("planes in the fp32 mode", "f32", 0, {"flags": L.CONV_OUT_BF3}, False, "conv[0]: bf16x3-plane tensors need the split-operand mode"),
    ("squared planes", "p3", 1, {"flags": L.CONV_IN_BF3 | L.CONV_SQUARE_IN}, False, "conv[0]: SQUARE_IN needs fp32 input"),
    ("plane output placement", "f32", 1, {"flags": L.CONV_OUT_BF3 | L.CONV_OUT_NCHW}, False, "conv[0]: bf16x3-plane output needs plain NHWC placement, N % 8 == 0 and ldo (groups) >= N/8"),
    ("bf16 segment", "bf16", 1, {"seg.0.ld": 24}, False, "conv[0]: bf16 segment 0 invalid"),
    ("bf16 segment alignment", "bf16", 1, {"seg.0.ptr": ADDR + 8}, False, "conv[0]: segment 0 not 16-byte aligned"),
    ("plane segment", "p3", 1, {"seg.0.C": 36}, False, "conv[0]: bf16x3 segment 0 invalid"),
    ("plane segment alignment", "p3", 1, {"seg.0.ptr": ADDR + 8}, False, "conv[0]: segment 0 not 16-byte aligned"),
    ("segment", "f32", 1, {"seg.0.ld": 16}, False, "conv[0]: segment 0 invalid"),
    ("segment alignment", "f32", 1, {"seg.0.ld": 34}, False, "conv[0]: segment 0 not 16-byte aligned"),
    ("segment pointer alignment", "f32", 1, {"seg.0.ptr": ADDR + 4}, False, "conv[0]: segment 0 not 16-byte aligned"),
    ("Cin", "f32", 1, {"seg.0.C": 24}, False, "conv[0]: Cin 24 not a multiple of 16"),
    ("input window", "f32", 1, {"B": 262144}, False, "conv[0]: input window larger than 2 GiB (32-bit buffer offsets)"),
    ("packed weights", "f32", 1, {"N": 1250000}, False, "conv[0]: packed weights larger than 2 GiB"),
    ("segment boundary", "2seg", 1, {"seg.0.C": 16}, False, "conv[0]: segment boundary 16 not a multiple of BK=32"),
    ("mixed BK", "f32", 0, {"seg.0.C": 16}, True, "conv group mixes BK=32 and BK=16 problems"),
    ("output grid", "f32", 1, {"Ho": 13}, False, "conv[0]: output grid larger than the input allows"),
    ("PS2", "f32", 1, {"flags": L.CONV_PS2}, False, "conv[0]: PS2 geometry"),
    ("placement", "f32", 1, {"osy": 0}, False, "conv[0]: output placement outside Hf x Wf"),
    ("placement extent", "f32", 1, {"Hf": 7}, False, "conv[0]: output placement outside Hf x Wf"),
    ("N", "f32", 1, {"N": 30}, False, "conv[0]: N 30 not a multiple of 4"),
    ("output pitch alignment", "f32", 1, {"ldo": 34}, False, "conv[0]: output/bias not 16-byte aligned"),
    ("bias alignment", "f32", 1, {"bias": ADDR + 4}, False, "conv[0]: output/bias not 16-byte aligned"),
    ("operand alignment", "f32", 1, {"post.ptr": ADDR + 4}, False, "conv[0]: epilogue operand not aligned"),
    ("ldo", "f32", 1, {"ldo": 16}, False, "conv[0]: ldo 16 < channels"),
    ("pixels", "f32", 1, {"Ho": BIG, "Wo": BIG, "pad_y": BIG, "pad_x": BIG, "Hf": BIG, "Wf": BIG}, False, "conv[0]: too many pixels"),
    ("flag bits", "f32", 1, {"flags": 1 << 20}, False, "conv[0]: unknown flag bits 0x100000"),
    ("dual problem on planes", "p3", 1, {"seg.0.C": 16}, False, "conv[0]: a 16-channel multi-tap problem takes one fp32 input segment (its weights are packed two taps per chunk)"),
    ("GELU gradient without mul", "f32", 1, {"flags": L.CONV_MUL_GELU_GRAD}, False, "conv[0]: VAM_CONV_MUL_GELU_GRAD needs an fp32 mul operand (the GELU's pre-activation)"),
    ("preact", "f32", 1, {"preact.ptr": ADDR, "preact.ld": 16}, False, "conv[0]: preact is an fp32 NHWC tensor indexed like the output (16-byte aligned, ld % 4 == 0, ld >= channels)"),
]


@pytest.fixture()
def conv_lib():
    lib = L.load()
    mode0 = lib.vam_conv_get_mode()
    yield lib
    lib.vam_conv_set_mode(mode0)


def test_every_base_problem_plans(conv_lib):
    """The cap of the refusal table: each base is accepted in each mode a row uses it in, alone and behind itself in a
    group, so a row can only be refused for the one thing it changes."""
    for kind, mode in sorted({(r[1], r[2]) for r in REFUSALS}):
        assert conv_lib.vam_conv_set_mode(mode) == 0
        c = _base(kind)
        if mode == 3:
            continue          # the fp16x2 row IS the unedited base: its refusal is the mode's own rule (in_amax)
        for probs in ([c], [c, _base(kind)]):
            rc, ch = _plan(conv_lib, probs)
            assert rc == 0, (kind, mode, conv_lib.vam_last_error())
            assert ch.blocks == 8 * len(probs)      # 64 positions x 32 channels: one tile per problem whatever the tile
    conv_lib.vam_conv_set_mode(3)
    c = _base()
    c.in_amax[0] = ADDR
    assert _plan(conv_lib, [c])[0] == 0


@pytest.mark.parametrize("row", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_invalid_problem_is_refused_with_its_message(conv_lib, row):
    _, kind, mode, edits, grouped, message = row
    assert conv_lib.vam_conv_set_mode(mode) == 0
    c = _base(kind)
    for path, v in edits.items():
        _edit(c, path, v)
    rc, _ = _plan(conv_lib, [_base(kind), c] if grouped else [c])
    text = conv_lib.vam_last_error().decode()
    assert rc == VAM_EINVAL, (rc, text)
    assert (message.replace("conv[0]", "conv[1]") if grouped else message) in text, text


def test_group_size_and_null_arguments_are_refused(conv_lib):
    ch = L.VamConvChoice()
    nine = (L.VamConv * 9)(*[_base() for _ in range(9)])
    for arr, n in ((nine, 0), (nine, 9), (None, 1)):
        assert conv_lib.vam_conv_plan(arr, n, C.byref(ch)) == VAM_EINVAL
        assert "vam_conv_group: 1..8 problems" in conv_lib.vam_last_error().decode()
    assert conv_lib.vam_conv_plan(nine, 1, None) == VAM_EINVAL


# (what, {argument: value}, message with {who}); the valid base packs a 32 -> 32 3x3 convolution
PACK_BASE = dict(mode=L.PACK_CONV, phase=-1, kh=3, kw=3, cin=32, n=32)
PACK_RULES = [
    ("PS2", dict(mode=L.PACK_PS2, n=30), "PS2 pack needs N % 4 == 0"),
    ("merged deconv", dict(mode=L.PACK_DECONV5S2, kh=5), "merged deconv pack needs 3x3, N=4*Cout"),
    ("deconv phase", dict(mode=L.PACK_DECONV5S2, phase=1), "deconv phase 1 needs kh/kw = 3|2"),
    ("deconv phase number", dict(mode=L.PACK_DECONV5S2, phase=4, kh=2, kw=2), "deconv phase 4 needs kh/kw = 3|2"),
    ("GDN", dict(mode=L.PACK_GDN), "GDN pack is 1x1 and square"),
    ("GDN transposed", dict(mode=L.PACK_GDN_T, kh=1, kw=1, n=64), "GDN pack is 1x1 and square"),
]


@pytest.fixture(scope="module")
def pack_buffers():
    """(src, dst) for the pack entry points.  Every row is refused before anything is launched; should one ever not be, the
    launch must find real memory where there is a GPU (and fails cleanly where there is none)."""
    import torch
    if torch.cuda.is_available():
        t = torch.zeros(2, 1 << 20, device="cuda")
        return t[0].data_ptr(), t[1].data_ptr(), t
    return ADDR, ADDR, None


@pytest.mark.parametrize("rule", PACK_RULES + [
    ("geometry", dict(kh=0), "vam_pack_conv_weights: bad arguments"),
    ("mode", dict(mode=9), "vam_pack_conv_weights: bad mode 9")], ids=lambda r: r[0])
def test_pack_conv_weights_refusals(conv_lib, pack_buffers, rule):
    src, dst, _ = pack_buffers
    a = dict(PACK_BASE, **rule[1])
    rc = conv_lib.vam_pack_conv_weights(src, dst, a["mode"], a["phase"], a["kh"], a["kw"], a["cin"], a["n"], None)
    assert rc == VAM_EINVAL and rule[2] in conv_lib.vam_last_error().decode(), conv_lib.vam_last_error()


def test_pack_entry_points_refuse_null_buffers(conv_lib, pack_buffers):
    src, dst, _ = pack_buffers
    a = PACK_BASE
    for fn, who in ((conv_lib.vam_pack_conv_weights, "vam_pack_conv_weights"), (conv_lib.vam_pack_conv_weights_bf16, "vam_pack_conv_weights_bf16")):
        for s, d in ((None, dst), (src, None)):
            assert fn(s, d, a["mode"], a["phase"], a["kh"], a["kw"], a["cin"], a["n"], None) == VAM_EINVAL
            assert f"{who}: bad arguments" in conv_lib.vam_last_error().decode()
        assert fn(src, dst, 9, a["phase"], a["kh"], a["kw"], a["cin"], a["n"], None) == VAM_EINVAL
        assert f"{who}: bad mode 9" in conv_lib.vam_last_error().decode()
    # the rules the bf16-storage pack shares with the others
    for _, edit, message in PACK_RULES[:4]:
        b = dict(a, **edit)
        assert conv_lib.vam_pack_conv_weights_bf16(src, dst, b["mode"], b["phase"], b["kh"], b["kw"], b["cin"], b["n"], None) == VAM_EINVAL
        assert message in conv_lib.vam_last_error().decode()


@pytest.mark.parametrize("rule", PACK_RULES + [
    ("geometry", dict(kh=0), "vam_pack_group: job 1: bad geometry / mode"),
    ("mode", dict(mode=9), "vam_pack_group: job 1: bad geometry / mode"),
    ("null source", dict(src=None), "vam_pack_group: job 1: bad arguments"),
    ("channels", dict(n=0), "vam_pack_group: job 1: bad arguments")], ids=lambda r: r[0])
def test_pack_group_refusals(conv_lib, pack_buffers, rule):
    """The grouped pack of the split-operand mode validates every job before its one launch: a bias job, then the job
    under test."""
    src, dst, _ = pack_buffers
    assert conv_lib.vam_conv_set_mode(1) == 0
    a = dict(dict(PACK_BASE, src=src), **rule[1])
    jobs = (L.VamPackJob * 2)()
    jobs[0].src, jobs[0].dst, jobs[0].bias, jobs[0].mode, jobs[0].n = src, dst, 1, L.PACK_CONV, 32
    j = jobs[1]
    j.src, j.dst, j.bias, j.mode, j.phase, j.kh, j.kw, j.cin, j.n = a["src"], dst, 0, a["mode"], a["phase"], a["kh"], a["kw"], a["cin"], a["n"]
    rc = conv_lib.vam_pack_group(jobs, 2, None)
    assert rc == VAM_EINVAL and rule[2] in conv_lib.vam_last_error().decode(), conv_lib.vam_last_error()
    assert conv_lib.vam_pack_group(jobs, 0, None) == VAM_EINVAL and "vam_pack_group: no jobs" in conv_lib.vam_last_error().decode()
