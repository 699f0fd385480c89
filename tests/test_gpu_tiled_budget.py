"""Tiled pictures whose rounds end at byte budgets, end to end on the GPU (vampic.tiled.encode(allocation="picture",
max_bytes=), tiled.budget_marks, evaluate.tiled_rd_at_sizes).  The oracle is the existing path: a
budgeted stream is byte for byte the stream ``encode(marks=)`` gives for the solved qualities, those hold the budgets on
the real bytes, and the same call with every quality raised by q_tol does not.  No time and no PSNR value is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_embedded_schedule import _net, _x                      # noqa: E402
from vampic import embedded as EB, evaluate as EV, tiled as TL      # noqa: E402

MARKS = [0.5, 2.5, 6.6]
Q_TOL = 1e-3
PIC = dict(tile=64, overlap=16)                                      # section 9w's 150 x 200 picture: 3 x 4 tiles
_CACHE = {}


def _image():
    return _x(1, 150, 200)[0]


def _marked(marks, **kw):
    """encode(allocation="picture", marks=) on the existing path, coded once per argument set."""
    key = ("marks", tuple(marks), tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = TL.encode(_net(), _image(), marks=list(marks), allocation="picture", **dict(dict(PIC, group=4), **kw))
    return _CACHE[key]


def _budgeted(budgets, **kw):
    key = ("bytes", tuple(budgets), tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = TL.encode(_net(), _image(), max_bytes=list(budgets), allocation="picture", q_tol=Q_TOL,
                                **dict(dict(PIC, group=4), **kw))
    return _CACHE[key]


def _r():
    """r_0, r_1, r_2: where the rounds of the reference marks end."""
    return TL.layout(_marked(MARKS))["round_end"][:3]


def test_budgets_at_the_reference_s_round_ends_reach_its_marks():
    r = _r()
    data = _budgeted(r)
    lay = TL.layout(data)
    assert data[4] == 2 and lay["allocation"] == "picture" and lay["n_rounds"] == 4 and len(lay["marks"]) == 3
    got = TL.budget_marks(data)
    assert [q for q, _ in got] == lay["marks"] and [e for _, e in got] == lay["round_end"][:3]
    for k, (q, end) in enumerate(got):
        print(f"budget {r[k]}: q = {q!r}, round_end = {end}")
        assert q >= MARKS[k] - Q_TOL and end <= r[k]


@pytest.mark.parametrize("shift", [-1, 1000])
def test_a_budgeted_stream_is_the_marked_stream_of_the_solved_qualities(shift):
    net = _net()
    budgets = [v + shift for v in _r()]
    data = _budgeted(budgets)
    solved = TL.budget_marks(data)
    qs = [q for q, _ in solved]
    again = _marked(qs)
    assert again == data                                             # byte-identical to the existing path
    raised = TL.layout(_marked([min(q + Q_TOL, 10.0) for q in qs]))["round_end"]
    for k, (q, end) in enumerate(solved):
        print(f"budget {budgets[k]}: q = {q!r}, round_end = {end}, at q + q_tol: {raised[k]}")
        assert end <= budgets[k]
        assert q == 10.0 or raised[k] > budgets[k]                   # maximal at q_tol
        assert len(TL.extract(data, rounds=k + 1)) <= budgets[k]
    if shift < 0:
        ref = TL.PictureDecoder(net, again, group=4)
        for k, (_, end) in enumerate(solved):                        # decode(mark=) checks the pooled counts on its own sigma
            cut = TL.PictureDecoder(net, data[:end], group=4).decode(mark=k)
            assert torch.equal(cut, ref.decode(mark=k)), k
    heads = [data[o:o + n] for row in TL.layout(data)["head"] for o, n in row if n]
    count = np.asarray([EB.layout(h)["marks"]["count"] for h in heads], dtype=np.float64)            # [tiles, marks, ns]
    frac = count[:, 1].sum(-1) / (net.ns0 * net.dim_chunk * 16)
    assert len(set(frac.tolist())) >= 2, frac                        # a busy tile spends more of the budget than a flat one


def test_a_budget_above_the_whole_picture_gives_quality_ten():
    whole = len(_marked(MARKS))
    data = _budgeted([whole + 100000])
    assert [q for q, _ in TL.budget_marks(data)] == [10.0]
    assert TL.layout(data)["round_end"][0] <= whole + 100000
    assert _marked([10.0]) == data


def test_the_bytes_do_not_depend_on_the_group():
    budgets = [v - 1 for v in _r()]
    assert _budgeted(budgets, group=1) == _budgeted(budgets) == _budgeted(budgets, group=5)


def test_the_device_coder_on_lanes_solves_what_the_host_coder_solves():
    wide = TL.layout(_marked(MARKS, lanes=64, base_lanes=8))["round_end"][:3]      # 64 states per stream: longer heads and rounds
    budgets = [v - 1 for v in wide]
    host = _budgeted(budgets, lanes=64, base_lanes=8, coder="host")
    dev = _budgeted(budgets, lanes=64, base_lanes=8, coder="device", group=6)
    assert TL.budget_marks(dev) == TL.budget_marks(host) and dev == host
    lay = TL.layout(dev)
    assert (lay["lanes"], lay["base_lanes"]) == (64, 8) and all(e <= N for e, N in zip(lay["round_end"], budgets))
    narrow = [v - 1 for v in _r()]                                   # one lane: other strings, other budgets
    assert _budgeted(narrow, coder="device") == _budgeted(narrow, coder="host")


def test_every_refusal_names_its_budget_and_a_correct_call_follows():
    net, x, r = _net(), _image(), _r()
    enc = lambda **kw: TL.encode(net, x, allocation=kw.pop("allocation", "picture"), **dict(PIC, **kw))
    heads_end = TL.layout(_budgeted(r))["need_bytes"]                 # three marks: the header, then every tile's head
    with pytest.raises(ValueError, match="give max_bytes or marks, not both"):
        enc(max_bytes=r, marks=MARKS)
    with pytest.raises(ValueError, match="give max_bytes or schedule, not both"):
        enc(max_bytes=r, schedule=torch.ones((1, 150, 200), device="cuda"), allocation="tile")
    for allocation in ("tile", "image"):
        with pytest.raises(ValueError, match="max_bytes goes with allocation='picture'|allocation is one of"):
            enc(max_bytes=r, allocation=allocation)
    with pytest.raises(ValueError, match=rf"budget 1, {r[0]} bytes, does not exceed budget 0, {r[0]} bytes"):
        enc(max_bytes=[r[0], r[0], r[2]])
    with pytest.raises(ValueError, match=rf"budget 0, {heads_end - 1} bytes, is below heads_end = {heads_end} bytes"):
        enc(max_bytes=[heads_end - 1, r[1], r[2]])
    with pytest.raises(ValueError, match=rf"budget 0, {heads_end + 4} bytes, holds the heads \({heads_end} bytes\) but no round: the "
                                         r"smallest quality tried, [0-9.e-]+, needs \d+ bytes"):
        enc(max_bytes=[heads_end + 4, r[1], r[2]])
    whole = len(_marked(MARKS))
    with pytest.raises(ValueError, match=rf"budgets 1 and 2, {whole + 5000} and {whole + 5001} bytes, solve to the same quality 10"):
        enc(max_bytes=[r[0], whole + 5000, whole + 5001])
    with pytest.raises(ValueError, match="1 .. 32 budgets, got 33"):
        enc(max_bytes=list(range(r[0], r[0] + 33)))
    with pytest.raises(ValueError, match="q_tol must be > 0"):
        enc(max_bytes=r, q_tol=0.0)
    with pytest.raises(ValueError, match="not picture-wide"):
        TL.budget_marks(TL.encode(net, x, marks=MARKS, **PIC))
    assert enc(max_bytes=r, group=4) == _budgeted(r)
    assert enc(max_bytes=r[1], group=4) == _budgeted([r[1]])          # one budget, given as a number


def test_tiled_rd_at_sizes_runs():
    r = _r()
    rows = EV.tiled_rd_at_sizes(_net(), _image(), r, tile=64, overlap=16, group=4, q_tol=Q_TOL)
    solved = TL.budget_marks(_budgeted(r))
    for k, row in enumerate(rows):
        assert (row["q"], row["bytes"]) == solved[k] and row["bytes"] <= row["budget"] == r[k]
        assert row["bpp"] == 8.0 * row["bytes"] / (150 * 200) and np.isfinite(row["psnr"]) and row["allocation"] == "picture"
        assert 0 <= row["kept_min"] <= row["kept_max"] <= 1
    assert any(row["kept_min"] < row["kept_max"] for row in rows)
