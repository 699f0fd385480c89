"""The interleaved base of an "embedded-4" container on the host: z and the base slices as interleaved
strings on Kb lanes, the strict rule that needs them whole, and the host-only container helpers.  No GPU is needed."""
import numpy as np
import pytest

from vampic import bitstream as bs
from vampic import embedded as EB
import rans_interleaved_ref as ref
from base_lanes_cases import GEOMETRIES, container, window_case, window_jobs
from test_rans_core_cpu import _tables

LANES = [1, 2, 8, 64]


@pytest.fixture(scope="module")
def tables():
    return _tables(widths=tuple(range(1, 33)))               # 32 tables: idx = NULL on 32 channels has one each


@pytest.fixture(scope="module")
def windows(tables):
    """geometry -> (jobs with an index buffer, jobs with index = channel), built once."""
    out = {}
    for g, geom in enumerate(GEOMETRIES):
        out[geom] = tuple(window_jobs(*window_case(tables, geom, seed=11 + 2 * g + ch, channel_index=bool(ch)), geom) for ch in (0, 1))
    return out


@pytest.mark.parametrize("K", LANES)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_window_jobs_are_the_restatements_strings(tables, windows, geom, K):
    """n = 12 < K = 64, n = 512 a multiple of every K, n = 1000 a multiple of 8 but not of 64."""
    B, h, w, ld, c0, C, ns = geom
    for jobs in windows[geom]:
        assert len(jobs) == B * ns and all(s.shape == (C, h, w) for s, _ in jobs)
        got = bs.encode_interleaved_streams(jobs, tables, lanes=K)
        for (sym, idx), string in zip(jobs[:2] + jobs[-1:], got[:2] + got[-1:]):          # the restatement is slow: three per case
            assert string == ref.encode(sym, idx, tables, K)
        if K == 1:
            assert got == bs.encode_streams(jobs, tables)
        for (sym, idx), string in zip(jobs, got):
            assert np.array_equal(bs.decode_interleaved_strict(string, idx, tables, K), sym.reshape(-1))


@pytest.mark.parametrize("K", [2, 8, 64])
def test_the_base_is_needed_whole(tables, windows, K):
    geom = GEOMETRIES[0]                                     # n = 12: every proper byte prefix is tried
    sym, idx = windows[geom][0][1]
    string = bs.encode_interleaved(sym, idx, tables, K)
    out, count, st = bs.decode_interleaved_counted(string, idx, tables, K)
    assert (count, st) == (sym.size, 0) and np.array_equal(out, sym.reshape(-1))
    for cut in range(len(string)):
        out, count, st = bs.decode_interleaved_counted(string[:cut], idx, tables, K)
        assert st == 0 and count < sym.size, cut
        assert np.array_equal(out[:count], sym.reshape(-1)[:count]) and not out[count:].any()
        with pytest.raises(ValueError, match=rf"base stream \(image 1, slice 0\): bitstream truncated \({count} of 12 elements"):
            bs.decode_interleaved_strict(string[:cut], idx, tables, K, "base stream (image 1, slice 0)")
    bad = idx.copy().reshape(-1)
    bad[7] = tables.cdf.shape[0]                             # one corrupted index
    out, count, st = bs.decode_interleaved_counted(string, bad, tables, K)
    assert (count, st) == (7, 2)                            # the lanes below the failing one finish their element
    with pytest.raises(ValueError, match=r"z stream \(image 0\): index out of range"):
        bs.decode_interleaved_strict(string, bad, tables, K, "z stream (image 0)")


def test_a_longer_string_is_cut_at_every_word(tables, windows):
    sym, idx = windows[GEOMETRIES[2]][0][0]                  # n = 1000 on 64 lanes
    string = bs.encode_interleaved(sym, idx, tables, 64)
    for cut in range(0, len(string), 4):
        assert bs.decode_interleaved_counted(string[:cut], idx, tables, 64)[1] < sym.size, cut
    assert np.array_equal(bs.decode_interleaved_strict(string, idx, tables, 64), sym.reshape(-1))


# ------------------------------------------------------------------------------------------------ container helpers
def _lens(c):
    return [len(s) for s in c["embedded"]]


@pytest.mark.parametrize("scheduled", [False, True])
def test_check_container_accepts_the_new_format(scheduled):
    c = container(scheduled)
    assert EB._check_container(c) == 2 and EB._base_lanes(c) == 8 and EB._scheduled(c) is scheduled
    assert EB._check_container(container(scheduled, lanes=1)) == 1           # "lanes" is carried for K = 1 too
    assert EB.container_bytes(c) == [10, 10, 100]
    with pytest.raises(ValueError, match='format \'embedded-4\' carries "base_lanes", this one lacks it'):
        EB._check_container({k: v for k, v in c.items() if k != "base_lanes"})
    with pytest.raises(ValueError, match='carries base_lanes > 1; "base_lanes": 1 is format \'embedded-1\''):
        EB._check_container(dict(c, base_lanes=1))
    for bad in (3, 128, 0, 2.0, True, None):
        with pytest.raises(ValueError, match="base_lanes: lanes is a power of two in 1 .. 64"):
            EB._check_container(dict(c, base_lanes=bad))
    with pytest.raises(ValueError, match="power of two"):                       # "lanes" is required, as in "embedded-3"
        EB._check_container({k: v for k, v in c.items() if k != "lanes"})
    with pytest.raises(ValueError, match="not an embedded container"):
        EB._check_container(dict(c, format="embedded-5"))


def test_a_scheduled_container_needs_its_schedule_keys():
    c = container(True)
    for key in ("side_bytes",):
        with pytest.raises(ValueError, match="a scheduled 'embedded-4' container carries"):
            EB._check_container({k: v for k, v in c.items() if k != key})
    with pytest.raises(ValueError, match="a scheduled 'embedded-4' container carries"):
        EB._check_container(dict(c, marks=dict(container(False)["marks"])))     # marked by q
    with pytest.raises(ValueError, match='an unscheduled \'embedded-4\' container carries marks by "q"'):
        EB._check_container({k: v for k, v in c.items() if k != "schedule"})    # no schedule: marks by stage do not fit


def test_truncate_an_unscheduled_container():
    c = container(False)
    t = EB.truncate(c, q=2.5)
    assert _lens(t) == [16, 24] and t["embedded"] == [bytes(range(16)), bytes(range(100, 124))] and _lens(c) == [40, 60]
    for key in ("format", "lanes", "base_lanes", "z", "base", "marks", "shape"):
        assert t[key] == c[key]
    assert t.keys() == c.keys()
    with pytest.raises(ValueError, match="stage= cuts a scheduled container .* this one is 'embedded-4' without one; cut it with q="):
        EB.truncate(c, stage=1)
    with pytest.raises(ValueError, match="quality 3.0 is not marked"):
        EB.truncate(c, q=3.0)
    with pytest.raises(ValueError, match="already cut"):
        EB.truncate(t, q=10.0)
    # z + base = 20 by their length, whatever their lanes; the marks add 20 / 40 / 100
    for budget, want in ((10 ** 6, [40, 60]), (120, [40, 60]), (119, [16, 24]), (60, [16, 24]), (59, [8, 12]), (40, [8, 12]),
                         (39, [0, 0]), (20, [0, 0])):
        assert _lens(EB.truncate(c, max_bytes=budget)) == want, budget
    with pytest.raises(ValueError, match="z and the base slices take 20 bytes, more than max_bytes = 19"):
        EB.truncate(c, max_bytes=19)
    assert EB.truncate(c, slice_bytes=[3, 0])["embedded"] == [bytes(range(3)), b""]
    assert _lens(EB.truncate(c, slice_bytes=[1000, 7])) == [40, 7]
    with pytest.raises(ValueError, match="slice_bytes takes 2 lengths"):
        EB.truncate(c, slice_bytes=[1])


def test_truncate_a_scheduled_container():
    c = container(True)
    t = EB.truncate(c, stage=1)
    assert _lens(t) == [16, 24] and t["schedule"] is c["schedule"]
    for key in ("format", "lanes", "base_lanes", "z", "base", "marks", "side_bytes"):
        assert t[key] == c[key]
    with pytest.raises(ValueError, match=r"a scheduled container \('embedded-4'\) is marked by stage.*cut it with stage="):
        EB.truncate(c, q=2.5)
    with pytest.raises(ValueError, match="stage 3 is not marked"):
        EB.truncate(c, stage=3)
    side = c["side_bytes"]                                   # 120, counted with z and the base
    for budget, want in ((240, [40, 60]), (239, [16, 24]), (179, [8, 12]), (159, [0, 0]), (140, [0, 0])):
        t = EB.truncate(c, max_bytes=budget)
        assert _lens(t) == want and sum(EB.container_bytes(t)) + side <= budget
    with pytest.raises(ValueError, match="and the schedule take 140 bytes"):
        EB.truncate(c, max_bytes=139)
    assert _lens(EB.truncate(c, slice_bytes=[5, 6])) == [5, 6]


@pytest.mark.parametrize("scheduled", [False, True])
def test_delta_between_cuts(scheduled):
    c = container(scheduled)
    short = EB.truncate(c, stage=0) if scheduled else EB.truncate(c, q=0.5)
    assert EB.delta(c, short) == [bytes(range(8, 40)), bytes(range(112, 160))]
    assert EB.delta(c, c) == [b"", b""]
    with pytest.raises(ValueError, match=r"differ in their base_lanes \(8 and 64\)"):
        EB.delta(dict(c, base_lanes=64), short)
    with pytest.raises(ValueError, match=r"differ in their lanes \(2 and 4\)"):
        EB.delta(dict(c, lanes=4), short)
    with pytest.raises(ValueError, match="differ in their format"):
        EB.delta(c, dict(short, format="embedded-3" if scheduled else "embedded-2"))
    with pytest.raises(ValueError, match="base stream of slice 1 differs"):
        EB.delta(c, dict(short, base=[[b"a" * 4], [b"c" * 6]]))
    with pytest.raises(ValueError, match="slice 0: the shorter container's 8 bytes are no prefix"):
        EB.delta(c, dict(short, embedded=[b"x" * 8, short["embedded"][1]]))


def test_an_embedded_1_container_goes_through_unchanged():
    c = {k: v for k, v in container(False).items() if k not in ("lanes", "base_lanes")}
    c["format"] = "embedded-1"
    assert EB._check_container(c) == 1 and EB._base_lanes(c) == 1 and EB._scheduled(c) is False
    t = EB.truncate(c, q=2.5)
    assert t.keys() == c.keys() and "base_lanes" not in t and "lanes" not in t and t["format"] == "embedded-1"
    assert _lens(t) == [16, 24] and _lens(EB.truncate(c, max_bytes=59)) == [8, 12]
    assert EB.delta(c, t) == [bytes(range(16, 40)), bytes(range(124, 160))]
    assert EB.container_bytes(c) == [10, 10, 100]
    assert EB._check_container(dict(c, base_lanes=8)) == 1                       # the key means nothing outside "embedded-4"
    with pytest.raises(ValueError, match="stage= cuts a scheduled container"):
        EB.truncate(c, stage=0)
