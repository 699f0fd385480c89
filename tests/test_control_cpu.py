"""The shared skeletons of the control layer (control.py; DESIGN sections 9f, 9h-9j) on the host: target normalisation,
distinct levels and their scatter, the per-image points of a solver pass with recording evaluators, the quality
sub-batches, and the plan size that both modules read."""
import sys

import numpy as np
import pytest
import torch

import vampic                              # noqa: F401
from vampic import control as C

M = sys.modules["vampic.models"]


# ----------------------------------------------------------------------------------------------- _targets
def test_targets_scalar_list_and_tensor_agree():
    B = 3
    want = np.array([[0.5] * B, [1.25] * B])
    a = C._targets([0.5, 1.25], B, "target_bpp")
    b = C._targets(torch.tensor(want), B, "target_bpp")
    assert a.dtype == b.dtype == np.float64 and np.array_equal(a, want) and np.array_equal(b, want)
    s = C._targets(0.5, B, "target_bpp")
    assert s.dtype == np.float64 and np.array_equal(s, want[:1])
    assert np.array_equal(C._targets(np.float32(0.5), B, "target_bpp"), want[:1])


@pytest.mark.parametrize("bad", [np.zeros((2, 4)), np.zeros((2, 3, 1))])
def test_targets_refuse_other_shapes_by_name(bad):
    with pytest.raises(ValueError, match="target_bytes"):
        C._targets(bad, 3, "target_bytes")


# ----------------------------------------------------------------------------------------------- _distinct_levels
def test_distinct_levels_chunks_and_scatter():
    prs = [2.5, 0, 1.0, 2.5, 7.0]
    chunks, rows, cols = C._distinct_levels(prs, 2)
    assert chunks == [[1.0, 2.5], [7.0]]
    f = lambda q: 3.0 * q + 1.0
    per_level = np.array([f(q) for chunk in chunks for q in chunk])       # what the launches return, chunk after chunk
    out = np.full(len(prs), -1.0)
    out[rows] = per_level[cols]
    assert out.tolist() == [f(2.5), -1.0, f(1.0), f(2.5), f(7.0)]         # input order; the zero row untouched


@pytest.mark.parametrize("prs", [[], [0, 0.0, 0]])
def test_distinct_levels_without_a_positive_quality_has_no_chunk(prs):
    chunks, rows, cols = C._distinct_levels(prs, 2)
    assert chunks == [] and rows.size == 0 and cols.size == 0
    assert np.zeros((len(prs), 4))[rows].shape == (0, 4)                  # usable as indexes all the same


# ----------------------------------------------------------------------------------------------- _points
T, B, N = 2, 3, 5


def _f(b, q):
    return (b + 1) * 10.0 + 2.0 * np.asarray(q)                           # monotone in q, different per image


class _Evaluators:
    def __init__(self):
        self.same_calls, self.own_calls = [], []

    def same(self, points):
        self.same_calls.append(np.array(points))
        return np.stack([_f(b, points) for b in range(B)])

    def own(self, pts):
        self.own_calls.append([np.array(u) for u in pts])
        return [_f(b, u) for b, u in enumerate(pts)]


def _check_points(q, need, ev):
    got = C._points(q, need, ev.same, ev.own)
    want = np.where(need, np.stack([_f(b, q[:, b]) for b in range(B)], 1), 0.0)
    assert got.shape == q.shape and np.array_equal(got, want)


def test_points_nothing_needed_calls_nothing():
    ev = _Evaluators()
    q = np.random.default_rng(0).uniform(0.1, 10, (T, B, N))
    _check_points(q, np.zeros((T, B, N), dtype=bool), ev)
    assert ev.same_calls == [] and ev.own_calls == []


def test_points_same_for_all_images_run_batched_once():
    ev = _Evaluators()
    row = np.array([4.0, 0.5, 4.0, 9.0, 0.5])                             # repeats inside an image
    q = np.broadcast_to(np.stack([row, row[::-1]])[:, None, :], (T, B, N)).copy()
    _check_points(q, np.ones((T, B, N), dtype=bool), ev)
    assert ev.own_calls == [] and len(ev.same_calls) == 1
    assert ev.same_calls[0].tolist() == [0.5, 4.0, 9.0]


def test_points_of_their_own_run_per_image():
    ev = _Evaluators()
    q = np.array([[[1.0, 2.0, 2.0, 3.0, 1.0], [5.0, 5.0, 6.0, 7.0, 8.0], [0.25, 0.5, 0.25, 0.5, 9.0]],
                  [[3.0, 3.0, 1.5, 2.0, 4.0], [8.0, 7.5, 6.0, 5.0, 5.0], [0.25, 9.0, 9.0, 0.75, 0.5]]])
    need = np.ones((T, B, N), dtype=bool)
    need[0, 0, -1] = need[1, 1, 0] = False
    need[:, 2, 1] = False
    _check_points(q, need, ev)
    assert ev.same_calls == [] and len(ev.own_calls) == 1
    assert [u.tolist() for u in ev.own_calls[0]] == [[1.0, 1.5, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 7.5, 8.0], [0.25, 0.5, 0.75, 9.0]]
    # an image that wants nothing beside images that do
    ev2 = _Evaluators()
    need[:, 1] = False
    _check_points(q, need, ev2)
    assert ev2.same_calls == [] and ev2.own_calls[0][1].size == 0


# ----------------------------------------------------------------------------------------------- sub-batches
def test_quality_sub_batches_zeros_first_then_positives():
    assert list(C._quality_sub_batches([0, 2, 0, 3, 4], 2)) == [(True, [0, 2]), (False, [1, 3]), (False, [4])]
    assert list(C._quality_sub_batches([1.0, 2.0], 8)) == [(False, [0, 1])]
    assert list(C._quality_sub_batches([0.0], 1)) == [(True, [0])]


def test_both_modules_follow_a_patched_plan_size(monkeypatch):
    assert M.sweep_groups is C.sweep_groups
    assert len(M.sweep_groups(0, 3, 64, 64)) == len(C.sweep_groups(0, 3, 64, 64)) == 1
    monkeypatch.setattr(M, "MAX_PLAN_PIXELS", 2 * 64 * 64)
    want = [(0, 2, [(0, 1), (1, 2), (2, 3)]), (2, 3, [(0, 2), (2, 3)])]
    assert M.sweep_groups(3, 3, 64, 64) == want and C.sweep_groups(3, 3, 64, 64) == want
    assert M._max_images_per_plan(torch.zeros(3, 3, 64, 64)) == 2
