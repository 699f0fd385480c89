"""Rate sweep grouping (models.sweep_groups) on the host: which image sub-batches and level groups a
sweep over a quality list runs as."""
import sys

import pytest

import vampic                              # noqa: F401
from vampic import _lib as L

M = sys.modules["vampic.models"]


@pytest.mark.parametrize("hw,B,n_levels,want", [
    ((256, 256), 1, 1, [(0, 1, [(0, 1)])]),
    ((256, 256), 1, 15, [(0, 1, [(0, 8), (8, 15)])]),
    ((256, 256), 24, 7, [(0, 24, [(0, 7)])]),
    ((256, 256), 24, 15, [(0, 24, [(0, 7), (7, 14), (14, 15)])]),
    ((256, 256), 32, 7, [(0, 32, [(0, 5), (5, 7)])]),
    ((256, 256), 32, 15, [(0, 32, [(0, 5), (5, 10), (10, 15)])]),
    ((256, 256), 32, 20, [(0, 32, [(0, 5), (5, 10), (10, 15), (15, 20)])]),
    ((512, 768), 1, 7, [(0, 1, [(0, 7)])]),
    ((512, 768), 1, 20, [(0, 1, [(0, 8), (8, 16), (16, 20)])]),
    ((512, 768), 24, 1, [(0, 24, [(0, 1)])]),
    ((512, 768), 32, 7, [(0, 28, [(k, k + 1) for k in range(7)]), (28, 32, [(0, 7)])]),
])
def test_sweep_groups_expected(hw, B, n_levels, want):
    assert M.sweep_groups(n_levels, B, *hw) == want


@pytest.mark.parametrize("hw", [(256, 256), (512, 768)])
@pytest.mark.parametrize("B", [1, 24, 32])
@pytest.mark.parametrize("n_levels", [1, 7, 15, 20])
def test_sweep_groups_cover_everything_within_one_plan(hw, B, n_levels):
    H, W = hw
    nb = M.MAX_PLAN_PIXELS // (H * W)
    groups = M.sweep_groups(n_levels, B, H, W)
    assert [i for i0, i1, _ in groups for i in range(i0, i1)] == list(range(B))       # every image once, in order
    for i0, i1, lv in groups:
        b = i1 - i0
        assert 1 <= b <= nb
        assert [k for l0, l1, in lv for k in range(l0, l1)] == list(range(n_levels))    # every level once, in order
        for l0, l1 in lv:
            assert 1 <= l1 - l0 <= L.VAM_MAX_MASK_LEVELS and (l1 - l0) * b <= nb


def test_sweep_groups_follow_the_plan_size(monkeypatch):
    monkeypatch.setattr(M, "MAX_PLAN_PIXELS", 2 * 64 * 64)
    assert M.sweep_groups(3, 3, 64, 64) == [(0, 2, [(0, 1), (1, 2), (2, 3)]), (2, 3, [(0, 2), (2, 3)])]
    assert M.sweep_groups(0, 1, 64, 64) == [(0, 1, [])]
