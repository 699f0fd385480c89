"""The support arithmetic of plans._SliceChain on the host, pinned to the model's own ``determine_support`` (the port of
pic.py:264-270) and, for the base slices, to ``y_hat_base[:, :32 * min(max_support_slices, i)]`` (pic.py:524-527)."""
import argparse

import pytest
import torch

import vampic
from vampic import ops
from vampic.plans import _SliceChain

from conftest import README_ARGS


@pytest.fixture(scope="module")
def model():
    return vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu")


def _latent(seed, d):
    """A [1, 2, 2, d] NHWC buffer whose value names its tensor and channel."""
    return ops.View((1000.0 * seed + torch.arange(d, dtype=torch.float32)).expand(1, 2, 2, d).contiguous(), 0, d)


def _cat(views):
    return torch.cat([v.torch_nchw() for v in views], 1)


@pytest.mark.parametrize("all_scalable", [True, False])
@pytest.mark.parametrize("sp", [0, 2, 5, 8])
def test_progressive_supports_are_determine_support(model, sp, all_scalable, monkeypatch):
    monkeypatch.setattr(model, "support_progressive_slices", sp)
    monkeypatch.setattr(model, "all_scalable", all_scalable)
    d, C = model.division_dimension[0], model.dim_chunk
    sc = _SliceChain(model, lambda: _latent(0, d))
    yb, mu_tot, std_p, yp = (_latent(k, d) for k in (1, 2, 3, 4))
    slices = lambda v: list(v.torch_nchw().split(C, 1))
    hist_m, hist_s = (mu_tot, std_p) if all_scalable else (yp, yp)            # pic.py:586-587
    assert model.ns0 == 10
    for j in range(model.ns0):
        ms, ss = sc.prog_supports(j, yb, mu_tot, std_p, yp)
        assert torch.equal(_cat(ms), torch.cat(model.determine_support(slices(yb), j, slices(hist_m)), 1))
        assert torch.equal(_cat(ss), torch.cat(model.determine_support(slices(yb), j, slices(hist_s)), 1))


def test_base_support_is_the_leading_base_slices(model):
    d = model.division_dimension[0]
    sc, yb = _SliceChain(model, lambda: _latent(0, d)), _latent(1, d)
    for i in range(model.ns0):
        want = yb.torch_nchw()[:, :32 * min(model.max_support_slices, i)]
        sup = sc.base_support(yb, i)
        assert torch.equal(_cat(sup) if sup else want.new_zeros(want.shape), want)
        assert bool(sup) == (i > 0)
