"""The oracle's restatement of the training forward over [0, q1, ..., qL] (tests/levels_oracle.py) against the existing
two-level oracle step (bit for bit) and against the reference's own three-level step (tests/golden/first_train_levels.npz,
written by scripts/gen_golden_levels.py)."""
import argparse
import os
import warnings

import numpy as np
import torch

import vampic
import vampic.synth as synth
import vampic_oracle as O
import levels_oracle as LO
from conftest import README_ARGS
from test_oracle_golden import _close, train_fixture_inputs

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def levels_fixture_inputs():
    """Inputs of tests/golden/first_train_levels.npz (scripts/gen_golden_levels.py): the two-level fixture's image and
    draws, and one more block of draws for the second level."""
    x, ny, nz = train_fixture_inputs()
    return x, torch.cat([ny, synth.uniform((2, 320, 4, 4), 203) - 0.5], 1), nz


def _sd():
    net = vampic.get_model(argparse.Namespace(model="pic", **README_ARGS), "cpu")
    return synth.synth_state_dict(net.state_dict(), seed=0)


def test_levels_oracle_with_one_level_is_the_two_level_step():
    sd = _sd()
    x, ny, nz = train_fixture_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = LO.first_train_step_levels(sd, x, [0, 10], ny, nz, [0.0055, 0.04])
        b = O.first_train_step(sd, x, [0, 10], ny, nz, [0.0055, 0.04])
    for k in ("loss", "bpp_loss", "bpp_base", "bpp_scalable", "bpp_hype", "mse_loss"):
        assert torch.equal(a["crit"][k], b["crit"][k]), k
    assert torch.equal(a["out"]["x_hat"], b["out"]["x_hat"])
    for k in ("y", "y_prog", "z"):
        assert torch.equal(a["out"]["likelihoods"][k], b["out"]["likelihoods"][k]), k
    assert sorted(k for k, g in a["grads"].items() if g is not None) == sorted(k for k, g in b["grads"].items() if g is not None)
    for k, g in b["grads"].items():
        if g is not None:
            assert torch.equal(a["grads"][k], g), k


def test_levels_oracle_matches_reference_three_levels():
    """forward(x, [0, 2.5, 10], training=True) + ScalableRateDistortionLoss(lmbda_list=[0.0055, 0.015, 0.04]) + backward:
    loss terms, likelihoods, reconstructions and all 1065 gradient tensors (norm + every 997th element) against the
    reference's run, at the tolerances of test_oracle_first_train_step_matches_reference."""
    sd = _sd()
    gold = np.load(os.path.join(GOLD, "first_train_levels.npz"))
    x, ny, nz = levels_fixture_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = LO.first_train_step_levels(sd, x, [0, 2.5, 10], ny, nz, [0.0055, 0.015, 0.04])
    got = [float(r["crit"][k].mean()) for k in ("loss", "bpp_loss", "bpp_base", "bpp_scalable", "bpp_hype")]
    for a, b in zip(got, gold["loss"]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b))
    _close(r["crit"]["mse_loss"], gold["mse"], 1e-6)
    _close(r["out"]["likelihoods"]["y"], gold["lik_y"], 1e-5)
    _close(r["out"]["likelihoods"]["z"], gold["lik_z"], 1e-5)
    _close(r["out"]["likelihoods"]["y_prog"], gold["lik_y_prog"], 1e-5)
    _close(r["out"]["x_hat"][:, :, :, ::4, ::4], gold["x_hat"], 2e-5)
    _close(r["out"]["y_base"], gold["y_hat_base"], 2e-5)
    _close(r["out"]["y_prog"], gold["y_hat_prog"], 2e-5)
    names = [str(n) for n in gold["grad_names"]]
    assert sorted(k for k, g in r["grads"].items() if g is not None) == sorted(names)
    assert len(names) == 1065
    off, num, den = 0, 0.0, 0.0
    for name, norm in zip(names, gold["grad_norms"]):
        g = r["grads"][name].reshape(-1)
        s_ = g[::997].numpy()
        ref = gold["grad_samples"][off:off + len(s_)]
        off += len(s_)
        assert abs(float(g.double().norm()) - norm) <= 2e-5 * norm + 1e-9, name
        num += float(((s_ - ref).astype(np.float64) ** 2).sum())
        den += float((ref.astype(np.float64) ** 2).sum())
    assert off == len(gold["grad_samples"])
    assert (num / den) ** 0.5 <= 1e-5
