"""Writes tests/golden/first_train_levels.npz: the reference's own first-stage training step over THREE quality levels —
``forward(x, quality=[0, 2.5, 10], training=True)`` (models/pic.py:301-491), ScalableRateDistortionLoss with one lambda
per level (training/loss.py:6-66) and backward with every parameter trainable — recorded as tests/golden/first_train_step.npz
records the two-level step (oracle/gen_golden.py section 10: same synthetic weights, image and gradient-sample stride).

Noise: the reference's ``uniform_`` draws are replaced, for the duration of the call, by a deterministic queue (z, the
base slices 0..9, then slices 0..9 of level 1 and of level 2): ``noise_y`` [2, 960, 4, 4] holds them in that order — the
two-level fixture's draws (synth.uniform((2, 640, 4, 4), 201) - 0.5) for the base and level 1, then
synth.uniform((2, 320, 4, 4), 203) - 0.5 for level 2.

Needs the reference source tree (``--ref``, default $VAMPIC_REF or ../reference/src); imports it, copies nothing of it.
    python scripts/gen_golden_levels.py --ref /path/to/reference/src
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = [0, 2.5, 10]
LMBDA = [0.0055, 0.015, 0.04]


def inputs():
    """(x, noise_y [2, 320 * 3, 4, 4], noise_z) of the fixture (tests/test_oracle_levels.py and
    tests/test_gpu_train_levels.py regenerate them)."""
    import vampic.synth as synth
    ny = torch.cat([synth.uniform((2, 640, 4, 4), 201), synth.uniform((2, 320, 4, 4), 203)], 1) - 0.5
    return synth.synth_image(2, 64, 64, seed=5), ny, synth.uniform((2, 192, 1, 1), 202) - 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("VAMPIC_REF", os.path.join(os.path.dirname(ROOT), "reference", "src")))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "first_train_levels.npz"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "oracle", "ref_stubs"), a.ref, ROOT]
    sys.dont_write_bytecode = True
    import vampic.synth as synth
    from models import get_model                         # the reference
    spec = importlib.util.spec_from_file_location("ref_training_loss", os.path.join(a.ref, "training", "loss.py"))
    loss_mod = importlib.util.module_from_spec(spec)    # training/__init__.py pulls torchvision: load loss.py on its own
    spec.loader.exec_module(loss_mod)

    args = argparse.Namespace(model="pic", N=192, M=640, multiple_decoder=True, multiple_encoder=True, multiple_hyperprior=True,
                              dim_chunk=32, division_dimension=[320, 640], mask_policy="point-based-std",
                              support_progressive_slices=5, delta_encode=True, total_mu_rep=True, all_scalable=True)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = get_model(args, "cpu").train()
    sd = synth.synth_state_dict(net.state_dict(), 0)
    torch.nn.Module.load_state_dict(net, sd)
    for p_ in net.parameters():
        p_.requires_grad = True
    xt, ny, nz = inputs()
    queue = [nz.transpose(0, 1).reshape(192, 1, -1)] + list(ny.chunk(10 * len(QUALITIES), 1))
    real = torch.Tensor.uniform_

    def fake(self, lo=0.0, hi=1.0):
        src = queue.pop(0)
        assert tuple(src.shape) == tuple(self.shape) and (lo, hi) == (-0.5, 0.5), (src.shape, self.shape, lo, hi)
        with torch.no_grad():
            return self.copy_(src)
    torch.Tensor.uniform_ = fake
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # the criterion's broadcasting mse_loss (training/loss.py:41)
            o = net(xt, quality=list(QUALITIES), training=True)
            crit = loss_mod.ScalableRateDistortionLoss(lmbda_list=LMBDA, device="cpu")(o, xt)
    finally:
        torch.Tensor.uniform_ = real
    assert not queue, len(queue)
    crit["loss"].backward()
    rec = {"loss": np.array([crit[k].mean().item() for k in ("loss", "bpp_loss", "bpp_base", "bpp_scalable", "bpp_hype")], dtype=np.float64),
           "mse": crit["mse_loss"].detach().double().numpy(),
           "x_hat": o["x_hat"].detach()[:, :, :, ::4, ::4].numpy(), "lik_y": o["likelihoods"]["y"].detach().numpy(),
           "lik_y_prog": o["likelihoods"]["y_prog"].detach().numpy(), "lik_z": o["likelihoods"]["z"].detach().numpy(),
           "y_hat_base": o["y_hat"][0].detach().numpy(), "y_hat_prog": o["y_hat"][-1].detach().numpy()}
    names, norms, samples = [], [], []
    for k, p_ in net.named_parameters():
        assert p_.grad is not None, k
        gflat = p_.grad.detach().reshape(-1)
        names.append(k)
        norms.append(gflat.double().norm().item())
        samples.append(gflat[::997].numpy())
    rec.update({"grad_names": np.array(names), "grad_norms": np.array(norms, dtype=np.float64),
                "grad_samples": np.concatenate(samples).astype(np.float32)})
    np.savez_compressed(a.out, **rec)
    print(f"{a.out}: {os.path.getsize(a.out) / 1024:.1f} KiB, loss {rec['loss'][0]:.6f}")


if __name__ == "__main__":
    main()
