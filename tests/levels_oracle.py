"""CPU restatement of the reference's training forward over a quality list [0, q1, ..., qL] (models/pic.py:301-491),
composed from the oracle's functions, with the reference's step around it (ScalableRateDistortionLoss, autograd).

The reference creates ``mu_total`` / ``std_total`` once, outside its quality loop, and ``determine_support`` slices them
by absolute position (pic.py:264-270,380-478): every level after the first reads level 1's entries, so with
all_scalable every level's progressive (mu, sigma) equal level 1's.  This module keeps that indexing literally (each
level evaluates the stacks again, on the same values), so autograd forms the gradients the reference's graph has.

Noise: ``noise_y`` [B, d * (L+1), h, w] = the base block, then one block per level (the reference's uniform_ draws in
queue order: base slices 0..9, then slices 0..9 of level 1, level 2, ...).  ``force`` (tests only) = {"z_sym",
"base_sym", "prog_sym": [per level], "mask": [per level]}: hard decisions imposed instead of recomputed."""
from typing import Optional, Sequence

import torch

import vampic_oracle as O


def training_forward_levels(sd, x: torch.Tensor, qualities: Sequence[float], noise_y: torch.Tensor, noise_z: torch.Tensor,
                            force: Optional[dict] = None, *, div: int = 320, chunk: int = 32, max_support: int = 5,
                            prog_support: int = 5) -> dict:
    """README configuration (dual encoder / decoder / hyperprior, delta_encode, total_mu_rep, all_scalable)."""
    force = force or {}
    qs = list(qualities)
    assert qs[0] == 0 and len(qs) >= 2
    n_lv = len(qs) - 1
    fsl = lambda t, j: None if t is None else t[:, j * chunk:(j + 1) * chunk]
    y = torch.cat([O.g_a(sd, "g_a.0.", x), O.g_a(sd, "g_a.1.", x)], 1)                 # pic.py:306-311
    z = O.h_a(sd, y)                                                                     # :280
    z_lik = O.eb_likelihood_noise_bounded(sd, z, noise_z)
    med = sd["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    z_hat = O._ste_forced(z - med, force.get("z_sym")) + med                             # :282-284
    means_h = torch.cat([O.h_s(sd, "h_mean_s.0.", z_hat), O.h_s(sd, "h_mean_s.1.", z_hat)], 1)
    scales_h = torch.cat([O.h_s(sd, "h_scale_s.0.", z_hat), O.h_s(sd, "h_scale_s.1.", z_hat)], 1)
    ns0 = div // chunk
    ys = y.chunk(y.shape[1] // chunk, 1)
    nys = noise_y.chunk(noise_y.shape[1] // chunk, 1)
    assert len(nys) == ns0 * (n_lv + 1), "noise_y: the base block and one block per level"
    yhat_b, lik_b, mu_b, std_b = [], [], [], []
    for i in range(ns0):                                                                 # :330-367
        sup = yhat_b[:min(max_support, i)]
        msup = torch.cat([means_h[:, :div]] + sup, 1)
        ssup = torch.cat([scales_h[:, :div]] + sup, 1)
        mu = O.cc_stack(sd, f"cc_mean_transforms.{i}.", msup)
        sc = O.cc_stack(sd, f"cc_scale_transforms.{i}.", ssup)
        mu_b.append(mu)
        std_b.append(sc)
        lik_b.append(O.gaussian_likelihood_noise(ys[i], sc, mu, nys[i]))
        yh = O._ste_forced(ys[i] - mu, fsl(force.get("base_sym"), i)) + mu
        lrp = O.cc_stack(sd, f"lrp_transforms.{i}.", torch.cat([msup, yh], 1))
        yhat_b.append(yh + 0.5 * torch.tanh(lrp))
    y_base = torch.cat(yhat_b, 1)
    lik_base = torch.cat(lik_b, 1)
    x_hats = [O.g_s(sd, "g_s.0.", y_base)]                                               # :372
    mu_tot, std_tot = [], []                                                             # :380-381, ONCE for every level
    y_progs, lik_levels, masks_all, mu_p, std_p = [], [], [], [], []
    for lv, q in enumerate(qs[1:]):                                                      # :384
        f_sym = force["prog_sym"][lv] if "prog_sym" in force else None
        f_mask = force["mask"][lv] if "mask" in force else None
        lik_p, yhat_p, masks = [], [], []
        for j in range(ns0):                                                             # :396-457
            r = ys[ns0 + j] - ys[j]                                                      # :397-398 (delta_encode)
            s = min(prog_support, j)
            msup = torch.cat([means_h[:, div:], yhat_b[j]] + mu_tot[j - s:j], 1)         # determine_support: absolute positions
            ssup = torch.cat([scales_h[:, div:], yhat_b[j]] + std_tot[j - s:j], 1)
            mu = O.cc_stack(sd, f"cc_mean_transforms_prog.{j}.", msup)
            sc = O.cc_stack(sd, f"cc_scale_transforms_prog.{j}.", ssup)
            mu_tot.append(mu + yhat_b[j])                                                # :416 (total_mu_rep)
            std_tot.append(sc)
            if lv == n_lv - 1:
                mu_p.append(mu)
                std_p.append(sc)
            m = O.variance_mask(sc.detach(), q) if f_mask is None else fsl(f_mask, j)     # channel_mask.py:132-151
            masks.append(m)
            lik_p.append(O.gaussian_likelihood_noise((r - mu) * m, sc * m, None, nys[ns0 * (lv + 1) + j]))
            rh = O._ste_forced(r - mu, fsl(f_sym, j)) * m + mu                           # :443
            lrp = O.cc_stack(sd, f"lrp_transforms_prog.{j}.", torch.cat([msup, rh], 1))
            yhat_p.append(rh + 0.5 * torch.tanh(lrp) + yhat_b[j])
        y_prog = torch.cat(yhat_p, 1)
        x_hats.append(O.g_s(sd, "g_s.1.", y_prog))                                      # :462-466
        y_progs.append(y_prog)
        lik_levels.append(torch.cat([lik_base] + lik_p, 1))                             # :471-472
        masks_all.append(torch.cat(masks, 1))
    return {"x_hat": torch.stack(x_hats, 0), "likelihoods": {"y": lik_base, "y_prog": torch.stack(lik_levels, 0), "z": z_lik},
            "y_hat": [y_base] + y_progs, "y_base": y_base, "y_prog": y_progs[-1], "y": y, "z": z,
            "mu_base": torch.cat(mu_b, 1), "std_base": torch.cat(std_b, 1), "mu": torch.cat(mu_p, 1), "std": torch.cat(std_p, 1),
            "mask": masks_all}


def first_train_step_levels(sd, x: torch.Tensor, qualities: Sequence[float], noise_y: torch.Tensor, noise_z: torch.Tensor,
                            lmbda, force: Optional[dict] = None) -> dict:
    """``vampic_oracle.first_train_step`` over :func:`training_forward_levels`: every floating-point parameter trainable."""
    skip = ("entropy_bottleneck._offset", "entropy_bottleneck._quantized_cdf", "entropy_bottleneck._cdf_length",
            "gaussian_conditional.")
    leaves = {}
    for k, v in sd.items():
        if torch.is_tensor(v) and v.dtype.is_floating_point and not k.startswith(skip) and "reparam" not in k and \
                not k.endswith((".target", ".bound", ".pedestal")) and not k.startswith("post_latent."):
            leaves[k] = v.detach().clone().requires_grad_(True)
    sdt = dict(sd)
    sdt.update(leaves)
    out = training_forward_levels(sdt, x, qualities, noise_y, noise_z, force)
    crit = O.scalable_rd_loss(out, x, lmbda)
    crit["loss"].backward()

    def det(t):
        if isinstance(t, dict):
            return {k: det(v) for k, v in t.items()}
        if isinstance(t, list):
            return [det(v) for v in t]
        return t.detach() if torch.is_tensor(t) else t
    return {"out": det(out), "crit": det(crit), "grads": {k: v.grad for k, v in leaves.items()}}
