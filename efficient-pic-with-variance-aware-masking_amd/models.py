"""Host-side mirror of the reference's model classes (``src/models/*.py``).

``get_model(args, device)``, ``models``, ``VarianceMaskingPIC`` and
``VarianceMaskingPICREM`` keep the reference's constructor arguments, attribute names,
sub-module tree and ``state_dict`` keys (so ``src/demo.py`` / ``src/train.py`` style
callers and reference checkpoints map onto them), while ``forward_single_quality`` is
lowered once per input shape into a :class:`engine.Plan` of libvampic launches
(optionally replayed as one hipGraph).

Reference: models/__init__.py:5-55, models/base.py:6-70, models/builder.py:4-136,
models/pic.py:25-666, models/rem_pic.py:8-422.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E
from . import gs_train as G
from . import layers as Ly
from . import ops
from .entropy_models import EntropyBottleneck, GaussianConditional, get_scale_table


# ----------------------------------------------------------------------------- builders
def define_encoder(multiple_encoder, N, M, dimensions_M):
    """models/builder.py:39-67."""
    def one(out):
        return Ly.TransformStack(
            Ly.conv(3, N, 5, 2), Ly.GDN(N), Ly.conv(N, N, 5, 2), Ly.GDN(N),
            Ly.Win_noShift_Attention(dim=N, num_heads=8, window_size=8, shift_size=4),
            Ly.conv(N, N, 5, 2), Ly.GDN(N), Ly.conv(N, out, 5, 2),
            Ly.Win_noShift_Attention(dim=out, num_heads=8, window_size=4, shift_size=2))
    return nn.ModuleList(one(dimensions_M[0]) for _ in range(2)) if multiple_encoder else one(M)


def define_decoder(multiple_decoder, N, M, dimensions_M):
    """models/builder.py:4-32."""
    def one():
        d = dimensions_M[0]
        return Ly.TransformStack(
            Ly.Win_noShift_Attention(dim=d, num_heads=8, window_size=4, shift_size=2),
            Ly.deconv(d, N, 5, 2), Ly.GDN(N, inverse=True), Ly.deconv(N, N, 5, 2), Ly.GDN(N, inverse=True),
            Ly.Win_noShift_Attention(dim=N, num_heads=8, window_size=8, shift_size=4),
            Ly.deconv(N, N, 5, 2), Ly.GDN(N, inverse=True), Ly.deconv(N, 3, 5, 2))
    return nn.ModuleList(one() for _ in range(2)) if multiple_decoder else one()


def _hyper_synthesis(cin, c0, cout):
    return Ly.ConvStack(Ly.conv3x3(cin, c0), Ly.GELU(), Ly.subpel_conv3x3(c0, 224, 2), Ly.GELU(),
                        Ly.conv3x3(224, 256), Ly.GELU(), Ly.subpel_conv3x3(256, 288, 2), Ly.GELU(),
                        Ly.conv3x3(288, cout))


def define_hyperprior(multiple_hyperprior, M, N, dimensions_M):
    """models/builder.py:71-136."""
    h_a = Ly.ConvStack(Ly.conv3x3(M, 320), Ly.GELU(), Ly.conv3x3(320, 288), Ly.GELU(), Ly.conv3x3(288, 256, stride=2),
                       Ly.GELU(), Ly.conv3x3(256, 224), Ly.GELU(), Ly.conv3x3(224, N, stride=2))
    if multiple_hyperprior:
        h_mean_s = nn.ModuleList(_hyper_synthesis(N, 192, dimensions_M[0]) for _ in range(2))
        h_scale_s = nn.ModuleList(_hyper_synthesis(N, 192, dimensions_M[0]) for _ in range(2))
    else:
        h_mean_s = _hyper_synthesis(N, N, M)
        h_scale_s = _hyper_synthesis(192, 192, M)
    return h_a, h_mean_s, h_scale_s


def _param_stack(cin, c_head):
    """Five conv3x3 with GELU between: cin -> 224 -> 176 -> 128 -> 64 -> 32 (models/pic.py:83-164).
    ``c_head``: how many leading input channels are the hyperprior tensor (the rest are support slices).  The fused
    plans compute the first layer as  conv(hyper; W[:, :c_head]) + conv(supports; W[:, c_head:])  (engine.lower_stack_heads);
    a module-level call ``stack(torch.cat([hyper, *supports]))`` must associate the sum the same way, or the decoder of
    the progressive container (module-level calls, test/functions_decode.py) would see a sigma that differs from the
    encoder's (fused plan) in the last bit — enough to desynchronise the range coder."""
    widths = (cin, 224, 176, 128, 64, 32)
    mods = []
    for a, b in zip(widths[:-1], widths[1:]):
        mods += [Ly.conv(a, b, kernel_size=3, stride=1), Ly.GELU()]
    st = Ly.ConvStack(*mods[:-1])
    st.c_head = c_head
    return st


class CompressionModel(nn.Module):
    """models/base.py:6-70 (conv weights kaiming-normal at construction, zero biases)."""

    def __init__(self, init_weights=True):
        super().__init__()

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def update(self, force=False):
        """models/base.py:41-60."""
        updated = False
        for m in self.children():
            if isinstance(m, EntropyBottleneck):
                updated |= m.update(force=force)
        return updated


def _resize_cdf_buffers(module, prefix, names, state_dict):
    """models/utils.py:41-93 'resize_if_empty': let checkpoints carrying CDF tables load."""
    bufs = dict(module.named_buffers())
    for n in names:
        key = f"{prefix}.{n}"
        if key in state_dict and n in bufs and bufs[n].numel() == 0:
            bufs[n].resize_(state_dict[key].size())


class VarianceMaskingPIC(CompressionModel):
    """models/pic.py:25-967."""

    def __init__(self, N=192, M=640, division_dimension=[320, 640], dim_chunk=32, multiple_decoder=True,
                 multiple_encoder=True, multiple_hyperprior=True, support_progressive_slices=5, delta_encode=True,
                 total_mu_rep=True, all_scalable=True, mask_policy="point-based-std", **kwargs):
        super().__init__(**kwargs)
        self.N, self.M, self.dim_chunk = N, M, dim_chunk
        self.num_slices = int(M // dim_chunk)
        self.multiple_encoder, self.multiple_decoder = multiple_encoder, multiple_decoder
        self.multiple_hyperprior = multiple_hyperprior
        self.division_channel = division_dimension[0]
        self.division_dimension = division_dimension
        self.support_progressive_slices = support_progressive_slices
        self.delta_encode, self.total_mu_rep, self.all_scalable = delta_encode, total_mu_rep, all_scalable
        self.mask_policy = mask_policy
        self.quality_list = [0, 10]
        self.max_support_slices = 5
        self.entropy_bottleneck = EntropyBottleneck(N)
        self.gaussian_conditional = GaussianConditional(None)
        self.masking = Ly.ChannelMask(mask_policy)
        self.num_slice_cumulative_list = [p // dim_chunk for p in division_dimension]
        self.ns0, self.ns1 = self.num_slice_cumulative_list[0], self.num_slice_cumulative_list[1]
        d0 = division_dimension[0]
        delta = division_dimension[1] - division_dimension[0]
        sp1 = support_progressive_slices + 1

        self.g_a = define_encoder(multiple_encoder, N, M, division_dimension)
        self.g_s = define_decoder(multiple_decoder, N, M, division_dimension)
        self.h_a, self.h_mean_s, self.h_scale_s = define_hyperprior(multiple_hyperprior, M, N, division_dimension)
        nb, np_ = self.ns0, self.ns1 - self.ns0
        self.cc_mean_transforms = nn.ModuleList(_param_stack(d0 + 32 * min(i, 5), d0) for i in range(nb))
        self.cc_scale_transforms = nn.ModuleList(_param_stack(d0 + 32 * min(i, 5), d0) for i in range(nb))
        self.lrp_transforms = nn.ModuleList(_param_stack(d0 + 32 * min(i + 1, 6), d0) for i in range(nb))
        self.cc_mean_transforms_prog = nn.ModuleList(_param_stack(delta + 32 * min(i + 1, sp1), delta) for i in range(np_))
        self.cc_scale_transforms_prog = nn.ModuleList(_param_stack(delta + 32 * min(i + 1, sp1), delta) for i in range(np_))
        self.lrp_transforms_prog = nn.ModuleList(_param_stack(delta + 32 * min(i + 2, sp1 + 1), delta) for i in range(nb))
        self._plans: Dict[tuple, "_FsqPlan"] = {}
        self._dec_plans: Dict[tuple, "_DecPlan"] = {}
        self.use_graph = True
        # "fp32" (default; every parity claim) or "bf16": BASELINE configs[2] — the large feature maps of g_a / g_s are
        # stored in bf16 and multiplied by bf16-rounded weights (fp32 accumulation); the entropy-parameter stacks, the
        # variance mask and the likelihoods stay fp32.  Differences to the fp32 path are MEASURED (bench.py --dtype bf16).
        self.storage = "fp32"

    # ---- reference helpers kept for the harness
    def freeze_all(self):
        for p in self.parameters():
            p.requires_grad = False

    def unfreeze_decoder(self, lrp=False):
        target = self.g_s if not self.multiple_decoder else self.g_s[1]
        for p in target.parameters():
            p.requires_grad = True
        if lrp:
            for p in self.lrp_transforms_prog.parameters():
                p.requires_grad = True

    def unfreeze_encoder(self):
        target = self.g_s if not self.multiple_encoder else self.g_a[1]   # (sic) pic.py:189-191
        for p in target.parameters():
            p.requires_grad = True

    def print_information(self):
        for name in ("g_a", "h_a", "h_mean_s", "h_scale_s", "cc_mean_transforms", "cc_scale_transforms",
                     "cc_mean_transforms_prog", "cc_scale_transforms_prog", "lrp_transforms", "g_s"):
            print(f" {name}: ", sum(p.numel() for p in getattr(self, name).parameters()))
        tr = sum(p.numel() for p in self.parameters() if p.requires_grad)
        print(" trainable parameters: ", tr)
        print(" freeze parameterss: ", sum(p.numel() for p in self.parameters() if not p.requires_grad))
        return tr

    def update(self, scale_table=None, force=True):
        """models/pic.py:230-237: scale table + CDF tables of both entropy models."""
        if scale_table is None:
            scale_table = get_scale_table()
        self.gaussian_conditional.update_scale_table([float(s) for s in scale_table])
        self.entropy_bottleneck.update(force=force)
        self._drop_plans()
        return True

    def load_state_dict(self, state_dict, strict=True):
        _resize_cdf_buffers(self.gaussian_conditional, "gaussian_conditional",
                            ["_quantized_cdf", "_offset", "_cdf_length", "scale_table"], state_dict)
        _resize_cdf_buffers(self.entropy_bottleneck, "entropy_bottleneck",
                            ["_quantized_cdf", "_offset", "_cdf_length"], state_dict)
        self._drop_plans()
        for em in (self.gaussian_conditional, self.entropy_bottleneck):      # loaded CDF tables replace the cached host copies
            object.__setattr__(em, "_tables_generation", getattr(em, "_tables_generation", 0) + 1)
        return nn.Module.load_state_dict(self, state_dict, strict=strict)

    def _drop_plans(self):
        """Forget every plan: their executable graphs are handed to ops' deferred-destroy list explicitly (not left to
        whenever the garbage collector finds the plans' reference cycles) and destroyed at the next plan entry point,
        after their last replay has finished."""
        for p in list(self._plans.values()) + list(self._dec_plans.values()):
            p.close()
        self._plans.clear()
        self._dec_plans.clear()

    def _apply(self, fn, *a, **k):
        self._drop_plans()
        self.__dict__.pop("_sig_params", None)
        return super()._apply(fn, *a, **k)

    def __deepcopy__(self, memo):
        """Plans hold device pointers, HIP graphs and streams of THIS instance: a copy starts without them."""
        import copy
        held = self._plans, self._dec_plans
        self._plans, self._dec_plans = {}, {}
        self.__dict__.pop("_sig_params", None)
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self._plans, self._dec_plans = held
        return new

    def define_quality(self, quality):
        if quality is None:
            return self.quality_list
        if isinstance(quality, list):
            return quality if quality[0] == 0 else [0] + quality
        return [quality]

    def determine_support(self, y_hat_base, current_index, y_hat_quality):
        bi = y_hat_base[current_index]
        if current_index == 0 or self.support_progressive_slices == 0:
            return [bi]
        s = min(self.support_progressive_slices, current_index)
        return [bi] + y_hat_quality[current_index - s:current_index]

    def merge(self, y_base, y_enhanced):
        return y_base + y_enhanced

    def compute_hyperprior(self, y, quality=10):
        """models/pic.py:278-298 on NCHW tensors (module-level path of the harness)."""
        z = self.h_a(y)
        z_hat, z_lik = self.entropy_bottleneck(z, training=False)
        if not self.multiple_hyperprior:
            return self.h_mean_s(z_hat), self.h_scale_s(z_hat), z_lik
        if quality == 0:
            return self.h_mean_s[0](z_hat), self.h_scale_s[0](z_hat), z_lik
        means = torch.cat([self.h_mean_s[0](z_hat), self.h_mean_s[1](z_hat)], dim=1)
        scales = torch.cat([self.h_scale_s[0](z_hat), self.h_scale_s[1](z_hat)], dim=1)
        return means, scales, z_lik

    # ---- the hot path
    def _check_config(self):
        """What the lowering needs.  Every flag of models/__init__.py:11-55 is accepted (single or dual
        encoder / decoder / hyperprior, any support_progressive_slices, delta_encode, total_mu_rep, all_scalable);
        the slice geometry is the one the reference itself can run: 32-channel slices (the stacks end in 32 channels,
        pic.py:83-164) and division [d, 2d] with M = 2d (the progressive stacks read latent_means[:, d:], whose width
        must equal division[1] - division[0], pic.py:75,596-599)."""
        if self.dim_chunk != 32 or self.ns1 != 2 * self.ns0 or self.M != 2 * self.division_dimension[0]:
            raise NotImplementedError(f"slice geometry dim_chunk={self.dim_chunk}, division={self.division_dimension}, M={self.M}: "
                                      "the channel-conditional stacks are built for 32-channel slices and division [d, 2d] "
                                      "with M = 2d (as the reference's own stacks are, pic.py:83-164)")
        if self.support_progressive_slices < 0:
            raise ValueError("support_progressive_slices must be >= 0")

    def _mask_policy(self, mask_pol):
        """``mask_pol``, or the model's for None: the plans implement point-based-std and two-levels."""
        mask_pol = self.mask_policy if mask_pol is None else mask_pol
        if mask_pol not in ("point-based-std", "two-levels"):
            raise NotImplementedError()
        return mask_pol

    def _cached_plan(self, plans: dict, key, build, wsig=None, rem_idx: Optional[int] = None):
        """The plan under ``key`` in ``plans``; ``build()`` makes it when there is none or the kept one is stale: built
        under another ``wsig`` (a packed weight was edited in place: param.data.copy_, nn.init, optimizer step), or REM
        ``rem_idx`` changed since the plan packed it (``rem_sig``).  None compares nothing.  A replaced plan is closed."""
        p = plans.get(key)
        if p is not None and ((wsig is not None and p.wsig != wsig) or
                              (rem_idx is not None and p.rem_sig != _version_sig(self.post_latent[rem_idx]))):
            plans.pop(key).close()
            p = None
        if p is None:
            p = plans[key] = build()
            p.wsig = wsig
        return p

    def _plan(self, x, base_only: bool, rem_idx: Optional[int] = None, symbols: bool = False,
              train: bool = False, own_ck: bool = False, train_gs: bool = False, train_lrp: bool = False,
              per_image: bool = False) -> "_FsqPlan":
        B, H, W = _check_input(x)
        key = (B, H, W, base_only, rem_idx, str(x.device)) + ((True,) if symbols else ()) + (("train",) if train else ()) + \
            (("own_ck",) if own_ck else ()) + (("train_gs",) if train_gs else ()) + (("train_lrp",) if train_lrp else ()) + \
            (("bf16",) if getattr(self, "storage", "fp32") == "bf16" else ()) + (("per_image",) if per_image else ())
        if getattr(self, "storage", "fp32") == "bf16" and (train or symbols):
            raise NotImplementedError("bf16 storage is an inference configuration (forward_single_quality): training and "
                                      "the bitstream path run in fp32")
        if ops.f16x2_mode() and (train or symbols):
            raise NotImplementedError(F16X2_REFUSAL)
        # training plans re-pack what they train every step: wsig leaves those modules out, a training REM plan its REM
        trained = ([self._decoder_in_use(base_only)] if train_gs else []) + ([self.lrp_transforms_prog] if train_lrp else [])
        return self._cached_plan(self._plans, key,
                                 lambda: _FsqPlan(self, B, H, W, base_only, rem_idx, x.device, symbols=symbols, train=train,
                                                  own_ck=own_ck, train_gs=train_gs, train_lrp=train_lrp, per_image=per_image),
                                 self._weights_sig(trained), None if train else rem_idx)

    def _decoder_in_use(self, base_only: bool):
        return (self.g_s[0 if base_only else 1] if self.multiple_decoder else self.g_s)

    def _weights_sig(self, trained: Sequence[nn.Module] = ()):
        """(_version, data_ptr) of every parameter the plans pack ONCE (everything except ``post_latent`` — and except
        ``trained``, the modules a training plan re-packs in place every step): a plan built before an in-place edit
        of a weight must not be replayed."""
        cache = self.__dict__.setdefault("_sig_params", {})
        key = tuple(id(t) for t in trained)
        ps = cache.get(key)
        if ps is None:
            skip = {id(p) for t in trained for p in t.parameters()}
            ps = [p for n, p in self.named_parameters() if not n.startswith("post_latent.") and id(p) not in skip]
            cache[key] = ps
        h = 0
        for p in ps:
            h = (h * 1000003 + p._version * 31 + (p.data_ptr() >> 4)) & 0xFFFFFFFFFFFFFFF
        return h

    def _trainable_outside_rem(self):
        return [n for n, p in self.named_parameters() if p.requires_grad and not n.startswith("post_latent.")]

    def forward_single_quality(self, x, quality, mask_pol="point-based-std", training=False, clone=True, noise=None):
        """models/pic.py:497-666.  Returns the reference's dict; tensors are NCHW-shaped.  ``training=True``: the
        additive-uniform-noise likelihoods of the training forward (entropy_models.py:132-138; the latents themselves
        are STE-rounded, so every other output equals the eval pass) — VALUES only: the transforms outside the REMs have
        no backward kernels in this build, so asking for their gradients fails loudly instead of silently
        returning none.  ``noise`` = {"y": NCHW, "z": NCHW} injects fixed draws."""
        train_gs = train_lrp = False
        if training and torch.is_grad_enabled() and self._trainable_outside_rem():
            # `--training_type refine_gs` (train.py:150-157,216-218): the synthesis transform in use trains, with `--lrp`
            # (unfreeze_decoder(lrp=True), pic.py:171-184) the progressive latent-residual-prediction stacks as well
            dec_ids = {id(p) for p in self._decoder_in_use(quality == 0).parameters()}
            lrp_ps = list(self.lrp_transforms_prog.parameters())
            lrp_ids = {id(p) for p in lrp_ps}
            other = [n for n, p in self.named_parameters()
                     if p.requires_grad and not n.startswith("post_latent.") and id(p) not in dec_ids and id(p) not in lrp_ids]
            n_lrp = sum(p.requires_grad for p in lrp_ps)
            if other or not self.all_scalable or (n_lrp and (quality == 0 or n_lrp != len(lrp_ps))) or \
                    not any(p.requires_grad for p in self._decoder_in_use(quality == 0).parameters()):
                # anything beyond the decoder-refinement subsets (first_train: everything; refine_gs_ga: g_s[1] + g_a[1],
                # train.py:219-222): the complete training plan (full_train.py)
                return self._forward_full_train(x, [quality], mask_pol, noise, single=True)
            train_gs, train_lrp = True, bool(n_lrp)
        mask_pol = self._mask_policy(mask_pol)
        Ly._no_autograd(x)
        L.require_gpu()
        self._check_config()
        pr = _mask_quality(mask_pol, quality)
        nb = _max_images_per_plan(x)
        if train_gs and x.shape[0] > nb:                # one tape per plan: sub-batches would overwrite each other's
            raise NotImplementedError(f"training with gradients: at most {nb} images of {x.shape[2]}x{x.shape[3]} per step "
                                      "(one plan's 32-bit addressing range); split the batch and accumulate")
        if x.shape[0] > nb:                            # tensors of one plan are addressed with 32-bit byte offsets
            sub = lambda i: None if noise is None else {k: v[i:i + nb] for k, v in noise.items()}
            return _cat_outputs([self.forward_single_quality(x[i:i + nb], quality, mask_pol, training, True, sub(i))
                                 for i in range(0, x.shape[0], nb)])
        plan = self._plan(x.detach(), base_only=(quality == 0), train=bool(training), train_gs=train_gs, train_lrp=train_lrp)
        out = plan.execute(x.detach(), pr, None, self.use_graph, clone, noise=noise)
        if train_gs:
            out["x_hat"] = _FsqTrainFn.apply(plan, out["x_hat"], self.use_graph, *plan.train_params)
        return out

    # ---- sweep, per-image qualities, rate and coded-size control (DESIGN sections 9f, 9h-9j): the drivers are control.py's
    def _batch_shareable(self) -> bool:
        """Can images at different qualities share one plan?  REM models (a per-quality REM and checkpoint), bf16 storage
        and VAMPIC_CONV=f16x2 (their bits depend on how the launches are batched) loop over single images instead."""
        return not isinstance(self, VarianceMaskingPICREM) and getattr(self, "storage", "fp32") == "fp32" and not ops.f16x2_mode()

    def _sweep_eligible(self) -> bool:
        """With all_scalable no quality reaches the front end (g_a, hyperprior, base slices, progressive (mu, sigma)
        chain): the sweep computes it once.  all_scalable=False (the chain reads the decoded slices of each quality) and
        the models that cannot share a batch (:meth:`_batch_shareable`) run one forward_single_quality per quality instead."""
        return self.all_scalable and self._batch_shareable()

    def _sweep_plan(self, x) -> "_SweepPlan":
        B, H, W = _check_input(x)
        return self._cached_plan(self._plans, ("sweep", B, H, W, str(x.device)), lambda: _SweepPlan(self, B, H, W, x.device),
                                 self._weights_sig())

    def _sweep(self, x, qualities, mask_pol, emit, per_image: bool = False):
        return control._sweep(self, x, qualities, mask_pol, emit, per_image)

    def forward_qualities(self, x, qualities, mask_pol=None):
        """One ``forward_single_quality(x, q, mask_pol, training=False)`` result dict per quality of the list, in list
        order (same keys, shapes and — log2_likelihood_sum up to its float64 summation order — bits; cloned tensors).
        Eligible models (:meth:`_sweep_eligible`) run the front end once for the whole list and the per-quality tail
        batched over the levels; the others loop."""
        return control.forward_qualities(self, x, qualities, mask_pol)

    def forward_per_image(self, x, qualities, mask_pol=None):
        """``forward_single_quality(x[b:b+1], qualities[b], mask_pol, training=False)`` for every image of the batch in ONE
        plan run: the same dict, image b's tensors bit-identical (log2_likelihood_sum up to its float64 summation order).
        ``qualities``: B numbers > 0.  The variance masks read each image's quality from a device table, so the plan keeps
        one hipGraph whatever the qualities.  Models that cannot share a batch (:meth:`_batch_shareable`) loop."""
        return control.forward_per_image(self, x, qualities, mask_pol)

    def forward_qualities_per_image(self, x, Q, mask_pol=None):
        """One result dict per row of ``Q`` [T, B] (a [B] vector: T = 1), shaped like :meth:`forward_qualities`' results, with
        image b of row t at quality Q[t][b].  A row is all zero (the base dict) or all positive.  Eligible models
        (:meth:`_sweep_eligible`) run one front end per sub-batch and the per-image tails in sweep_groups' groups; the
        others run :meth:`forward_per_image` per positive row."""
        return control.forward_qualities_per_image(self, x, Q, mask_pol)

    def compress_per_image(self, x, qualities, mask_pol=None):
        """``compress(x[b:b+1], qualities[b], mask_pol)`` for every image, as a list of B dicts {"strings", "shape",
        "quality"} whose strings and shape are exactly that call's.  The images at quality 0 run the base symbols plan as
        one sub-batch, the others the per-image symbols plan (one graph whatever the qualities); all streams are coded by
        the threaded stream coder (bitstream.encode_streams).  Models that cannot share a batch loop over compress."""
        return control.compress_per_image(self, x, qualities, mask_pol)

    def decompress_per_image(self, items, mask_pol=None):
        """{"x_hat": [B, 3, H, W]} from the list :meth:`compress_per_image` returns (same ``shape`` everywhere), in order:
        image b is what ``decompress(strings_b, shape, quality_b)`` returns.  Zeros and positives are sub-batched as in
        :meth:`compress_per_image`; the per-slice masks of the positives read each image's quality from a device table."""
        return control.decompress_per_image(self, items, mask_pol)

    def compress_to_bytes(self, x, target_bytes, q_tol=1e-3, mask_pol=None):
        """Compress every image to its own byte budget (``target_bytes``: a number or B numbers): :meth:`qualities_for_bytes`,
        then :meth:`compress_per_image` at those qualities.  Returns {"items": that list, "quality": float64 [B], "reached":
        bool [B], "bytes_hi": float64 [B] (the guaranteed upper size)}.  Where ``reached``, the item's strings weigh at most
        the budget (they are the strings of compress(x[b:b+1], q_b): the guarantee of qualities_for_bytes); elsewhere the
        item is the base (quality 0)."""
        return control.compress_to(self, x, target_bytes, q_tol, mask_pol, control.BYTES, "bytes_hi")

    def compress_to_bpp(self, x, target_bpp, q_tol=1e-3, mask_pol=None):
        """Compress every image to its own estimated-rate budget (``target_bpp``: a number or B numbers):
        :meth:`qualities_for_bpp`, then :meth:`compress_per_image`.  Returns {"items", "quality" [B], "reached" [B], "bpp" [B]
        (the estimated bpp at that quality; the coded size is not bounded by it)}."""
        return control.compress_to(self, x, target_bpp, q_tol, mask_pol, control.BPP, "bpp")

    def rate_curve(self, x, qualities, mask_pol=None):
        """The estimated rate of every image of ``x`` at every quality of the list (any order, repeats allowed, any count):
        {"log2_likelihood_sum": float64 [len(qualities), 2, B] (rows y and z, what forward_single_quality returns per
        quality, to its float64 summation order), "bpp": float64 [len(qualities), B] = -(y + z) / (H * W)}.  Eligible models
        (:meth:`_sweep_eligible`) run the front end once per sub-batch and, per group of up to VAM_MAX_LAYER_LEVELS distinct
        qualities, one vam_variance_layers and one vam_gauss_layer_bits launch: no masks, no LRP stacks, no g_s.  The
        others loop over forward_single_quality; REM models are refused."""
        return control.rate_curve(self, x, qualities, mask_pol)

    def qualities_for_bpp(self, x, target_bpp, q_tol=1e-3, mask_pol=None):
        """The largest quality whose estimated rate fits a budget, per image: ``target_bpp`` a float, T floats or a [T, B]
        tensor (per-image budgets).  Returns {"quality": float64 [T, B], "bpp": float64 [T, B] (the estimated bpp at that
        quality), "reached": bool [T, B]} on the host, with, per image b and target t:  bpp_b(q*) <= t;  q* = 10 or
        bpp_b(min(10, q* + q_tol)) > t;  and q* = 0 with reached = False when even the base exceeds the budget.
        Eligible models run the front end once per sub-batch and refine a bracket per (target, image) on grids of
        RATE_GRID points (:func:`rate_search`): a pass is vam_variance_layers + vam_gauss_layer_bits on the buffers the
        front end left in place and one host synchronisation.  The others bisect over forward_single_quality."""
        return control.solve(self, x, target_bpp, q_tol, mask_pol, control.BPP)

    def coded_size_curve(self, x, qualities, mask_pol=None):
        """The size of the strings of ``compress(x[b:b+1], q)`` — z, the base slices and, for q > 0, the progressive slices —
        for every image at every quality of the list (any order, repeats allowed, any count), without running it:
        {"bytes_lo", "bytes_hi": int64 [len(qualities), B] with bytes_lo <= actual <= bytes_hi guaranteed (each stream
        is one of at most two lengths, 4 bytes apart), "bits": float64 [len(qualities), B] the exact table cost}.  Eligible
        models (:meth:`_sweep_eligible`) run the front end once per sub-batch, price z and the base slices once, and per
        group of up to VAM_MAX_LAYER_LEVELS distinct qualities run one vam_variance_layers and one vam_coded_layer_bits
        launch.  The others loop over the real compress (bytes_lo == bytes_hi == the actual size); REM models are refused."""
        return control.coded_size_curve(self, x, qualities, mask_pol)

    def qualities_for_bytes(self, x, target_bytes, q_tol=1e-3, mask_pol=None):
        """The largest quality whose coded size fits a byte budget, per image: ``target_bytes`` a number, T numbers or a
        [T, B] tensor.  Returns {"quality": float64 [T, B], "bytes": float64 [T, B] (bytes_hi of coded_size_curve at that
        quality), "reached": bool [T, B]} on the host, with, per image b and target t: the strings of the real
        compress(x[b:b+1], q*) weigh <= t;  q* = 10 or bytes_hi(min(10, q* + q_tol)) > t (for a bytes_hi that does not
        decrease in q);  q* = 0 with reached = False when even the base exceeds t.  :func:`rate_search` over bytes_hi:
        one front end per sub-batch; the first pass is the batched size tail, every later pass one
        vam_variance_layers_per_image and one vam_coded_layer_bits launch for the sub-batch and one synchronisation."""
        return control.solve(self, x, target_bytes, q_tol, mask_pol, control.BYTES)

    def forward(self, x, quality=None, mask_pol=None, training=True, noise=None):
        """models/pic.py:301-491: the base pass plus one progressive pass per requested quality (default [0, 10]),
        stacked as the reference stacks them.  ``training=True`` evaluates the likelihoods with additive uniform noise;
        without trainable parameters the values only (see :meth:`forward_single_quality`), and the same noise tensors
        serve every quality.  With trainable parameters (first-stage training) the result is differentiable for any list
        [0, q1, ..., qL] with q_k > 0: x_hat [L+1, B, 3, H, W], likelihoods {"y": base, "y_prog": [L, B, 2d, h, w] (each
        level's block holds the base likelihoods again), "z"}; ``noise["y"]`` is then [B, d * (L+1), h, w] (base, then
        one block per level, the reference's draw order) or [B, 2d, h, w] (one progressive block shared by the levels)."""
        qs = self.define_quality(quality)
        if training and torch.is_grad_enabled() and self._trainable_outside_rem():
            return self._forward_full_train(x, qs, mask_pol, noise, single=False)
        sweep = None
        if not training and self._sweep_eligible():
            sweep = self.forward_qualities(x, [0] + list(qs[1:]), mask_pol)       # one front end for the whole list
        base = sweep[0] if sweep else self.forward_single_quality(x, 0, mask_pol, training, noise=noise)
        x_hats, y_prog, y_hat_total = [base["x_hat"].unsqueeze(0)], [], [base["y_hat"]]
        out = None
        for i, q in enumerate(qs[1:]):
            out = sweep[i + 1] if sweep else self.forward_single_quality(x, q, mask_pol, training, noise=noise)
            x_hats.append(out["x_hat"].unsqueeze(0))
            y_prog.append(out["likelihoods"]["y"].unsqueeze(0))
            y_hat_total.append(out["y_hat"])
        lik_b = base["likelihoods"]["y"]
        return {"x_hat": torch.cat(x_hats, 0),
                "likelihoods": {"y": lik_b, "y_prog": torch.cat(y_prog, 0) if y_prog else lik_b,
                                "z": base["likelihoods"]["z"]},
                "y_hat": y_hat_total, "y_base": base["y_hat"], "y_prog": out["y_hat"] if out else base["y_hat"]}

    def _forward_full_train(self, x, qs, mask_pol, noise, single: bool):
        """Training forward WITH gradients of every trainable parameter (BASELINE configs[3] `first_train`, train.py:146-149;
        `refine_gs_ga` as a subset): full_train.FullTrainPlan, autograd-connected through :class:`_FullTrainFn`.
        ``single`` = False: ``forward(x, [0, q])`` (pic.py:301-491); True: ``forward_single_quality(x, q)`` (:497-666)."""
        from .full_train import FullTrainPlan
        if ops.f16x2_mode():
            raise NotImplementedError(F16X2_REFUSAL)
        mask_pol = self._mask_policy(mask_pol)
        n_lv = 0 if single else len(qs) - 1
        if not single and (n_lv < 1 or qs[0] != 0 or any(not q_ > 0 for q_ in qs[1:])):
            raise NotImplementedError("training forward with gradients: quality lists [0, q1, ..., qL] with every q_k > 0 "
                                      f"(train.py:147: [0, 10]); got {qs}")
        if n_lv > 1 and not self.all_scalable:
            raise NotImplementedError("training forward with gradients over several quality levels is built for all_scalable=True "
                                      "(README config): the levels then share the progressive (mu, sigma) chain")
        if n_lv > L.VAM_MAX_MASK_LEVELS:
            raise NotImplementedError(f"training forward with gradients: at most {L.VAM_MAX_MASK_LEVELS} quality levels per step "
                                      f"(one vam_variance_mask_levels launch); got {n_lv}")
        Ly._no_autograd(x)
        L.require_gpu()
        self._check_config()
        q = qs[-1]
        nb = _max_images_per_plan(x)
        if x.shape[0] > nb:
            raise NotImplementedError(f"training with gradients: at most {nb} images of {x.shape[2]}x{x.shape[3]} per step")
        if n_lv > 1 and n_lv * x.shape[0] > nb:
            raise NotImplementedError(f"training with gradients over {n_lv} quality levels: the level tail runs as levels x images "
                                      f"= {n_lv * x.shape[0]} images of {x.shape[2]}x{x.shape[3]} in one plan, at most {nb}")
        B, H, W = _check_input(x)
        base_only = single and q == 0
        mode = "single" if single else ("multi" if n_lv == 1 else "levels")
        key = ("full_train", B, H, W, mode, base_only, str(x.device)) + ((n_lv,) if mode == "levels" else ())
        # no staleness check: the plan re-packs every module it reads at each step (the REMs are not on its path)
        plan = self._cached_plan(self._plans, key, lambda: FullTrainPlan(self, B, H, W, mode, base_only, x.device,
                                                                         n_levels=max(n_lv, 1)))
        pr = [_mask_quality(mask_pol, q_) for q_ in qs[1:]] if mode == "levels" else _mask_quality(mask_pol, q)
        raw = plan.execute(x.detach(), pr, self.use_graph, noise=noise)
        x_hat, lik, z_lik = _FullTrainFn.apply(plan, self.use_graph, getattr(self, "grad_reducer", None), raw["x_hat"], raw["lik"],
                                               raw["z_lik"], *plan.params)
        d = self.division_dimension[0]
        if single:
            yh = raw["y_base"] if base_only else raw["y_prog"]
            out = {"x_hat": x_hat[0], "likelihoods": {"y": lik, "z": z_lik}, "y_hat": yh, "y_base": raw["y_base"], "y_prog": yh,
                   "mu_base": raw["mu_base"], "std_base": raw["std_base"]}
            if not base_only:
                out.update({"mu": raw["mu"], "std": raw["std"], "mask": raw["mask"]})
            return out
        if mode == "levels":
            # lik = [base | level 1 | ... | level L] channel blocks; each level's y_prog entry repeats the base block
            # (pic.py:471-472): autograd sums the base's L+1 appearances
            lik_b = lik[:, :d]
            y_prog_lik = torch.stack([torch.cat([lik_b, lik[:, k * d:(k + 1) * d]], 1) for k in range(1, n_lv + 1)], 0)
            yps = list(raw["y_prog"].split(B, 0))
            return {"x_hat": x_hat, "likelihoods": {"y": lik_b, "y_prog": y_prog_lik, "z": z_lik},   # pic.py:480-491
                    "y_hat": [raw["y_base"]] + yps, "y_base": raw["y_base"], "y_prog": yps[-1],
                    "mu_base": raw["mu_base"], "std_base": raw["std_base"], "mu_prog": raw["mu"], "std_prog": raw["std"]}
        return {"x_hat": x_hat, "likelihoods": {"y": lik[:, :d], "y_prog": lik.unsqueeze(0), "z": z_lik},   # pic.py:389-390,471-472,486-491
                "y_hat": [raw["y_base"], raw["y_prog"]], "y_base": raw["y_base"], "y_prog": raw["y_prog"],
                "mu_base": raw["mu_base"], "std_base": raw["std_base"], "mu_prog": raw["mu"], "std_prog": raw["std"]}

    # ---- bitstream path (models/pic.py:671-967; rem_pic.py:425-818)
    def _rem_choice(self, quality, checkpoint_rep):
        return None                                    # no REM in the plain model

    def compress(self, x, quality=0.0, mask_pol=None, checkpoint_rep=None, real_compress=True):
        """One rANS stream per (slice, image) for y and per image for z.  The latents, entropy
        parameters, masks, symbols and table indexes come from the fused HIP plan; only the
        bit-serial coder runs on the host (as in the reference, entropy_models.py:231-239)."""
        mask_pol = self._mask_policy(mask_pol)
        Ly._no_autograd(x)
        L.require_gpu()
        self._check_config()
        base_only = quality <= 0
        rem_idx = None if base_only else self._rem_choice(quality, checkpoint_rep)
        pr = _mask_quality(mask_pol, quality)
        plan = self._plan(x, base_only=base_only, rem_idx=rem_idx, symbols=True)
        out = plan.execute(x, pr, checkpoint_rep if rem_idx is not None else None, self.use_graph, True)
        B, C = plan.B, self.dim_chunk
        n_sl = self.ns0 if base_only else self.ns1
        y_strings: List[List[bytes]] = []
        if real_compress:
            from . import bitstream as bs
            if plan.idx is None:
                raise ValueError(EMPTY_SCALE_TABLE.format("compress"))
            tg, te = bs.Tables.of(self.gaussian_conditional), bs.Tables.of(self.entropy_bottleneck)
            sym = plan.sym.buf.cpu().numpy()           # [B,h,w,C_lat] int32 (synchronises)
            idx = plan.idx.buf.cpu().numpy()
            zs = plan.z_sym.buf.cpu().numpy()
            for i in range(n_sl):                       # stream order: [C, h, w] per image, as the reference flattens
                sl = slice(i * C, (i + 1) * C)
                y_strings.append([bs.encode(sym[b, :, :, sl].transpose(2, 0, 1), idx[b, :, :, sl].transpose(2, 0, 1), tg)
                                  for b in range(B)])
            zi = torch.arange(self.N, dtype=torch.int32).numpy()[:, None, None]
            z_strings = [bs.encode(zs[b].transpose(2, 0, 1), np.broadcast_to(zi, (self.N,) + zs.shape[1:3]), te)
                         for b in range(B)]
        else:                                           # rem_pic.py:498-500,594-597: the quantised tensors instead of bytes
            sy = plan.sym.buf.permute(0, 3, 1, 2)
            y_strings = [sy[:, i * C:(i + 1) * C].float() for i in range(n_sl)]
            z_strings = [plan.z_sym.buf.permute(0, 3, 1, 2).float()]
        res = {"strings": [y_strings, z_strings], "shape": (plan.H // 64, plan.W // 64),
               "masks": [] if base_only else list(out["mask"].chunk(self.ns0, 1)), "y_hat": out["y_hat"]}
        if base_only:
            res.update({"mean_base": out["mu_base"], "scale_base": out["std_base"], "std_base": out["std_base"],
                        "y_hat_base": out["y_hat"]})
        return res

    def decompress(self, strings, shape, quality, mask_pol=None, checkpoint_rep=None):
        """models/pic.py:838-967: z -> hyper-synthesis -> slice by slice (entropy parameters on the
        GPU, rANS decode on the host, LRP on the GPU) -> g_s."""
        mask_pol = self._mask_policy(mask_pol)
        L.require_gpu()
        self._check_config()
        dev = self.entropy_bottleneck.quantiles.device
        B = len(strings[1])
        hz, wz = int(shape[0]), int(shape[1])
        base_only = quality == 0
        rem_idx = None if base_only else self._rem_choice(quality, checkpoint_rep)

        def build():
            if ops.f16x2_mode():
                raise NotImplementedError(F16X2_REFUSAL)
            return _DecPlan(self, B, hz, wz, base_only, rem_idx, dev)
        dp = self._cached_plan(self._dec_plans, (B, hz, wz, base_only, rem_idx, str(dev)), build, self._weights_sig(), rem_idx)
        return {"x_hat": dp.decode(strings, _mask_quality(mask_pol, quality), checkpoint_rep if rem_idx is not None else None)}

    def _prog_dec_plan(self, B, hz, wz, q_list) -> "_ProgDecPlan":
        """The plans of progressive.ProgressiveDecoder for one (B, z-shape, quality list), cached beside decompress's."""
        dev = self.entropy_bottleneck.quantiles.device
        return self._cached_plan(self._dec_plans, ("prog", B, hz, wz, tuple(float(q) for q in q_list), str(dev)),
                                 lambda: _ProgDecPlan(self, B, hz, wz, q_list, dev), self._weights_sig())


class VarianceMaskingPICREM(VarianceMaskingPIC):
    """models/rem_pic.py:8-818."""

    def __init__(self, N=192, M=640, division_dimension=[320, 416], dim_chunk=32, multiple_decoder=True,
                 multiple_encoder=True, multiple_hyperprior=True, support_progressive_slices=5, delta_encode=True,
                 total_mu_rep=True, all_scalable=True, mask_policy="point-based-std", check_levels=[0.01, 0.25, 1.75],
                 mu_std=True, dimension="big", **kwargs):
        super().__init__(N=N, M=M, division_dimension=division_dimension, dim_chunk=dim_chunk,
                         multiple_decoder=multiple_decoder, multiple_encoder=multiple_encoder,
                         multiple_hyperprior=multiple_hyperprior, support_progressive_slices=support_progressive_slices,
                         delta_encode=delta_encode, total_mu_rep=total_mu_rep, all_scalable=all_scalable,
                         mask_policy=mask_policy, **kwargs)
        self.dimension = dimension
        self.check_levels = check_levels
        self.num_rems = len(check_levels)
        self.enable_rem = [True] * self.num_rems
        self.mu_std = mu_std
        self.post_latent = nn.ModuleList(
            nn.ModuleList(Ly.LatentRateReduction(dim_chunk=dim_chunk, mu_std=mu_std, dimension=dimension) for _ in range(10))
            for _ in range(self.num_rems))

    def unfreeze_rems(self):
        for p in self.post_latent.parameters():
            p.requires_grad = True

    def load_state_dict(self, state_dict, strict=True):
        """Loads parent keys non-strictly and ``post_latent.*`` strictly, as rem_pic.py:66-78 intends
        (the reference forgets to strip the ``post_latent.`` prefix and fails on its own checkpoints;
        both prefixed and stripped keys are accepted here)."""
        own = self.state_dict()
        parent = {k: v for k, v in state_dict.items() if k in own and "post_latent" not in k}
        res = super().load_state_dict(parent, strict=False)
        post = {(k[len("post_latent."):] if k.startswith("post_latent.") else k): v
                for k, v in state_dict.items() if "post_latent" in k}
        if post:
            self.post_latent.load_state_dict(post, strict=True)
            self.enable_rem = [True] * self.num_rems
        else:
            print("This model does not have trained REMs.  self.enable_rem will be set to False")
            self.enable_rem = [False] * self.num_rems
        return res

    def find_check_quality(self, quality):
        """models/rem_pic.py:142-165."""
        cl = self.check_levels
        if quality <= cl[0]:
            return 0, 0, -1
        if len(cl) in (2, 3) and cl[0] < quality <= cl[1]:
            return cl[0], cl[1], 0
        if len(cl) == 2 and quality > cl[1]:
            return cl[1], 10, 1
        if len(cl) == 3 and cl[1] < quality <= cl[2]:
            return cl[1], cl[-1], 1
        return cl[-1], 10, -1

    def _rem_index(self, quality):
        """models/rem_pic.py:200-213."""
        cl = self.check_levels
        if self.num_rems == 1:
            return 0
        if self.num_rems == 2:
            return 0 if cl[0] < quality <= cl[1] else 1
        if cl[0] < quality <= cl[1]:
            return 0
        if cl[1] < quality <= cl[2]:
            return 1
        return 2

    def forward_single_quality(self, x, quality, mask_pol="point-based-std", training=False, checkpoint_ref=None,
                               clone=True, noise=None):
        return self.forward(x=x, quality=quality, mask_pol=mask_pol, training=training, checkpoint_ref=checkpoint_ref,
                            clone=clone, noise=noise)

    def forward(self, x, mask_pol="point-based-std", quality=0, training=True, checkpoint_ref=None, clone=True,
                noise=None):
        """models/rem_pic.py:229-422.  ``training=True`` is the REM fine-tune forward (BASELINE configs[4]):
        additive-noise likelihoods, autograd-connected to the ``post_latent`` parameters only."""
        if training:
            return self._forward_train(x, mask_pol, quality, checkpoint_ref, noise)
        mask_pol = self._mask_policy(mask_pol)
        Ly._no_autograd(x)
        L.require_gpu()
        self._check_config()
        nb = _max_images_per_plan(x)
        if x.shape[0] > nb:                            # tensors of one plan are addressed with 32-bit byte offsets
            return _cat_outputs([self.forward(x[i:i + nb], mask_pol, quality, False,
                                              None if checkpoint_ref is None else checkpoint_ref[i:i + nb], True)
                                 for i in range(0, x.shape[0], nb)])
        rem_idx = self._rem_choice(quality, checkpoint_ref) if quality != 0 else None
        pr = _mask_quality(mask_pol, quality)
        plan = self._plan(x, base_only=(quality == 0), rem_idx=rem_idx)
        return plan.execute(x, pr, checkpoint_ref if rem_idx is not None else None, self.use_graph, clone)

    def forward_finetune(self, x, quality, mask_pol="point-based-std", noise=None):
        """One fused plan for the fine-tune step's two forward passes: bit-identical to
        ``ck = ExtractChekpointRepr(x, q_ref, rc=False); forward_single_quality(x, quality, training=True,
        checkpoint_ref=ck)`` (training/step.py:67-76) because everything up to the progressive (mu, sigma) chain
        does not depend on the quality — the checkpoint latent is derived from the same front end instead of a
        second run of g_a / hyperprior / slices."""
        from .finetune import extract_quality_ref
        q_ref = extract_quality_ref(quality, self.check_levels)
        if q_ref is None:
            return self._forward_train(x, mask_pol, quality, None, noise)
        return self._forward_train(x, mask_pol, quality, "own", noise, ck_pr=q_ref)

    def _forward_train(self, x, mask_pol, quality, checkpoint_ref, noise, ck_pr=None):
        """Training-mode forward (rem_pic.py:229-422 with training=True; training/step.py:62-76).  Everything
        outside ``post_latent`` must be frozen (``freeze_all(); unfreeze_rems()``): those transforms have no
        backward kernels in this build, and silently dropping their gradients would be wrong."""
        rem_ids = {id(p) for p in self.post_latent.parameters()}
        loose = [n for n, p in self.named_parameters() if p.requires_grad and id(p) not in rem_ids]
        if loose:
            raise NotImplementedError("training-mode forward is built for --training_type rems only (call freeze_all(); "
                                      f"unfreeze_rems()); trainable non-REM parameters: {loose[:3]}...")
        mask_pol = self._mask_policy(mask_pol)
        L.require_gpu()
        self._check_config()
        own = isinstance(checkpoint_ref, str)
        if checkpoint_ref is not None and not own:
            checkpoint_ref = checkpoint_ref.detach()
        rem_idx = self._rem_choice(quality, checkpoint_ref) if quality != 0 else None
        pr = _mask_quality(mask_pol, quality)
        own = own and rem_idx is not None
        if own:
            ck_pr = _mask_quality(mask_pol, ck_pr)
        plan = self._plan(x.detach(), base_only=(quality == 0), rem_idx=rem_idx, train=True, own_ck=own)
        out = plan.execute(x.detach(), pr, checkpoint_ref if (rem_idx is not None and not own) else None, self.use_graph,
                           True, noise=noise, ck_pr=ck_pr if own else None)
        if rem_idx is not None and torch.is_grad_enabled() and any(p.requires_grad for p in plan.train_params):
            out["likelihoods"]["y"] = _FsqTrainFn.apply(plan, out["likelihoods"]["y"], self.use_graph, *plan.train_params)
        return out

    def apply_latent_enhancement(self, current_index, quality, quality_bar, y_b_hat, mu_scale_base, mu_scale_enh,
                                 mu, scale, training=False, mask_pol="point-based-std", attention_mask=None):
        """models/rem_pic.py:167-220 on NCHW tensors (module-level surface used by the progressive
        harness, test/functions_encode.py:126-141): refine (mu, scale) of one progressive slice."""
        if attention_mask is None:
            attention_mask = self.masking(scale, pr=quality, mask_pol=mask_pol)
        if self.mu_std:
            attention_mask = torch.cat([attention_mask, attention_mask], dim=1)
        if quality <= self.check_levels[0]:
            return mu, scale
        block = self.post_latent[self._rem_index(quality)][current_index]
        enhanced = block(y_b_hat, mu_scale_base, mu_scale_enh, attention_mask)
        if self.mu_std:
            mu, scale = enhanced.chunk(2, 1)
            return mu, scale
        return mu, enhanced

    def _rem_choice(self, quality, checkpoint_rep):
        """Which REM (if any) refines the entropy parameters (rem_pic.py:197-213,363,566)."""
        if checkpoint_rep is None or quality <= self.check_levels[0]:
            return None
        _, _, right = self.find_check_quality(quality)
        return self._rem_index(quality) if self.enable_rem[right] else None

    def ExtractChekpointRepr(self, x, quality, rc=True, y_check=None):
        """rem_pic.py:121-132: compress(...)["y_hat"].  The coder is lossless, so y_hat does not
        depend on ``rc``; with rc=False no host coding happens at all."""
        if rc and self.gaussian_conditional._quantized_cdf.numel() == 0:
            rc = False                                 # tables not built: y_hat is the same without the bytes
        return self.compress(x, quality=quality, mask_pol="point-based-std", real_compress=rc,
                             checkpoint_rep=y_check)["y_hat"]


# ----------------------------------------------------------------------------- the fused plan
# Largest tensor of a plan: the 192-channel feature map at half resolution (and the 576-channel qkv at quarter
# resolution, smaller).  The kernels address a tensor with 32-bit BYTE offsets, so one plan holds at most
# 2^31 / (192 ch * 4 B) / (1/4) pixels of input; larger batches run as several plans over sub-batches.
MAX_PLAN_PIXELS = int((2 ** 31 - 2 ** 20) // (192 * 4) * 4)


def _max_images_per_plan(x) -> int:
    return max(1, MAX_PLAN_PIXELS // (x.shape[2] * x.shape[3]))


def _check_input(x):
    """(B, H, W) of an image batch the plans accept."""
    B, C_, H, W = x.shape
    if C_ != 3 or H % 64 or W % 64:
        raise ValueError(f"expected [B,3,H,W] with H,W multiples of 64 (reference pads to 64), got {tuple(x.shape)}")
    return B, H, W


def _mask_quality(mask_pol, q):
    """The quality the variance mask is computed at (channel_mask.py:152-153: two-levels is all ones unless pr == 0)."""
    return 10 if (mask_pol == "two-levels" and q != 0) else q


EMPTY_SCALE_TABLE = "empty scale table: call model.update() before {}()"

F16X2_REFUSAL = ("the fp16x2 arithmetic (VAMPIC_CONV=f16x2) is an evaluation-forward configuration: its results depend, in "
                 "the last bits, on the power-of-two scale of each launch (batch composition, plan structure), so the "
                 "bitstream path (encoder and decoder must agree bit for bit) and training run in the default bf16x3 arithmetic")


def _mask_table_buffer(B: int, device) -> torch.Tensor:
    """A plan's device table for ops.variance_masks_per_image: one record per image, refilled before each replay."""
    import ctypes
    return torch.zeros((B * ctypes.sizeof(L.VamLayerParams),), dtype=torch.uint8, device=device)


def _cat_outputs(outs):
    """Concatenate per-sub-batch result dicts along the batch dimension (every image is an independent unit)."""
    def cat(vals):
        v0 = vals[0]
        if isinstance(v0, dict):
            return {k: cat([v[k] for v in vals]) for k in v0}
        if isinstance(v0, (list, tuple)):
            return type(v0)(cat([v[i] for v in vals]) for i in range(len(v0)))
        if torch.is_tensor(v0):
            if v0.dim() == 2 and v0.dtype == torch.float64:          # log2_likelihood_sum [2, B]
                return torch.cat(vals, dim=1)
            return torch.cat(vals, dim=0)
        return v0
    return cat(outs)


def _slice_stack_heads(plan, m, means_h, scales_h, which):
    """Hyperprior part of the first layer of every slice stack (engine.lower_stack_heads): base stacks read the first
    ``d`` channels of the hyper tensors, progressive ones the second (pic.py:528-529,598-599); the LRP stacks share the
    MEAN support of their slice (pic.py:548,635).  ``which`` = "base" or "prog".  Encoder and decoder plans both call
    this, so both associate the first-layer sum the same way."""
    d, ns = m.division_dimension[0], m.ns0
    stacks, hyp, sup = [], [], []
    if which == "base":
        mh0, sh0 = means_h.window(0, d), scales_h.window(0, d)
        for i in range(ns):
            stacks += [m.cc_mean_transforms[i], m.cc_scale_transforms[i], m.lrp_transforms[i]]
            hyp += [mh0, sh0, mh0]
            sup += [i > 0, i > 0, True]
    else:
        mh1, sh1 = means_h.window(d, d), scales_h.window(d, d)
        for j in range(ns):
            stacks += [m.cc_mean_transforms_prog[j], m.cc_scale_transforms_prog[j], m.lrp_transforms_prog[j]]
            hyp += [mh1, sh1, mh1]
            sup += [True, True, True]
    return E.lower_stack_heads(plan, stacks, hyp, sup)


def _lower_hyper_synthesis(plan, m, z_hat, base_only):
    """compute_hyperprior's synthesis half (pic.py:285-298): with multiple_hyperprior two (mean, scale) pairs of d
    channels each — only the first at quality 0 —, otherwise ONE pair with M channels whose halves feed the base and
    the progressive stacks.  Returns (means_h, scales_h)."""
    d = m.division_dimension[0]
    B, hz, wz = z_hat.B, z_hat.H, z_hat.W
    if m.multiple_hyperprior:
        nh = 1 if base_only else 2
        means_h, scales_h = plan.buf(B, 4 * hz, 4 * wz, nh * d), plan.buf(B, 4 * hz, 4 * wz, nh * d)
        E.lower_stacks(plan, [m.h_mean_s[k] for k in range(nh)] + [m.h_scale_s[k] for k in range(nh)], [[z_hat]] * (2 * nh),
                       [means_h.window(k * d, d) for k in range(nh)] + [scales_h.window(k * d, d) for k in range(nh)])
    else:
        means_h, scales_h = plan.buf(B, 4 * hz, 4 * wz, m.M), plan.buf(B, 4 * hz, 4 * wz, m.M)
        E.lower_stacks(plan, [m.h_mean_s, m.h_scale_s], [[z_hat]] * 2, [means_h, scales_h])
    return means_h, scales_h


def _version_sig(mod: nn.Module):
    return tuple(p._version for p in mod.parameters())


def _check_tape(ctx):
    """The tape lives in the plan's buffers: it belongs to ONE execute() of the plan."""
    if ctx.plan.generation != ctx.generation:
        raise RuntimeError(
            "the training plan for this shape ran again before this backward(): its tape (activations, noise, "
            "mask) now belongs to the later forward.  Call loss.backward() before the next training forward of "
            "the same shape (gradient accumulation: backward after every forward).")


class _FsqTrainFn(torch.autograd.Function):
    """One output of a training-mode _FsqPlan as a differentiable function of the parameters the plan trains:
    likelihoods["y"] under ``--training_type rems`` (the REM parameters, train.py:223-226), x_hat under ``refine_gs``
    (the synthesis transform's, with ``--lrp`` the progressive LRP stacks' as well, train.py:216-218)."""

    @staticmethod
    def forward(ctx, plan, out, use_graph, *params):
        ctx.plan, ctx.use_graph, ctx.generation = plan, use_graph, plan.generation
        return out.clone()

    @staticmethod
    def backward(ctx, g):
        _check_tape(ctx)
        grads = ctx.plan._backward(g, ctx.use_graph)
        return (None, None, None) + tuple(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[3:]))


class _FullTrainFn(torch.autograd.Function):
    """(x_hat, likelihoods y, likelihoods z) of the complete training plan as differentiable functions of every parameter
    on the path.  backward() runs the plan's backward (and, when the model carries a ``grad_reducer``, the bucketed
    gradient exchange of a multi-GPU job while it runs) and hands each parameter its slice of the flat buffer."""

    @staticmethod
    def forward(ctx, plan, use_graph, reducer, x_hat, lik, z_lik, *params):
        ctx.plan, ctx.use_graph, ctx.reducer, ctx.generation = plan, use_graph, reducer, plan.generation
        return x_hat, lik, z_lik

    @staticmethod
    def backward(ctx, g_xhat, g_lik, g_z):
        _check_tape(ctx)
        plan = ctx.plan
        plan.backward(g_xhat, g_lik, g_z, ctx.use_graph, ctx.reducer)
        need = ctx.needs_input_grad[6:]
        # ONE copy of the flat gradient buffer (the plan overwrites its own at the next backward); every parameter's
        # gradient is a view of the copy, so the clip can run as one reduction over it (finetune.clip_grad_norm_)
        flat = plan.flat.clone()
        plan.handout = (flat, sum(1 for n in need if n), all(need))
        return (None,) * 6 + tuple(flat[o:o + p.numel()].view(p.shape) if n else None
                                   for o, p, n in zip(plan.offsets, plan.params, need))


class _FsqPlan:
    """``forward_single_quality`` for one (B,H,W) lowered to libvampic launches."""

    def __init__(self, m: VarianceMaskingPIC, B, H, W, base_only, rem_idx, device, symbols=False, train=False,
                 own_ck=False, train_gs=False, train_lrp=False, sweep=False, per_image=False):
        assert not sweep or (m.all_scalable and not base_only and rem_idx is None and not (symbols or train))
        # per_image: the variance masks read each image's quality from a device table
        assert not per_image or not (sweep or base_only or train or own_ck or rem_idx is not None)
        self.per_image = per_image
        self.qtable = _mask_table_buffer(B, device) if per_image else None
        self.m, self.B, self.H, self.W = m, B, H, W
        self.train_gs = train_gs    # the synthesis transform in use is being trained (refine_gs): taped g_s + backward plan
        self.train_lrp = train_lrp  # ... and the progressive LRP stacks with it (refine_gs --lrp)
        self.own_ck, self.ck_pr = own_ck, 0.0     # fine-tune: derive the checkpoint latent inside this plan
        self.base_only, self.rem_idx = base_only, rem_idx
        self.symbols = symbols
        self.train = train          # additive-noise likelihoods (+ taped REM and a backward plan when rem_idx is set)
        self.bwd = None             # backward plan of a training plan (REM fine-tune or refine_gs): see _backward
        self.generation = 0         # bumped by every execute(): which forward the training tape belongs to
        self.pr = 0.0
        self.runner = E.Runner(device, cap=32)      # forward graphs per (pr, ck_pr)
        self.bwd_runner = E.Runner(device)          # the backward's graph (no cap), replayed on self.runner's stream
        plan = self.plan = E.Plan(device)
        h, w = H // 16, W // 16
        d = m.division_dimension[0]
        ns = m.ns0
        f32 = dict(dtype=torch.float32, device=device)
        self.x_in = torch.empty((B, 3, H, W), **f32)
        self.x_hat = torch.empty((B, 3, H, W), **f32)
        self.log2sum = torch.zeros((2, B), dtype=torch.float64, device=device)   # [y, z] per image
        plan.keep += [self.x_in, self.x_hat, self.log2sum]
        ls_y, ls_z = self.log2sum[0], self.log2sum[1]
        plan.call(lambda: ops.memset_zero(self.log2sum))

        # ---- analysis transforms (both encoders in lockstep)                      pic.py:506-508
        x_s2d = plan.buf(B, H // 2, W // 2, 16)
        plan.call(lambda: L.check(L.load().vam_s2d_input(self.x_in.data_ptr(), x_s2d.ptr, B, H, W, ops.stream_ptr()),
                                  "vam_s2d_input"))
        y = self.y = plan.buf(B, h, w, 2 * d)
        plan.set_class("g_a")
        act16 = getattr(m, "storage", "fp32") == "bf16"
        plan.act16 = act16
        if m.multiple_encoder:
            E.lower_g_a(plan, [m.g_a[0], m.g_a[1]], x_s2d, [y.window(0, d), y.window(d, d)])
        else:                                            # one encoder with M output channels (builder.py:56-67)
            E.lower_g_a(plan, [m.g_a], x_s2d, [y])
        plan.act16 = False

        # ---- hyperprior                                                            pic.py:278-298
        z = plan.buf(B, h // 4, w // 4, m.N)
        plan.set_class("hyperprior")
        self.z = z
        E.lower_stacks(plan, [m.h_a], [[y]], [z])
        self.z_hat = plan.buf(B, h // 4, w // 4, m.N)
        self.z_lik = plan.buf(B, h // 4, w // 4, m.N)
        # the entropy coder's z symbols (compress) — kept in sweep mode too: coded_size_curve prices them
        self.z_sym = ops.new_iview(B, h // 4, w // 4, m.N, device) if symbols or sweep else None
        plan.keep.append(self.z_sym)
        self.noise_z = plan.buf(B, h // 4, w // 4, m.N) if train else None
        self.noise_y = plan.buf(B, h, w, d if base_only else 2 * d) if train else None
        plan.call(lambda: ops.eb_forward(z, m.entropy_bottleneck.packed_params(), self.z_hat, self.z_lik, ls_z, sym=self.z_sym,
                                         noise=self.noise_z))
        means_h, scales_h = _lower_hyper_synthesis(plan, m, self.z_hat, base_only)
        self.means_h, self.scales_h = means_h, scales_h

        # ---- base slices                                                           pic.py:522-554
        C = m.dim_chunk
        yq = plan.buf(B, h, w, d)                      # round(y-mu)+mu before the LRP correction
        yb = self.y_base = plan.buf(B, h, w, d)        # base y_hat (after LRP)
        self.mu_b = plan.buf(B, h, w, d)
        self.std_b = plan.buf(B, h, w, d)
        self.lik = plan.buf(B, h, w, d if base_only else 2 * d)
        # entropy-coder inputs (compress only): quantised symbols and scale-table indexes
        self.sym = ops.new_iview(B, h, w, d if base_only else 2 * d, device) if symbols else None
        table = m.gaussian_conditional.scale_table
        indexes = symbols and table.numel() > 0        # without update() only real_compress=False is possible
        self.idx = ops.new_iview(B, h, w, d if base_only else 2 * d, device) if indexes else None
        plan.keep += [self.sym, self.idx]
        sl = lambda v, i, n=1: v.window(i * C, n * C)
        mh0, sh0 = means_h.window(0, d), scales_h.window(0, d)
        hyper_done = plan.record() if not base_only else None
        plan.set_class("stack_heads")
        heads = _slice_stack_heads(plan, m, means_h, scales_h, "base")     # hyperprior part of every first layer, up front
        plan.set_class("slice_chain")

        def base_group(idx: List[int]):
            sup = [sl(yb, 0, min(m.max_support_slices, idx[0]))] if idx[0] > 0 else []
            E.lower_stacks(plan, [m.cc_mean_transforms[i] for i in idx] + [m.cc_scale_transforms[i] for i in idx],
                           [sup] * (2 * len(idx)),
                           [sl(self.mu_b, i) for i in idx] + [sl(self.std_b, i) for i in idx], heads=heads)
            i0, n = idx[0], len(idx)
            plan.call(lambda: ops.gauss_tail(sl(y, i0, n), sl(self.mu_b, i0, n), sl(self.std_b, i0, n),
                                             yhat=sl(yq, i0, n), lik=sl(self.lik, i0, n), log2sum=ls_y,
                                             sym=sl(self.sym, i0, n) if symbols else None))
            if train:        # quantize "noise": likelihood at y + U(-.5,.5) - mu (entropy_models.py:132-138,643-651)
                plan.call(lambda: ops.gauss_train(sl(y, i0, n), sl(self.mu_b, i0, n), sl(self.std_b, i0, n),
                                                  sl(self.noise_y, i0, n), lik=sl(self.lik, i0, n)))
            if indexes:                                                               # pic.py:737
                plan.call(lambda: ops.build_indexes(sl(self.std_b, i0, n), table, out=sl(self.idx, i0, n)))
            E.lower_stacks(plan, [m.lrp_transforms[i] for i in idx], [sup + [sl(yq, i)] for i in idx],
                           [sl(yb, i) for i in idx],
                           [dict(act=L.ACT_HALF_TANH, post=sl(yq, i)) for i in idx], heads=heads)

        base_done = {}                                   # slice -> event "its y_hat_base is final"
        for i in range(min(ns, m.max_support_slices)):
            base_group([i])
            if not base_only:
                base_done[i] = plan.record()
        if ns > m.max_support_slices:
            base_group(list(range(m.max_support_slices, ns)))   # slices 5..9 only see slices 0..4
            if not base_only:
                ev = plan.record()
                for i in range(m.max_support_slices, ns):
                    base_done[i] = ev

        if base_only:
            if not symbols:                              # compress() does not decode (pic.py:671-860)
                plan.set_class("g_s")
                if train_gs:
                    self._lower_g_s_train(plan, m.g_s[0] if m.multiple_decoder else m.g_s, yb)
                else:
                    plan.act16 = act16
                    E.lower_g_s(plan, [m.g_s[0] if m.multiple_decoder else m.g_s], [yb], [self.x_hat])
                    plan.act16 = False
            return

        # ---- progressive slices                                                    pic.py:577-643
        self.mu_p = plan.buf(B, h, w, d)
        self.std_p = plan.buf(B, h, w, d)
        # support vector of the mean chain: mu + y_hat_base with total_mu_rep (pic.py:601), else mu itself
        mu_tot = plan.buf(B, h, w, d) if m.total_mu_rep else self.mu_p
        sp = m.support_progressive_slices
        mu_std = getattr(m, "mu_std", True)
        y_top = y.window(d, d)
        y_sub = y.window(0, d) if m.delta_encode else None                        # pic.py:583-584
        yp = self.y_prog = plan.buf(B, h, w, d)
        g_s = m.g_s[1] if m.multiple_decoder else m.g_s
        if train and not m.all_scalable:
            raise NotImplementedError("training-mode plans are built for all_scalable=True (README config)")

        def supports(j):
            """determine_support (pic.py:264-270): base slice j + the last min(sp, j) entries of the support vectors
            (mu_total / std_total with all_scalable, the decoded progressive slices otherwise, pic.py:586-587)."""
            s = min(sp, j)
            sm, ss_ = (mu_tot, self.std_p) if m.all_scalable else (yp, yp)
            return ([sl(yb, j)] + ([sl(sm, j - s, s)] if s else []), [sl(yb, j)] + ([sl(ss_, j - s, s)] if s else []))

        if not m.all_scalable:
            self._lower_prog_sequential(plan, heads, means_h, scales_h, hyper_done, supports, y_top, y_sub, yb, yp, ls_y,
                                        table if indexes else None, symbols)
            if not symbols:
                plan.set_class("g_s")
                E.lower_g_s(plan, [g_s], [yp], [self.x_hat])
            return
        msups, ssups = [], []
        # With all_scalable the progressive mu/sigma chain only needs y_hat_base[j] and its own history
        # (pic.py:586-612), so it runs on a second HIP stream concurrently with base slices > j.
        plan.branch(1)
        plan.wait(hyper_done)
        plan.set_class("stack_heads")
        heads.update(_slice_stack_heads(plan, m, means_h, scales_h, "prog"))   # on the chain's stream, beside base slice 0
        plan.set_class("slice_chain")
        for j in range(ns):
            plan.wait(base_done[j])
            ms, ss = supports(j)                                               # the hyperprior part is in `heads`
            msups.append(ms)
            ssups.append(ss)
            E.lower_stacks(plan, [m.cc_mean_transforms_prog[j], m.cc_scale_transforms_prog[j]], [ms, ss],
                           [sl(self.mu_p, j), sl(self.std_p, j)], heads=heads)
            if m.total_mu_rep:
                plan.call(lambda j=j: ops.add(sl(self.mu_p, j), sl(yb, j), sl(mu_tot, j)))   # pic.py:601
        chain_done = plan.record()
        plan.branch(0)
        plan.wait(chain_done)
        if sweep:
            # rate sweep (_SweepPlan): everything up to here does not depend on the quality; the per-level tail and the
            # base reconstruction are plans of their own over these buffers
            self.mu_f, self.std_f = self.mu_p, self.std_p
            self.sweep_parts = dict(heads=heads, yb=yb, mu=self.mu_p, std=self.std_p, mu_tot=mu_tot, y_top=y_top, y_sub=y_sub,
                                    g_s=g_s)
            return

        mu_f, std_f = self.mu_p, self.std_p
        if rem_idx is not None:                                                       # rem_pic.py:363-377
            plan.set_class("rem")
            self.ck = plan.buf(B, h, w, d)
            if own_ck:
                # y_hat at the check level from the SAME front end (everything up to here is quality independent;
                # at q <= check_levels[0] no REM applies): what ExtractChekpointRepr(x, q_ref) returns, pic.py:621-641
                m_ck, rq_ck, junk = plan.buf(B, h, w, d), plan.buf(B, h, w, d), plan.buf(B, h, w, d)
                plan.call(lambda: ops.variance_mask(self.std_p, self.ck_pr, m_ck, n_slice=ns))
                plan.call(lambda: ops.gauss_tail(y_top, self.mu_p, self.std_p, y2=y_sub, mask=m_ck, yhat=rq_ck, lik=junk))
                E.lower_stacks(plan, [m.lrp_transforms_prog[j] for j in range(ns)],
                               [msups[j] + [sl(rq_ck, j)] for j in range(ns)], [sl(self.ck, j) for j in range(ns)],
                               [dict(act=L.ACT_HALF_TANH, post=sl(rq_ck, j), post2=sl(yb, j)) for j in range(ns)], heads=heads)
            att = self.att = plan.buf(B, h, w, d)
            plan.call(lambda: self._vmask(self.std_p, att, ns))
            std_f = plan.buf(B, h, w, d)
            mu_f = plan.buf(B, h, w, d) if mu_std else self.mu_p      # without mu_std only sigma is refined (rem_pic.py:214-218)
            mods = [m.post_latent[rem_idx][j] for j in range(ns)]
            rem_io = ([sl(self.ck, j) for j in range(ns)],
                      [[sl(self.mu_b, j), sl(self.std_b, j)] for j in range(ns)],
                      [([sl(self.mu_p, j)] if mu_std else []) + [sl(self.std_p, j)] for j in range(ns)],
                      [sl(att, j) for j in range(ns)],
                      [([sl(mu_f, j)] if mu_std else []) + [sl(std_f, j)] for j in range(ns)])
            if train:
                self.train_params = [p for mod in mods for p in mod.parameters()]
                self.packs = G.TransformPacks(*E.rem_trained_convs(mods))
                self.packs.record_refresh(plan)
                tape = E.lower_rem_blocks_train(plan, mods, *rem_io, self.packs)
            else:
                self.rem_sig = _version_sig(m.post_latent[rem_idx])
                E.lower_rem_blocks(plan, mods, *rem_io)
        self.mu_f, self.std_f = mu_f, std_f
        plan.set_class("lrp_prog")
        self.mask = plan.buf(B, h, w, d)
        self.thr = torch.empty((B * ns,), **f32)
        plan.keep.append(self.thr)
        plan.call(lambda: self._vmask(std_f, self.mask, ns, self.thr))                              # pic.py:621-622
        rq = plan.buf(B, h, w, d)
        plan.call(lambda: ops.gauss_tail(y_top, mu_f, std_f, y2=y_sub, mask=self.mask, yhat=rq,
                                         lik=self.lik.window(d, d), log2sum=ls_y,
                                         sym=self.sym.window(d, d) if symbols else None))           # pic.py:625-629
        if train:
            yr, y0, nz = y_top, y_sub, self.noise_y.window(d, d)
            plan.call(lambda: ops.gauss_train(yr, mu_f, std_f, nz, y2=y0, mask=self.mask, lik=self.lik.window(d, d)))
            if rem_idx is not None:
                # ---- backward plan: dL/dlik (progressive half) -> (dmu', dsigma') -> REM parameters
                bw = self.bwd = E.Plan(device)
                glik = bw.buf(B, h, w, d)
                self._bwd_in = lambda g: glik.buf.copy_(g[:, d:].permute(0, 2, 3, 1))       # dL/dlikelihoods["y"], NCHW
                dmu, dsg = bw.buf(B, h, w, d), bw.buf(B, h, w, d)
                self.dmu, self.dsg, self.rem_io, self.rem_tape = dmu, dsg, rem_io, tape     # kept for teacher-forced gradient checks
                grads = self._grad_buffer()
                bw.call(lambda: ops.gauss_train(yr, mu_f, std_f, nz, y2=y0, mask=self.mask, grad_lik=glik,
                                                dmu=dmu, dsigma=dsg), "likelihood backward")
                E.lower_rem_backward(bw, tape, mods, [sl(dmu, j) for j in range(ns)], [sl(dsg, j) for j in range(ns)],
                                     rem_io[3], self.packs, grads)
        if indexes:                                                                   # pic.py:813
            plan.call(lambda: ops.build_indexes(std_f, table, mask=self.mask, out=self.idx.window(d, d)))
        lrp = None
        if train_lrp:
            # y_hat_j = rq_j + 0.5 tanh(stack_j(cat(supports, rq_j))) + base_j  (pic.py:635-641); a TRAINED stack runs its
            # first layer whole (the eval plan hoists the hyperprior part: same sum, different association)
            stacks = [m.lrp_transforms_prog[j] for j in range(ns)]
            lpk = [G.TransformPacks(st) for st in stacks]
            for pk_ in lpk:
                pk_.record_refresh(plan)
            mh1 = means_h.window(d, d)
            tapes = G.lower_stacks_train(plan, stacks, [[mh1] + msups[j] + [sl(rq, j)] for j in range(ns)], [None] * ns, lpk)
            for j in range(ns):
                plan.call(lambda j=j: ops.ew(L.EW_HTANH_FWD, [tapes[j]["out"], sl(rq, j), sl(yb, j)], [sl(yp, j)]), "lrp tail")
            lrp = dict(tapes=tapes, packs=lpk, params=[p for st in stacks for p in st.parameters()])
        else:
            E.lower_stacks(plan, [m.lrp_transforms_prog[j] for j in range(ns)], [msups[j] + [sl(rq, j)] for j in range(ns)],
                           [sl(yp, j) for j in range(ns)],
                           [dict(act=L.ACT_HALF_TANH, post=sl(rq, j), post2=sl(yb, j)) for j in range(ns)], heads=heads)   # :635-641
        if not symbols:
            plan.set_class("g_s")
            if train_gs:
                self._lower_g_s_train(plan, g_s, yp, lrp)
            else:
                plan.act16 = act16
                E.lower_g_s(plan, [g_s], [yp], [self.x_hat])
                plan.act16 = False

    def _lower_g_s_train(self, plan, dec, y_in, lrp=None):
        """refine_gs: taped synthesis transform + its backward plan (gs_train.py); ``lrp`` = the taped progressive LRP
        stacks when they train too (refine_gs --lrp): their gradients come from dL/dy_hat, the input gradient of g_s."""
        self.train_params = list(dec.parameters()) + (lrp["params"] if lrp else [])
        self.gs_packs = G.TransformPacks(dec)
        self.gs_packs.record_refresh(plan)
        tape = G.lower_g_s_train(plan, dec, y_in, self.x_hat, self.gs_packs)
        bw = self.bwd = E.Plan(self.x_in.device)
        self.g_xhat = torch.zeros_like(self.x_hat)
        self._bwd_in = self.g_xhat.copy_                                  # dL/dx_hat
        grads = self._grad_buffer()
        bw.keep.append(self.g_xhat)
        d_y = G.lower_g_s_backward(bw, tape, self.x_hat, self.g_xhat, self.gs_packs, grads, need_input_grad=lrp is not None)
        if lrp is not None:
            self.lrp_tapes, self.d_yhat = lrp["tapes"], d_y                    # kept for teacher-forced gradient checks
            dz = []
            for j, t in enumerate(lrp["tapes"]):
                z, dy = t["out"], d_y.window(32 * j, 32)
                o = bw.buf(z.B, z.H, z.W, z.C)
                bw.call(lambda z=z, dy=dy, o=o: ops.ew(L.EW_HTANH_BWD, [z, dy], [o]), "lrp tail bwd")
                dz.append(o)
            # the stacks' inputs (hyperprior means, supports, rq_j) have no trainable producer in this schedule
            G.lower_stacks_backward(bw, lrp["tapes"], dz, lrp["packs"], grads, need_dx=False)

    def _grad_buffer(self) -> Dict[int, torch.Tensor]:
        """The backward plan's flat gradient buffer over ``train_params``: {id(param): its view}."""
        self.gflat, views, self.goffs = G.flat_grads(self.train_params, self.x_in.device)
        self.bwd.keep += [self.gflat, views]
        return {id(p): g for p, g in zip(self.train_params, views)}

    def _backward(self, grad: torch.Tensor, use_graph: bool) -> List[torch.Tensor]:
        """Run the backward plan for the incoming gradient (dL/dlikelihoods["y"] of the REM fine-tune, dL/dx_hat of
        refine_gs), capturing its graph at the first graph run; returns fresh tensors in ``train_params`` order."""
        with self.runner.on_stream():
            self._bwd_in(grad)
            self.bwd_runner.replay("backward", self.bwd.run, use_graph)
            flat = self.gflat.clone()
        return [flat[o:o + p.numel()].view(p.shape) for o, p in zip(self.goffs, self.train_params)]

    def _lower_prog_sequential(self, plan, heads, means_h, scales_h, hyper_done, supports, y_top, y_sub, yb, yp, ls_y,
                               table, symbols):
        """all_scalable = False (pic.py:586-587): the (mu, sigma) stacks of progressive slice j read the DECODED
        progressive slices j-sp..j-1, so mask, quantisation and LRP of a slice must finish before the next slice's
        stacks start — one slice at a time, on the caller's stream."""
        m, C, ns = self.m, self.m.dim_chunk, self.m.ns0
        B, h, w, d = self.B, self.H // 16, self.W // 16, self.m.division_dimension[0]
        sl = lambda v, i, n=1: v.window(i * C, n * C)
        mu_std = getattr(m, "mu_std", True)
        rem_idx = self.rem_idx
        plan.set_class("stack_heads")
        heads.update(_slice_stack_heads(plan, m, means_h, scales_h, "prog"))
        plan.set_class("slice_chain")
        self.mask = plan.buf(B, h, w, d)
        self.thr = None                                   # per-slice launches: thresholds are not collected
        rq = plan.buf(B, h, w, d)
        mu_f, std_f = self.mu_p, self.std_p
        if rem_idx is not None:
            self.ck = plan.buf(B, h, w, d)
            att = self.att = plan.buf(B, h, w, d)
            std_f = plan.buf(B, h, w, d)
            mu_f = plan.buf(B, h, w, d) if mu_std else self.mu_p
            self.rem_sig = _version_sig(m.post_latent[rem_idx])
        self.mu_f, self.std_f = mu_f, std_f
        for j in range(ns):
            ms, ss = supports(j)
            E.lower_stacks(plan, [m.cc_mean_transforms_prog[j], m.cc_scale_transforms_prog[j]], [ms, ss],
                           [sl(self.mu_p, j), sl(self.std_p, j)], heads=heads)
            if rem_idx is not None:                                                   # rem_pic.py:363-377
                plan.call(lambda j=j: self._vmask(sl(self.std_p, j), sl(att, j), 1))
                E.lower_rem_blocks(plan, [m.post_latent[rem_idx][j]], [sl(self.ck, j)], [[sl(self.mu_b, j), sl(self.std_b, j)]],
                                   [([sl(self.mu_p, j)] if mu_std else []) + [sl(self.std_p, j)]], [sl(att, j)],
                                   [([sl(mu_f, j)] if mu_std else []) + [sl(std_f, j)]])
            plan.call(lambda j=j: self._vmask(sl(std_f, j), sl(self.mask, j), 1))                                 # pic.py:621-622
            plan.call(lambda j=j: ops.gauss_tail(sl(y_top, j), sl(mu_f, j), sl(std_f, j), y2=sl(y_sub, j) if y_sub is not None else None,
                                                 mask=sl(self.mask, j), yhat=sl(rq, j), lik=sl(self.lik, ns + j), log2sum=ls_y,
                                                 sym=sl(self.sym, ns + j) if symbols else None))                  # pic.py:625-629
            if table is not None:
                plan.call(lambda j=j: ops.build_indexes(sl(std_f, j), table, mask=sl(self.mask, j), out=sl(self.idx, ns + j)))
            E.lower_stacks(plan, [m.lrp_transforms_prog[j]], [ms + [sl(rq, j)]], [sl(yp, j)],
                           [dict(act=L.ACT_HALF_TANH, post=sl(rq, j), post2=sl(yb, j))], heads=heads)              # pic.py:635-641

    def _vmask(self, sigma, mask, n_slice, thr=None):
        """The variance mask at this execute's quality: the scalar ``pr``, or (per_image plans) each image's own, read from
        the plan's device table — one level, the same segments, so the same bits per image."""
        if self.per_image:
            ops.variance_masks_per_image(sigma, self.qtable, mask, n_slice=n_slice, thr=thr)
        else:
            ops.variance_mask(sigma, self.pr, mask, n_slice=n_slice, thr=thr)

    # -------------------------------------------------------------------------------------------
    def close(self):
        """Give up the executable graphs of this plan (ops.Graph.close: destroyed at the next safe point)."""
        self.runner.close()
        self.bwd_runner.close()

    def set_noise(self, noise=None):
        """Training: U(-.5,.5) for the likelihood proxies; ``noise`` = {"y": NCHW, "z": NCHW} injects fixed draws
        (parity tests), otherwise torch's generator fills the buffers like the reference's ``uniform_``."""
        for key, v in (("y", self.noise_y), ("z", self.noise_z)):
            if noise is not None and key in noise:
                v.buf.copy_(noise[key].to(v.buf.device).permute(0, 2, 3, 1))
            else:
                v.buf.uniform_(-0.5, 0.5)

    def execute(self, x, pr, checkpoint_ref, use_graph, clone, noise=None, ck_pr=None):
        """Run the plan on its runner's stream, ordered after / before the caller's current stream."""
        self.pr = float(pr)
        self.generation += 1
        self.ck_pr = float(ck_pr) if ck_pr is not None else 0.0
        if self.bwd is not None and self.runner.stale(self.train_params):
            self.close()                               # parameter storage replaced: captured pointers are stale
        with self.runner.on_stream():
            self.x_in.copy_(x)
            if self.train:
                self.set_noise(noise)
            if checkpoint_ref is not None:
                ck = ops.from_nchw(checkpoint_ref.to(self.x_in.device))
                self.ck.buf.copy_(ck.buf[..., ck.c0:ck.c0 + ck.C])
            self.runner.replay((self.pr, self.ck_pr), self.plan.run, use_graph)
        return self._outputs(clone)

    def execute_per_image(self, x, prs: Sequence[float], use_graph, clone=True):
        """:meth:`execute` of a per_image plan with image b at mask quality ``prs[b]`` (> 0).  The table is refilled on the
        runner's stream before the replay, outside the capture; the qualities are inputs of the plan's ONE graph."""
        assert self.per_image and len(prs) == self.B
        self.generation += 1
        h, w = self.H // 16, self.W // 16
        table = ops.mask_table([[p_] for p_ in prs], h * w, self.m.dim_chunk)
        with self.runner.on_stream():
            self.x_in.copy_(x)
            self.qtable.copy_(torch.from_numpy(table))
            self.runner.replay(("per_image",), self.plan.run, use_graph)
        return self._outputs(clone)

    def _outputs(self, clone):
        fin = (lambda t: t.clone()) if clone else (lambda t: t)
        nchw = lambda v: fin(v.torch_nchw())
        out = {"x_hat": fin(self.x_hat),
               "likelihoods": {"y": nchw(self.lik), "z": nchw(self.z_lik)},
               "log2_likelihood_sum": fin(self.log2sum)}
        if self.base_only:
            yh = nchw(self.y_base)
            out.update({"y_hat": yh, "y_base": yh, "y_prog": yh, "mu": nchw(self.mu_b), "std": nchw(self.std_b),
                        "mu_base": nchw(self.mu_b), "std_base": nchw(self.std_b), "mu_prog": [], "std_prog": []})
        else:
            yh = nchw(self.y_prog)
            out.update({"y_hat": yh, "y_base": nchw(self.y_base), "y_prog": yh, "mu_base": nchw(self.mu_b),
                        "mu": nchw(self.mu_f), "std_base": nchw(self.std_b), "std": nchw(self.std_f),
                        "mask": nchw(self.mask)})
        return out


class _RateTail:
    """The rate-only tail of a _SweepPlan's front end for ``n_levels`` sorted distinct qualities > 0: one
    vam_variance_layers launch on the progressive sigma gives every element the first level whose mask holds it, one
    vam_gauss_layer_bits launch bins the in-mask log2 likelihoods by that level.  No masks, no replicated supports, no LRP
    stacks, no g_s.  ``acc`` [2, B, n_levels + 1]: the float64 sums and (as int64) the counts."""

    def __init__(self, fp, n_levels: int):
        m, parts = fp.m, fp.sweep_parts
        sg = parts["std"]
        assert 1 <= n_levels <= L.VAM_MAX_LAYER_LEVELS
        dev = sg.buf.device
        self.parts, self.ns, self.n_levels, self.B = parts, m.ns0, n_levels, sg.B
        self.prs = (0.0,) * n_levels
        self.outside = ops.log2_lik_outside(dev)         # log2 L(0, 0) (outside any capture: it synchronises)
        self.runner = E.Runner(dev, cap=32)              # one graph per tuple of qualities, replayed on the owner's stream
        self.layer = torch.empty((sg.B, sg.H, sg.W, sg.C), dtype=torch.uint8, device=dev)
        self.acc = torch.zeros((2, sg.B, n_levels + 1), dtype=torch.float64, device=dev)
        P = self.plan = E.Plan(dev)
        P.keep += [self.layer, self.acc]
        P.set_class("lrp_prog")
        P.call(lambda: ops.memset_zero(self.acc))
        P.call(lambda: self.launch(self.prs, self.acc), "layers + layer bits (rate)")

    def launch(self, prs: Sequence[float], acc: torch.Tensor, b: Optional[int] = None):
        """The two kernels for the whole sub-batch, or (``b``) for image b alone with its own qualities; ``acc`` cleared."""
        img = (lambda v: v) if b is None else (lambda v: ops.View(v.buf[b:b + 1], v.c0, v.C))
        pa = self.parts
        layer = self.layer if b is None else self.layer[b:b + 1]
        ops.variance_layers(img(pa["std"]), prs, layer, n_slice=self.ns)                      # pic.py:621-622, all levels
        ops.gauss_layer_bits(img(pa["y_top"]), img(pa["mu"]), img(pa["std"]), layer, len(prs), acc[0], acc[1].view(torch.int64),
                             y2=None if pa["y_sub"] is None else img(pa["y_sub"]))

    def level_sums(self, acc: torch.Tensor, n_levels: int) -> torch.Tensor:
        """[..., n_levels] progressive log2 sums from ``acc`` [2, ..., >= n_levels + 1]: level k holds the elements of layers
        <= k at their in-mask likelihood and every other element at log2 L(0, 0)."""
        bits, count = acc[0][..., :n_levels + 1], acc[1].view(torch.int64)[..., :n_levels + 1]
        n = count.sum(-1, keepdim=True)
        inside = count[..., :n_levels].cumsum(-1)
        return bits[..., :n_levels].cumsum(-1) + (n - inside).double() * self.outside

    def close(self):
        self.runner.close()


class _SizeTail:
    """The coded-size tail of a _SweepPlan's front end, beside _RateTail.  Once per front end
    (``front``): z (vam_coded_symbol_bits on the front end's z symbols) and the base slices (vam_coded_layer_bits with no
    layer ids) are priced per stream.  Per list of n sorted distinct qualities > 0 (``levels``): one zero-fill, one
    vam_variance_layers on the progressive sigma and one vam_coded_layer_bits, which bins the exact price of every
    element's (symbol, index) pair by (image, slice, layer).  No masks, no LRP stacks, no g_s, no coder.  The bins go to
    the host once; the stream lengths are host arithmetic (bitstream.stream_bytes)."""

    def __init__(self, fp):
        m, parts = fp.m, fp.sweep_parts
        sg = parts["std"]
        dev = sg.buf.device
        self.fp, self.m, self.parts, self.ns, self.B, self.dev = fp, m, parts, m.ns0, sg.B, dev
        self.C = m.dim_chunk
        self.n_y = self.C * sg.H * sg.W                              # symbols of one y stream
        self.n_z = m.N * fp.z_sym.buf.shape[1] * fp.z_sym.buf.shape[2]
        self.runner = E.Runner(dev, cap=32)              # ("front",) and one graph per tuple of qualities
        self.layer = torch.empty((sg.B, sg.H, sg.W, sg.C), dtype=torch.uint8, device=dev)
        # z: [B, 1, 2] sums and counts, then the base slices: [B, ns, 2] sums and counts, one buffer and one zero-fill
        B, ns = sg.B, self.ns
        self.acc0 = torch.zeros((4 * B + 4 * B * ns,), dtype=torch.float64, device=dev)
        a = self.acc0
        self.z_bits, self.z_cnt = a[:2 * B].view(B, 1, 2), a[2 * B:4 * B].view(torch.int64).view(B, 1, 2)
        self.b_bits = a[4 * B:4 * B + 2 * B * ns].view(B, ns, 2)
        self.b_cnt = a[4 * B + 2 * B * ns:].view(torch.int64).view(B, ns, 2)
        d = m.division_dimension[0]
        P = self.front_plan = E.Plan(dev)
        P.keep += [self.acc0, self.layer]
        P.set_class("lrp_prog")
        P.call(lambda: ops.memset_zero(self.acc0))
        P.call(lambda: ops.coded_symbol_bits(fp.z_sym, None, None, 1, self.te, m.N, self.z_bits, self.z_cnt), "z prices (size)")
        P.call(lambda: ops.coded_layer_bits(fp.y.window(0, d), fp.mu_b, fp.std_b, None, 1, self.table, self.tg, self.C,
                                            self.b_bits, self.b_cnt), "base prices (size)")
        self.tails: Dict[int, SimpleNamespace] = {}      # n_levels -> what make_tail returns
        self.tg = self.te = None
        self._base = None

    def refresh(self):
        """The coder's tables on the device (built on the host and copied: outside any capture).  Graphs captured with
        replaced tables are given up."""
        from . import bitstream as bs
        m = self.m
        tg = bs.DeviceTables.of(m.gaussian_conditional, self.dev)
        te = bs.DeviceTables.of(m.entropy_bottleneck, self.dev)
        if tg is not self.tg or te is not self.te:
            self.runner.close()
            self.tg, self.te = tg, te
            self.table = m.gaussian_conditional.scale_table.detach().to(self.dev, torch.float32).contiguous()
            self.c_out = float(tg.zero_cost[bs.sigma0_index(self.table)])      # compress: symbol 0 at build_indexes(0)
            self.c_out_layer = float(tg.zero_cost[0])                           # a container layer: symbol 0 in table 0

    def front(self, use_graph: bool):
        """Price z and the base slices of the front end that has just run (on the owner's stream)."""
        self.refresh()
        self.runner.replay(("front",), self.front_plan.run, use_graph)
        self._base = None

    def make_tail(self, n_levels: int) -> SimpleNamespace:
        """The tail of ``n_levels`` sorted distinct qualities > 0, shaped like a _RateTail (``prs``, ``plan``, ``runner``: this
        object's, one hipGraph per list); ``acc``: its bins [2, B, ns, n_levels + 1]."""
        assert 1 <= n_levels <= L.VAM_MAX_LAYER_LEVELS
        acc = torch.zeros((2, self.B, self.ns, n_levels + 1), dtype=torch.float64, device=self.dev)
        t = SimpleNamespace(prs=(0.0,) * n_levels, plan=E.Plan(self.dev), runner=self.runner, acc=acc)
        t.plan.keep += [acc]
        t.plan.set_class("lrp_prog")
        t.plan.call(lambda: ops.memset_zero(acc))
        t.plan.call(lambda: self.launch(t.prs, acc), "layers + coded layer bits (size)")
        return t

    def launch(self, prs, acc: torch.Tensor, per_image: bool = False):
        """The two kernels for the whole sub-batch: one quality list for all images, or (``per_image``) one per image;
        ``acc`` [2, B, ns, n + 1] cleared."""
        pa = self.parts
        if per_image:
            ops.variance_layers_per_image(pa["std"], prs, self.layer, n_slice=self.ns)
        else:
            ops.variance_layers(pa["std"], prs, self.layer, n_slice=self.ns)                  # pic.py:621-622, all levels
        ops.coded_layer_bits(pa["y_top"], pa["mu"], pa["std"], self.layer, acc.shape[-1] - 1, self.table, self.tg, self.C,
                             acc[0], acc[1].view(torch.int64), y2=pa["y_sub"])

    # ---- host arithmetic on the bins
    def base_sizes(self):
        """(bytes_lo, bytes_hi, bits), each [B]: z and the base slices, the strings of compress(x, 0).  Synchronises."""
        from . import bitstream as bs
        if self._base is None:
            a = self.acc0.cpu()
            B, ns = self.B, self.ns
            zb = a[:2 * B].view(B, 1, 2).numpy()[:, :, 0]
            bb = a[4 * B:4 * B + 2 * B * ns].view(B, ns, 2).numpy()[:, :, 0]
            zl, zh = bs.stream_bytes(zb, self.n_z)
            bl, bh = bs.stream_bytes(bb, self.n_y)
            self._base = (zl.sum(1) + bl.sum(1), zh.sum(1) + bh.sum(1), zb.sum(1) + bb.sum(1))
            self._parts = ((zl.sum(1), zh.sum(1)), (bl.sum(1), bh.sum(1)))
        return self._base

    def stream_bits(self, acc: np.ndarray, n_levels, c_out: float, cumulative: bool = True) -> np.ndarray:
        """[..., ns, n_levels] table cost of each progressive stream from host bins ``acc`` [2 (sums, counts as float64
        bit patterns), ..., ns, >= n_levels + 1].  ``cumulative``: compress at level k, the elements of layers <= k at their
        price and every other element at ``c_out``; else container layer k alone."""
        bits, count = acc[0][..., :n_levels], acc[1].view(np.int64)[..., :n_levels]
        if cumulative:
            bits, count = np.cumsum(bits, -1), np.cumsum(count, -1)
        return bits + (self.n_y - count).astype(np.float64) * c_out

    def level_sizes(self, accs: Sequence[torch.Tensor], ns_levels: Sequence[int]):
        """(bytes_lo, bytes_hi, bits), each [B, total levels]: the progressive strings of compress at every level of the
        groups' bins (what _SweepPlan.size returned).  One host synchronisation."""
        from . import bitstream as bs
        lo, hi, bits = [], [], []
        for acc, n in zip([a.cpu().numpy() for a in accs], ns_levels):
            S = self.stream_bits(acc, n, self.c_out)                    # [B, ns, n]
            l, h = bs.stream_bytes(S, self.n_y)
            lo.append(l.sum(1)); hi.append(h.sum(1)); bits.append(S.sum(1))
        if not lo:
            z = np.zeros((self.B, 0))
            return z.astype(np.int64), z.astype(np.int64), z
        return np.concatenate(lo, 1), np.concatenate(hi, 1), np.concatenate(bits, 1)

    def close(self):
        self.runner.close()


class _SweepTail:
    """The per-level part of a rate sweep for ``n_levels`` qualities over the shared buffers of a _SweepPlan's front end
    (pic.py:621-651 once per level), run as n_levels * B images: level k is images k*B .. (k+1)*B-1 of every buffer here.
    The masks are one vam_variance_mask_levels launch, quantisation and likelihood one vam_gauss_levels_eval launch; the
    ten LRP stacks and g_s[1] run once over the level batch.  The stacks' shared inputs — the stack heads (bias + the
    hyperprior part of the first layer, computed once at B images: the eval plan's association of that sum), y_hat_base
    and mu_total — are replicated per level.

    ``decode``: the quantised latents come from decoded symbols instead (_ProgDecPlan): one vam_gauss_levels_decode launch
    over the plan's symbols and container layer ids, with the container-layer cut-offs ``ks`` in place of the qualities
    (level g keeps the elements of layers <= ks[g]); no masks and no likelihoods.  The rest of the tail is the same."""

    def __init__(self, fp, n_levels: int, decode: bool = False, per_image: bool = False):
        """``per_image``: level g of image b is masked at that image's own quality, read from ``qtable`` (which
        _SweepPlan.tail_per_image refills before each replay); the rest of the tail is the same."""
        assert not (decode and per_image)
        m, parts = fp.m, fp.sweep_parts
        yb0 = parts["yb"]
        B, h, w = yb0.B, yb0.H, yb0.W
        H, W = 16 * h, 16 * w
        assert 1 <= n_levels <= L.VAM_MAX_MASK_LEVELS
        NL, LB = n_levels, n_levels * B
        d, ns, C = m.division_dimension[0], m.ns0, m.dim_chunk
        dev = yb0.buf.device
        self.n_levels, self.B = NL, B
        self.prs = (0.0,) * NL            # eval: the mask qualities of the levels
        self.ks = (0,) * NL               # decode: the container-layer cut-offs of the levels
        self.runner = E.Runner(dev, cap=32)     # one graph per tuple of levels, replayed on the owner's stream
        self.qtable = _mask_table_buffer(B, dev) if per_image else None
        P = self.plan = E.Plan(dev)
        P.keep.append(self.qtable)
        sl = lambda v, i, n=1: v.window(i * C, n * C)
        self.log2sum = torch.zeros((NL, B), dtype=torch.float64, device=dev)      # level k's progressive log2 sums per image
        self.x_hat = torch.empty((LB, 3, H, W), dtype=torch.float32, device=dev)
        P.keep += [self.log2sum, self.x_hat]
        self.rq, self.y_prog = P.buf(LB, h, w, d), P.buf(LB, h, w, d)
        self.mask = self.lik = None
        stacks = [m.lrp_transforms_prog[j] for j in range(ns)]
        heads = parts["heads"]
        reps = [(heads[id(st)][0], P.buf(LB, h, w, heads[id(st)][0].C)) for st in stacks]
        reps += [(parts["yb"], P.buf(LB, h, w, d)), (parts["mu_tot"], P.buf(LB, h, w, d))]

        def replicate():
            for src, dst in reps:
                dst.buf.view(NL, B, h, w, dst.ld).copy_(src.buf[..., src.c0:src.c0 + src.C].unsqueeze(0))
        P.set_class("lrp_prog")
        if decode:                                  # functions_decode.py:186-207: the decoded layers <= k, + mu
            P.call(lambda: ops.gauss_levels_decode(parts["sym"], parts["layer"], parts["mu"], self.ks, self.rq),
                   "dequantise levels (decode)")
        else:
            self.mask, self.lik = P.buf(LB, h, w, d), P.buf(LB, h, w, d)
            P.call(lambda: ops.memset_zero(self.log2sum))
            if per_image:
                P.call(lambda: ops.variance_masks_per_image(parts["std"], self.qtable, self.mask, n_slice=ns),
                       "variance masks per image (sweep)")
            else:
                P.call(lambda: ops.variance_mask_levels(parts["std"], self.prs, self.mask, n_slice=ns), "variance masks (sweep)")   # :621-622
            P.call(lambda: ops.gauss_levels_eval(parts["y_top"], parts["mu"], parts["std"], self.mask, NL, y2=parts["y_sub"],
                                                 yhat=self.rq, lik=self.lik, log2sum=self.log2sum), "quantise + likelihood (sweep)")   # :625-629
        P.call(replicate, "supports per level")
        heads_l = {id(st): (dst, False) for st, (_, dst) in zip(stacks, reps)}
        yb_l, mt_l = reps[ns][1], reps[ns + 1][1]
        sp = m.support_progressive_slices
        ins = []
        for j in range(ns):
            s_ = min(sp, j)
            ins.append([sl(yb_l, j)] + ([sl(mt_l, j - s_, s_)] if s_ else []) + [sl(self.rq, j)])
        E.lower_stacks(P, stacks, ins, [sl(self.y_prog, j) for j in range(ns)],
                       [dict(act=L.ACT_HALF_TANH, post=sl(self.rq, j), post2=sl(yb_l, j)) for j in range(ns)], heads=heads_l)   # :635-641
        P.set_class("g_s")
        E.lower_g_s(P, [parts["g_s"]], [self.y_prog], [self.x_hat])

    def level(self, v: ops.View, k: int) -> ops.View:
        return ops.View(v.buf[k * self.B:(k + 1) * self.B], v.c0, v.C)

    def close(self):
        self.runner.close()


class _SweepPlan:
    """``forward_qualities`` for one (B, H, W) (all_scalable, fp32 storage): the quality-independent
    front end (g_a, hyperprior, base slices, progressive (mu, sigma) chain, stack heads — an _FsqPlan in sweep mode) runs
    once, g_s[0] on y_hat_base only when 0 is asked for, and the per-level tail once per group of levels (_SweepTail,
    one plan per group size, one hipGraph per tuple of mask qualities)."""

    def __init__(self, m: VarianceMaskingPIC, B, H, W, device):
        self.m, self.B, self.H, self.W = m, B, H, W
        self.fp = _FsqPlan(m, B, H, W, False, None, device, sweep=True)
        self.p_base = E.Plan(device)
        self.p_base.set_class("g_s")
        E.lower_g_s(self.p_base, [m.g_s[0] if m.multiple_decoder else m.g_s], [self.fp.y_base], [self.fp.x_hat])
        self.tails: Dict[int, _SweepTail] = {}
        self.pi_tails: Dict[int, _SweepTail] = {}        # per-image qualities: one plan AND one graph per group size
        self.rate_tails: Dict[int, _RateTail] = {}
        self.size_tail: Optional[_SizeTail] = None
        self.runner = E.Runner(device, cap=32)           # ("front",) and ("base",); the tails run on its stream

    def front(self, x, use_graph: bool):
        with self.runner.on_stream():
            self.fp.x_in.copy_(x)
            self.runner.replay(("front",), self.fp.plan.run, use_graph)

    def base(self, use_graph: bool):
        with self.runner.on_stream():
            self.runner.replay(("base",), self.p_base.run, use_graph)

    def _tail(self, tails: dict, n: int, make, prs: Optional[Sequence[float]] = None, use_graph: bool = False):
        """The tail of ``n`` levels kept in ``tails`` (``make(n)`` at first use); with ``prs`` set to those qualities and
        replayed on the plan's stream: one plan per list length, one hipGraph per list."""
        t = tails.get(n)
        if t is None:
            t = tails[n] = make(n)
        if prs is not None:
            t.prs = tuple(float(p_) for p_ in prs)
            with self.runner.on_stream():
                t.runner.replay(t.prs, t.plan.run, use_graph)
        return t

    def tail(self, prs: Sequence[float], use_graph: bool) -> _SweepTail:
        return self._tail(self.tails, len(prs), lambda n: _SweepTail(self.fp, n), prs, use_graph)

    def tail_per_image(self, Q_group: Sequence[Sequence[float]], use_graph: bool) -> _SweepTail:
        """:meth:`tail` with level g of image b at mask quality ``Q_group[g][b]``."""
        n = len(Q_group)
        assert all(len(row) == self.B for row in Q_group)
        t = self._tail(self.pi_tails, n, lambda n_: _SweepTail(self.fp, n_, per_image=True))
        sg = self.fp.sweep_parts["std"]
        table = ops.mask_table([[float(Q_group[g][b]) for g in range(n)] for b in range(self.B)], sg.H * sg.W, self.m.dim_chunk)
        with self.runner.on_stream():
            t.qtable.copy_(torch.from_numpy(table))
            t.runner.replay(("per_image",), t.plan.run, use_graph)
        return t

    def rate_tail(self, n_levels: int, prs: Optional[Sequence[float]] = None, use_graph: bool = False) -> _RateTail:
        return self._tail(self.rate_tails, n_levels, lambda n: _RateTail(self.fp, n), prs, use_graph)

    def rate(self, prs: Sequence[float], use_graph: bool) -> torch.Tensor:
        """[B, len(prs)] float64: the progressive log2 sums at the sorted distinct qualities ``prs`` (> 0)."""
        t = self.rate_tail(len(prs), prs, use_graph)
        return t.level_sums(t.acc, len(prs))

    # ---- coded sizes
    def size_front(self, use_graph: bool) -> _SizeTail:
        """Price z and the base slices of the front end that has just run; the plan's size tail."""
        if self.size_tail is None:
            self.size_tail = _SizeTail(self.fp)
        with self.runner.on_stream():
            self.size_tail.front(use_graph)
        return self.size_tail

    def size(self, prs: Sequence[float], use_graph: bool) -> torch.Tensor:
        """The bins [2, B, ns, len(prs) + 1] of the sorted distinct qualities ``prs`` (> 0) (after :meth:`size_front`)."""
        return self._tail(self.size_tail.tails, len(prs), self.size_tail.make_tail, prs, use_graph).acc.clone()

    def size_eager(self, prs: Sequence[float]) -> np.ndarray:
        """Host bins [2, B, ns, len(prs) + 1] of a non-decreasing list that is asked for once (no graph); synchronises."""
        st = self.size_tail
        acc = torch.zeros((2, self.B, st.ns, len(prs) + 1), dtype=torch.float64, device=st.dev)
        with self.runner.on_stream():
            st.launch([float(p_) for p_ in prs], acc)
        return acc.cpu().numpy()

    def close(self):
        self.fp.close()
        self.runner.close()
        for t in list(self.tails.values()) + list(self.pi_tails.values()) + list(self.rate_tails.values()) + \
                ([self.size_tail] if self.size_tail else []):
            t.close()


class _DecPlan:
    """``decompress`` for one (B, z-shape): the same kernels as the encoder's plan, cut where the
    host rANS decoder has to deliver the symbols of a slice (models/pic.py:862-960).  The conv
    kernel's K order is canonical, so mu / sigma / masks / indexes are bit-identical to the
    encoder's although the launches are grouped differently."""

    def __init__(self, m: VarianceMaskingPIC, B, hz, wz, base_only, rem_idx, device, prog_chain: bool = False,
                 per_image: bool = False):
        """``prog_chain``: stop after the base slices (hyper-synthesis of both halves and every stack head included) and
        keep g_s[0] on y_hat_base in ``p_syn``; _ProgDecPlan lowers the progressive part itself.  ``per_image``: the
        per-slice masks read each image's quality from ``qtable`` (decode_per_image refills it)."""
        assert not per_image or not (base_only or prog_chain or rem_idx is not None)
        self.m, self.B, self.base_only, self.rem_idx = m, B, base_only, rem_idx
        self.per_image = per_image
        self.qtable = _mask_table_buffer(B, device) if per_image else None
        self.rem_sig = _version_sig(m.post_latent[rem_idx]) if rem_idx is not None else None
        self.device = torch.device(device)
        self.pr = 0.0
        self.runner = E.Runner(device, cap=32)           # stream ordering; _ProgDecPlan's ("base",) graph
        h, w = hz * 4, wz * 4
        self.h, self.w, self.hz, self.wz = h, w, hz, wz
        d, C, ns = m.division_dimension[0], m.dim_chunk, m.ns0
        f32 = dict(dtype=torch.float32, device=device)
        table = m.gaussian_conditional.scale_table
        if table.numel() == 0:
            raise ValueError("empty scale table: call model.update() before decompress()")
        nv, ni = (lambda c, hh=h, ww=w: ops.new_view(B, hh, ww, c, device)), (lambda c, hh=h, ww=w: ops.new_iview(B, hh, ww, c, device))
        sl = lambda v, i, n=1: v.window(i * C, n * C)
        self.x_hat = torch.empty((B, 3, h * 16, w * 16), **f32)
        # ---- z
        self.z_sym = ni(m.N, hz, wz)
        med = nv(m.N, hz, wz)
        med.buf.copy_(m.entropy_bottleneck._get_medians().detach().reshape(1, 1, 1, -1).expand_as(med.buf))
        z_hat = nv(m.N, hz, wz)
        P = self.p_hyper = E.Plan(device)
        P.call(lambda: ops.dequantize(self.z_sym, med, z_hat))                       # entropy_models.py:520-525
        means_h, scales_h = _lower_hyper_synthesis(P, m, z_hat, base_only)
        heads = _slice_stack_heads(P, m, means_h, scales_h, "base")                 # same association as the encoder's plan
        if not base_only:
            heads.update(_slice_stack_heads(P, m, means_h, scales_h, "prog"))
        # ---- base slices
        yq, yb, mu_b, std_b = nv(d), nv(d), nv(d), nv(d)
        self.idx_b, self.sym_b = ni(d), ni(d)
        self.mu_b, self.std_b = mu_b, std_b
        self.p_base = []
        for i in range(ns):
            sup = [sl(yb, 0, min(m.max_support_slices, i))] if i > 0 else []
            Pa, Pb = E.Plan(device), E.Plan(device)
            E.lower_stacks(Pa, [m.cc_mean_transforms[i], m.cc_scale_transforms[i]], [sup, sup],
                           [sl(mu_b, i), sl(std_b, i)], heads=heads)
            Pa.call(lambda i=i: ops.build_indexes(sl(std_b, i), table, out=sl(self.idx_b, i)))          # pic.py:879
            Pb.call(lambda i=i: ops.dequantize(sl(self.sym_b, i), sl(mu_b, i), sl(yq, i)))               # pic.py:884
            E.lower_stacks(Pb, [m.lrp_transforms[i]], [sup + [sl(yq, i)]], [sl(yb, i)],
                           [dict(act=L.ACT_HALF_TANH, post=sl(yq, i))], heads=heads)
            self.p_base.append((Pa, Pb))
        self.p_syn = E.Plan(device)
        self.heads, self.yb = heads, yb
        if base_only or prog_chain:
            E.lower_g_s(self.p_syn, [m.g_s[0] if m.multiple_decoder else m.g_s], [yb], [self.x_hat])
            return
        # ---- progressive slices
        mu_p, std_p, mask, rq, yp = nv(d), nv(d), nv(d), nv(d), nv(d)
        mu_tot = nv(d) if m.total_mu_rep else mu_p                                    # pic.py:601
        mu_std = getattr(m, "mu_std", True)
        std_f = nv(d) if rem_idx is not None else std_p
        mu_f = nv(d) if (rem_idx is not None and mu_std) else mu_p
        self.ck = nv(d) if rem_idx is not None else None
        att = nv(d) if rem_idx is not None else None
        self.idx_p, self.sym_p = ni(d), ni(d)
        sp = m.support_progressive_slices
        self.p_prog = []
        for j in range(ns):
            s_ = min(sp, j)
            sm, ss_v = (mu_tot, std_p) if m.all_scalable else (yp, yp)                # pic.py:586-587
            ms = [sl(yb, j)] + ([sl(sm, j - s_, s_)] if s_ else [])
            ss = [sl(yb, j)] + ([sl(ss_v, j - s_, s_)] if s_ else [])
            Pa, Pb = E.Plan(device), E.Plan(device)
            E.lower_stacks(Pa, [m.cc_mean_transforms_prog[j], m.cc_scale_transforms_prog[j]], [ms, ss], [sl(mu_p, j), sl(std_p, j)],
                           heads=heads)
            if m.total_mu_rep:
                Pa.call(lambda j=j: ops.add(sl(mu_p, j), sl(yb, j), sl(mu_tot, j)))
            if rem_idx is not None:
                Pa.call(lambda j=j: self._vmask(sl(std_p, j), sl(att, j)))
                E.lower_rem_blocks(Pa, [m.post_latent[rem_idx][j]], [sl(self.ck, j)], [[sl(mu_b, j), sl(std_b, j)]],
                                   [([sl(mu_p, j)] if mu_std else []) + [sl(std_p, j)]], [sl(att, j)],
                                   [([sl(mu_f, j)] if mu_std else []) + [sl(std_f, j)]])
            Pa.call(lambda j=j: self._vmask(sl(std_f, j), sl(mask, j)))                                 # pic.py:942
            Pa.call(lambda j=j: ops.build_indexes(sl(std_f, j), table, mask=sl(mask, j), out=sl(self.idx_p, j)))  # :945
            Pb.call(lambda j=j: ops.dequantize(sl(self.sym_p, j), sl(mu_f, j), sl(rq, j)))               # :948
            E.lower_stacks(Pb, [m.lrp_transforms_prog[j]], [ms + [sl(rq, j)]], [sl(yp, j)],
                           [dict(act=L.ACT_HALF_TANH, post=sl(rq, j), post2=sl(yb, j))], heads=heads)
            self.p_prog.append((Pa, Pb))
        E.lower_g_s(self.p_syn, [m.g_s[1] if m.multiple_decoder else m.g_s], [yp], [self.x_hat])

    def _vmask(self, sigma, mask):
        """One slice's mask at this decode's quality: the scalar ``pr``, or (per_image) each image's own from the table."""
        if self.per_image:
            ops.variance_masks_per_image(sigma, self.qtable, mask, n_slice=1)
        else:
            ops.variance_mask(sigma, self.pr, mask, n_slice=1)

    def _decode_slice(self, strings, idx_view: ops.IView, sym_view: ops.IView, tables, C):
        """indexes GPU -> host, rANS decode per image, symbols host -> GPU (NHWC window)."""
        from . import bitstream as bs
        B, h, w = self.B, idx_view.buf.shape[1], idx_view.buf.shape[2]
        self.runner.stream.synchronize()
        idx = idx_view.buf[..., idx_view.c0:idx_view.c0 + C].cpu().numpy()          # [B,h,w,C]
        out = np.empty((B, h, w, C), dtype=np.int32)
        for b in range(B):
            dec = bs.decode(strings[b], idx[b].transpose(2, 0, 1), tables)           # stream order [C,h,w]
            out[b] = dec.reshape(C, h, w).transpose(1, 2, 0)
        sym_view.buf[..., sym_view.c0:sym_view.c0 + C].copy_(torch.from_numpy(out).to(self.device))

    def _decode_base(self, y_strings, z_strings, tg, te):
        """z (host decode) -> hyper-synthesis -> base slices, each slice's symbols decoded on the host; on the runner's
        stream."""
        from . import bitstream as bs
        m, C = self.m, self.m.dim_chunk
        zi = np.broadcast_to(np.arange(m.N, dtype=np.int32)[:, None, None], (m.N, self.hz, self.wz))
        zs = np.stack([bs.decode(z_strings[b], zi, te).reshape(m.N, self.hz, self.wz).transpose(1, 2, 0)
                       for b in range(self.B)])
        self.z_sym.buf.copy_(torch.from_numpy(zs).to(self.device))
        self.p_hyper.run()
        for i, (Pa, Pb) in enumerate(self.p_base):
            Pa.run()
            self._decode_slice(y_strings[i], self.idx_b.window(i * C, C), self.sym_b.window(i * C, C), tg, C)
            Pb.run()

    def decode(self, strings, pr, checkpoint_rep):
        """``pr``: the mask quality, or (per_image plans) one per image."""
        from . import bitstream as bs
        m = self.m
        if self.per_image:
            assert len(pr) == self.B
            table = ops.mask_table([[float(p_)] for p_ in pr], self.h * self.w, m.dim_chunk)
            with self.runner.on_stream():
                self.qtable.copy_(torch.from_numpy(table))
        else:
            self.pr = float(pr)
        y_strings, z_strings = strings[0], strings[1]
        n_need = m.ns0 if self.base_only else m.ns1
        if len(y_strings) < n_need or len(z_strings) != self.B:
            raise ValueError(f"expected {n_need} slice streams x {self.B} images, got {len(y_strings)} x {len(z_strings)}")
        tg, te = bs.Tables.of(m.gaussian_conditional), bs.Tables.of(m.entropy_bottleneck)
        C = m.dim_chunk
        with self.runner.on_stream():
            if checkpoint_rep is not None:
                ck = ops.from_nchw(checkpoint_rep.to(self.device))
                self.ck.buf.copy_(ck.buf[..., ck.c0:ck.c0 + ck.C])
            self._decode_base(y_strings, z_strings, tg, te)
            if not self.base_only:
                for j, (Pa, Pb) in enumerate(self.p_prog):
                    Pa.run()
                    self._decode_slice(y_strings[m.ns0 + j], self.idx_p.window(j * C, C), self.sym_p.window(j * C, C), tg, C)
                    Pb.run()
            self.p_syn.run()
        return self.x_hat.clone()

    def close(self):
        self.runner.close()


class _ProgDecPlan(_DecPlan):
    """progressive.ProgressiveDecoder for one (B, z-shape, quality list) (all_scalable): _DecPlan's z,
    hyper-synthesis and base slices with their host round trips, then the progressive (mu, sigma) chain with no mask and
    no host round trip — with all_scalable it reads only y_hat_base and its own history (pic.py:586-612) —, the container
    layer id of every element (vam_variance_layers on the chain's sigma) and the unmasked table indexes
    (src/test/utils.py:35-54, functions_decode.py:186-203).  ``sweep_parts`` feeds _SweepTail in decode mode: level g is
    the decoded symbols of the layers <= ks[g], + mu, then the LRP stacks and g_s[1]; ``p_syn`` is level 0 (g_s[0])."""

    def __init__(self, m: VarianceMaskingPIC, B, hz, wz, q_list, device):
        super().__init__(m, B, hz, wz, False, None, device, prog_chain=True)
        h, w, d, C, ns = self.h, self.w, m.division_dimension[0], m.dim_chunk, m.ns0
        sl = lambda v, i, n=1: v.window(i * C, n * C)
        self.q_list = tuple(float(q) for q in q_list)
        nv = lambda: ops.new_view(B, h, w, d, device)
        mu_p, std_p = nv(), nv()
        mu_tot = nv() if m.total_mu_rep else mu_p                                    # pic.py:601
        yb, heads, sp = self.yb, self.heads, m.support_progressive_slices
        P = self.p_chain = E.Plan(device)
        for j in range(ns):                                                           # pic.py:586-612 with all_scalable
            s_ = min(sp, j)
            ms = [sl(yb, j)] + ([sl(mu_tot, j - s_, s_)] if s_ else [])
            ss = [sl(yb, j)] + ([sl(std_p, j - s_, s_)] if s_ else [])
            E.lower_stacks(P, [m.cc_mean_transforms_prog[j], m.cc_scale_transforms_prog[j]], [ms, ss], [sl(mu_p, j), sl(std_p, j)],
                           heads=heads)
            if m.total_mu_rep:
                P.call(lambda j=j: ops.add(sl(mu_p, j), sl(yb, j), sl(mu_tot, j)))
        self.layer = torch.empty((B, h, w, d), dtype=torch.uint8, device=device)
        self.idx_l, self.sym = ops.new_iview(B, h, w, d, device), ops.new_iview(B, h, w, d, device)
        P.keep += [mu_p.buf, std_p.buf, mu_tot.buf, self.layer, self.idx_l.buf, self.sym.buf]
        table = m.gaussian_conditional.scale_table
        P.call(lambda: ops.variance_layers(std_p, self.q_list, self.layer, n_slice=ns), "container layers")
        P.call(lambda: ops.build_indexes(std_p, table, out=self.idx_l))                # functions_decode.py:179-180
        self.sweep_parts = dict(heads=heads, yb=yb, mu=mu_p, std=std_p, mu_tot=mu_tot, sym=self.sym, layer=self.layer,
                                g_s=m.g_s[1] if m.multiple_decoder else m.g_s)
        self.tails: Dict[int, _SweepTail] = {}
        self.owner = None                   # the ProgressiveDecoder whose base and chain the buffers hold

    def front(self, y_strings, z_strings):
        """Base slices (host round trips) and the progressive chain, layer ids and indexes of every image."""
        from . import bitstream as bs
        tg, te = bs.Tables.of(self.m.gaussian_conditional), bs.Tables.of(self.m.entropy_bottleneck)
        with self.runner.on_stream():
            self._decode_base(y_strings, z_strings, tg, te)
            self.p_chain.run()

    def base(self, use_graph: bool):
        with self.runner.on_stream():
            self.runner.replay(("base",), self.p_syn.run, use_graph)

    def tail(self, ks: Sequence[int], use_graph: bool) -> _SweepTail:
        t = self.tails.get(len(ks))
        if t is None:
            t = self.tails[len(ks)] = _SweepTail(self, len(ks), decode=True)
        t.ks = tuple(int(k) for k in ks)
        with self.runner.on_stream():
            t.runner.replay(t.ks, t.plan.run, use_graph)
        return t

    def close(self):
        super().close()
        for t in self.tails.values():
            t.close()


models = {"pic": VarianceMaskingPIC, "rem": VarianceMaskingPICREM}


def get_model(args, device):
    """models/__init__.py:11-55 (``cnn`` = the legacy WACNN baseline, out of scope: SURVEY §2 #11)."""
    common = dict(N=args.N, M=args.M, multiple_decoder=args.multiple_decoder, multiple_encoder=args.multiple_encoder,
                  multiple_hyperprior=args.multiple_hyperprior, dim_chunk=args.dim_chunk,
                  division_dimension=args.division_dimension, mask_policy=args.mask_policy,
                  support_progressive_slices=args.support_progressive_slices, delta_encode=args.delta_encode,
                  total_mu_rep=args.total_mu_rep, all_scalable=args.all_scalable)
    if args.model == "pic":
        net = VarianceMaskingPIC(**common)
    elif args.model == "rem":
        net = VarianceMaskingPICREM(**common, check_levels=args.check_levels, mu_std=args.mu_std,
                                    dimension=args.dimension)
    else:
        raise NotImplementedError
    return net.to(device)


from . import control                                                                                   # noqa: E402
from .control import RATE_GRID, rate_search, rate_search_grid, rate_search_passes, rate_search_step, sweep_groups   # noqa: E402,F401
