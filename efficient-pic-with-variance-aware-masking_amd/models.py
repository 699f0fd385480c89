"""Host-side mirror of the reference's model classes (``src/models/*.py``).

``get_model(args, device)``, ``models``, ``VarianceMaskingPIC`` and
``VarianceMaskingPICREM`` keep the reference's constructor arguments, attribute names,
sub-module tree and ``state_dict`` keys (so ``src/demo.py`` / ``src/train.py`` style
callers and reference checkpoints map onto them), while ``forward_single_quality`` is
lowered once per input shape into a :class:`engine.Plan` of libvampic launches
(optionally replayed as one hipGraph).  The plans are ``plans.py``'s; their caches are here.

Reference: models/__init__.py:5-55, models/base.py:6-70, models/builder.py:4-136,
models/pic.py:25-666, models/rem_pic.py:8-422.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import layers as Ly
from . import ops
from .entropy_models import EntropyBottleneck, GaussianConditional, get_scale_table
from .plans import _DecPlan, _EmbDecPlan, _FsqPlan, _FsqTrainFn, _FullTrainFn, _ProgDecPlan, _SweepPlan, _version_sig


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
        # "host" (default): the rANS coder of csrc/rans.cpp; "device": the same wire format coded and decoded by the kernels
        # of csrc/rans_device.hip.  Read at each compress / decompress call.
        self.coder = "host"
        # Lanes per stream of compress / decompress and their per-image and quality-map siblings, on both coders (DESIGN
        # section 9o): a power of two in 1 .. 64, read at each call.  1 (default) is the wire format of rans.cpp; K > 1 splits
        # every y and z stream into K independent lanes behind a header of K lengths, about 12 K bytes more per stream.  The
        # value is NOT stored in the strings: the decoder must be set to the encoder's, like the quality and the shape.
        self.coder_lanes = 1

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
              per_image: bool = False, quality_map: bool = False) -> "_FsqPlan":
        B, H, W = _check_input(x)
        key = (B, H, W, base_only, rem_idx, str(x.device)) + ((True,) if symbols else ()) + (("train",) if train else ()) + \
            (("own_ck",) if own_ck else ()) + (("train_gs",) if train_gs else ()) + (("train_lrp",) if train_lrp else ()) + \
            (("bf16",) if getattr(self, "storage", "fp32") == "bf16" else ()) + (("per_image",) if per_image else ()) + \
            (("quality_map",) if quality_map else ())
        if getattr(self, "storage", "fp32") == "bf16" and (train or symbols):
            raise NotImplementedError("bf16 storage is an inference configuration (forward_single_quality): training and "
                                      "the bitstream path run in fp32")
        if ops.f16x2_mode() and (train or symbols):
            raise NotImplementedError(F16X2_REFUSAL)
        # training plans re-pack what they train every step: wsig leaves those modules out, a training REM plan its REM
        trained = ([self._decoder_in_use(base_only)] if train_gs else []) + ([self.lrp_transforms_prog] if train_lrp else [])
        return self._cached_plan(self._plans, key,
                                 lambda: _FsqPlan(self, B, H, W, base_only, rem_idx, x.device, symbols=symbols, train=train,
                                                  own_ck=own_ck, train_gs=train_gs, train_lrp=train_lrp, per_image=per_image,
                                                  quality_map=quality_map),
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

    # ---- sweep, per-image qualities, rate and coded-size control, quality maps (DESIGN sections 9f, 9h-9k): the drivers are control.py's
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
        self._refuse_lanes_for_sizes("compress_to_bytes")
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
        self._refuse_lanes_for_sizes("coded_size_curve")
        return control.coded_size_curve(self, x, qualities, mask_pol)

    def qualities_for_bytes(self, x, target_bytes, q_tol=1e-3, mask_pol=None):
        """The largest quality whose coded size fits a byte budget, per image: ``target_bytes`` a number, T numbers or a
        [T, B] tensor.  Returns {"quality": float64 [T, B], "bytes": float64 [T, B] (bytes_hi of coded_size_curve at that
        quality), "reached": bool [T, B]} on the host, with, per image b and target t: the strings of the real
        compress(x[b:b+1], q*) weigh <= t;  q* = 10 or bytes_hi(min(10, q* + q_tol)) > t (for a bytes_hi that does not
        decrease in q);  q* = 0 with reached = False when even the base exceeds t.  :func:`rate_search` over bytes_hi:
        one front end per sub-batch; the first pass is the batched size tail, every later pass one
        vam_variance_layers_per_image and one vam_coded_layer_bits launch for the sub-batch and one synchronisation."""
        self._refuse_lanes_for_sizes("qualities_for_bytes")
        return control.solve(self, x, target_bytes, q_tol, mask_pol, control.BYTES)

    # ---- quality maps: region-of-interest coding
    def forward_quality_map(self, x, qmap, mask_pol=None):
        """``forward_single_quality(..., training=False)``'s dict for a quality that varies INSIDE the images: ``qmap``
        [B, H/16, W/16] (the latent grid; :func:`evaluate.latent_quality_map` makes one from a pixel map), entries >= 0, at
        most VAM_MAX_LAYER_LEVELS distinct values per image.  For every slice j, latent position p and channel c the mask is
        the one ``forward_single_quality(x[b:b+1], qmap[b, p])`` computes there, bit for bit; with all_scalable so are
        ``likelihoods["y"]``, ``mu`` and ``std`` (they do not depend on the other positions' qualities), while ``y_hat`` and
        ``x_hat`` mix the positions through the LRP stacks and g_s.  A 0 masks that position out of the progressive half; it
        does NOT select the base plan, even for a map that is 0 everywhere: g_s[1] still reconstructs.  ``two-levels`` maps
        every non-zero entry to 10.  One plan run per sub-batch of one plan's worth; table and map are graph inputs, so a
        plan keeps ONE hipGraph whatever the maps.  Refused (NotImplementedError): REM models (a REM and its checkpoint
        belong to one quality), bf16 storage and VAMPIC_CONV=f16x2 (:meth:`_batch_shareable`)."""
        return control.forward_quality_map(self, x, qmap, mask_pol)

    def compress_quality_map(self, x, qmap, mask_pol=None):
        """The bitstreams of :meth:`forward_quality_map`: one item per image, {"strings": [[one stream per slice], [z]] in the
        stream order of :meth:`compress_per_image` (always ns1 slice streams: a map never selects the base plan), "shape",
        "quality_map": {"levels": the image's sorted distinct mask qualities as float64, "index": uint8 ndarray [h, w] of each
        position's index in them}, "side_bytes": 8 * len(levels) + h * w}.  The map is carried raw (no entropy coding of the
        map); the decoder needs it to rebuild the masks.  An item whose map is constant q > 0 has the strings of
        ``compress_per_image`` at q.  Refusals as :meth:`forward_quality_map`."""
        return control.compress_quality_map(self, x, qmap, mask_pol)

    def decompress_quality_map(self, items, mask_pol=None):
        """{"x_hat": [B, 3, H, W]} from items of :meth:`compress_quality_map` (one ``shape`` per call): bit-identical to
        :meth:`forward_quality_map`'s ``x_hat``.  The stored float64 levels are used as they are (``mask_pol`` was applied
        by the encoder)."""
        return control.decompress_quality_map(self, items, mask_pol)

    def quality_map_rate(self, x, qmap, mask_pol=None):
        """The estimated rate of a map without masks, LRP stacks or g_s: {"log2_likelihood_sum": float64 [2, B] (what
        :meth:`forward_quality_map` returns, to its float64 summation order), "bpp": float64 [B]}.  all_scalable models run
        the sweep plan's front end, one vam_variance_layers_per_image on each image's levels and one vam_gauss_layer_bits
        with one bin row per latent position: a position at level index k holds the elements of layers <= k at their
        in-mask likelihood, every other element counts log2 L(0, 0).  The others call :meth:`forward_quality_map`."""
        return control.quality_map_rate(self, x, qmap, mask_pol)

    def quality_map_for_bpp(self, x, floor_map, target_bpp, q_tol=1e-3, mask_pol=None):
        """Spend a rate budget around a region of interest: per image b and target t the largest uniform quality q* in
        [0, 10] such that the map max(floor_map, q*) stays within t (a region of interest is a floor map with q_roi inside and
        0 outside; at most 8 distinct values per image).  ``target_bpp``: a float, T floats or [T, B].  Returns {"quality",
        "bpp", "reached": [T, B], "quality_map": float64 [T, B, h, w] = max(floor_map, q*)} on the host with, for
        bpp_b(q) = quality_map_rate(max(floor_map, q)):  bpp_b(q*) <= t;  q* = 10 or bpp_b(min(10, q* + q_tol)) > t;  q* = 0 and
        reached = False when the floor map alone exceeds t.  :func:`rate_search` on grids of 24 points: a pass is one
        vam_variance_layers_per_image (floor levels and grid points in one list) and one vam_gauss_layer_bits.
        point-based-std only (ValueError otherwise, as :meth:`qualities_for_bpp`); all_scalable=False is refused."""
        return control.quality_map_for_bpp(self, x, floor_map, target_bpp, q_tol, mask_pol)

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

    def _coder(self) -> str:
        if self.coder not in ("host", "device"):
            raise ValueError(f"model.coder is 'host' or 'device', got {self.coder!r}")
        return self.coder

    def _coder_lanes(self) -> int:
        from . import bitstream as bs
        try:
            return bs.check_lanes(self.coder_lanes)
        except ValueError:
            raise ValueError(f"model.coder_lanes is a power of two in 1 .. 64, got {self.coder_lanes!r}") from None

    def _refuse_lanes_for_sizes(self, what: str):
        """The coded-size functions bracket the bytes of coder_lanes = 1 strings: refuse to answer for any other setting."""
        if self._coder_lanes() != 1:
            raise ValueError(f"{what} brackets the bytes of model.coder_lanes = 1 strings; with coder_lanes = {self.coder_lanes} "
                             "every stream carries a header and one final state per lane, and the bracket no longer holds")

    def _encode_plan_device(self, plan, n_sl: int, lanes: int = 1):
        """The streams of an executed symbol plan from the device coder: (y strings [slice][image], z strings [image]).  One
        launch for the n_sl * B slice streams straight from the plan's NHWC symbol and index views, one for the B z streams
        (no index buffer: table index = channel).  ``lanes``: model.coder_lanes, for both."""
        from . import bitstream as bs
        dev = plan.sym.buf.device
        tg = bs.DeviceCoderTables.of(self.gaussian_conditional, dev)
        te = bs.DeviceCoderTables.of(self.entropy_bottleneck, dev)
        ys = bs.encode_streams_device(plan.sym, plan.idx, n_sl, self.dim_chunk, tg, lanes=lanes)
        zs = bs.encode_streams_device(plan.z_sym, None, 1, self.N, te, lanes=lanes)
        return ys, zs[0]

    def compress(self, x, quality=0.0, mask_pol=None, checkpoint_rep=None, real_compress=True):
        """One rANS stream per (slice, image) for y and per image for z.  The latents, entropy
        parameters, masks, symbols and table indexes come from the fused HIP plan; only the
        bit-serial coder runs on the host (as in the reference, entropy_models.py:231-239).
        ``model.coder_lanes`` = K > 1 splits every stream into K lanes; K is not stored in the strings,
        so :meth:`decompress` must run with the same value, as with the same quality and shape."""
        mask_pol = self._mask_policy(mask_pol)
        coder, lanes = self._coder(), self._coder_lanes()
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
        if real_compress and coder == "device":
            if plan.idx is None:
                raise ValueError(EMPTY_SCALE_TABLE.format("compress"))
            y_strings, z_strings = self._encode_plan_device(plan, n_sl, lanes)
        elif real_compress:
            from . import bitstream as bs
            if plan.idx is None:
                raise ValueError(EMPTY_SCALE_TABLE.format("compress"))
            tg, te = bs.Tables.of(self.gaussian_conditional), bs.Tables.of(self.entropy_bottleneck)
            sym = plan.sym.buf.cpu().numpy()           # [B,h,w,C_lat] int32 (synchronises)
            idx = plan.idx.buf.cpu().numpy()
            zs = plan.z_sym.buf.cpu().numpy()
            enc = bs.encode if lanes == 1 else (lambda s_, i_, t_: bs.encode_lanes(s_, i_, t_, lanes))
            for i in range(n_sl):                       # stream order: [C, h, w] per image, as the reference flattens
                sl = slice(i * C, (i + 1) * C)
                y_strings.append([enc(sym[b, :, :, sl].transpose(2, 0, 1), idx[b, :, :, sl].transpose(2, 0, 1), tg)
                                  for b in range(B)])
            zi = torch.arange(self.N, dtype=torch.int32).numpy()[:, None, None]
            z_strings = [enc(zs[b].transpose(2, 0, 1), np.broadcast_to(zi, (self.N,) + zs.shape[1:3]), te)
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
        GPU, rANS decode on the host, LRP on the GPU) -> g_s.  ``model.coder_lanes`` must be what it was for
        :meth:`compress`: the strings do not store it, and a wrong value gives a VamError or a wrong image."""
        mask_pol = self._mask_policy(mask_pol)
        coder, lanes = self._coder(), self._coder_lanes()
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
            return _DecPlan(self, B, hz, wz, base_only, rem_idx, dev, coder=coder)
        dp = self._cached_plan(self._dec_plans, (B, hz, wz, base_only, rem_idx, str(dev)) + ((coder,) if coder != "host" else ()),
                               build, self._weights_sig(), rem_idx)
        return {"x_hat": dp.decode(strings, _mask_quality(mask_pol, quality), checkpoint_rep if rem_idx is not None else None,
                                   lanes=lanes)}

    def _prog_dec_plan(self, B, hz, wz, q_list, coder: str = "host") -> "_ProgDecPlan":
        """The plans of progressive.ProgressiveDecoder for one (B, z-shape, quality list, coder), cached beside decompress's."""
        dev = self.entropy_bottleneck.quantiles.device
        return self._cached_plan(self._dec_plans, ("prog", B, hz, wz, tuple(float(q) for q in q_list), str(dev))
                                 + ((coder,) if coder != "host" else ()),
                                 lambda: _ProgDecPlan(self, B, hz, wz, q_list, dev, coder=coder), self._weights_sig())

    def _emb_dec_plan(self, B, hz, wz, coder: str = "host", scheduled: bool = False) -> "_EmbDecPlan":
        """The plans of embedded.EmbeddedDecoder for one (B, z-shape, coder), cached beside decompress's: the cuts are graph
        inputs, so no quality list is part of the key.  ``scheduled``: the plan of scheduled containers;
        the key says so and carries no schedule, which is an input of the plan's device buffers."""
        dev = self.entropy_bottleneck.quantiles.device
        return self._cached_plan(self._dec_plans, ("emb", B, hz, wz, str(dev)) + ((coder,) if coder != "host" else ())
                                 + (("scheduled",) if scheduled else ()),
                                 lambda: _EmbDecPlan(self, B, hz, wz, dev, coder=coder, scheduled=scheduled), self._weights_sig())


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


# ----------------------------------------------------------------------------- what a plan accepts
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
