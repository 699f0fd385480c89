"""The plans that lower the models of ``models.py`` to libvampic launches — ``forward_single_quality`` (:class:`_FsqPlan`), the
quality sweeps with their rate and coded-size tails (:class:`_SweepPlan`), ``decompress`` (:class:`_DecPlan`), the progressive
container decoder (:class:`_ProgDecPlan`), the embedded-stream decoder (:class:`_EmbDecPlan`) — and the autograd functions of the training plans.  A plan takes the model as an
argument; nothing here imports ``models``.  How a slice is lowered is written once, in :class:`_SliceChain`: encoder, sweep
and decoder have to agree on it bit for bit, or a bitstream does not decode (models/pic.py:497-967, rem_pic.py:229-818).
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
from . import ops


def _mask_table_buffer(B: int, device) -> torch.Tensor:
    """A plan's device table for ops.variance_masks_per_image: one record per image, refilled before each replay."""
    import ctypes
    return torch.zeros((B * ctypes.sizeof(L.VamLayerParams),), dtype=torch.uint8, device=device)


def _slice_stack_heads(plan, m, means_h, scales_h, which):
    """Hyperprior part of the first layer of every slice stack (engine.lower_stack_heads): base stacks read the first
    ``d`` channels of the hyper tensors, progressive ones the second (pic.py:528-529,598-599); the LRP stacks share the
    MEAN support of their slice (pic.py:548,635).  ``which`` = "base" or "prog".  Encoder and decoder plans both call
    this, so both associate the first-layer sum the same way."""
    d, ns, prog = m.division_dimension[0], m.ns0, which == "prog"
    mh, sh = means_h.window(d * prog, d), scales_h.window(d * prog, d)
    means, scales, lrps = ((m.cc_mean_transforms_prog, m.cc_scale_transforms_prog, m.lrp_transforms_prog) if prog else
                           (m.cc_mean_transforms, m.cc_scale_transforms, m.lrp_transforms))
    stacks, hyp, sup = [], [], []
    for i in range(ns):
        stacks += [means[i], scales[i], lrps[i]]
        hyp += [mh, sh, mh]
        sup += [prog or i > 0, prog or i > 0, True]       # base slice 0 has no support: its first layers come complete
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


def _vmask(qtable, q, sigma, mask, n_slice, thr=None, level_map=None):
    """The variance masks of ``n_slice`` slices at the scalar quality ``q`` or, with ``qtable`` (per-image plans), at each
    image's own, read from the plan's device table — one level, the same segments, so the same bits per image.  With
    ``level_map`` (quality-map plans) the table holds each image's sorted list and every latent pixel
    takes the level the map names: still one launch and one mask."""
    if level_map is not None:
        ops.variance_mask_map(sigma, qtable, level_map, mask, n_slice=n_slice, thr=thr)
    elif qtable is not None:
        ops.variance_masks_per_image(sigma, qtable, mask, n_slice=n_slice, thr=thr)
    else:
        ops.variance_mask(sigma, q, mask, n_slice=n_slice, thr=thr)


def _fill_mask_table(qtable: torch.Tensor, rows: Sequence[Sequence[float]], n_pix: int, C: int):
    """Refill a per-image plan's table with image b's mask qualities ``rows[b]``: on the current stream, before the replay
    and outside the capture, so the qualities are inputs of the plan's ONE graph."""
    qtable.copy_(torch.from_numpy(ops.mask_table([[float(q) for q in row] for row in rows], n_pix, C)))


def _fill_quality_map(qtable: torch.Tensor, level_map: torch.Tensor, levels: Sequence[Sequence[float]], index, n_pix: int, C: int):
    """Refill a quality-map plan's two graph inputs: image b's sorted qualities ``levels[b]`` (ops.layer_table) and the uint8
    index map ``index`` [B, h, w] (host).  On the current stream, before the replay and outside the capture."""
    idx = torch.from_numpy(np.ascontiguousarray(index, dtype=np.uint8)).view(level_map.shape)
    qtable.copy_(torch.from_numpy(ops.layer_table([[float(q) for q in row] for row in levels], n_pix, C)))
    level_map.copy_(idx)


def _load_checkpoint(ck: ops.View, checkpoint: torch.Tensor):
    """Copy a checkpoint latent (NCHW) into a plan's ``ck`` buffer."""
    src = ops.from_nchw(checkpoint.to(ck.buf.device))
    ck.buf.copy_(src.buf[..., src.c0:src.c0 + src.C])


class _SliceChain:
    """The slice buffers of one plan and how the slices of model ``m`` are lowered over them (pic.py:522-554 the base slices,
    :577-643 the progressive ones, rem_pic.py:363-377 the REM step), each piece once.  The plans keep what differs between
    them: which engine.Plan a launch goes into, how slices are grouped, branches, events and launch classes."""

    def __init__(self, m, alloc, base_only=False, rem_idx=None):
        self.m, self.ns, self.alloc, self.rem_idx = m, m.ns0, alloc, rem_idx     # alloc(): a latent-shaped buffer of d channels
        self.heads: Dict[int, tuple] = {}               # the hoisted first layers (_slice_stack_heads)
        self.lrp_prog = [m.lrp_transforms_prog[j] for j in range(self.ns)]
        self.mu_std = getattr(m, "mu_std", True)        # without mu_std a REM refines sigma alone (rem_pic.py:214-218)
        self.rem_sig = self.ck = self.att = None
        # yq: round(y-mu)+mu before the LRP correction, yb: the base y_hat (after it)
        self.yq, self.yb, self.mu_b, self.std_b = (alloc() for _ in range(4))
        if base_only:
            return
        self.mu_p, self.std_p, self.yp, self.rq, self.mask = (alloc() for _ in range(5))
        # the support vector of the mean chain is mu + y_hat_base with total_mu_rep (pic.py:601), else mu itself; only
        # all_scalable reads it (:586-587), so only then is the sum lowered
        self.mu_tot = alloc() if (m.total_mu_rep and m.all_scalable) else self.mu_p
        self.mu_f, self.std_f = self.mu_p, self.std_p
        if rem_idx is not None:      # checkpoint latent, attention mask and the refined (mu, sigma)
            self.ck, self.att, self.std_f = alloc(), alloc(), alloc()
            self.mu_f = alloc() if self.mu_std else self.mu_p
            self.rem_sig = _version_sig(m.post_latent[rem_idx])    # models._cached_plan: an edited REM is packed again

    def sl(self, v, i, n=1):
        """Slices i .. i+n-1 of a latent-shaped view."""
        return v.window(i * self.m.dim_chunk, n * self.m.dim_chunk)

    def base_support(self, yb, i):
        """Base slice i reads the first min(max_support_slices, i) base slices (slices 5..9 only see slices 0..4)."""
        n = min(self.m.max_support_slices, i)
        return [self.sl(yb, 0, n)] if n else []

    def prog_supports(self, j, yb, mu_tot, std_p, yp=None):
        """determine_support (pic.py:264-270) for the mean and the scale stack of progressive slice j: base slice j + the
        last min(sp, j) slices of the support vectors — mu_total / std_total with all_scalable, the decoded progressive
        slices ``yp`` otherwise (pic.py:586-587).  Returns (ms, ss)."""
        s = min(self.m.support_progressive_slices, j)
        hist = (mu_tot, std_p) if self.m.all_scalable else (yp, yp)
        return tuple([self.sl(yb, j)] + ([self.sl(v, j - s, s)] if s else []) for v in hist)

    def lower_base_params(self, plan, idx: Sequence[int]):
        """The mean and scale stacks of a group of base slices with one support (their hyperprior part is in ``heads``)."""
        m, sl, sup = self.m, self.sl, self.base_support(self.yb, idx[0])
        E.lower_stacks(plan, [m.cc_mean_transforms[i] for i in idx] + [m.cc_scale_transforms[i] for i in idx],
                       [sup] * (2 * len(idx)), [sl(self.mu_b, i) for i in idx] + [sl(self.std_b, i) for i in idx], heads=self.heads)

    def lower_base_lrp(self, plan, idx: Sequence[int]):
        """y_hat_base_i = yq_i + 0.5 tanh(lrp_i(cat(supports, yq_i))) for the same group."""
        sl, yq, sup = self.sl, self.yq, self.base_support(self.yb, idx[0])
        E.lower_stacks(plan, [self.m.lrp_transforms[i] for i in idx], [sup + [sl(yq, i)] for i in idx],
                       [sl(self.yb, i) for i in idx], [dict(act=L.ACT_HALF_TANH, post=sl(yq, i)) for i in idx], heads=self.heads)

    def lower_prog_params(self, plan, j):
        """(mu, sigma) of progressive slice j (pic.py:586-612).  Returns the mean supports: the LRP stack shares them (:635)."""
        m, sl, yb, mu_p, mu_tot = self.m, self.sl, self.yb, self.mu_p, self.mu_tot
        ms, ss = self.prog_supports(j, yb, mu_tot, self.std_p, self.yp)
        E.lower_stacks(plan, [m.cc_mean_transforms_prog[j], m.cc_scale_transforms_prog[j]], [ms, ss],
                       [sl(mu_p, j), sl(self.std_p, j)], heads=self.heads)
        if mu_tot is not mu_p:
            plan.call(lambda: ops.add(sl(mu_p, j), sl(yb, j), sl(mu_tot, j)))     # pic.py:601
        return ms

    def lower_param_chain(self, plan, after: Optional[Dict[int, int]] = None):
        """all_scalable: the (mu, sigma) chain over all slices reads only y_hat_base and its own history (pic.py:586-612).
        ``after[j]``: the event "y_hat_base of slice j is final", waited for first.  Returns every slice's mean supports."""
        msups = []
        for j in range(self.ns):
            if after is not None:
                plan.wait(after[j])
            msups.append(self.lower_prog_params(plan, j))
        return msups

    def lower_prog_lrp(self, plan, js: Sequence[int], heads, msups, rq, yb, out):
        """y_hat_j = rq_j + 0.5 tanh(lrp_j(cat(supports, rq_j))) + y_hat_base_j (pic.py:635-641) for the slices ``js``;
        ``msups[k]``: the mean supports of slice js[k], rq: the quantised, masked residual + mu."""
        sl = self.sl
        E.lower_stacks(plan, [self.lrp_prog[j] for j in js], [ms + [sl(rq, j)] for ms, j in zip(msups, js)],
                       [sl(out, j) for j in js], [dict(act=L.ACT_HALF_TANH, post=sl(rq, j), post2=sl(yb, j)) for j in js],
                       heads=heads)

    def rem_io(self, js: Sequence[int]):
        """The REM blocks of the slices ``js`` and their five I/O lists (engine.lower_rem_blocks / lower_rem_blocks_train)."""
        sl = self.sl
        mu = (lambda v, j: [sl(v, j)]) if self.mu_std else (lambda v, j: [])
        return ([self.m.post_latent[self.rem_idx][j] for j in js], [sl(self.ck, j) for j in js],
                [[sl(self.mu_b, j), sl(self.std_b, j)] for j in js], [mu(self.mu_p, j) + [sl(self.std_p, j)] for j in js],
                [sl(self.att, j) for j in js], [mu(self.mu_f, j) + [sl(self.std_f, j)] for j in js])

    def lower_att_mask(self, plan, owner, js: Sequence[int]):
        """The REM's attention mask: the variance mask of the unrefined sigma, at ``owner``'s quality."""
        sl, j0, n = self.sl, js[0], len(js)
        plan.call(lambda: _vmask(owner.qtable, owner.pr, sl(self.std_p, j0, n), sl(self.att, j0, n), n))

    def lower_rem(self, plan, owner, js: Sequence[int]):
        """The REM step of the consecutive slices ``js`` (rem_pic.py:363-377): attention mask, then the blocks in lockstep."""
        self.lower_att_mask(plan, owner, js)
        E.lower_rem_blocks(plan, *self.rem_io(js))


class _FsqPlan:
    """``forward_single_quality`` for one (B,H,W) lowered to libvampic launches."""

    def __init__(self, m, B, H, W, base_only, rem_idx, device, symbols=False, train=False,
                 own_ck=False, train_gs=False, train_lrp=False, sweep=False, per_image=False, quality_map=False):
        assert not sweep or (m.all_scalable and not base_only and rem_idx is None and not (symbols or train))
        # per_image: the variance masks read each image's quality from a device table
        assert not per_image or not (sweep or base_only or train or own_ck or rem_idx is not None)
        # quality_map: every latent pixel takes its own level of its image's sorted list
        assert not quality_map or not (per_image or sweep or base_only or train or own_ck or rem_idx is not None)
        self.per_image, self.quality_map = per_image, quality_map
        self.qtable = _mask_table_buffer(B, device) if per_image or quality_map else None
        self.level_map = torch.zeros((B, (H // 16) * (W // 16)), dtype=torch.uint8, device=device) if quality_map else None
        self.m, self.B, self.H, self.W = m, B, H, W
        self.train_gs = train_gs    # the synthesis transform in use is being trained (refine_gs): taped g_s + backward plan
        self.train_lrp = train_lrp  # ... and the progressive LRP stacks with it (refine_gs --lrp)
        self.own_ck, self.ck_pr = own_ck, 0.0     # fine-tune: derive the checkpoint latent inside this plan
        self.base_only, self.rem_idx, self.symbols = base_only, rem_idx, symbols
        self.train = train          # additive-noise likelihoods (+ taped REM and a backward plan when rem_idx is set)
        self.bwd = None             # backward plan of a training plan (REM fine-tune or refine_gs): see _backward
        self.generation = 0         # bumped by every execute(): which forward the training tape belongs to
        self.pr = 0.0
        self.runner = E.Runner(device, cap=32)      # forward graphs per (pr, ck_pr)
        self.bwd_runner = E.Runner(device)          # the backward's graph (no cap), replayed on self.runner's stream
        plan = self.plan = E.Plan(device)
        d, ns = m.division_dimension[0], m.ns0
        sc = self.sc = _SliceChain(m, lambda: plan.buf(B, H // 16, W // 16, d), base_only, rem_idx)
        f32 = dict(dtype=torch.float32, device=device)
        self.x_in = torch.empty((B, 3, H, W), **f32)
        self.x_hat = torch.empty((B, 3, H, W), **f32)
        self.log2sum = torch.zeros((2, B), dtype=torch.float64, device=device)   # [y, z] per image
        plan.keep += [self.x_in, self.x_hat, self.log2sum]
        plan.call(lambda: ops.memset_zero(self.log2sum))
        self.act16 = getattr(m, "storage", "fp32") == "bf16"
        self._lower_front_end(z_symbols=symbols or sweep)    # sweep mode keeps the z symbols: coded_size_curve prices them
        hyper_done, base_done = self._lower_base_slices()
        if base_only:
            self._lower_synthesis(m.g_s[0] if m.multiple_decoder else m.g_s, self.y_base)
            return
        if train and not m.all_scalable:
            raise NotImplementedError("training-mode plans are built for all_scalable=True (README config)")
        g_s = m.g_s[1] if m.multiple_decoder else m.g_s
        self.mu_p, self.std_p, self.y_prog, self.mask = sc.mu_p, sc.std_p, sc.yp, sc.mask
        self.mu_f, self.std_f, self.ck, self.att, self.rem_sig = sc.mu_f, sc.std_f, sc.ck, sc.att, sc.rem_sig
        self.y_top = self.y.window(d, d)
        self.y_sub = self.y.window(0, d) if m.delta_encode else None                        # pic.py:583-584
        # the masks' thresholds — not collected by the per-slice launches of the sequential schedule
        # (a quality-map plan: one row per level of the longest list)
        self.thr = torch.empty(((L.VAM_MAX_LAYER_LEVELS if quality_map else 1) * B * ns,), **f32) if m.all_scalable and not sweep else None
        plan.keep += [self.thr, self.level_map]
        if not m.all_scalable:
            # pic.py:586-587: the (mu, sigma) stacks of progressive slice j read the DECODED progressive slices j-sp..j-1,
            # so mask, quantisation and LRP of a slice must finish before the next slice's stacks start — one slice at a
            # time, on the caller's stream
            plan.set_class("stack_heads")
            sc.heads.update(_slice_stack_heads(plan, m, self.means_h, self.scales_h, "prog"))
            plan.set_class("slice_chain")
            for j in range(ns):
                ms = sc.lower_prog_params(plan, j)
                if rem_idx is not None:
                    self._lower_rem([j], [ms])
                self._lower_quality_tail([j], [ms])
            if not symbols:
                plan.set_class("g_s")
                E.lower_g_s(plan, [g_s], [self.y_prog], [self.x_hat])
            return
        msups = self._lower_prog_chain(hyper_done, base_done)
        if sweep:
            # everything up to here does not depend on the quality; the per-level tail and the base reconstruction are
            # plans of their own over these buffers
            self.sweep_parts = dict(heads=sc.heads, yb=sc.yb, mu=sc.mu_p, std=sc.std_p, mu_tot=sc.mu_tot,
                                    y_top=self.y_top, y_sub=self.y_sub, g_s=g_s)
            return
        if rem_idx is not None:
            plan.set_class("rem")
            self._lower_rem(range(ns), msups)
        plan.set_class("lrp_prog")
        lrp = self._lower_quality_tail(range(ns), msups)
        self._lower_synthesis(g_s, self.y_prog, lrp)

    def _lower_front_end(self, z_symbols: bool):
        """x -> y (g_a), z (h_a), z_hat and its likelihoods (entropy bottleneck), the hyperprior tensors (hyper-synthesis)."""
        m, plan, B, H, W = self.m, self.plan, self.B, self.H, self.W
        h, w, d = H // 16, W // 16, m.division_dimension[0]
        # ---- analysis transforms (both encoders in lockstep)                      pic.py:506-508
        x_s2d = plan.buf(B, H // 2, W // 2, 16)
        plan.call(lambda: L.check(L.load().vam_s2d_input(self.x_in.data_ptr(), x_s2d.ptr, B, H, W, ops.stream_ptr()),
                                  "vam_s2d_input"))
        y = self.y = plan.buf(B, h, w, 2 * d)
        plan.set_class("g_a")
        plan.act16 = self.act16
        if m.multiple_encoder:
            E.lower_g_a(plan, [m.g_a[0], m.g_a[1]], x_s2d, [y.window(0, d), y.window(d, d)])
        else:                                            # one encoder with M output channels (builder.py:56-67)
            E.lower_g_a(plan, [m.g_a], x_s2d, [y])
        plan.act16 = False
        # ---- hyperprior                                                            pic.py:278-298
        z = self.z = plan.buf(B, h // 4, w // 4, m.N)
        plan.set_class("hyperprior")
        E.lower_stacks(plan, [m.h_a], [[y]], [z])
        self.z_hat = plan.buf(B, h // 4, w // 4, m.N)
        self.z_lik = plan.buf(B, h // 4, w // 4, m.N)
        self.z_sym = ops.new_iview(B, h // 4, w // 4, m.N, plan.device) if z_symbols else None   # the entropy coder's z symbols
        plan.keep.append(self.z_sym)
        self.noise_z = plan.buf(B, h // 4, w // 4, m.N) if self.train else None
        self.noise_y = plan.buf(B, h, w, d if self.base_only else 2 * d) if self.train else None
        ls_z = self.log2sum[1]
        plan.call(lambda: ops.eb_forward(z, m.entropy_bottleneck.packed_params(), self.z_hat, self.z_lik, ls_z, sym=self.z_sym,
                                         noise=self.noise_z))
        self.means_h, self.scales_h = _lower_hyper_synthesis(plan, m, self.z_hat, self.base_only)

    def _lower_base_slices(self):
        """pic.py:522-554.  Returns the events "the hyperprior is done" and {slice: "its y_hat_base is final"}."""
        m, plan, sc, sl = self.m, self.plan, self.sc, self.sc.sl
        d, ns, y, h, w = m.division_dimension[0], m.ns0, self.y, self.H // 16, self.W // 16
        base_only, symbols, train = self.base_only, self.symbols, self.train
        yq, self.y_base, self.mu_b, self.std_b = sc.yq, sc.yb, sc.mu_b, sc.std_b
        self.lik = plan.buf(self.B, h, w, d if base_only else 2 * d)
        # entropy-coder inputs (compress only): quantised symbols and scale-table indexes
        self.sym = ops.new_iview(self.B, h, w, self.lik.C, plan.device) if symbols else None
        table = m.gaussian_conditional.scale_table
        indexes = symbols and table.numel() > 0        # without update() only real_compress=False is possible
        self.idx = ops.new_iview(self.B, h, w, self.lik.C, plan.device) if indexes else None
        self.table = table if indexes else None
        plan.keep += [self.sym, self.idx]
        ls_y = self.log2sum[0]
        hyper_done, base_done = (plan.record() if not base_only else None), {}
        plan.set_class("stack_heads")
        sc.heads.update(_slice_stack_heads(plan, m, self.means_h, self.scales_h, "base"))   # hyperprior part of every first layer, up front
        plan.set_class("slice_chain")
        msup = m.max_support_slices
        # one slice at a time while the support grows; slices 5..9 only see slices 0..4: one group
        for idx in [[i] for i in range(min(ns, msup))] + ([list(range(msup, ns))] if ns > msup else []):
            i0, n = idx[0], len(idx)
            sc.lower_base_params(plan, idx)
            plan.call(lambda i0=i0, n=n: ops.gauss_tail(sl(y, i0, n), sl(self.mu_b, i0, n), sl(self.std_b, i0, n),
                                                        yhat=sl(yq, i0, n), lik=sl(self.lik, i0, n), log2sum=ls_y,
                                                        sym=sl(self.sym, i0, n) if symbols else None))
            if train:        # quantize "noise": likelihood at y + U(-.5,.5) - mu (entropy_models.py:132-138,643-651)
                plan.call(lambda i0=i0, n=n: ops.gauss_train(sl(y, i0, n), sl(self.mu_b, i0, n), sl(self.std_b, i0, n),
                                                             sl(self.noise_y, i0, n), lik=sl(self.lik, i0, n)))
            if indexes:                                                               # pic.py:737
                plan.call(lambda i0=i0, n=n: ops.build_indexes(sl(self.std_b, i0, n), table, out=sl(self.idx, i0, n)))
            sc.lower_base_lrp(plan, idx)
            if not base_only:
                ev = plan.record()
                base_done.update({i: ev for i in idx})
        return hyper_done, base_done

    def _lower_prog_chain(self, hyper_done, base_done):
        """With all_scalable the progressive mu/sigma chain only needs y_hat_base[j] and its own history
        (pic.py:586-612), so it runs on a second HIP stream concurrently with base slices > j.  Returns the mean supports."""
        plan = self.plan
        plan.branch(1)
        plan.wait(hyper_done)
        plan.set_class("stack_heads")
        self.sc.heads.update(_slice_stack_heads(plan, self.m, self.means_h, self.scales_h, "prog"))   # on the chain's stream, beside base slice 0
        plan.set_class("slice_chain")
        msups = self.sc.lower_param_chain(plan, after=base_done)
        chain_done = plan.record()
        plan.branch(0)
        plan.wait(chain_done)
        return msups

    def _lower_rem(self, js, msups):
        """The REM step of the slices ``js`` (rem_pic.py:363-377): (mu, sigma) -> (mu_f, std_f).  A training plan tapes it
        and gets its backward plan: dL/dlik (progressive half) -> (dmu', dsigma') -> REM parameters."""
        m, plan, sc, sl = self.m, self.plan, self.sc, self.sc.sl
        d, n = m.division_dimension[0], len(js)
        if self.own_ck:
            # y_hat at the check level from the SAME front end (everything up to here is quality independent;
            # at q <= check_levels[0] no REM applies): what ExtractChekpointRepr(x, q_ref) returns, pic.py:621-641
            m_ck, rq_ck, junk = sc.alloc(), sc.alloc(), sc.alloc()
            plan.call(lambda: ops.variance_mask(self.std_p, self.ck_pr, m_ck, n_slice=n))
            plan.call(lambda: ops.gauss_tail(self.y_top, self.mu_p, self.std_p, y2=self.y_sub, mask=m_ck, yhat=rq_ck, lik=junk))
            sc.lower_prog_lrp(plan, js, sc.heads, msups, rq_ck, sc.yb, self.ck)
        if not self.train:
            return sc.lower_rem(plan, self, js)
        sc.lower_att_mask(plan, self, js)
        mods, *rem_io = sc.rem_io(js)
        self.train_params = [p for mod in mods for p in mod.parameters()]
        self.packs = G.TransformPacks(*E.rem_trained_convs(mods))
        self.packs.record_refresh(plan)
        tape = E.lower_rem_blocks_train(plan, mods, *rem_io, self.packs)
        bw = self.bwd = E.Plan(plan.device)
        glik, dmu, dsg = (bw.buf(self.B, self.H // 16, self.W // 16, d) for _ in range(3))
        self._bwd_in = lambda g: glik.buf.copy_(g[:, d:].permute(0, 2, 3, 1))       # dL/dlikelihoods["y"], NCHW
        self.dmu, self.dsg, self.rem_io, self.rem_tape = dmu, dsg, tuple(rem_io), tape     # kept for teacher-forced gradient checks
        grads = self._grad_buffer()
        bw.call(lambda: ops.gauss_train(self.y_top, self.mu_f, self.std_f, self.noise_y.window(d, d), y2=self.y_sub,
                                        mask=self.mask, grad_lik=glik, dmu=dmu, dsigma=dsg), "likelihood backward")
        E.lower_rem_backward(bw, tape, mods, [sl(dmu, j) for j in js], [sl(dsg, j) for j in js], rem_io[3], self.packs, grads)

    def _lower_quality_tail(self, js, msups):
        """Mask, quantisation + likelihood, table indexes and LRP stacks of the slices ``js`` (pic.py:621-641): what depends
        on the quality.  Returns the taped LRP stacks when they train (``train_lrp``), else None."""
        m, plan, sc, sl = self.m, self.plan, self.sc, self.sc.sl
        ns, j0, n, rq, ls_y = m.ns0, js[0], len(js), sc.rq, self.log2sum[0]
        y_top, mu_f, std_f, mask = sl(self.y_top, j0, n), sl(self.mu_f, j0, n), sl(self.std_f, j0, n), sl(self.mask, j0, n)
        y_sub = sl(self.y_sub, j0, n) if self.y_sub is not None else None
        lik = sl(self.lik, ns + j0, n)
        plan.call(lambda: _vmask(self.qtable, self.pr, std_f, mask, n, self.thr, self.level_map))      # pic.py:621-622
        plan.call(lambda: ops.gauss_tail(y_top, mu_f, std_f, y2=y_sub, mask=mask, yhat=sl(rq, j0, n), lik=lik, log2sum=ls_y,
                                         sym=sl(self.sym, ns + j0, n) if self.symbols else None))      # pic.py:625-629
        if self.train:
            plan.call(lambda: ops.gauss_train(y_top, mu_f, std_f, sl(self.noise_y, ns + j0, n), y2=y_sub, mask=mask, lik=lik))
        if self.table is not None:                                                    # pic.py:813
            plan.call(lambda: ops.build_indexes(std_f, self.table, mask=mask, out=sl(self.idx, ns + j0, n)))
        if self.train_lrp:
            return self._lower_lrp_train(msups)
        sc.lower_prog_lrp(plan, js, sc.heads, msups, rq, sc.yb, sc.yp)

    def _lower_lrp_train(self, msups):
        """refine_gs --lrp: y_hat_j = rq_j + 0.5 tanh(stack_j(cat(supports, rq_j))) + base_j (pic.py:635-641) with the
        stacks taped; a TRAINED stack runs its first layer whole (the eval plan hoists the hyperprior part: same sum,
        different association)."""
        plan, sl, ns, stacks, rq, d = self.plan, self.sc.sl, self.m.ns0, self.sc.lrp_prog, self.sc.rq, self.m.division_dimension[0]
        lpk = [G.TransformPacks(st) for st in stacks]
        for pk_ in lpk:
            pk_.record_refresh(plan)
        mh1 = self.means_h.window(d, d)
        tapes = G.lower_stacks_train(plan, stacks, [[mh1] + msups[j] + [sl(rq, j)] for j in range(ns)], [None] * ns, lpk)
        for j in range(ns):
            plan.call(lambda j=j: ops.ew(L.EW_HTANH_FWD, [tapes[j]["out"], sl(rq, j), sl(self.y_base, j)], [sl(self.y_prog, j)]),
                      "lrp tail")
        return dict(tapes=tapes, packs=lpk, params=[p for st in stacks for p in st.parameters()])

    def _lower_synthesis(self, dec, y_in, lrp=None):
        """g_s on the final latent — not for compress(), which does not decode (pic.py:671-860)."""
        if self.symbols:
            return
        self.plan.set_class("g_s")
        if self.train_gs:
            return self._lower_g_s_train(self.plan, dec, y_in, lrp)
        self.plan.act16 = self.act16
        E.lower_g_s(self.plan, [dec], [y_in], [self.x_hat])
        self.plan.act16 = False

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
                _load_checkpoint(self.ck, checkpoint_ref)
            self.runner.replay((self.pr, self.ck_pr), self.plan.run, use_graph)
        return self._outputs(clone)

    def execute_per_image(self, x, prs: Sequence[float], use_graph, clone=True):
        """:meth:`execute` of a per_image plan with image b at mask quality ``prs[b]`` (> 0).  The table is refilled on the
        runner's stream before the replay, outside the capture; the qualities are inputs of the plan's ONE graph."""
        assert self.per_image and len(prs) == self.B
        self.generation += 1
        with self.runner.on_stream():
            self.x_in.copy_(x)
            _fill_mask_table(self.qtable, [[p_] for p_ in prs], (self.H // 16) * (self.W // 16), self.m.dim_chunk)
            self.runner.replay(("per_image",), self.plan.run, use_graph)
        return self._outputs(clone)

    def execute_quality_map(self, x, levels: Sequence[Sequence[float]], index, use_graph, clone=True):
        """:meth:`execute` of a quality_map plan: latent pixel p of image b at mask quality ``levels[b][index[b, p]]``
        (``levels[b]`` sorted, ``index`` uint8 [B, h, w] on the host).  Table and map are refilled on the runner's stream
        before the replay, outside the capture: they are inputs of the plan's ONE graph."""
        assert self.quality_map and len(levels) == self.B
        self.generation += 1
        with self.runner.on_stream():
            self.x_in.copy_(x)
            _fill_quality_map(self.qtable, self.level_map, levels, index, (self.H // 16) * (self.W // 16), self.m.dim_chunk)
            self.runner.replay(("quality_map",), self.plan.run, use_graph)
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

    def map_bins(self, levels: Sequence[Sequence[float]]) -> torch.Tensor:
        """The bins of a quality map's rate, eagerly: one vam_variance_layers_per_image on image b's sorted
        list ``levels[b]`` and one vam_gauss_layer_bits at pix_per_item = 1.  Returns [2, B, h * w, n + 1] (n = the longest
        list): per latent pixel the float64 sums and (as int64) the counts by level, slot n = no level."""
        pa, sg = self.parts, self.parts["std"]
        n = max(len(r) for r in levels)
        acc = torch.zeros((2, sg.B, sg.H * sg.W, n + 1), dtype=torch.float64, device=sg.buf.device)
        ops.variance_layers_per_image(pa["std"], levels, self.layer, n_slice=self.ns)
        ops.gauss_layer_bits(pa["y_top"], pa["mu"], pa["std"], self.layer, n, acc[0], acc[1].view(torch.int64), y2=pa["y_sub"],
                             pix_per_item=1)
        return acc

    def map_values(self, acc: torch.Tensor) -> torch.Tensor:
        """[B, h * w, n] from :meth:`map_bins`: the progressive log2 sum of each latent pixel were it at level k — the
        elements of layers <= k at their in-mask likelihood, every other element at log2 L(0, 0)."""
        n = acc.shape[-1] - 1
        bits, count = acc[0], acc[1].view(torch.int64)
        total = count.sum(-1, keepdim=True)
        return bits[..., :n].cumsum(-1) + (total - count[..., :n].cumsum(-1)).double() * self.outside

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
        d, ns, sc = m.division_dimension[0], m.ns0, fp.sc
        dev = yb0.buf.device
        self.n_levels, self.B = NL, B
        self.prs = (0.0,) * NL            # eval: the mask qualities of the levels
        self.ks = (0,) * NL               # decode: the container-layer cut-offs of the levels
        self.runner = E.Runner(dev, cap=32)     # one graph per tuple of levels, replayed on the owner's stream
        self.qtable = _mask_table_buffer(B, dev) if per_image else None
        P = self.plan = E.Plan(dev)
        P.keep.append(self.qtable)
        self.log2sum = torch.zeros((NL, B), dtype=torch.float64, device=dev)      # level k's progressive log2 sums per image
        self.x_hat = torch.empty((LB, 3, H, W), dtype=torch.float32, device=dev)
        P.keep += [self.log2sum, self.x_hat]
        self.rq, self.y_prog = P.buf(LB, h, w, d), P.buf(LB, h, w, d)
        self.mask = self.lik = None
        stacks, heads = sc.lrp_prog, parts["heads"]
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
                P.call(lambda: _vmask(self.qtable, None, parts["std"], self.mask, ns), "variance masks per image (sweep)")
            else:
                P.call(lambda: ops.variance_mask_levels(parts["std"], self.prs, self.mask, n_slice=ns), "variance masks (sweep)")   # :621-622
            P.call(lambda: ops.gauss_levels_eval(parts["y_top"], parts["mu"], parts["std"], self.mask, NL, y2=parts["y_sub"],
                                                 yhat=self.rq, lik=self.lik, log2sum=self.log2sum), "quantise + likelihood (sweep)")   # :625-629
        P.call(replicate, "supports per level")
        heads_l = {id(st): (dst, False) for st, (_, dst) in zip(stacks, reps)}
        yb_l, mt_l = reps[ns][1], reps[ns + 1][1]
        msups = [sc.prog_supports(j, yb_l, mt_l, mt_l)[0] for j in range(ns)]      # the mean supports (all_scalable)
        sc.lower_prog_lrp(P, range(ns), heads_l, msups, self.rq, yb_l, self.y_prog)
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

    def __init__(self, m, B, H, W, device):
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
        with self.runner.on_stream():
            _fill_mask_table(t.qtable, [[Q_group[g][b] for g in range(n)] for b in range(self.B)], sg.H * sg.W, self.m.dim_chunk)
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

    def __init__(self, m, B, hz, wz, base_only, rem_idx, device, per_image: bool = False, quality_map: bool = False,
                 coder: str = "host"):
        """``per_image``: the per-slice masks read each image's quality from ``qtable`` (decode_per_image refills it);
        ``quality_map``: each latent pixel's from ``qtable`` and ``level_map``.  ``coder`` "device"
        (DESIGN section 9n): every string is uploaded once at the start of :meth:`decode`, a slice's cut is one
        vam_rans_decode_device launch on the runner's stream, and the status codes are read once after g_s."""
        assert not (per_image or quality_map) or not (base_only or rem_idx is not None)
        assert not (per_image and quality_map)
        self.m, self.B, self.base_only, self.rem_idx = m, B, base_only, rem_idx
        self.coder, self.up, self.up_at = coder, None, 0
        self.lanes = 1                                   # lanes per stream: decode() sets it per call
        self.interleaved = False                         # the lanes share one word stream: front() sets it
        self.per_image, self.quality_map = per_image, quality_map
        self.qtable = _mask_table_buffer(B, device) if per_image or quality_map else None
        self.level_map = torch.zeros((B, 16 * hz * wz), dtype=torch.uint8, device=device) if quality_map else None
        self.device = torch.device(device)
        self.pr = 0.0
        self.runner = E.Runner(device, cap=32)           # stream ordering; _ProgDecPlan's ("base",) graph
        h, w = hz * 4, wz * 4
        self.h, self.w, self.hz, self.wz = h, w, hz, wz
        d, ns = m.division_dimension[0], m.ns0
        table = m.gaussian_conditional.scale_table
        if table.numel() == 0:
            raise ValueError("empty scale table: call model.update() before decompress()")
        nv, ni = (lambda c, hh=h, ww=w: ops.new_view(B, hh, ww, c, device)), (lambda c, hh=h, ww=w: ops.new_iview(B, hh, ww, c, device))
        self.x_hat = torch.empty((B, 3, h * 16, w * 16), dtype=torch.float32, device=device)
        sc = self.sc = _SliceChain(m, lambda: nv(d), base_only, rem_idx)
        sl, heads = sc.sl, sc.heads
        self.rem_sig, self.ck, self.mu_b, self.std_b, self.heads, self.yb = sc.rem_sig, sc.ck, sc.mu_b, sc.std_b, heads, sc.yb
        # ---- z
        self.z_sym = ni(m.N, hz, wz)
        med = nv(m.N, hz, wz)
        med.buf.copy_(m.entropy_bottleneck._get_medians().detach().reshape(1, 1, 1, -1).expand_as(med.buf))
        z_hat = nv(m.N, hz, wz)
        P = self.p_hyper = E.Plan(device)
        P.call(lambda: ops.dequantize(self.z_sym, med, z_hat))                       # entropy_models.py:520-525
        means_h, scales_h = _lower_hyper_synthesis(P, m, z_hat, base_only)
        heads.update(_slice_stack_heads(P, m, means_h, scales_h, "base"))           # same association as the encoder's plan
        if not base_only:
            heads.update(_slice_stack_heads(P, m, means_h, scales_h, "prog"))
        # ---- base slices
        self.idx_b, self.sym_b = ni(d), ni(d)
        self.p_base = []
        for i in range(ns):
            Pa, Pb = E.Plan(device), E.Plan(device)
            sc.lower_base_params(Pa, [i])
            Pa.call(lambda i=i: ops.build_indexes(sl(sc.std_b, i), table, out=sl(self.idx_b, i)))        # pic.py:879
            Pb.call(lambda i=i: ops.dequantize(sl(self.sym_b, i), sl(sc.mu_b, i), sl(sc.yq, i)))         # pic.py:884
            sc.lower_base_lrp(Pb, [i])
            self.p_base.append((Pa, Pb))
        self.p_syn = E.Plan(device)
        if base_only:
            E.lower_g_s(self.p_syn, [m.g_s[0] if m.multiple_decoder else m.g_s], [sc.yb], [self.x_hat])
        else:
            self._lower_progressive()       # a stage _ProgDecPlan replaces: it may read only what is set above this line

    def _lower_progressive(self):
        """The progressive slices, each cut around its host decode like the base slices, and g_s[1]."""
        m, sc, sl, device, d = self.m, self.sc, self.sc.sl, self.device, self.m.division_dimension[0]
        table = m.gaussian_conditional.scale_table
        self.idx_p, self.sym_p = (ops.new_iview(self.B, self.h, self.w, d, device) for _ in range(2))
        self.p_prog = []
        for j in range(m.ns0):
            Pa, Pb = E.Plan(device), E.Plan(device)
            ms = sc.lower_prog_params(Pa, j)
            if self.rem_idx is not None:
                sc.lower_rem(Pa, self, [j])
            Pa.call(lambda j=j: _vmask(self.qtable, self.pr, sl(sc.std_f, j), sl(sc.mask, j), 1, level_map=self.level_map))   # pic.py:942
            Pa.call(lambda j=j: ops.build_indexes(sl(sc.std_f, j), table, mask=sl(sc.mask, j), out=sl(self.idx_p, j)))  # :945
            Pb.call(lambda j=j: ops.dequantize(sl(self.sym_p, j), sl(sc.mu_f, j), sl(sc.rq, j)))                  # :948
            sc.lower_prog_lrp(Pb, [j], sc.heads, [ms], sc.rq, sc.yb, sc.yp)
            self.p_prog.append((Pa, Pb))
        E.lower_g_s(self.p_syn, [m.g_s[1] if m.multiple_decoder else m.g_s], [sc.yp], [self.x_hat])

    def _decode_slice(self, strings, idx_view: ops.IView, sym_view: ops.IView, tables, C, name: str = "slice"):
        """indexes GPU -> host, rANS decode per image, symbols host -> GPU (NHWC window).  ``name`` words the slice in the
        refusal of an interleaved string."""
        from . import bitstream as bs
        if self.coder == "device":       # the B strings of this slice are the next B uploaded ones: one launch, no round trip
            tg = bs.DeviceCoderTables.of(self.m.gaussian_conditional, self.device)
            if self.interleaved:
                bs.decode_window_interleaved_uploaded(self.up, self.up_at, idx_view, sym_view, 1, C, tg, self.lanes)
            else:
                bs.decode_uploaded(self.up, self.up_at, idx_view, sym_view, 1, C, tg, lanes=self.lanes)
            self.up_at += self.B
            return
        B, h, w = self.B, idx_view.buf.shape[1], idx_view.buf.shape[2]
        self.runner.stream.synchronize()
        idx = idx_view.buf[..., idx_view.c0:idx_view.c0 + C].cpu().numpy()          # [B,h,w,C]
        out = np.empty((B, h, w, C), dtype=np.int32)
        for b in range(B):
            dec = self._host_decode(strings[b], idx[b].transpose(2, 0, 1), tables, f"base stream (image {b}, {name})")   # stream order [C,h,w]
            out[b] = dec.reshape(C, h, w).transpose(1, 2, 0)
        sym_view.buf[..., sym_view.c0:sym_view.c0 + C].copy_(torch.from_numpy(out).to(self.device))

    def _host_decode(self, string, idx, tables, what: str = "stream"):
        from . import bitstream as bs
        if self.interleaved:             # the tolerant decode, the whole stream required
            return bs.decode_interleaved_strict(string, idx, tables, self.lanes, what)
        return bs.decode(string, idx, tables) if self.lanes == 1 else bs.decode_lanes(string, idx, tables, self.lanes)

    def _decode_base(self, y_strings, z_strings, tg, te):
        """z (host decode) -> hyper-synthesis -> base slices, each slice's symbols decoded on the host; on the runner's
        stream."""
        from . import bitstream as bs
        m = self.m
        if self.coder == "device":       # z: the first B uploaded strings, table index = channel
            tz = bs.DeviceCoderTables.of(m.entropy_bottleneck, self.device)
            if self.interleaved:
                bs.decode_window_interleaved_uploaded(self.up, 0, None, self.z_sym, 1, m.N, tz, self.lanes)
            else:
                bs.decode_uploaded(self.up, 0, None, self.z_sym, 1, m.N, tz, lanes=self.lanes)
            self.up_at = self.B
        else:
            zi = np.broadcast_to(np.arange(m.N, dtype=np.int32)[:, None, None], (m.N, self.hz, self.wz))
            zs = np.stack([self._host_decode(z_strings[b], zi, te, f"z stream (image {b})").reshape(m.N, self.hz, self.wz).transpose(1, 2, 0)
                           for b in range(self.B)])
            self.z_sym.buf.copy_(torch.from_numpy(zs).to(self.device))
        self.p_hyper.run()
        self._run_slices(self.p_base, y_strings, self.idx_b, self.sym_b, tg)

    def _run_slices(self, pairs, strings, idx: ops.IView, sym: ops.IView, tg):
        """Slice by slice: entropy parameters and indexes, the host's rANS decode, then dequantisation and LRP."""
        for i, (Pa, Pb) in enumerate(pairs):
            Pa.run()
            self._decode_slice(strings[i], self.sc.sl(idx, i), self.sc.sl(sym, i), tg, self.m.dim_chunk, f"slice {i}")
            Pb.run()

    def decode(self, strings, pr, checkpoint_rep, quality_map=None, lanes: int = 1):
        """``pr``: the mask quality, or (per_image plans) one per image; ``quality_map`` (quality_map plans): (levels per
        image, uint8 index map [B, h, w] on the host), and ``pr`` is not read.  ``lanes``: the lanes per stream of every y
        and z string (model.coder_lanes at this call); nothing of the plan depends on it."""
        from . import bitstream as bs
        m = self.m
        self.lanes = bs.check_lanes(lanes)
        if self.quality_map:
            levels, index = quality_map
            assert len(levels) == self.B
            with self.runner.on_stream():
                _fill_quality_map(self.qtable, self.level_map, levels, index, self.h * self.w, m.dim_chunk)
        elif self.per_image:
            assert len(pr) == self.B
            with self.runner.on_stream():
                _fill_mask_table(self.qtable, [[p_] for p_ in pr], self.h * self.w, m.dim_chunk)
        else:
            self.pr = float(pr)
        y_strings, z_strings = strings[0], strings[1]
        n_need = m.ns0 if self.base_only else m.ns1
        if len(y_strings) < n_need or len(z_strings) != self.B:
            raise ValueError(f"expected {n_need} slice streams x {self.B} images, got {len(y_strings)} x {len(z_strings)}")
        tg, te = bs.Tables.of(m.gaussian_conditional), bs.Tables.of(m.entropy_bottleneck)
        if self.coder == "device" and any(len(row) != self.B for row in y_strings[:n_need]):
            raise ValueError(f"expected {self.B} strings per slice")
        with self.runner.on_stream():
            if self.coder == "device":   # one upload: z first, then the slices in decoding order
                self.up = bs.upload_streams(list(z_strings) + [s_ for row in y_strings[:n_need] for s_ in row], self.device, self.lanes)
            if checkpoint_rep is not None:
                _load_checkpoint(self.ck, checkpoint_rep)
            self._decode_base(y_strings, z_strings, tg, te)
            if not self.base_only:
                self._run_slices(self.p_prog, y_strings[m.ns0:], self.idx_p, self.sym_p, tg)
            self.p_syn.run()
        x_hat = self.x_hat.clone()
        if self.coder == "device":       # the one read of the status codes: string k is z of image k, then slice-major
            up, self.up, B = self.up, None, self.B
            bs.check_status(up, B, "decompress", lambda k: f"z stream (image {k})" if k < B else
                            f"stream (image {k % B}, slice {k // B - 1})")
        return x_hat

    def close(self):
        self.runner.close()


class _ProgDecPlan(_DecPlan):
    """progressive.ProgressiveDecoder for one (B, z-shape, quality list) (all_scalable): _DecPlan's z,
    hyper-synthesis and base slices with their host round trips, then the progressive (mu, sigma) chain with no mask and
    no host round trip — with all_scalable it reads only y_hat_base and its own history (pic.py:586-612) —, the container
    layer id of every element (vam_variance_layers on the chain's sigma) and the unmasked table indexes
    (src/test/utils.py:35-54, functions_decode.py:186-203).  ``sweep_parts`` feeds _SweepTail in decode mode: level g is
    the decoded symbols of the layers <= ks[g], + mu, then the LRP stacks and g_s[1]; ``p_syn`` is level 0 (g_s[0])."""

    def __init__(self, m, B, hz, wz, q_list, device, coder: str = "host"):
        """``coder`` "device" (DESIGN section 9p): z and the base slices are decoded by the device coder as in _DecPlan, and
        the decoder hands the layers to ``sym`` with one layered launch per level request."""
        self.q_list = tuple(float(q) for q in q_list)      # before super().__init__: it runs _lower_progressive, which reads it
        super().__init__(m, B, hz, wz, False, None, device, coder=coder)
        self.tails: Dict[int, _SweepTail] = {}
        self.owner = None                   # the ProgressiveDecoder whose base and chain the buffers hold

    def _lower_progressive(self):
        m, sc, B, h, w, device = self.m, self.sc, self.B, self.h, self.w, self.device
        d, ns, mu_p, std_p = m.division_dimension[0], m.ns0, sc.mu_p, sc.std_p
        E.lower_g_s(self.p_syn, [m.g_s[0] if m.multiple_decoder else m.g_s], [sc.yb], [self.x_hat])       # level 0
        P = self.p_chain = E.Plan(device)
        sc.lower_param_chain(P)
        self.layer = torch.empty((B, h, w, d), dtype=torch.uint8, device=device)
        self.idx_l, self.sym = ops.new_iview(B, h, w, d, device), ops.new_iview(B, h, w, d, device)
        P.keep += [self.layer, self.idx_l.buf, self.sym.buf]
        P.call(lambda: ops.variance_layers(std_p, self.q_list, self.layer, n_slice=ns), "container layers")
        P.call(lambda: ops.build_indexes(std_p, m.gaussian_conditional.scale_table, out=self.idx_l))   # functions_decode.py:179-180
        self.sweep_parts = dict(heads=sc.heads, yb=sc.yb, mu=mu_p, std=std_p, mu_tot=sc.mu_tot, sym=self.sym, layer=self.layer,
                                g_s=m.g_s[1] if m.multiple_decoder else m.g_s)

    def front(self, y_strings, z_strings, lanes: int = 1, interleaved: bool = False):
        """Base slices (host round trips) and the progressive chain, layer ids and indexes of every image.  ``lanes``: the
        lanes per stream of every string; ``interleaved``: they share one word stream (bitstream.encode_interleaved, DESIGN
        section 9t) and every string is needed whole — ValueError on the host coder, status 1 on the device — where the
        default is the lane-split string of section 9o.  Device coder: z and the base go up in one copy, no round trip
        follows, the symbol window is zeroed, and the upload is returned for the caller to read its status codes later
        (host: None)."""
        from . import bitstream as bs
        tg, te = bs.Tables.of(self.m.gaussian_conditional), bs.Tables.of(self.m.entropy_bottleneck)
        self.lanes, self.interleaved = bs.check_lanes(lanes), bool(interleaved)
        with self.runner.on_stream():
            if self.coder == "device":            # an interleaved string has one status code, whatever its lanes
                self.up = bs.upload_streams(list(z_strings) + [s_ for row in y_strings for s_ in row], self.device,
                                            1 if self.interleaved else self.lanes)
            self._decode_base(y_strings, z_strings, tg, te)
            self.p_chain.run()
            if self.coder == "device":
                self.sym.buf.zero_()
        up, self.up = self.up, None
        return up

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


class _EmbDecPlan(_ProgDecPlan):
    """embedded.EmbeddedDecoder for one (B, z-shape) (all_scalable): _ProgDecPlan with the rank order
    of the chain's sigma (vam_variance_rank) where the parent assigns container layers, and the unmasked table indexes in
    that order for the host's prefix decode.  It owns ``perm``, the ranked symbols, one count table per group size and the
    layer-id buffer that turns a caller's qualities into counts on the device (vam_variance_layers on the same sigma, then
    vam_rank_counts: count = #(layer id <= k) per segment).  A tail is vam_rank_scatter — the ranked symbols below each
    level's count back to the NHWC view, with the level ids in ``layer`` — and then the parent's _SweepTail in decode mode
    with the fixed cut-offs 0 .. G-1.  The count table is a graph input, copied before the replay on the runner's stream
    and outside any capture, so the plan keeps ONE hipGraph per group size whatever the cuts.

    ``scheduled``: the rank order is the scheduled one — vam_variance_layers_per_image on the schedule's
    levels, vam_stage_ids, vam_variance_rank_staged — from three device buffers (embedded.schedule_buffers) that
    :meth:`fill_schedule` refills on the runner's stream before the chain runs and outside any capture.  The tails read
    ``perm`` and counts only, so they, and their one graph per group size, are the plain plan's whatever the schedule."""

    def __init__(self, m, B, hz, wz, device, coder: str = "host", scheduled: bool = False):
        """``coder`` "device" (DESIGN section 9q): z and the base slices are decoded by the device coder as in _ProgDecPlan,
        and the decoder prefix-decodes the embedded strings from ``idx_r`` into ``ranked`` with one launch."""
        self.scheduled = bool(scheduled)                   # before super().__init__: it runs _lower_progressive, which reads it
        super().__init__(m, B, hz, wz, (), device, coder=coder)
        self.counts: Dict[int, torch.Tensor] = {}          # group size -> int32 [G, B, ns], the tails' graph input

    def _lower_progressive(self):
        m, sc, B, h, w, device = self.m, self.sc, self.B, self.h, self.w, self.device
        d, ns, mu_p, std_p = m.division_dimension[0], m.ns0, sc.mu_p, sc.std_p
        n = m.dim_chunk * h * w
        E.lower_g_s(self.p_syn, [m.g_s[0] if m.multiple_decoder else m.g_s], [sc.yb], [self.x_hat])       # level 0
        P = self.p_chain = E.Plan(device)
        sc.lower_param_chain(P)
        self.layer = torch.full((B, h, w, d), L.LAYER_NONE, dtype=torch.uint8, device=device)    # the tails' level ids
        self.qlayer = torch.empty((B, h, w, d), dtype=torch.uint8, device=device)                # a quality list's layers
        self.idx_l, self.sym = ops.new_iview(B, h, w, d, device), ops.new_iview(B, h, w, d, device)
        self.perm = torch.empty((B, ns, n), dtype=torch.int32, device=device)
        self.ranked = torch.zeros((B, ns, n), dtype=torch.int32, device=device)                  # decoded symbols, rank order
        self.idx_r = torch.empty((B, ns, n), dtype=torch.int32, device=device)                   # table indexes, rank order
        self.rank_ws = ops.rank_workspace(std_p, ns, device)
        P.keep += [self.layer, self.qlayer, self.idx_l.buf, self.sym.buf, self.perm, self.ranked, self.idx_r, self.rank_ws]
        if self.scheduled:
            from .embedded import schedule_buffers
            self.sched_table, self.stage_map, self.n_stages = schedule_buffers(B, h * w, device)
            self.stage = torch.empty((B, h, w, d), dtype=torch.uint8, device=device)             # stage id of every element
            P.keep += [self.sched_table, self.stage_map, self.n_stages, self.stage]
            P.call(lambda: ops.variance_layers_table(std_p, self.sched_table, self.qlayer, n_slice=ns), "schedule layers")
            P.call(lambda: ops.stage_ids(self.qlayer, self.stage_map, self.n_stages, self.stage), "stage ids")
            P.call(lambda: ops.variance_rank_staged(std_p, self.stage, self.perm, n_slice=ns, workspace=self.rank_ws),
                   "scheduled rank order")
        else:
            P.call(lambda: ops.variance_rank(std_p, self.perm, n_slice=ns, workspace=self.rank_ws), "rank order")
        P.call(lambda: ops.build_indexes(std_p, m.gaussian_conditional.scale_table, out=self.idx_l))   # functions_decode.py:179-180
        P.call(lambda: ops.rank_gather(self.perm, ns, self.idx_l, self.idx_r), "indexes in rank order")
        self.sweep_parts = dict(heads=sc.heads, yb=sc.yb, mu=mu_p, std=std_p, mu_tot=sc.mu_tot, sym=self.sym, layer=self.layer,
                                g_s=m.g_s[1] if m.multiple_decoder else m.g_s)

    def quality_counts(self, qs: Sequence[float]) -> torch.Tensor:
        """int32 [len(qs), B, ns] on the device: how many leading elements of every segment's rank order the mask of each
        quality of the non-decreasing list ``qs`` (up to L.VAM_MAX_LAYER_LEVELS) keeps, from the decoder's own sigma."""
        ns = self.m.ns0
        count = torch.empty((len(qs), self.B, ns), dtype=torch.int32, device=self.device)
        with self.runner.on_stream():
            ops.variance_layers(self.sc.std_p, [float(q) for q in qs], self.qlayer, n_slice=ns)
            ops.rank_counts(self.qlayer, self.perm, ns, len(qs), count)
        return count

    def fill_schedule(self, levels, index):
        """Refill the scheduled plan's inputs from embedded.check_schedule's (levels, index [B, L, h, w]): on the runner's
        stream, before :meth:`front` runs the chain that reads them, outside any capture."""
        from .embedded import fill_schedule
        assert self.scheduled and len(levels) == self.B
        with self.runner.on_stream():
            fill_schedule(self.sched_table, self.stage_map, self.n_stages, levels, index, self.h * self.w, self.m.dim_chunk)

    def stage_counts(self, n_stages: int) -> torch.Tensor:
        """int32 [n_stages, B, ns] on the device: #(stage id <= k) per segment, the prefix of the scheduled order that
        stage k's map keeps."""
        ns = self.m.ns0
        count = torch.empty((n_stages, self.B, ns), dtype=torch.int32, device=self.device)
        with self.runner.on_stream():
            ops.rank_counts(self.stage, self.perm, ns, n_stages, count)
        return count

    def tail_counts(self, count, use_graph: bool) -> _SweepTail:
        """The tail of G = count.shape[0] levels, level g keeping the first count[g, b, j] ranked elements of every segment
        (int32 [G, B, ns], host or device, non-decreasing in g)."""
        G = int(count.shape[0])
        t = self.tails.get(G)
        if t is None:
            t = self.tails[G] = _SweepTail(self, G, decode=True)
            t.ks = tuple(range(G))
            self.counts[G] = torch.zeros((G, self.B, self.m.ns0), dtype=torch.int32, device=self.device)
        table = self.counts[G]

        def run():
            ops.rank_scatter(self.ranked, self.perm, table, G, self.m.ns0, self.sym, self.layer)
            t.plan.run()
        with self.runner.on_stream():
            table.copy_(torch.as_tensor(count, dtype=torch.int32).reshape(table.shape))
            t.runner.replay(("counts",), run, use_graph)
        return t
