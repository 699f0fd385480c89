"""Single-bitstream progressive container (second half): a base layer plus one
rANS layer per quality step, each layer carrying only the latents that the variance mask ADDS
between two consecutive qualities (``ProgMask(q_k) - ProgMask(q_{k-1})``).

Same container and call surface as the reference harness (src/test/functions_encode.py:15-198,
functions_decode.py:9-229, test/utils.py:16-54) so that ``demo.py`` can import these two functions
instead:  ``bitstreams = {"q_list", "shape", "z", "base", "progressive"}``.  Everything numeric goes
through the model's module-level surface (HIP kernels); this file is orchestration only.

Model variants: like the reference's harness this one follows ``multiple_encoder`` (functions_encode.py:78-83),
``multiple_decoder`` (functions_decode.py:107,224), ``multiple_hyperprior`` (test/utils.py:20-31) and any
``support_progressive_slices``; and like it, it is defined for ``delta_encode=True`` (functions_encode.py:113-114
names the residual only there) and ``all_scalable=True`` (the parameter chain of test/utils.py:35-54 never sees a mask).

:func:`encode_batch` and :class:`ProgressiveDecoder` write and read the same container for a batch of images on the fused
plans: with all_scalable the layers differ only in which elements they carry, so one front end and one
set of symbols serve every layer, and a decoded level equals ``forward_single_quality(x, q_k)`` bit for bit.
"""
from __future__ import annotations

import math
import os
import pickle
from typing import List, Optional, Sequence

import numpy as np
import torch

Q_LIST = [0.002, 0.05, 0.5, 0.75, 1, 1.5, 2, 2.5, 3, 4, 5, 5.5, 6, 6.6]     # functions_encode.py:11


def _prog_params(model, j, y_base_slices, mu_hist, std_hist, means_h, scales_h):
    """Entropy parameters of progressive slice j from the decoded base latents and the
    parameter history (test/utils.py:35-54)."""
    d = model.division_dimension[0]
    sup_m = model.determine_support(y_base_slices, j, mu_hist)
    sup_s = model.determine_support(y_base_slices, j, std_hist)
    mean_support = torch.cat([means_h[:, d:]] + sup_m, dim=1)
    scale_support = torch.cat([scales_h[:, d:]] + sup_s, dim=1)
    mu = model.cc_mean_transforms_prog[j](mean_support)
    scale = model.cc_scale_transforms_prog[j](scale_support)
    mu_t = mu + y_base_slices[j] if model.total_mu_rep else mu
    return mean_support, mu, mu_t, scale


def _refine(model, j, mu, scale, mu_base, std_base, y_checkpoints):
    """Optional REM refinement with every available checkpoint (functions_encode.py:126-141)."""
    for r, ck in enumerate(y_checkpoints):
        y_b = ck.chunk(10, 1)[j]
        ms_base = torch.cat([mu_base[j], std_base[j]], dim=1)
        ms_prog = torch.cat([mu, scale], dim=1) if model.mu_std else scale
        nxt = model.check_levels[r + 1] if r < model.num_rems - 1 else 10
        mu, scale = model.apply_latent_enhancement(j, model.check_levels[r], nxt, y_b, ms_base, ms_prog, mu, scale)
    return mu, scale


def _chain(model, y_hat_base, mu_base, std_base, means_h, scales_h, rems, y_checkpoints):
    ns = model.ns0
    yb = list(y_hat_base.chunk(ns, 1))
    mb, sb = list(mu_base.chunk(ns, 1)), list(std_base.chunk(ns, 1))
    mu_hist, std_hist, mus, scales, supports = [], [], [], [], []
    for j in range(ns):
        sup, mu, mu_t, scale = _prog_params(model, j, yb, mu_hist, std_hist, means_h, scales_h)
        if rems and y_checkpoints is not None:
            assert len(y_checkpoints) == model.num_rems
            mu, scale = _refine(model, j, mu, scale, mb, sb, y_checkpoints)
        mu_hist.append(mu_t)
        std_hist.append(scale)
        mus.append(mu)
        scales.append(scale)
        supports.append(sup)
    return yb, mus, scales, supports


def _check_variant(model):
    if not (model.delta_encode and getattr(model, "all_scalable", True)):
        raise NotImplementedError("the progressive container is defined for delta_encode=True and all_scalable=True "
                                  "(reference src/test/functions_encode.py:113-114, test/utils.py:35-54)")


def _synthesis(model, i):
    return model.g_s[i] if model.multiple_decoder else model.g_s


def encode(model, x_padded, save_path=None, rems=False, q_list: Sequence[float] = Q_LIST, y_checkpoints=None):
    """functions_encode.py:15-66.  Returns (bitstreams, [bits_z, bits_base, bits_per_layer])."""
    assert x_padded.shape[0] == 1, "the progressive container is per image (ProgMask squeezes batch 1)"
    _check_variant(model)
    with torch.no_grad():
        base = model.compress(x_padded, quality=0)
        bit = {"q_list": list(q_list), "shape": base["shape"], "z": base["strings"][1], "base": base["strings"][0]}
        bits_z = 8.0 * sum(len(s) for s in bit["z"])
        bits_base = 8.0 * sum(len(s[0]) for s in bit["base"])
        # residual latents and their parameters (functions_encode.py:79-160)
        y = torch.cat([model.g_a[0](x_padded), model.g_a[1](x_padded)], dim=1) if model.multiple_encoder else model.g_a(x_padded)
        means_h, scales_h, _ = model.compute_hyperprior(y)
        yb, mus, scales, _ = _chain(model, base["y_hat_base"], base["mean_base"], base["scale_base"], means_h, scales_h,
                                    rems, y_checkpoints)
        ys = y.chunk(model.num_slices, 1)
        gc = model.gaussian_conditional
        r_sym = torch.stack([gc.quantize((ys[model.ns0 + j] - ys[j]) - mus[j], "symbols") for j in range(model.ns0)]).squeeze(1)
        idx = torch.stack([gc.build_indexes(scales[j]).int() for j in range(model.ns0)]).squeeze(1)       # [10,32,h,w]
        layers, bits = [], []
        for k, q in enumerate(q_list):                                   # functions_encode.py:168-196
            q0 = 0 if k == 0 else q_list[k - 1]
            delta = model.masking.ProgMask(scales, q) - model.masking.ProgMask(scales, q0)
            streams = gc.compress(r_sym * delta, idx * delta, already_quantize=True)
            layers.append(streams)
            bits.append(8.0 * sum(len(s) for s in streams))
        bit["progressive"] = layers
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        with open(os.path.join(save_path, "bits.pkl"), "wb") as f:
            pickle.dump(bit, f)
    return bit, [bits_z, bits_base, bits]


def _decode_hyper(model, z_strings, shape, q_ind):
    """test/utils.py:16-33."""
    z_hat = model.entropy_bottleneck.decompress(z_strings, shape)
    if not model.multiple_hyperprior:          # one hyper-synthesis pair delivers the parameters of both halves
        return z_hat, model.h_mean_s(z_hat), model.h_scale_s(z_hat), [z_hat.shape[2] * 4, z_hat.shape[3] * 4]
    means = [model.h_mean_s[0](z_hat)]
    scales = [model.h_scale_s[0](z_hat)]
    if q_ind != 0:
        means.append(model.h_mean_s[1](z_hat))
        scales.append(model.h_scale_s[1](z_hat))
    return z_hat, torch.cat(means, 1), torch.cat(scales, 1), [z_hat.shape[2] * 4, z_hat.shape[3] * 4]


def _decode_base(model, strings, means_h, scales_h):
    """functions_decode.py:9-55."""
    d, gc = model.division_dimension[0], model.gaussian_conditional
    y_hat, mus, scales = [], [], []
    for i in range(model.ns0):
        sup = y_hat[:min(model.max_support_slices, i)]
        m_sup = torch.cat([means_h[:, :d]] + sup, dim=1)
        s_sup = torch.cat([scales_h[:, :d]] + sup, dim=1)
        mu, sc = model.cc_mean_transforms[i](m_sup), model.cc_scale_transforms[i](s_sup)
        rv = gc.decompress(strings[i], gc.build_indexes(sc)).reshape(mu.shape)
        yh = gc.dequantize(rv, mu)
        yh = yh + 0.5 * torch.tanh(model.lrp_transforms[i](torch.cat([m_sup, yh], dim=1)))
        y_hat.append(yh)
        mus.append(mu)
        scales.append(sc)
    return {"y_hat": torch.cat(y_hat, 1), "scale": torch.cat(scales, 1), "mu": torch.cat(mus, 1)}


def decode(model, bitstreams, q_ind=0, res_base=None, index_hat_slice=None, mean=None, z_data=None, entropy_data=None,
           y_checkpoints=None, rems=False):
    """functions_decode.py:58-229: decode the first ``q_ind`` progressive layers (0 = base only).
    ``z_data`` / ``res_base`` / ``entropy_data`` returned by a previous call can be passed back so
    that moving to the next quality only decodes the new layer's parameters once."""
    q_list, shape = bitstreams["q_list"], bitstreams["shape"]
    assert q_ind <= len(q_list)
    _check_variant(model)
    with torch.no_grad():
        if z_data is None:
            z_data = list(_decode_hyper(model, bitstreams["z"], shape, q_ind))
        z_hat, means_h, scales_h, y_shape = z_data
        if res_base is None:
            res_base = _decode_base(model, bitstreams["base"], means_h, scales_h)
        y_hat_base = res_base["y_hat"]
        if q_ind == 0:
            x_hat = _synthesis(model, 0)(y_hat_base).clamp_(0, 1)
            return {"x_hat": x_hat, "y_hat": y_hat_base, "mu": res_base["mu"], "scale": res_base["scale"],
                    "z_data": z_data, "res_base": res_base}
        if model.multiple_hyperprior and means_h.shape[1] == model.division_dimension[0]:     # z_data came from a q_ind == 0 call
            z_data = list(_decode_hyper(model, bitstreams["z"], shape, q_ind))
            z_hat, means_h, scales_h, y_shape = z_data
        gc = model.gaussian_conditional
        if entropy_data is None:
            yb, mus, scales, supports = _chain(model, y_hat_base, res_base["mu"], res_base["scale"], means_h, scales_h,
                                               rems, y_checkpoints)
            idx = torch.stack([gc.build_indexes(s).int() for s in scales]).squeeze(1)
            entropy_data = [torch.cat(mus, 1).squeeze(0), None, supports, scales, idx]
        mean, _, supports, scales, idx = entropy_data
        M, (h, w) = model.division_channel, y_shape
        acc = torch.zeros(M, h, w, device=mean.device)
        for k, q in enumerate(q_list[:q_ind]):                             # functions_decode.py:186-203
            q0 = 0 if k == 0 else q_list[k - 1]
            delta = model.masking.ProgMask(scales, q) - model.masking.ProgMask(scales, q0)
            sym = gc.decompress(bitstreams["progressive"][k], idx * delta)
            acc += sym.reshape(M, h, w) * delta.reshape(M, h, w)
        r_hat = (acc + mean).reshape(1, M, h, w).chunk(model.ns0, 1)
        yb = y_hat_base.chunk(model.ns0, 1)
        y_prog = []
        for j in range(model.ns0):                                         # functions_decode.py:209-220
            r = r_hat[j] + 0.5 * torch.tanh(model.lrp_transforms_prog[j](torch.cat([supports[j], r_hat[j]], dim=1)))
            y_prog.append(model.merge(r, yb[j]))
        y_prog = torch.cat(y_prog, 1)
        x_hat = _synthesis(model, 1)(y_prog)
    return {"x_hat": x_hat, "z_data": z_data, "entropy_data": entropy_data, "y_hat_base": y_hat_base, "y_prog": y_prog,
            "res_base": res_base}


# ---------------------------------------------------------------- batched container on the fused plans
_EAGER = "the eager harness (progressive.encode / progressive.decode)"


def check_q_list(q_list: Sequence[float]) -> List[float]:
    """A container's quality list: 1..VAM_MAX_LAYER_LEVELS qualities >= 0, non-decreasing (the variance masks are then
    nested, so each element belongs to exactly one layer)."""
    from . import _lib as L
    qs = [float(q) for q in q_list]
    if not 1 <= len(qs) <= L.VAM_MAX_LAYER_LEVELS:
        raise ValueError(f"q_list: 1..{L.VAM_MAX_LAYER_LEVELS} qualities, got {len(qs)}")
    if any(not (q >= 0.0) or math.isinf(q) for q in qs):
        raise ValueError(f"q_list: qualities must be finite and >= 0, got {qs}")
    if any(b < a for a, b in zip(qs, qs[1:])):
        raise ValueError(f"q_list must be non-decreasing (each layer adds the elements of the next quality), got {qs}")
    return qs


def q_list_for_bpps(model, x, target_bpps: Sequence[float]) -> List[float]:
    """The quality list of a container of ONE image whose level k lands at the k-th target: per target the largest
    quality whose estimated rate fits it (VarianceMaskingPIC.qualities_for_bpp), sorted and de-duplicated, as
    :func:`encode_batch` / :class:`ProgressiveDecoder` accept it.  Targets below the base rate are dropped (the base is
    level 0 of every container); the rates are the likelihood estimate, not coded bytes."""
    if x.shape[0] != 1:
        raise ValueError(f"q_list_for_bpps resolves one image's list (the qualities differ between images), got a batch of {x.shape[0]}")
    sol = model.qualities_for_bpp(x, [float(t) for t in target_bpps])
    qs = sorted({float(q) for q, ok in zip(sol["quality"][:, 0].tolist(), sol["reached"][:, 0].tolist()) if ok})
    if not qs:
        raise ValueError(f"no target of {list(target_bpps)} reaches the base rate of this image")
    return check_q_list(qs)


def container_sizes(model, x, q_list: Sequence[float] = Q_LIST) -> List[dict]:
    """What the containers of ``encode_batch(model, x, q_list)`` weigh, without encoding: per image
    {"z": [lo, hi], "base": [lo, hi], "progressive": [[lo, hi] per layer]} in bytes, with lo <= actual <= hi guaranteed
    for every group of streams.  One front end per sub-batch, one vam_variance_layers and one vam_coded_layer_bits
    launch; a layer's stream costs its elements' exact table prices plus the price of symbol 0 in table 0 for every other
    element.  The refusals are encode_batch's.  The brackets describe K = 1 containers, from either coder; a lane-split
    container (``encode_batch(..., lanes=K)``) adds a header and K - 1 final states to every stream."""
    from . import bitstream as bs
    from . import control
    _check_variant(model)
    _check_batched(model)
    qs = check_q_list(q_list)
    m = model
    out: List[dict] = []
    with torch.no_grad():
        control._prepare(m, what="container_sizes", need_tables=True, policy=False)
        for i0, i1, sw in control._fronts(m, x):
            st = sw.size_front(m.use_graph)
            acc = sw.size(qs, m.use_graph).cpu().numpy()
            st.base_sizes()
            (zl, zh), (bl, bh) = st._parts
            S = st.stream_bits(acc, len(qs), st.c_out_layer, cumulative=False)        # [b, ns, L]
            lo, hi = bs.stream_bytes(S, st.n_y)
            lo, hi = lo.sum(1), hi.sum(1)
            for b in range(i1 - i0):
                out.append({"z": [int(zl[b]), int(zh[b])], "base": [int(bl[b]), int(bh[b])],
                            "progressive": [[int(lo[b, k]), int(hi[b, k])] for k in range(len(qs))]})
    return out


def solve_q_list_for_bytes(layer_hi, fixed_hi: float, target_bytes: Sequence[float], q_tol: float = 1e-3, n_grid: int = 31):
    """The level-by-level arithmetic of :func:`q_list_for_bytes` on host numbers, no model and no GPU of its own.
    ``layer_hi(q_prev, qs)`` returns the upper size in bytes of ONE container layer that adds the elements between the
    masks of q_prev and of each q of ``qs`` (ascending, every q >= q_prev; q == q_prev is the empty layer, which still
    pays its stream overheads), non-decreasing in q; ``fixed_hi`` the upper size of z and the base.  The targets are taken
    in ascending order; level k gets the largest quality q_k in [q_{k-1}, 10] with
    fixed_hi + sum_{j<=k} layer_hi(q_{j-1}, q_j) <= target_k, found by successive refinement on grids of ``n_grid`` points
    (the bracket shrinks by n_grid per pass, as rate_search's).  A target that does not even admit the empty layer (or lies
    below the base) is dropped, and so is every target after the mask is full (q = 10).  Returns (qualities, the targets
    kept, the upper size up to each level)."""
    from .control import rate_search_grid, rate_search_passes, rate_search_step
    qs, kept, sizes = [], [], []
    q_prev, used = 0.0, float(fixed_hi)
    for t in sorted(float(t_) for t_ in target_bytes):
        if q_prev >= 10.0:
            break
        budget = t - used
        lo, r_lo = q_prev, float(np.asarray(layer_hi(q_prev, np.array([q_prev])), dtype=np.float64)[0])
        if t < fixed_hi or r_lo > budget:
            continue
        hi = 10.0
        for _ in range(rate_search_passes(q_tol, n_grid)):
            if not hi > lo:
                break
            pts = rate_search_grid(np.float64(lo), np.float64(hi), n_grid)               # ascending, the last one is hi
            r = np.asarray(layer_hi(q_prev, pts), dtype=np.float64)
            gq, gr = np.concatenate([[lo], pts]), np.concatenate([[r_lo], r])
            n_lo, n_rlo, n_hi, _, _ = rate_search_step(gq, gr, np.float64(budget))
            lo, r_lo, hi = float(n_lo), float(n_rlo), float(n_hi)
        used += r_lo
        q_prev = lo
        qs.append(lo)
        kept.append(t)
        sizes.append(used)
    return qs, kept, sizes


def q_list_for_bytes(model, x, target_bytes: Sequence[float], q_tol: float = 1e-3, return_targets: bool = False):
    """The quality list of a container of ONE image whose level k is guaranteed to fit the k-th byte budget:
    ``bits_up_to(c, k) / 8 <= target_k`` for the container c of ``encode_batch(model, x, q_list)``, with the largest such
    quality level by level (:func:`solve_q_list_for_bytes`): a layer's size depends on the previous cut, and every layer
    adds its own stream overheads.  Targets below the base (z + base slices) are dropped.  One front end; every
    refinement pass is one vam_variance_layers and one vam_coded_layer_bits launch.  ``return_targets``: also the targets
    kept, one per level.  The guarantee describes K = 1 containers (``lanes=1``, from either coder), not lane-split ones."""
    from . import _lib as L
    from . import bitstream as bs
    from . import control
    if x.shape[0] != 1:
        raise ValueError(f"q_list_for_bytes resolves one image's list (the qualities differ between images), got a batch of {x.shape[0]}")
    _check_variant(model)
    _check_batched(model)
    m = model
    with torch.no_grad():
        control._prepare(m, what="q_list_for_bytes", need_tables=True, policy=False)
        _, _, sw = next(control._fronts(m, x))                                    # one image: one sub-batch
        st = sw.size_front(m.use_graph)
        fixed_hi = float(st.base_sizes()[1][0])

        def layer_hi(q_prev, qs_):
            # slot 0 takes the elements the previous levels already carry; the layer up to qs_[i] is slots 1..i+1
            qs_ = [float(q) for q in np.asarray(qs_).reshape(-1)]
            acc = sw.size_eager([float(q_prev)] + qs_)[:, 0]                      # [2, ns, n + 2]
            S = st.stream_bits(acc[..., 1:], len(qs_), st.c_out_layer)            # cumulative over slots 1..
            return bs.stream_bytes(S, st.n_y)[1].sum(0)

        qs, kept, _ = solve_q_list_for_bytes(layer_hi, fixed_hi, target_bytes, q_tol,
                                             n_grid=min(31, L.VAM_MAX_LAYER_LEVELS - 1))
    if not qs:
        raise ValueError(f"no target of {list(target_bytes)} reaches the base size of this image ({fixed_hi:.0f} bytes and one layer)")
    qs = check_q_list(qs)
    return (qs, kept) if return_targets else qs


def container_bits(c) -> list:
    """[bits_z, bits_base, bits_per_layer] of one image's container (what :func:`encode` returns beside it)."""
    return [8.0 * sum(len(s) for s in c["z"]), 8.0 * sum(len(s[0]) for s in c["base"]),
            [8.0 * sum(len(s) for s in layer) for layer in c["progressive"]]]


def bits_up_to(c, k: int) -> float:
    """Bits a decoder reads for level k of container c: z, the base and layers 1..k (level 0 = the base)."""
    if not 0 <= k <= len(c["progressive"]):
        raise ValueError(f"level {k} outside 0..{len(c['progressive'])}")
    bz, bb, bl = container_bits(c)
    return bz + bb + sum(bl[:k])


def _check_batched(model):
    """What the plan-backed container needs beyond the eager one (_check_variant)."""
    from . import ops
    from .models import VarianceMaskingPICREM
    if isinstance(model, VarianceMaskingPICREM):
        raise NotImplementedError("batched progressive containers: REM models refine sigma with the checkpoints, so the layers "
                                  f"depend on them; use {_EAGER} with rems=True")
    if not (model.delta_encode and getattr(model, "all_scalable", True)):
        raise NotImplementedError("batched progressive containers are defined for delta_encode=True and all_scalable=True, as "
                                  f"the container itself (src/test/functions_encode.py:113-114); {_EAGER} refuses them too")
    if getattr(model, "storage", "fp32") != "fp32" or ops.f16x2_mode():
        raise NotImplementedError("batched progressive containers run in fp32 storage and the default bf16x3 arithmetic "
                                  "(encoder and decoder must agree bit for bit): not with bf16 storage or VAMPIC_CONV=f16x2; "
                                  f"use {_EAGER}")


def _check_coder(model, coder) -> str:
    """``coder`` None reads model.coder; anything but "host" / "device" is a ValueError."""
    if coder is None:
        return model._coder()
    if coder not in ("host", "device"):
        raise ValueError(f"coder is 'host' or 'device' (None: model.coder), got {coder!r}")
    return coder


def check_containers(containers):
    """(shape, q_list, lanes) shared by a batch of containers for one :class:`ProgressiveDecoder`: every container must have
    the same shape, quality list and ``"lanes"`` value (a container without the key is K = 1).  Host arithmetic only."""
    from . import bitstream as bs
    cs = list(containers)
    if not cs:
        raise ValueError("ProgressiveDecoder: no containers")
    shape, q0 = tuple(cs[0]["shape"]), [float(q) for q in cs[0]["q_list"]]
    for c in cs[1:]:
        if tuple(c["shape"]) != shape or [float(q) for q in c["q_list"]] != q0:
            raise ValueError("ProgressiveDecoder: every container must have the same shape and q_list, got "
                             f"{shape} / {q0} and {tuple(c['shape'])} / {list(c['q_list'])}; decode them separately")
    lanes = [bs.check_lanes(c.get("lanes", 1)) for c in cs]
    if any(k != lanes[0] for k in lanes):
        raise ValueError(f"ProgressiveDecoder: every container must have the same lanes per stream, got {sorted(set(lanes))}; "
                         "decode them separately")
    return shape, check_q_list(q0), lanes[0]


def _encode_batch_device(m, plan, layer, n_levels: int, lanes: int):
    """z, the base slices and all layers from the device coder: (z [image], base [slice][image], layers
    [level][slice][image]).  The progressive window of the plan's symbols and indexes is copied on the device into buffers
    of the layer ids' geometry; nothing but lengths, status codes and coded bytes comes to the host."""
    from . import bitstream as bs
    from . import ops
    d, C, ns = m.division_dimension[0], m.dim_chunk, m.ns0
    dev = plan.sym.buf.device
    tg, te = bs.DeviceCoderTables.of(m.gaussian_conditional, dev), bs.DeviceCoderTables.of(m.entropy_bottleneck, dev)
    z_str = bs.encode_streams_device(plan.z_sym, None, 1, m.N, te, lanes=lanes)[0]
    base = bs.encode_streams_device(plan.sym, plan.idx, ns, C, tg, lanes=lanes)
    win = lambda v: ops.IView(v.buf[..., v.c0 + d:v.c0 + 2 * d].contiguous(), 0, d)
    prog = bs.encode_layers_device(win(plan.sym), win(plan.idx), layer, n_levels, ns, C, tg, lanes=lanes, first_level=1)
    return z_str, base, prog


def encode_batch(model, x, q_list: Sequence[float] = Q_LIST, save_path=None, *, coder: Optional[str] = None, lanes: int = 1):
    """:func:`encode` for a batch x [B,3,H,W] (H, W multiples of 64, as for ``compress``) on the fused plans: the
    ``compress(x, 10)`` plan (symbols round(r - mu), unmasked indexes), then vam_variance_layers on its sigma assigns every
    element its layer.  Returns (containers, bits): per image the container of :func:`encode` and [bits_z, bits_base,
    bits_per_layer].

    ``coder`` (None: ``model.coder``): "host" brings the symbols, indexes, layer ids and z symbols to the host once and codes
    z, the base slices and the layers with the threaded stream coder; "device"  codes z and the base
    slices with one launch each and ALL layers with one more, and fetches lengths, status codes and coded bytes only.  The
    containers are the same byte for byte.  ``lanes`` = K > 1 splits every stream into K lanes on either
    coder; such a container carries ``"lanes": K`` (a K = 1 container has no such key) and is read from the argument only,
    never from ``model.coder_lanes``."""
    from . import _lib as L
    from . import bitstream as bs
    from . import ops
    from .models import EMPTY_SCALE_TABLE
    _check_variant(model)
    _check_batched(model)
    qs = check_q_list(q_list)
    coder, K = _check_coder(model, coder), bs.check_lanes(lanes)
    m = model
    B, _, H, W = x.shape
    d, C, ns = m.division_dimension[0], m.dim_chunk, m.ns0
    with torch.no_grad():
        L.require_gpu()
        m._check_config()
        plan = m._plan(x, base_only=False, symbols=True)
        if plan.idx is None:
            raise ValueError(EMPTY_SCALE_TABLE.format("encode_batch"))
        plan.execute(x, 10.0, None, m.use_graph, False)
        layer = torch.empty((B, H // 16, W // 16, d), dtype=torch.uint8, device=x.device)
        ops.variance_layers(plan.std_p, qs, layer, n_slice=ns)              # functions_encode.py:168-196's delta masks
        if coder == "device":
            z_str, base, prog = _encode_batch_device(m, plan, layer, len(qs), K)
        else:
            nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu().numpy()
            sym, idx, lay, zs = nchw(plan.sym.buf), nchw(plan.idx.buf), nchw(layer), nchw(plan.z_sym.buf)
    if coder == "host":
        tg, te = bs.Tables.of(m.gaussian_conditional), bs.Tables.of(m.entropy_bottleneck)
        zi = np.broadcast_to(np.arange(m.N, dtype=np.int32)[:, None, None], zs.shape[1:])
        z_str = bs.encode_streams([(zs[b], zi) for b in range(B)], te, lanes=K)
        sl = lambda a, b, i: a[b, i * C:(i + 1) * C]
        jobs = [(sl(sym, b, i), sl(idx, b, i)) for i in range(ns) for b in range(B)]
        jobs += [(sl(sym, b, ns + j), sl(idx, b, ns + j), sl(lay, b, j), k) for k in range(len(qs)) for j in range(ns) for b in range(B)]
        y_str = bs.encode_streams(jobs, tg, lanes=K)
        base = [y_str[i * B:(i + 1) * B] for i in range(ns)]
        prog = [[y_str[(ns + k * ns + j) * B:(ns + k * ns + j + 1) * B] for j in range(ns)] for k in range(len(qs))]
    containers, bits = [], []
    for b in range(B):
        c = {"q_list": list(q_list), "shape": (H // 64, W // 64), "z": [z_str[b]], "base": [[base[i][b]] for i in range(ns)],
             "progressive": [[prog[k][j][b] for j in range(ns)] for k in range(len(qs))]}
        if K > 1:
            c["lanes"] = K
        containers.append(c)
        bits.append(container_bits(c))
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        for b, c in enumerate(containers):
            with open(os.path.join(save_path, "bits.pkl" if B == 1 else f"bits_{b}.pkl"), "wb") as f:
                pickle.dump(c, f)
    return containers, bits


class ProgressiveDecoder:
    """Decodes the levels of a batch of containers (all of one shape, quality list and lanes per stream) on the fused plans.
    Level 0 is the base, level k (1 <= k <= len(q_list)) quality q_list[k-1]; each equals ``forward_single_quality(x, q)``
    bit for bit.  The base slices and the progressive (mu, sigma) chain run once; a layer's streams are entropy-decoded
    only the first time a level needs them (:attr:`layers_decoded`).

    ``coder`` (None: ``model.coder``): "host" decodes on the host's thread pool and copies the symbols up at each level
    request; "device"  uploads z and the base in one copy, and for a level request the strings of the
    layers it still needs in one more, decoded by ONE launch into the plan's symbol window; the status codes are read once
    per :meth:`decode_levels`, after the tail.  Either reads the other's containers."""

    def __init__(self, model, containers, coder: Optional[str] = None):
        _check_variant(model)
        _check_batched(model)
        cs = list(containers)
        shape, self.q_list, self.lanes = check_containers(cs)
        self.coder = _check_coder(model, coder)
        self.m, self.containers, self.B = model, cs, len(cs)
        from .control import _prepare, sweep_groups
        _prepare(model, policy=False)
        hz, wz = int(shape[0]), int(shape[1])
        self.H, self.W = 64 * hz, 64 * wz
        if len(sweep_groups(1, self.B, self.H, self.W)) > 1:
            raise NotImplementedError(f"ProgressiveDecoder: {self.B} images of {self.H}x{self.W} exceed one plan; decode "
                                      "the containers in smaller batches")
        self.dp = model._prog_dec_plan(self.B, hz, wz, self.q_list, self.coder)
        self._pending = []                   # device coder: (upload, first level or None for z + base) not yet checked
        self._front()
        if self.coder == "device":           # this decoder's own copy of the layers decoded so far, on the device
            self.sym = torch.zeros_like(self.dp.sym.buf)
        else:
            nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu().numpy()
            self.idx, self.layer = nchw(self.dp.idx_l.buf), nchw(self.dp.layer)
            self.sym = np.zeros(self.idx.shape, dtype=np.int32)          # [B, d, h, w]: the layers decoded so far
        self.layers_decoded = 0

    def _front(self):
        cs, ns = self.containers, self.m.ns0
        up = self.dp.front([[c["base"][i][0] for c in cs] for i in range(ns)], [c["z"][0] for c in cs], self.lanes)
        if up is not None:
            self._pending.append((up, None))
        self.dp.owner = self

    def _need(self, k: int):
        """Entropy-decode layers up to k and hand the symbols to the plans."""
        from . import bitstream as bs
        if not 0 <= k <= len(self.q_list):
            raise ValueError(f"level {k} outside 0..{len(self.q_list)}")
        restore = self.dp.owner is not self
        if restore:                                      # another decoder ran on the same plans since
            self._front()
        C, ns = self.m.dim_chunk, self.m.ns0
        if self.coder == "device":
            return self._need_device(k, restore)
        if k > self.layers_decoded:
            sl = lambda a, b, j: a[b, j * C:(j + 1) * C]
            jobs = [(c["progressive"][kk][j], sl(self.idx, b, j), sl(self.sym, b, j), sl(self.layer, b, j), kk)
                    for kk in range(self.layers_decoded, k) for j in range(ns) for b, c in enumerate(self.containers)]
            bs.decode_streams(jobs, bs.Tables.of(self.m.gaussian_conditional), lanes=self.lanes)
            self.layers_decoded = k
        self.dp.sym.buf.copy_(torch.from_numpy(self.sym).to(self.dp.device).permute(0, 2, 3, 1))

    def _need_device(self, k: int, restore: bool):
        """The plan's symbol window holds this decoder's layers: restored from its own copy after another decoder used the
        plans, then the layers [layers_decoded, k) in one upload and one launch.  No synchronisation."""
        from . import bitstream as bs
        dp, k0 = self.dp, self.layers_decoded
        with dp.runner.on_stream():
            if restore:
                dp.sym.buf.copy_(self.sym)
            if k > k0:
                strings = [c["progressive"][kk][j] for kk in range(k0, k) for j in range(self.m.ns0) for c in self.containers]
                up = bs.upload_streams(strings, dp.device, self.lanes)
                bs.decode_layers_uploaded(up, 0, dp.idx_l, dp.sym, dp.layer, k0, k - k0, self.m.ns0, self.m.dim_chunk,
                                          bs.DeviceCoderTables.of(self.m.gaussian_conditional, dp.device), self.lanes)
                self.sym.copy_(dp.sym.buf)
                self._pending.append((up, k0 + 1))
                self.layers_decoded = k

    def _check_pending(self):
        """The one read of the device coder's status codes.  After a failure the decoder starts over at its next call."""
        from . import bitstream as bs
        pending, self._pending, B = self._pending, [], self.B
        try:
            for up, first_level in pending:
                if first_level is None:      # string k is z of image k, then the base slices slice-major
                    bs.check_status(up, B, "ProgressiveDecoder", lambda k: f"z stream (image {k})" if k < B else
                                    f"base stream (image {k % B}, slice {k // B - 1})")
                else:
                    bs.check_layer_status(up, B, self.m.ns0, "ProgressiveDecoder", first_level)
        except Exception:
            self.layers_decoded = 0
            self.sym.zero_()
            self.dp.owner = None
            raise

    def decode_levels(self, ks: Sequence[int]) -> List[dict]:
        """{"x_hat", "y_hat"} of the batch for every level of ``ks``, the levels > 0 through the batched tail."""
        from .control import sweep_groups
        ks = [int(k) for k in ks]
        if not ks or min(ks) < 0:
            raise ValueError(f"levels must be >= 0, got {ks}")
        with torch.no_grad():
            self._need(max(ks))
            out: List[Optional[dict]] = [None] * len(ks)
            dp, use_graph = self.dp, self.m.use_graph
            if 0 in ks:
                dp.base(use_graph)
                for g, k in enumerate(ks):
                    if k == 0:
                        out[g] = {"x_hat": dp.x_hat.clone(), "y_hat": dp.yb.torch_nchw().clone()}
            lv = [g for g, k in enumerate(ks) if k > 0]
            for _, _, groups in sweep_groups(len(lv), self.B, self.H, self.W):
                for l0, l1 in groups:
                    gs = lv[l0:l1]
                    t = dp.tail([ks[g] - 1 for g in gs], use_graph)         # level k keeps the layers 0..k-1
                    for i, g in enumerate(gs):
                        out[g] = {"x_hat": t.x_hat[i * self.B:(i + 1) * self.B].clone(),
                                  "y_hat": t.level(t.y_prog, i).torch_nchw().clone()}
            if self._pending:
                self._check_pending()
        return out

    def decode(self, k: int) -> dict:
        """{"x_hat", "y_hat"} of level k for the batch (0 = base, k = quality q_list[k-1])."""
        return self.decode_levels([k])[0]

    def bits(self, k: int) -> List[float]:
        """Each image's bits up to level k."""
        return [bits_up_to(c, k) for c in self.containers]
