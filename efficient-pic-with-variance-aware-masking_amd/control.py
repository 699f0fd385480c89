"""Host-side drivers over the plans of ``plans.py``: the quality sweep, rate control (9h), coded-size
control (9i), per-image qualities (9j) and quality maps (9k).  The public methods of ``VarianceMaskingPIC`` delegate here (their docstrings
are the contracts); a function validates, splits the batch into sub-batches of one plan's worth, replays the plans and
does the host arithmetic.  ``models.MAX_PLAN_PIXELS`` is read through the module at call time, never bound by name."""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from . import layers as Ly
from . import models as M
from . import ops
from .plans import _DecPlan

_REM_RATE_REFUSAL = ("rate control on REM models: the rate at a quality q needs the checkpoint representation of q's "
                     "check level (the REM refines (mu, sigma) per level), so neither one front end nor one layer pass "
                     "gives the curve; call forward_single_quality(x, q, checkpoint_ref=...) per quality")
_REM_SIZE_REFUSAL = ("coded-size control on REM models: the symbols and indexes at a quality q depend on the checkpoint "
                     "representation of q's check level (the REM refines (mu, sigma) per level), so neither one front end "
                     "nor one layer pass prices them; call compress(x, q, checkpoint_rep=...) per quality")


# ----------------------------------------------------------------------------- shared skeletons
def _prepare(model, x=None, mask_pol=None, what=None, need_tables=False, policy=True, rem_refusal=None):
    """What every driver checks before GPU work; returns the resolved mask policy.  ``rem_refusal``: REM models are refused
    with it; ``x`` None skips the autograd check, ``policy`` False the policy (the progressive container has neither);
    ``need_tables``: the coder's tables, for ``what``()."""
    if rem_refusal and isinstance(model, M.VarianceMaskingPICREM):
        raise NotImplementedError(rem_refusal)
    if policy:
        mask_pol = model._mask_policy(mask_pol)
    if x is not None:
        Ly._no_autograd(x)
    L.require_gpu()
    model._check_config()
    if need_tables and model.gaussian_conditional.scale_table.numel() == 0:
        raise ValueError(M.EMPTY_SCALE_TABLE.format(what))
    return mask_pol


def _targets(target, B: int, what: str, noun: str = "number") -> np.ndarray:
    """float64 [T, B] from a number, T numbers (the same for every image) or a [T, B] tensor."""
    tg = np.atleast_1d(torch.as_tensor(target, dtype=torch.float64).cpu().numpy())
    if tg.ndim == 1:
        tg = np.repeat(tg[:, None], B, axis=1)
    if tg.ndim != 2 or tg.shape[1] != B:
        raise ValueError(f"{what}: a {noun}, T {noun}s or a [T, {B}] tensor, got shape {tuple(tg.shape)}")
    return tg


def sweep_groups(n_levels: int, B: int, H: int, W: int) -> List[tuple]:
    """How a rate sweep over ``n_levels`` qualities (q != 0) of B images of HxW runs: [(i0, i1, [(l0, l1), ...]), ...].
    Images are split into sub-batches of at most one plan's worth (``_max_images_per_plan``), as forward_single_quality
    splits them; the levels of a sub-batch of b images run in groups of at most min(VAM_MAX_MASK_LEVELS, nb // b) levels,
    so that a group's level batch (levels * b images) fits one plan and its masks one vam_variance_mask_levels launch."""
    nb = max(1, M.MAX_PLAN_PIXELS // (H * W))
    out = []
    for i0 in range(0, B, nb):
        b = min(nb, B - i0)
        g = max(1, min(L.VAM_MAX_MASK_LEVELS, nb // b))
        out.append((i0, i0 + b, [(l0, min(l0 + g, n_levels)) for l0 in range(0, n_levels, g)]))
    return out


def _fronts(model, x):
    """(i0, i1, sweep plan) per sub-batch of ``x``, the front end of x[i0:i1] just run.  A generator: sub-batches of equal
    shape share one cached plan, so the caller is done with its buffers before it asks for the next."""
    for i0, i1, _ in sweep_groups(0, x.shape[0], x.shape[2], x.shape[3]):
        xb = x[i0:i1].detach()
        sw = model._sweep_plan(xb)
        sw.front(xb, model.use_graph)
        yield i0, i1, sw


def _distinct_levels(prs, G: int):
    """(chunks, rows, cols) of the mask qualities ``prs``: the sorted distinct positive ones in chunks of at most ``G``,
    and for every positive entry its row in ``prs`` and its column among the concatenated chunks.  No positive entry: no
    chunk, so no launch."""
    levels = sorted({p_ for p_ in prs if p_ != 0})
    col = {p_: j for j, p_ in enumerate(levels)}
    rows = np.array([k for k, p_ in enumerate(prs) if p_ != 0], dtype=np.int64)
    cols = np.array([col[p_] for p_ in prs if p_ != 0], dtype=np.int64)
    return [levels[l0:l0 + G] for l0 in range(0, len(levels), G)], rows, cols


def _points(q, need, same, own):
    """A solver curve on host arrays: values at the points q [T, B, n] wanted by ``need`` (0 elsewhere).  Each image's
    sorted distinct points are evaluated once: by ``same(points) -> [B, n_points]`` when all images ask for the same ones,
    else by ``own([points of image b]) -> [values of image b]``; by neither when no point is wanted."""
    B = q.shape[1]
    pts, inv = zip(*(np.unique(q[:, b][need[:, b]], return_inverse=True) for b in range(B)))
    out = np.zeros(q.shape)
    if not max(u.size for u in pts):
        return out
    vals = same(pts[0]) if all(np.array_equal(u, pts[0]) for u in pts) else own(list(pts))
    for b in range(B):
        out[:, b][need[:, b]] = np.asarray(vals[b])[inv[b]]
    return out


def _quality_sub_batches(qs, nb: int):
    """(base_only, image ids) per plan run of a batch with one quality per image: the images at quality 0 first (the base
    plan), then the positive ones, each in runs of at most ``nb``."""
    for base_only in (True, False):
        ids = [b for b, q in enumerate(qs) if (q == 0) == base_only]
        for i in range(0, len(ids), nb):
            yield base_only, ids[i:i + nb]


def _mask_qualities(mask_pol, qs) -> List[float]:
    return [float(M._mask_quality(mask_pol, q)) for q in qs]


# ----------------------------------------------------------------------------- the sweep
def _sweep(model, x, qualities, mask_pol, emit, per_image: bool = False):
    """Run the sweep over ``qualities`` and hand each result to ``emit(i0, i1, sweep_plan, tail, ks)`` while its buffers hold
    it (the next group overwrites them): images i0..i1 of x; ``tail`` None = the base reconstruction (the entries ks of
    ``qualities`` equal to 0), else a _SweepTail whose level g is quality ``qualities[ks[g]]``.  ``emit`` runs on the caller's
    stream, after its group and before the next one.  ``per_image``: every entry of ``qualities`` is a row of B qualities;
    the base is emitted for the rows that hold a 0 anywhere, a tail level for the rows that hold a positive quality
    anywhere (a 0 inside such a row masks everything out: the caller takes that image from the base)."""
    mask_pol = _prepare(model, x, mask_pol)
    row = (lambda r: r) if per_image else (lambda q: (q,))
    lv = [k for k, r in enumerate(qualities) if any(q != 0 for q in row(r))]
    zeros = [k for k, r in enumerate(qualities) if any(q == 0 for q in row(r))]
    B, _, H, W = x.shape
    level_groups = [groups for _, _, groups in sweep_groups(len(lv), B, H, W)]
    for (i0, i1, sw), groups in zip(_fronts(model, x), level_groups):
        if zeros:
            sw.base(model.use_graph)
            emit(i0, i1, sw, None, zeros)
        for l0, l1 in groups:
            ks = lv[l0:l1]
            if per_image:
                t = sw.tail_per_image([_mask_qualities(mask_pol, qualities[k][i0:i1]) for k in ks], model.use_graph)
            else:
                t = sw.tail(_mask_qualities(mask_pol, [qualities[k] for k in ks]), model.use_graph)
            emit(i0, i1, sw, t, ks)


def _sweep_dicts(model, parts: List[list]):
    """An ``emit`` for :func:`_sweep` that appends to ``parts[k]`` the result dict of entry k for each sub-batch."""
    d = model.division_dimension[0]

    def emit(i0, i1, sw, t, ks):
        fp = sw.fp
        nchw = lambda v: v.torch_nchw().clone()
        for g, k in enumerate(ks):
            if t is None:                                           # pic.py:558: the base reconstruction
                yh = nchw(fp.y_base)
                parts[k].append({"x_hat": fp.x_hat.clone(), "likelihoods": {"y": nchw(fp.lik.window(0, d)), "z": nchw(fp.z_lik)},
                                 "log2_likelihood_sum": fp.log2sum.clone(), "y_hat": yh, "y_base": yh, "y_prog": yh,
                                 "mu": nchw(fp.mu_b), "std": nchw(fp.std_b), "mu_base": nchw(fp.mu_b), "std_base": nchw(fp.std_b),
                                 "mu_prog": [], "std_prog": []})
                continue
            ls = fp.log2sum.clone()
            ls[0] += t.log2sum[g]
            yh = nchw(t.level(t.y_prog, g))
            parts[k].append({"x_hat": t.x_hat[g * t.B:(g + 1) * t.B].clone(),
                             "likelihoods": {"y": torch.cat([fp.lik.window(0, d).torch_nchw(), t.level(t.lik, g).torch_nchw()], 1),
                                             "z": nchw(fp.z_lik)},
                             "log2_likelihood_sum": ls, "y_hat": yh, "y_base": nchw(fp.y_base), "y_prog": yh, "mu_base": nchw(fp.mu_b),
                             "mu": nchw(fp.mu_p), "std_base": nchw(fp.std_b), "std": nchw(fp.std_p),
                             "mask": nchw(t.level(t.mask, g))})
    return emit


def _swept(model, x, qualities, mask_pol, per_image: bool):
    parts: List[list] = [[] for _ in qualities]
    _sweep(model, x, qualities, mask_pol, _sweep_dicts(model, parts), per_image)
    return [p_[0] if len(p_) == 1 else M._cat_outputs(p_) for p_ in parts]


def forward_qualities(model, x, qualities, mask_pol=None):
    qualities = list(qualities)
    mask_pol = model.mask_policy if mask_pol is None else mask_pol
    if not model._sweep_eligible():
        return [model.forward_single_quality(x, q, mask_pol, training=False) for q in qualities]
    return _swept(model, x, qualities, mask_pol, per_image=False)


# ----------------------------------------------------------------------------- per-image qualities
def _quality_vector(x, qualities, what, allow_zero: bool) -> List[float]:
    qs = [float(q) for q in (qualities.tolist() if torch.is_tensor(qualities) else list(qualities))]
    if len(qs) != x.shape[0]:
        raise ValueError(f"{what}: one quality per image, got {len(qs)} for a batch of {x.shape[0]}")
    bad = [q for q in qs if not q >= 0]
    if bad:
        raise ValueError(f"{what}: qualities must be >= 0 (and not NaN), got {bad[0]}")
    zero = [b for b, q in enumerate(qs) if q == 0]
    if zero and not allow_zero:
        raise ValueError(f"{what}: quality 0 runs the base plan (other transforms): split the batch, e.g. "
                         f"forward_single_quality(x[zero], 0) for zero = {zero} and {what} for the rest")
    return qs


def forward_per_image(model, x, qualities, mask_pol=None):
    qs = _quality_vector(x, qualities, "forward_per_image", allow_zero=False)
    mask_pol = model.mask_policy if mask_pol is None else mask_pol
    if not model._batch_shareable():
        return M._cat_outputs([model.forward_single_quality(x[b:b + 1], q, mask_pol, training=False) for b, q in enumerate(qs)])
    mask_pol = _prepare(model, x, mask_pol)
    nb = M._max_images_per_plan(x)
    outs = []
    for i in range(0, x.shape[0], nb):
        xb = x[i:i + nb].detach()
        plan = model._plan(xb, base_only=False, per_image=True)
        outs.append(plan.execute_per_image(xb, _mask_qualities(mask_pol, qs[i:i + nb]), model.use_graph, True))
    return outs[0] if len(outs) == 1 else M._cat_outputs(outs)


def forward_qualities_per_image(model, x, Q, mask_pol=None):
    Qt = torch.as_tensor(Q, dtype=torch.float64).cpu()
    if Qt.dim() == 1:
        Qt = Qt.unsqueeze(0)
    if Qt.dim() != 2 or Qt.shape[1] != x.shape[0]:
        raise ValueError(f"forward_qualities_per_image: Q is [T, {x.shape[0]}] (or one row of {x.shape[0]}), got shape {tuple(Qt.shape)}")
    if not bool((Qt >= 0).all()):
        raise ValueError("forward_qualities_per_image: qualities must be >= 0 (and not NaN)")
    rows = Qt.tolist()
    for t, row in enumerate(rows):
        if any(q == 0 for q in row) and any(q != 0 for q in row):
            raise ValueError(f"forward_qualities_per_image: row {t} mixes quality 0 (the base plan) with positive "
                             "qualities; a row is all zero or all positive")
    mask_pol = model.mask_policy if mask_pol is None else mask_pol
    if not model._sweep_eligible():
        return [model.forward_single_quality(x, 0, mask_pol, training=False) if row[0] == 0 else
                model.forward_per_image(x, row, mask_pol) for row in rows]
    return _swept(model, x, rows, mask_pol, per_image=True)


def _encode_jobs(jobs, t, lanes: int):
    """The host coder's strings of (symbols, indexes) jobs: the threaded stream coder, or lane-split strings one by one."""
    from . import bitstream as bs
    return bs.encode_streams(jobs, t) if lanes == 1 else [bs.encode_lanes(s_, i_, t, lanes) for s_, i_ in jobs]


def compress_per_image(model, x, qualities, mask_pol=None):
    from . import bitstream as bs
    qs = _quality_vector(x, qualities, "compress_per_image", allow_zero=True)
    if not model._batch_shareable():
        outs = ((q, model.compress(x[b:b + 1], q, mask_pol)) for b, q in enumerate(qs))
        return [{"strings": out["strings"], "shape": out["shape"], "quality": q} for q, out in outs]
    coder, lanes = model._coder(), model._coder_lanes()
    mask_pol = _prepare(model, x, mask_pol, "compress", need_tables=True)
    tg, te = bs.Tables.of(model.gaussian_conditional), bs.Tables.of(model.entropy_bottleneck)
    C = model.dim_chunk
    y_jobs, z_jobs, where = [], [], []                  # where: (image, number of y streams) per image, in job order
    ys, zstr = [], []                                   # the device coder's strings, in the same order
    with torch.no_grad():
        for base_only, sub in _quality_sub_batches(qs, M._max_images_per_plan(x)):
            xb = x[sub].detach().contiguous()
            plan = model._plan(xb, base_only=base_only, symbols=True, per_image=not base_only)
            if base_only:
                plan.execute(xb, 0.0, None, model.use_graph, False)
            else:
                plan.execute_per_image(xb, _mask_qualities(mask_pol, [qs[b] for b in sub]), model.use_graph, False)
            n_sl = model.ns0 if base_only else model.ns1
            if coder == "device":                       # one launch per sub-batch for y, one for z
                y_dev, z_dev = model._encode_plan_device(plan, n_sl, lanes)
                for k, b in enumerate(sub):
                    ys += [y_dev[s_][k] for s_ in range(n_sl)]
                    zstr.append(z_dev[k])
                    where.append((b, n_sl))
                continue
            sym = plan.sym.buf.cpu().numpy()           # [b,h,w,C_lat] int32 (synchronises)
            idx = plan.idx.buf.cpu().numpy()
            zs = plan.z_sym.buf.cpu().numpy()
            zi = np.broadcast_to(np.arange(model.N, dtype=np.int32)[:, None, None], (model.N,) + zs.shape[1:3])
            for k, b in enumerate(sub):                 # stream order: [C, h, w] per image, as compress flattens
                for s_ in range(n_sl):
                    ch = slice(s_ * C, (s_ + 1) * C)
                    y_jobs.append((sym[k, :, :, ch].transpose(2, 0, 1), idx[k, :, :, ch].transpose(2, 0, 1)))
                z_jobs.append((zs[k].transpose(2, 0, 1), zi))
                where.append((b, n_sl))
    if coder == "host":
        ys, zstr = _encode_jobs(y_jobs, tg, lanes), _encode_jobs(z_jobs, te, lanes)
    items: List[Optional[dict]] = [None] * len(qs)
    shape = (x.shape[2] // 64, x.shape[3] // 64)
    o = 0
    for k, (b, n_sl) in enumerate(where):
        items[b] = {"strings": [[[s_] for s_ in ys[o:o + n_sl]], [zstr[k]]], "shape": shape, "quality": qs[b]}
        o += n_sl
    return items


def decompress_per_image(model, items, mask_pol=None):
    items = list(items)
    if not items:
        raise ValueError("decompress_per_image: no items")
    shape = tuple(int(v) for v in items[0]["shape"])
    if any(tuple(int(v) for v in it["shape"]) != shape for it in items):
        raise ValueError("decompress_per_image: all items must have the same shape; decode other shapes in a call of their own")
    qs = [float(it["quality"]) for it in items]
    if any(not q >= 0 for q in qs):
        raise ValueError("decompress_per_image: qualities must be >= 0 (and not NaN)")
    coder, lanes = model._coder(), model._coder_lanes()
    if not model._batch_shareable():
        return {"x_hat": torch.cat([model.decompress(it["strings"], shape, q, mask_pol)["x_hat"] for it, q in zip(items, qs)], 0)}
    mask_pol = _prepare(model, None, mask_pol)
    dev = model.entropy_bottleneck.quantiles.device
    hz, wz = shape
    x_hat = torch.empty((len(items), 3, hz * 64, wz * 64), dtype=torch.float32, device=dev)
    for base_only, sub in _quality_sub_batches(qs, max(1, M.MAX_PLAN_PIXELS // (hz * wz * 64 * 64))):
        n_sl = model.ns0 if base_only else model.ns1
        for b in sub:
            if len(items[b]["strings"][0]) < n_sl or len(items[b]["strings"][1]) != 1:
                raise ValueError(f"decompress_per_image: item {b}: expected {n_sl} slice streams and one z stream of one image")
        strings = [[[items[b]["strings"][0][s_][0] for b in sub] for s_ in range(n_sl)], [items[b]["strings"][1][0] for b in sub]]
        if base_only:
            x_hat[sub] = model.decompress(strings, shape, 0, mask_pol)["x_hat"]
            continue

        def build(B=len(sub)):
            if ops.f16x2_mode():
                raise NotImplementedError(M.F16X2_REFUSAL)
            return _DecPlan(model, B, hz, wz, False, None, dev, per_image=True, coder=coder)
        dp = model._cached_plan(model._dec_plans, (len(sub), hz, wz, False, None, str(dev), "per_image")
                                + ((coder,) if coder != "host" else ()), build, model._weights_sig())
        x_hat[sub] = dp.decode(strings, _mask_qualities(mask_pol, [qs[b] for b in sub]), None, lanes=lanes)
    return {"x_hat": x_hat}


def compress_to(model, x, target, q_tol, mask_pol, metric, out_key):
    """compress_to_bytes / compress_to_bpp: :func:`solve` for one budget per image (a scalar or B values), then compress."""
    t = torch.as_tensor(target, dtype=torch.float64).cpu().reshape(-1)
    if t.numel() not in (1, x.shape[0]):
        raise ValueError(f"compress_to_{metric.key}: one budget, or one per image ({x.shape[0]}), got {t.numel()}")
    sol = solve(model, x, t if t.numel() == 1 else t.reshape(1, -1), q_tol, mask_pol, metric)
    q = sol["quality"][0]
    return {"items": model.compress_per_image(x, q.tolist(), mask_pol), "quality": q, "reached": sol["reached"][0],
            out_key: sol[metric.key][0]}


# ----------------------------------------------------------------------------- the solver
RATE_GRID = 32          # grid points of one refinement pass of qualities_for_bpp (= VAM_MAX_LAYER_LEVELS: one launch)


def rate_search_passes(q_tol: float, n_grid: int = RATE_GRID) -> int:
    """Passes after which a bracket that starts as [0, 10] and shrinks by ``n_grid`` per pass is no wider than q_tol."""
    n, w = 0, 10.0
    while w > q_tol:
        w /= n_grid
        n += 1
    return n


def rate_search_grid(lo, hi, n_grid: int = RATE_GRID):
    """[..., n_grid] ascending points that split each bracket (lo, hi] evenly; the last one is hi itself."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    f = np.arange(1, n_grid + 1, dtype=np.float64) / n_grid
    g = lo[..., None] + (hi - lo)[..., None] * f
    g[..., -1] = hi
    return g


def rate_search_step(grid_q, grid_bpp, targets):
    """One refinement of the bracket arithmetic of qualities_for_bpp, on host arrays: ``grid_q`` [..., G] ascending
    qualities whose FIRST point is the bracket's lower end, ``grid_bpp`` [..., G] the (non-decreasing) rate there,
    ``targets`` [...].  Returns (lo, bpp_lo, hi, bpp_hi, reached): lo = the largest grid point whose rate is within the
    target (reached False, and lo = the first point, when not even that one is), hi = the grid point after lo (lo itself
    when lo is the last one: the budget covers the whole grid)."""
    q, r = np.asarray(grid_q, dtype=np.float64), np.asarray(grid_bpp, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    ok = r <= t[..., None]
    G = q.shape[-1]
    # the LAST point within budget (a non-decreasing curve makes `ok` a prefix; taking the last keeps bpp(lo) <= t anyway)
    last = G - 1 - np.argmax(ok[..., ::-1], axis=-1)
    reached = ok.any(axis=-1)
    i_lo = np.where(reached, last, 0)
    i_hi = np.minimum(i_lo + 1, G - 1)
    i_hi = np.where(reached, i_hi, 0)
    take = lambda a, i: np.take_along_axis(a, i[..., None], axis=-1)[..., 0]
    return take(q, i_lo), take(r, i_lo), take(q, i_hi), take(r, i_hi), reached


def rate_search(curve, bpp0, targets, q_tol: float, n_grid: int = RATE_GRID):
    """Successive refinement for qualities_for_bpp on host arrays, no model and no GPU of its own.  ``curve(q, need)``
    returns the rate at the qualities q [T, B, n] (entries outside ``need`` [T, B, n] are not read), non-decreasing in q
    per image; ``bpp0`` [B] the rate at q = 0; ``targets`` [T, B].  Pass 1 evaluates n_grid points of (0, 10]; later passes
    the n_grid - 1 interior points of each (target, image)'s bracket (both ends are known), so the bracket shrinks by
    n_grid per pass and rate_search_passes(q_tol, n_grid) passes end it.  Returns (quality, bpp, reached), each [T, B]."""
    t = np.asarray(targets, dtype=np.float64)
    T, B = t.shape
    lo = np.zeros((T, B))
    r_lo = np.broadcast_to(np.asarray(bpp0, dtype=np.float64), (T, B)).copy()
    hi, r_hi = np.full((T, B), 10.0), np.full((T, B), np.inf)
    reached = r_lo <= t
    active = reached.copy()                                    # brackets still open
    for p in range(rate_search_passes(q_tol, n_grid)):
        if not active.any():
            break
        pts = rate_search_grid(lo, hi, n_grid)                 # [T, B, n]; from pass 2 on the last point (hi) is known
        need = np.broadcast_to(active[..., None], pts.shape).copy()
        if p > 0:
            need[..., -1] = False
        r = np.where(need, curve(pts, need), r_hi[..., None])
        gq = np.concatenate([lo[..., None], pts], axis=-1)
        gr = np.concatenate([r_lo[..., None], r], axis=-1)
        n_lo, n_rlo, n_hi, n_rhi, _ = rate_search_step(gq, gr, t)
        lo, r_lo = np.where(active, n_lo, lo), np.where(active, n_rlo, r_lo)
        hi, r_hi = np.where(active, n_hi, hi), np.where(active, n_rhi, r_hi)
        active &= hi > lo                                      # lo == hi: the budget covers q = 10
    return np.where(reached, lo, 0.0), r_lo, reached


# What solve() searches.  ``key`` of the result, ``noun`` of a target, ``curve``: the call that gives the whole curve, ``rem_refusal``
# for REM models, ``tol_first``: q_tol is checked before _prepare's checks, not after (each call's order so far); ``start(sw)`` ->
# (the value at q = 0 as [b] on the host, state); ``points(sw, state, q, need)``; ``fallback(model, xs, q, mask_pol)`` -> [b], slowly.
_Metric = namedtuple("_Metric", "key noun curve rem_refusal tol_first need_tables start points fallback")


def solve(model, x, targets, q_tol, mask_pol, metric: _Metric):
    """qualities_for_bpp / qualities_for_bytes: the largest quality whose ``metric`` fits each target, per image: {"quality",
    metric.key, "reached"}, each [T, B] on the host.  Eligible models run the front end once per sub-batch and
    :func:`rate_search` on it; the others bisect (n_grid = 2) over the slow path, one evaluation per distinct (image, quality)."""
    what = f"qualities_for_{metric.key}"
    if isinstance(model, M.VarianceMaskingPICREM):
        raise NotImplementedError(metric.rem_refusal)
    mask_pol = model._mask_policy(mask_pol)
    if mask_pol != "point-based-std":
        raise ValueError(f"{what} searches the point-based-std curve; the {mask_pol!r} curve has two values "
                         f"(q == 0 and q != 0): read them from {metric.curve}(x, [0, 10])")
    bad_tol = None if q_tol > 0 else ValueError(f"q_tol must be > 0, got {q_tol}")
    if bad_tol and metric.tol_first:
        raise bad_tol
    _prepare(model, x, mask_pol, what, metric.need_tables)
    if bad_tol:
        raise bad_tol
    B = x.shape[0]
    tg = _targets(targets, B, f"target_{metric.key}", metric.noun)
    quality, value, reached = (np.zeros(tg.shape), np.zeros(tg.shape), np.zeros(tg.shape, dtype=bool))
    with torch.no_grad():
        if not model._sweep_eligible():
            def curve(q, need):
                out = np.zeros(q.shape)
                for b in range(B):
                    qs = q[:, b][need[:, b]]
                    val = {v: metric.fallback(model, x[b:b + 1], v, mask_pol)[0] for v in np.unique(qs).tolist()}
                    out[:, b][need[:, b]] = [val[v] for v in qs.tolist()]
                return out
            quality, value, reached = rate_search(curve, metric.fallback(model, x, 0.0, mask_pol), tg, q_tol, n_grid=2)
        else:
            for i0, i1, sw in _fronts(model, x):
                v0, state = metric.start(sw)
                curve = lambda q, need, sw=sw, state=state: metric.points(sw, state, q, need)
                quality[:, i0:i1], value[:, i0:i1], reached[:, i0:i1] = rate_search(curve, v0, tg[:, i0:i1], q_tol)
    return {"quality": torch.from_numpy(quality), metric.key: torch.from_numpy(value), "reached": torch.from_numpy(reached)}


# ----------------------------------------------------------------------------- rate control
def _rate_loop(model, x, qualities, mask_pol) -> torch.Tensor:
    """[len(qualities), 2, B] from one forward_single_quality per quality (models that are not _sweep_eligible)."""
    if not len(qualities):
        return torch.zeros((0, 2, x.shape[0]), dtype=torch.float64, device=x.device)
    return torch.stack([model.forward_single_quality(x, q, mask_pol, training=False)["log2_likelihood_sum"] for q in qualities])


def _rate_result(ls: torch.Tensor, x) -> Dict[str, torch.Tensor]:
    return {"log2_likelihood_sum": ls, "bpp": -ls.sum(-2) / float(x.shape[2] * x.shape[3])}


def rate_curve(model, x, qualities, mask_pol=None):
    qualities = [float(q) for q in qualities]
    mask_pol = _prepare(model, x, mask_pol, rem_refusal=_REM_RATE_REFUSAL)
    with torch.no_grad():
        if not model._sweep_eligible():
            return _rate_result(_rate_loop(model, x, qualities, mask_pol), x)
        chunks, rows, cols = _distinct_levels(_mask_qualities(mask_pol, qualities), L.VAM_MAX_LAYER_LEVELS)
        out = torch.zeros((len(qualities), 2, x.shape[0]), dtype=torch.float64, device=x.device)
        rows, cols = torch.from_numpy(rows).to(x.device), torch.from_numpy(cols).to(x.device)
        for i0, i1, sw in _fronts(model, x):
            out[:, :, i0:i1] = sw.fp.log2sum                           # q == 0: the base-only sums (the sweep's zeros branch)
            prog = [sw.rate(levels, model.use_graph) for levels in chunks]
            if prog:
                out[rows, 0, i0:i1] += torch.cat(prog, 1).t()[cols]
    return _rate_result(out, x)


def rate_points(sw, base: torch.Tensor, q, need):
    """qualities_for_bpp's curve on one front end (``base`` [2, B]: its log2 sums): the bpp at the points of :func:`_points`;
    one host synchronisation.  The same points for all images (the first pass): the batched rate tail and its graph; else
    the two kernels run per image (n_batch = 1 at the image's offset), VAM_MAX_LAYER_LEVELS points at a time, eagerly: the
    points of a pass are never asked for again, so a graph of them would only be captured and dropped."""
    G = L.VAM_MAX_LAYER_LEVELS
    tot = base.sum(0)                                                      # [B]

    def same(points):
        sums = torch.cat([sw.rate(points[l0:l0 + G].tolist(), sw.m.use_graph) for l0 in range(0, points.size, G)], 1)
        return (sums + tot[:, None]).cpu().numpy()                         # [B, n_points]

    def own(pts):
        jobs = [(b, l0, min(G, u.size - l0)) for b, u in enumerate(pts) for l0 in range(0, u.size, G)]
        t = sw.rate_tail(G)
        acc = torch.zeros((2, len(jobs), G + 1), dtype=torch.float64, device=base.device)     # a row per launch; unused slots stay 0
        with sw.runner.on_stream():
            for j, (b, l0, n) in enumerate(jobs):
                t.launch(pts[b][l0:l0 + n].tolist(), acc[:, j], b)
        # a launch of n < G levels leaves its no-layer count in slot n: it only reaches the levels >= n, which are not read
        host = (t.level_sums(acc, G) + tot[[b for b, _, _ in jobs]][:, None]).cpu().numpy()   # [jobs, G]
        vals = [np.zeros(u.size) for u in pts]
        for j, (b, l0, n) in enumerate(jobs):
            vals[b][l0:l0 + n] = host[j, :n]
        return vals
    return _points(q, need, same, own) / -float(sw.H * sw.W)


def _bpp_start(sw):
    base = sw.fp.log2sum.clone()                      # [2, b]: y (base slices) and z
    return (-base.sum(0) / float(sw.H * sw.W)).cpu().numpy(), base


BPP = _Metric(
    "bpp", "float", "rate_curve", _REM_RATE_REFUSAL, True, False, _bpp_start, rate_points,
    lambda model, xs, q, mask_pol: _rate_result(_rate_loop(model, xs, [q], mask_pol)[0], xs)["bpp"].cpu().numpy())


# ----------------------------------------------------------------------------- coded-size control
def _compress_size(model, xb, q, mask_pol):
    """(bytes, table cost in bits) of the strings of the real ``compress(xb, q)`` for ONE image, the cost priced on the
    host from that plan's own symbol and index buffers (models that are not _sweep_eligible)."""
    from . import bitstream as bs
    out = model.compress(xb, q, mask_pol)
    nbytes = sum(len(s_) for part in out["strings"][0] for s_ in part) + sum(len(s_) for s_ in out["strings"][1])
    plan = model._plan(xb, base_only=q <= 0, rem_idx=None, symbols=True)
    tg, te = bs.Tables.of(model.gaussian_conditional), bs.Tables.of(model.entropy_bottleneck)
    zs = plan.z_sym.buf.cpu().numpy()
    bits = bs.price(plan.sym.buf.cpu().numpy(), plan.idx.buf.cpu().numpy(), tg).sum() + \
        bs.price(zs, np.arange(model.N)[None, None, None, :], te).sum()
    return nbytes, float(bits)


def coded_size_curve(model, x, qualities, mask_pol=None):
    qualities = [float(q) for q in qualities]
    mask_pol = _prepare(model, x, mask_pol, "coded_size_curve", need_tables=True, rem_refusal=_REM_SIZE_REFUSAL)
    B = x.shape[0]
    lo, hi = np.zeros((len(qualities), B), dtype=np.int64), np.zeros((len(qualities), B), dtype=np.int64)
    bits = np.zeros((len(qualities), B))
    with torch.no_grad():
        if not model._sweep_eligible():
            for b in range(B):
                seen: Dict[float, tuple] = {}
                for k, q in enumerate(qualities):
                    if q not in seen:
                        seen[q] = _compress_size(model, x[b:b + 1], q, mask_pol)
                    lo[k, b] = hi[k, b] = seen[q][0]
                    bits[k, b] = seen[q][1]
        else:
            chunks, rows, cols = _distinct_levels(_mask_qualities(mask_pol, qualities), L.VAM_MAX_LAYER_LEVELS)
            for i0, i1, sw in _fronts(model, x):
                sz = sw.size_front(model.use_graph)
                prog = [sw.size(levels, model.use_graph) for levels in chunks]
                base = sz.base_sizes()                                  # (lo, hi, bits), each [b]
                pl = sz.level_sizes(prog, [len(levels) for levels in chunks])           # each [b, n_levels]
                for dst, b0, pv in zip((lo, hi, bits), base, pl):
                    dst[:, i0:i1] = b0
                    dst[rows, i0:i1] = (b0[:, None] + pv[:, cols]).T
    return {"bytes_lo": torch.from_numpy(lo), "bytes_hi": torch.from_numpy(hi), "bits": torch.from_numpy(bits)}


def size_points(sw, _state, q, need):
    """qualities_for_bytes' curve on one front end (after ``size_front``): bytes_hi of compress at the points of
    :func:`_points`; one host synchronisation.  The same points for all images (the first pass): the batched size tail and
    its graph; else, VAM_MAX_LAYER_LEVELS points at a time, ONE vam_variance_layers_per_image and one vam_coded_layer_bits
    launch serve the whole sub-batch, eagerly."""
    from . import bitstream as bs
    G = L.VAM_MAX_LAYER_LEVELS
    st = sw.size_tail
    base_hi = st.base_sizes()[1]

    def same(points):
        ns = [min(G, points.size - l0) for l0 in range(0, points.size, G)]
        accs = [sw.size(points[l0:l0 + n].tolist(), sw.m.use_graph) for l0, n in zip(range(0, points.size, G), ns)]
        return base_hi[:, None] + st.level_sizes(accs, ns)[1]              # [B, n_points]

    def own(pts):
        accs = []
        with sw.runner.on_stream():
            for l0 in range(0, max(u.size for u in pts), G):
                acc = torch.zeros((2, sw.B, st.ns, G + 1), dtype=torch.float64, device=st.dev)
                # an image with no point left in this chunk gets the list [0]: no element in any layer, its row is not read
                st.launch([u[l0:l0 + G].tolist() or [0.0] for u in pts], acc, per_image=True)
                accs.append(acc)
        host = [a.cpu().numpy() for a in accs]
        vals = [np.zeros(u.size) for u in pts]
        for b, u in enumerate(pts):
            for c, l0 in enumerate(range(0, u.size, G)):
                n = min(G, u.size - l0)
                # a list of n < G levels leaves its no-layer elements in slot G: only the first n slots are read
                S = st.stream_bits(host[c][:, b], n, st.c_out)             # [ns, n]
                vals[b][l0:l0 + n] = base_hi[b] + bs.stream_bytes(S, st.n_y)[1].sum(0)
        return vals
    return _points(q, need, same, own)


BYTES = _Metric(
    "bytes", "number", "coded_size_curve", _REM_SIZE_REFUSAL, False, True,
    lambda sw: (sw.size_front(sw.m.use_graph).base_sizes()[1].astype(np.float64), None), size_points,
    lambda model, xs, q, mask_pol: np.array([_compress_size(model, xs[b:b + 1], q, mask_pol)[0] for b in range(xs.shape[0])],
                                            dtype=np.float64))


# ----------------------------------------------------------------------------- quality maps
MAP_FLOOR_LEVELS = 8        # distinct values of a floor map per image (quality_map_for_bpp)
MAP_GRID = 24               # grid points of one refinement pass: floor levels + grid points fit VAM_MAX_LAYER_LEVELS, one launch
_REM_MAP_REFUSAL = ("quality maps on REM models: a REM and its checkpoint representation belong to ONE quality (the REM refines "
                    "(mu, sigma) per check level), so the positions of one image cannot be at different qualities")
_SHARE_MAP_REFUSAL = ("quality maps with {}: the bits of this configuration depend on how the launches are batched "
                      "(VarianceMaskingPIC._batch_shareable), so a map cannot be stated as 'each position as at its own "
                      "quality'; run the map in the default fp32 storage and bf16x3 arithmetic")


def quality_map_levels(x_shape, qmap, mask_pol):
    """Validate a quality map for images of ``x_shape`` [B, 3, H, W] and split it into the kernel's two inputs.  ``qmap``:
    [B, H/16, W/16] (the latent grid), entries >= 0; ``two-levels`` maps every non-zero entry to 10 (_mask_quality).
    Returns (levels, index): per image the sorted distinct mask qualities (float64 array, at most VAM_MAX_LAYER_LEVELS) and
    the uint8 array [B, H/16, W/16] of each position's index in its image's list.  Pure host code."""
    B, H, W = int(x_shape[0]), int(x_shape[2]), int(x_shape[3])
    want = (B, H // 16, W // 16)
    try:
        qm = torch.as_tensor(qmap).detach().to("cpu", torch.float64).numpy()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"quality map: expected a tensor of shape [B, H/16, W/16] = {list(want)} (the latent grid), got {type(qmap).__name__}") from e
    if tuple(qm.shape) != want:
        raise ValueError(f"quality map: expected shape [B, H/16, W/16] = {list(want)} (the latent grid of images {H}x{W}), "
                         f"got {list(qm.shape)}")
    if np.isnan(qm).any():
        raise ValueError("quality map: qualities must be >= 0 (and not NaN), got NaN")
    if (qm < 0).any():
        raise ValueError(f"quality map: qualities must be >= 0 (and not NaN), got {float(qm.min())}")
    if mask_pol == "two-levels":
        qm = np.where(qm != 0, 10.0, 0.0)
    levels, index = [], np.zeros(want, dtype=np.uint8)
    for b in range(B):
        u, inv = np.unique(qm[b], return_inverse=True)
        if u.size > L.VAM_MAX_LAYER_LEVELS:
            raise ValueError(f"quality map: image {b} holds {u.size} distinct qualities, the limit is {L.VAM_MAX_LAYER_LEVELS} "
                             "(VAM_MAX_LAYER_LEVELS: the levels of one mask launch)")
        levels.append(u.astype(np.float64))
        index[b] = inv.reshape(want[1:]).astype(np.uint8)
    return levels, index


def _map_prepare(model, x, qmap, mask_pol, what, need_tables=False):
    """What every quality-map driver does before GPU work: (mask policy, levels, index).  The map is validated first, then
    the models that cannot run one are refused, then :func:`_prepare`."""
    mask_pol = model._mask_policy(mask_pol)
    M._check_input(x)
    levels, index = quality_map_levels(x.shape, qmap, mask_pol)
    _map_refuse(model)
    _prepare(model, x, mask_pol, what, need_tables)
    return mask_pol, levels, index


def _map_refuse(model):
    if isinstance(model, M.VarianceMaskingPICREM):
        raise NotImplementedError(_REM_MAP_REFUSAL)
    if getattr(model, "storage", "fp32") != "fp32":
        raise NotImplementedError(_SHARE_MAP_REFUSAL.format(f"{model.storage} storage"))
    if ops.f16x2_mode():
        raise NotImplementedError(_SHARE_MAP_REFUSAL.format("VAMPIC_CONV=f16x2"))


def forward_quality_map(model, x, qmap, mask_pol=None):
    mask_pol, levels, index = _map_prepare(model, x, qmap, mask_pol, "forward_quality_map")
    nb = M._max_images_per_plan(x)
    outs = []
    for i in range(0, x.shape[0], nb):
        xb = x[i:i + nb].detach()
        plan = model._plan(xb, base_only=False, quality_map=True)
        outs.append(plan.execute_quality_map(xb, levels[i:i + nb], index[i:i + nb], model.use_graph, True))
    return outs[0] if len(outs) == 1 else M._cat_outputs(outs)


def compress_quality_map(model, x, qmap, mask_pol=None):
    from . import bitstream as bs
    coder, lanes = model._coder(), model._coder_lanes()
    mask_pol, levels, index = _map_prepare(model, x, qmap, mask_pol, "compress", need_tables=True)
    tg, te = bs.Tables.of(model.gaussian_conditional), bs.Tables.of(model.entropy_bottleneck)
    C, n_sl, nb = model.dim_chunk, model.ns1, M._max_images_per_plan(x)
    y_jobs, z_jobs = [], []
    ys, zstr = [], []                                   # the device coder's strings, in the same order
    with torch.no_grad():
        for i in range(0, x.shape[0], nb):
            xb = x[i:i + nb].detach().contiguous()
            plan = model._plan(xb, base_only=False, symbols=True, quality_map=True)
            plan.execute_quality_map(xb, levels[i:i + nb], index[i:i + nb], model.use_graph, False)
            if coder == "device":                       # one launch per sub-batch for y, one for z
                y_dev, z_dev = model._encode_plan_device(plan, n_sl, lanes)
                for k in range(xb.shape[0]):
                    ys += [y_dev[s_][k] for s_ in range(n_sl)]
                    zstr.append(z_dev[k])
                continue
            sym = plan.sym.buf.cpu().numpy()           # [b,h,w,C_lat] int32 (synchronises)
            idx = plan.idx.buf.cpu().numpy()
            zs = plan.z_sym.buf.cpu().numpy()
            zi = np.broadcast_to(np.arange(model.N, dtype=np.int32)[:, None, None], (model.N,) + zs.shape[1:3])
            for k in range(xb.shape[0]):                # stream order: [C, h, w] per image, as compress flattens
                for s_ in range(n_sl):
                    ch = slice(s_ * C, (s_ + 1) * C)
                    y_jobs.append((sym[k, :, :, ch].transpose(2, 0, 1), idx[k, :, :, ch].transpose(2, 0, 1)))
                z_jobs.append((zs[k].transpose(2, 0, 1), zi))
    if coder == "host":
        ys, zstr = _encode_jobs(y_jobs, tg, lanes), _encode_jobs(z_jobs, te, lanes)
    shape = (x.shape[2] // 64, x.shape[3] // 64)
    return [{"strings": [[[s_] for s_ in ys[b * n_sl:(b + 1) * n_sl]], [zstr[b]]], "shape": shape,
             "quality_map": {"levels": [float(q) for q in levels[b]], "index": index[b].copy()},
             "side_bytes": 8 * len(levels[b]) + index[b].size} for b in range(x.shape[0])]


def _item_map(item, b: int, h: int, w: int):
    """(levels, index) of one item of compress_quality_map, checked against the latent grid [h, w]."""
    try:
        qm = item["quality_map"]
        lv = np.asarray(qm["levels"], dtype=np.float64).reshape(-1)
        ix = np.asarray(qm["index"])
    except (KeyError, TypeError) as e:
        raise ValueError(f"decompress_quality_map: item {b} has no quality_map {{'levels', 'index'}}") from e
    if not 1 <= lv.size <= L.VAM_MAX_LAYER_LEVELS or not (lv >= 0).all() or (np.diff(lv) < 0).any():
        raise ValueError(f"decompress_quality_map: item {b}: levels are 1..{L.VAM_MAX_LAYER_LEVELS} non-decreasing qualities >= 0")
    if ix.dtype != np.uint8 or tuple(ix.shape) != (h, w):
        raise ValueError(f"decompress_quality_map: item {b}: index is a uint8 array of shape [{h}, {w}] (the latent grid), "
                         f"got {ix.dtype} {list(ix.shape)}")
    if int(ix.max()) >= lv.size:
        raise ValueError(f"decompress_quality_map: item {b}: index {int(ix.max())} names no level of a list of {lv.size}")
    return lv, ix


def decompress_quality_map(model, items, mask_pol=None):
    items = list(items)
    if not items:
        raise ValueError("decompress_quality_map: no items")
    shape = tuple(int(v) for v in items[0]["shape"])
    if any(tuple(int(v) for v in it["shape"]) != shape for it in items):
        raise ValueError("decompress_quality_map: all items must have the same shape; decode other shapes in a call of their own")
    hz, wz = shape
    maps = [_item_map(it, b, 4 * hz, 4 * wz) for b, it in enumerate(items)]
    coder, lanes = model._coder(), model._coder_lanes()
    _map_refuse(model)
    _prepare(model, None, mask_pol)
    dev = model.entropy_bottleneck.quantiles.device
    n_sl = model.ns1
    for b, it in enumerate(items):
        if len(it["strings"][0]) < n_sl or len(it["strings"][1]) != 1:
            raise ValueError(f"decompress_quality_map: item {b}: expected {n_sl} slice streams and one z stream of one image")
    x_hat = torch.empty((len(items), 3, hz * 64, wz * 64), dtype=torch.float32, device=dev)
    nb = max(1, M.MAX_PLAN_PIXELS // (hz * wz * 64 * 64))
    for i in range(0, len(items), nb):
        sub = list(range(i, min(i + nb, len(items))))
        strings = [[[items[b]["strings"][0][s_][0] for b in sub] for s_ in range(n_sl)], [items[b]["strings"][1][0] for b in sub]]

        def build(B=len(sub)):
            if ops.f16x2_mode():
                raise NotImplementedError(M.F16X2_REFUSAL)
            return _DecPlan(model, B, hz, wz, False, None, dev, quality_map=True, coder=coder)
        dp = model._cached_plan(model._dec_plans, (len(sub), hz, wz, False, None, str(dev), "quality_map")
                                + ((coder,) if coder != "host" else ()), build, model._weights_sig())
        x_hat[sub] = dp.decode(strings, None, None, quality_map=([maps[b][0] for b in sub], np.stack([maps[b][1] for b in sub])),
                               lanes=lanes)
    return {"x_hat": x_hat}


def _map_pixel_values(sw, levels):
    """[b, h * w, n] float64 on the device, on the front end that has just run: the progressive log2 sum of every latent
    pixel at every level of its image's sorted list (n = the longest list; columns beyond an image's list are not
    meaningful).  One vam_variance_layers_per_image and one vam_gauss_layer_bits (pix_per_item = 1) launch."""
    t = sw.rate_tail(L.VAM_MAX_LAYER_LEVELS)
    with sw.runner.on_stream():
        return t.map_values(t.map_bins([[float(q) for q in row] for row in levels]))


def quality_map_rate(model, x, qmap, mask_pol=None):
    mask_pol, levels, index = _map_prepare(model, x, qmap, mask_pol, "quality_map_rate")
    with torch.no_grad():
        if not model.all_scalable:
            return _rate_result(model.forward_quality_map(x, qmap, mask_pol)["log2_likelihood_sum"], x)
        out = torch.zeros((2, x.shape[0]), dtype=torch.float64, device=x.device)
        for i0, i1, sw in _fronts(model, x):
            V = _map_pixel_values(sw, levels[i0:i1])                                     # [b, hw, n]
            k = torch.from_numpy(index[i0:i1].reshape(i1 - i0, -1).astype(np.int64)).to(x.device)
            out[:, i0:i1] = sw.fp.log2sum
            out[0, i0:i1] += V.gather(2, k.unsqueeze(-1))[..., 0].sum(1)
    return _rate_result(out, x)


def _floor_points(sw, base, levels, index, pts):
    """The bpp of the maps max(floor, q) for the points q = ``pts[b]`` (a sorted distinct array per image, any length) of the
    floor map (``levels``, ``index`` of :func:`quality_map_levels`), on the front end that has just run: a list of arrays.
    MAP_GRID points at a time: image b's list is floor levels | points, at most VAM_MAX_LAYER_LEVELS, so a chunk is one
    vam_variance_layers_per_image and one vam_gauss_layer_bits launch for the sub-batch; one host synchronisation."""
    B, dev = len(levels), base.device
    tot = base.sum(0)                                                            # [B]
    fidx = torch.from_numpy(index.reshape(B, -1).astype(np.int64)).to(dev)       # [B, hw]
    parts = []
    with torch.no_grad():
        for l0 in range(0, max(u.size for u in pts), MAP_GRID):
            chunk = [u[l0:l0 + MAP_GRID] for u in pts]
            lists = [np.union1d(lv, c) for lv, c in zip(levels, chunk)]          # sorted distinct
            V = _map_pixel_values(sw, lists)                                     # [B, hw, n]
            G = max(c.size for c in chunk)
            # where the floor's levels and the points sit in each image's list; an image with fewer points repeats its first level
            f_at = [np.searchsorted(ls, lv) for ls, lv in zip(lists, levels)]
            p_at = np.zeros((B, G), dtype=np.int64)
            for b, (ls, c) in enumerate(zip(lists, chunk)):
                p_at[b, :c.size] = np.searchsorted(ls, c)
            fk = torch.stack([torch.from_numpy(f_at[b].astype(np.int64)).to(dev)[fidx[b]] for b in range(B)])   # [B, hw]
            K = torch.maximum(fk.unsqueeze(1), torch.from_numpy(p_at).to(dev).unsqueeze(2))                      # [B, G, hw]
            parts.append(V.transpose(1, 2).gather(1, K).sum(2) + tot[:, None])   # max(floor, q) is a level of the list: the larger index
    host = torch.cat(parts, 1).cpu().numpy() / -float(sw.H * sw.W)
    return [host[b, :u.size] for b, u in enumerate(pts)]


def quality_map_for_bpp(model, x, floor_map, target_bpp, q_tol=1e-3, mask_pol=None):
    what = "quality_map_for_bpp"
    mask_pol = model._mask_policy(mask_pol)
    M._check_input(x)
    levels, index = quality_map_levels(x.shape, floor_map, mask_pol)
    many = [(b, lv.size) for b, lv in enumerate(levels) if lv.size > MAP_FLOOR_LEVELS]
    if many:
        raise ValueError(f"{what}: the floor map of image {many[0][0]} holds {many[0][1]} distinct qualities, the limit is "
                         f"{MAP_FLOOR_LEVELS} (they share one launch's {L.VAM_MAX_LAYER_LEVELS} levels with {MAP_GRID} grid points)")
    if mask_pol != "point-based-std":
        raise ValueError(f"{what} searches the point-based-std curve; the {mask_pol!r} curve has two values "
                         "(q == 0 and q != 0): read them from quality_map_rate")
    if not q_tol > 0:
        raise ValueError(f"q_tol must be > 0, got {q_tol}")
    _map_refuse(model)
    if not model.all_scalable:
        raise NotImplementedError(f"{what} on all_scalable=False: the progressive (mu, sigma) chain reads the decoded slices, so "
                                  "the rate of a map needs a whole forward; search over forward_quality_map yourself")
    _prepare(model, x, mask_pol, what)
    B = x.shape[0]
    tg = _targets(target_bpp, B, "target_bpp", "float")
    quality, value, reached = (np.zeros(tg.shape), np.zeros(tg.shape), np.zeros(tg.shape, dtype=bool))
    with torch.no_grad():
        for i0, i1, sw in _fronts(model, x):
            base = sw.fp.log2sum.clone()
            lv, ix = levels[i0:i1], index[i0:i1]
            own = lambda pts, sw=sw, base=base, lv=lv, ix=ix: _floor_points(sw, base, lv, ix, pts)
            same = lambda points, own=own, n=i1 - i0: own([points] * n)
            curve = lambda q, need, same=same, own=own: _points(q, need, same, own)
            bpp0 = np.array([v[0] for v in own([np.zeros(1)] * (i1 - i0))])
            quality[:, i0:i1], value[:, i0:i1], reached[:, i0:i1] = rate_search(curve, bpp0, tg[:, i0:i1], q_tol, n_grid=MAP_GRID)
    floor = np.stack([lv[ix_.astype(np.int64)] for lv, ix_ in zip(levels, index)])          # [B, h, w]
    return {"quality": torch.from_numpy(quality), "bpp": torch.from_numpy(value), "reached": torch.from_numpy(reached),
            "quality_map": torch.from_numpy(np.maximum(floor[None], quality[:, :, None, None]))}
