"""Embedded streams: every progressive slice coded ONCE, in rank order, as one rANS stream that is
decodable from any byte prefix.

The variance mask at quality q keeps, per (image, slice) segment, the elements whose sigma is at or above a quantile, so
the masks of all qualities are prefixes of one ordering: the elements sorted by descending sigma (vam_variance_rank).
With ``all_scalable=True`` the decoder knows that sigma before it reads one enhancement symbol, so both sides sort each
segment the same way; the rANS decoder reads a stream's words front to back, so its first n symbols depend only on the
words consumed so far.  Cutting a slice's stream after the n_q elements with sigma >= thr_q therefore reproduces
``forward_single_quality(x, q)`` for every q — chosen after encoding —, and cutting it anywhere else still decodes: the
elements present are dequantised, the others take mu.

A new format beside ``compress`` / ``decompress`` and the layered container of :mod:`progressive`, whose bytes it leaves
alone.  Container of one image::

    {"format": "embedded-1", "shape", "z", "base",
     "embedded": [bytes] * ns,
     "marks": {"q": [...], "count": int[L][ns], "bytes": int[L][ns]}}

z and the base slices are the layered container's, byte for byte.  The marks give, for each listed quality, the element
count of every slice (the project's own masks: vam_variance_layers on the same sigma) and the exact byte length that
decodes it (bitstream.prefix_bytes).  :func:`truncate` needs neither the model nor a GPU.

``lanes`` = K > 1 codes every embedded stream on K interleaved lanes (bitstream.encode_interleaved):
K coder states share one word stream in the decoder's reading order, so a wave decodes K elements per step and a byte
prefix is still a rank prefix.  Such a container carries ``"format": "embedded-2"`` and ``"lanes": K``; z and the base
slices stay the K = 1 strings.  ``coder="device"`` keeps symbols and indexes on the device on both sides.

A **schedule**  gives a region of interest the front of every stream: L quality maps
S[0] <= ... <= S[L-1] on the latent grid.  The masks of a pointwise non-decreasing sequence of maps are nested, so they are
prefixes of ONE ordering: ascending stage (the first map whose mask holds the element), within a stage descending sigma.
Both sides build it on the device from their own sigma and the schedule the container carries (vam_stage_ids,
vam_variance_rank_staged); a stream cut at stage k's mark reproduces ``forward_quality_map(x, S[k])``, any other cut is a
rank prefix, and the whole stream is still ``forward_single_quality(x, 10)``.  Such a container carries
``"format": "embedded-3"``, always ``"lanes"``, ``"schedule": {"levels", "index"}`` with its raw ``"side_bytes"``, and marks
by ``"stage"`` instead of ``"q"``.

A **resumable** decoder is a receiver whose bytes keep arriving: ``EmbeddedDecoder(..., resumable=True)``
keeps a checkpoint per stream at a group boundary (bitstream.Checkpoints), :meth:`EmbeddedDecoder.extend` takes the bytes
that follow — :func:`delta` cuts them on the transmitter's side — and only the new elements are entropy-decoded.  The
format is unchanged, and after every ``extend`` the decoder equals a fresh one on the concatenated containers bit for bit.

``base_lanes`` = Kb > 1 codes z and the base slices, too, as interleaved strings, on Kb lanes, so that
the device coder decodes them with one thread per lane instead of one wave per string.  Such a container carries
``"format": "embedded-4"``, always ``"lanes"`` and ``"base_lanes": Kb``; it is scheduled exactly when it carries
``"schedule"`` (then also ``"side_bytes"`` and marks by ``"stage"``).  Embedded streams, marks, counts and mark bytes are
those of ``base_lanes=1``.  z and the base are needed whole: a string that ends early is a ValueError at the decoder.

A **codestream**  is one container as ONE byte string whose every prefix decodes: a preamble, a
little-endian header with a CRC-32, z and the base whole, then the embedded streams in rounds, one round per mark, every
slice's bytes between two marks in slice order.  :func:`to_bytes` writes it, :func:`need_bytes`, :func:`layout` and
:func:`from_bytes` read it on the host alone, and :class:`StreamDecoder` is a receiver that is fed raw chunks: it turns
them into :meth:`EmbeddedDecoder.extend` calls by the header's arithmetic.  The containers and their coders are unchanged.
"""
from __future__ import annotations

import math
import os
import pickle
import struct
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import progressive as P
from .framing import MAX_HEADER, PREAMBLE_BYTES, Frame, check_total, chunk_view, same as _same, view as _view
from .progressive import Q_LIST

FORMAT = "embedded-1"
FORMAT_LANES = "embedded-2"          # embedded streams on K > 1 interleaved lanes; carries "lanes": K
FORMAT_SCHEDULED = "embedded-3"      # scheduled rank order; carries "lanes": K >= 1, "schedule" and "side_bytes"
FORMAT_BASE_LANES = "embedded-4"     # z and the base on Kb > 1 interleaved lanes; carries "lanes": K >= 1, "base_lanes": Kb
_FORMATS = (FORMAT, FORMAT_LANES, FORMAT_SCHEDULED, FORMAT_BASE_LANES)
_LAYERED = "the layered container (progressive.encode_batch / ProgressiveDecoder)"


def _check_model(model):
    """The refusals of the batched layered container (progressive._check_variant, _check_batched)."""
    P._check_variant(model)
    P._check_batched(model)


def _check_shape(model, B: int, H: int, W: int, what: str):
    from . import _lib as L
    from .control import sweep_groups
    if len(sweep_groups(1, B, H, W)) > 1:
        raise NotImplementedError(f"{what}: {B} images of {H}x{W} exceed one plan; code them in smaller batches")
    n = model.dim_chunk * (H // 16) * (W // 16)
    if n > L.VAM_MAX_RANK_ELEMENTS:
        raise NotImplementedError(f"{what}: a slice of a {H}x{W} image has {n} elements, the rank order sorts segments of up "
                                  f"to {L.VAM_MAX_RANK_ELEMENTS}; code the image in tiles or use {_LAYERED}")


def _map_threads(fn, items):
    from . import bitstream as bs
    items = list(items)
    with ThreadPoolExecutor(max_workers=bs.coder_threads()) as ex:          # the coder runs outside the interpreter lock
        return list(ex.map(fn, items))


def container_bytes(c) -> List[int]:
    """[bytes of z, bytes of the base slices, bytes of the embedded streams as held] of one image's container."""
    return [sum(len(s) for s in c["z"]), sum(len(s[0]) for s in c["base"]), sum(len(s) for s in c["embedded"])]


def schedule_buffers(B: int, n_pix: int, device):
    """The three device inputs of a scheduled rank order for B images of n_pix latent positions: the layer-parameter table
    (ops.layer_table), the stage index maps uint8 [B, VAM_MAX_LAYER_LEVELS, n_pix] and the stage counts int32 [B]."""
    import ctypes
    from . import _lib as L
    return (torch.zeros((B * ctypes.sizeof(L.VamLayerParams),), dtype=torch.uint8, device=device),
            torch.zeros((B, L.VAM_MAX_LAYER_LEVELS, n_pix), dtype=torch.uint8, device=device),
            torch.zeros((B,), dtype=torch.int32, device=device))


def fill_schedule(table, stage_map, n_stages, levels, index, n_pix: int, C: int):
    """Refill :func:`schedule_buffers` from :func:`check_schedule`'s (levels, index [B, L, h, w]) on the current stream: host
    arithmetic and three copies, outside any capture."""
    from . import ops
    B, n_st = index.shape[:2]
    maps = np.zeros(tuple(stage_map.shape), dtype=np.uint8)
    maps[:, :n_st] = np.asarray(index, dtype=np.uint8).reshape(B, n_st, n_pix)
    table.copy_(torch.from_numpy(ops.layer_table([[float(q) for q in row] for row in levels], n_pix, C)))
    stage_map.copy_(torch.from_numpy(maps))
    n_stages.copy_(torch.full((B,), n_st, dtype=torch.int32))


def check_schedule(schedule, B: int, h: int, w: int):
    """Validate a schedule for B images of latent grid h x w and split it into the kernels' inputs.  ``schedule``: L maps
    [B, h, w] (a sequence of them or one [L, B, h, w] array), 1 <= L <= VAM_MAX_LAYER_LEVELS, every entry finite and >= 0
    and, at every position, non-decreasing from one stage to the next.  Returns (levels, index): per image the sorted
    distinct values over all stages (float64 array, at most VAM_MAX_LAYER_LEVELS) and the uint8 array [B, L, h, w] of each
    stage's index into its image's list.  Pure host code; ValueError names what is wrong."""
    from . import _lib as L
    from .control import quality_map_levels
    G = L.VAM_MAX_LAYER_LEVELS
    want = (int(B), int(h), int(w))
    try:
        stages = list(schedule)
    except TypeError as e:
        raise ValueError(f"schedule: expected a sequence of quality maps [B, H/16, W/16] = {list(want)}, got "
                         f"{type(schedule).__name__}") from e
    if not 1 <= len(stages) <= G:
        raise ValueError(f"schedule: 1..{G} stages, got {len(stages)}")
    maps = []
    for k, m in enumerate(stages):
        try:                                                # a stage is a quality map: shape, NaN and sign as section 9k checks them
            lv, ix = quality_map_levels((want[0], 3, 16 * want[1], 16 * want[2]), m, None)
        except ValueError as e:
            raise ValueError(f"schedule: stage {k}: {e}") from e
        maps.append(np.stack([lv[b][ix[b]] for b in range(want[0])]))
        if np.isinf(maps[-1]).any():
            raise ValueError(f"schedule: stage {k}: qualities must be finite, got inf")
    S = np.stack(maps)                                      # [L, B, h, w]
    down = np.argwhere(S[1:] < S[:-1])
    if len(down):
        k, b, y, x = (int(v) for v in down[0])
        raise ValueError(f"schedule: image {b}, position ({y}, {x}): stage {k + 1} lowers the quality from {S[k, b, y, x]} to "
                         f"{S[k + 1, b, y, x]}; a schedule never decreases from one stage to the next")
    levels, index = [], np.zeros((want[0], len(maps)) + want[1:], dtype=np.uint8)
    for b in range(want[0]):
        u, inv = np.unique(S[:, b], return_inverse=True)
        if u.size > G:
            raise ValueError(f"schedule: image {b} holds {u.size} distinct qualities over its stages, the limit is {G} "
                             "(VAM_MAX_LAYER_LEVELS: the levels of one mask launch)")
        levels.append(u.astype(np.float64))
        index[b] = inv.reshape((len(maps),) + want[1:]).astype(np.uint8)
    return levels, index


def _schedule_of(cs):
    """(levels, index [B, L, h, w]) of a batch of scheduled containers, checked against the containers' own shape."""
    from . import _lib as L
    levels, index = [], []
    for b, c in enumerate(cs):
        sc = c.get("schedule")
        if not isinstance(sc, dict) or "levels" not in sc or "index" not in sc:
            raise ValueError(f"EmbeddedDecoder: container {b} is scheduled ({c.get('format')!r}) and carries no schedule")
        lv = np.asarray(sc["levels"], dtype=np.float64).reshape(-1)
        ix = np.asarray(sc["index"])
        h, w = 4 * int(c["shape"][0]), 4 * int(c["shape"][1])
        if ix.dtype != np.uint8 or ix.ndim != 3 or tuple(ix.shape[1:]) != (h, w) or not 1 <= ix.shape[0] <= L.VAM_MAX_LAYER_LEVELS:
            raise ValueError(f"EmbeddedDecoder: container {b}: the schedule's index is uint8 [1..{L.VAM_MAX_LAYER_LEVELS}, {h}, {w}], "
                             f"got {ix.dtype} {list(ix.shape)}")
        if not 1 <= lv.size <= L.VAM_MAX_LAYER_LEVELS or not np.all(np.isfinite(lv)) or (lv < 0).any() or (np.diff(lv) <= 0).any() \
                or int(ix.max()) >= lv.size or (np.diff(ix.astype(np.int16), axis=0) < 0).any():
            raise ValueError(f"EmbeddedDecoder: container {b}: not a schedule (1..{L.VAM_MAX_LAYER_LEVELS} increasing finite levels "
                             ">= 0, indexes into them that never decrease from stage to stage)")
        levels.append(lv)
        index.append(ix)
    if any(ix.shape[0] != index[0].shape[0] for ix in index):
        raise ValueError(f"EmbeddedDecoder: every container must have the same number of stages, got "
                         f"{sorted({int(ix.shape[0]) for ix in index})}; decode them separately")
    return levels, np.stack(index)


def encode_batch(model, x, marks: Optional[Sequence[float]] = None, save_path=None, coder: Optional[str] = None, lanes: int = 1,
                 schedule=None, base_lanes: int = 1) -> List[dict]:
    """Embedded containers of a batch x [B,3,H,W] (H, W multiples of 64, as for ``compress``) on the fused plans: the
    ``compress(x, 10)`` plan (symbols round(r - mu), unmasked indexes), vam_variance_rank on its progressive sigma, then
    vam_rank_gather writes symbols and indexes of every segment in rank order.  Each progressive slice becomes ONE
    stream; ``marks`` (1..32 non-decreasing qualities) are looked up for the receiver's convenience, they do not limit
    where a stream may be cut.

    ``coder`` (None: ``model.coder``): "host" brings the ranked symbols and indexes (and z and the base slices, coded as
    :func:`progressive.encode_batch` codes them) to the host and codes them on its threads; "device" 
    codes z and the base slices with the device coder's launches and ALL embedded streams with one more, which also gives
    the marks' bytes, and fetches lengths, status codes, marks and coded bytes only.  The containers are the same byte for
    byte.  ``lanes`` = K > 1: the embedded streams on K interleaved lanes, format ``"embedded-2"`` with ``"lanes": K``; read
    from the argument only, never from ``model.coder_lanes``.  K = 1 is format ``"embedded-1"`` with no new key.

    ``schedule`` (exclusive with ``marks``): L quality maps [B, H/16, W/16], non-decreasing from stage to
    stage (:func:`check_schedule`).  The streams are coded in the scheduled rank order — vam_variance_layers_per_image on the
    schedule's levels, vam_stage_ids, vam_variance_rank_staged — and marked per stage (vam_rank_counts on the stage ids);
    the coders are unchanged.  Format ``"embedded-3"``: ``"lanes"`` always, ``"schedule"`` and its raw ``"side_bytes"``,
    ``"marks": {"stage", "count", "bytes"}``; z and the base slices are byte for byte as before.

    ``base_lanes`` = Kb > 1 (read from the argument only, like ``lanes``): z and every base slice as an
    interleaved string on Kb lanes of the same elements in the same order (bitstream.encode_interleaved_streams; on the
    device one vam_rans_interleaved_encode_nhwc_device launch for z and one for all base slices).  Format ``"embedded-4"``
    with ``"lanes"`` always and ``"base_lanes": Kb``, scheduled exactly when it carries ``"schedule"``; everything else in
    the container is what ``base_lanes=1`` gives.  Kb = 1 changes nothing.

    The work is two passes, :func:`_encode_front` (everything but the marks' bytes) and :func:`_encode_finish` (the marks'
    bytes from the marks' counts), so that a caller can supply the counts later (tiled pictures); this
    function runs them back to back with the batch's own counts."""
    from . import bitstream as bs
    _check_model(model)
    if schedule is not None and marks is not None:
        raise ValueError("embedded.encode_batch: give marks or schedule, not both (a scheduled container is marked per stage)")
    B, _, H, W = x.shape
    if schedule is not None:
        levels, index = check_schedule(schedule, B, H // 16, W // 16)         # on the host, before any GPU work
        qs = list(range(index.shape[1]))
    else:
        qs = P.check_q_list(Q_LIST if marks is None else marks)
    coder, K, Kb = P._check_coder(model, coder), bs.check_lanes(lanes), bs.check_lanes(base_lanes)
    st = _encode_front(model, x, qs, coder, K, Kb, None if schedule is None else (levels, index))
    containers = _encode_finish(st)
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        for b, c in enumerate(containers):
            with open(os.path.join(save_path, "embedded.pkl" if B == 1 else f"embedded_{b}.pkl"), "wb") as f:
                pickle.dump(c, f)
    return containers


def _encode_front(model, x, qs, coder: str, K: int, Kb: int, schedule=None) -> dict:
    """The first pass of :func:`encode_batch` on checked arguments, everything that does not depend on the marks' counts: the
    network (once), the rank order, the gather into rank order, the batch's own counts, and the coding of z and the base; on
    the host coder also of the embedded strings.  Returns the state :func:`_encode_finish` turns into containers, now or
    later and with the batch's own counts or a caller's (``tiled.encode(allocation="picture")``).

    What the state keeps per image between the passes: the coded z, base (and, host coder, embedded) strings; the ranked
    table indexes int32 [ns, n]; on the device coder also the ranked symbols int32 [ns, n], both on the device; the own counts
    int32 [L, ns].  ``perm`` (int32 [B, ns, n]) and ``std_p`` (the plan's sigma view) are valid only until the model's next
    plan runs: a caller that pools keys (ops.pool_keys) does so at once and drops them."""
    from . import _lib as L
    from . import bitstream as bs
    from . import ops
    from .models import EMPTY_SCALE_TABLE
    B, _, H, W = x.shape
    m = model
    d, C, ns = m.division_dimension[0], m.dim_chunk, m.ns0
    st = {"m": m, "B": B, "H": H, "W": W, "qs": list(qs), "coder": coder, "K": K, "Kb": Kb, "schedule": schedule}
    with torch.no_grad():
        L.require_gpu()
        m._check_config()
        _check_shape(m, B, H, W, "embedded.encode_batch")
        plan = m._plan(x, base_only=False, symbols=True)
        if plan.idx is None:
            raise ValueError(EMPTY_SCALE_TABLE.format("embedded.encode_batch"))
        plan.execute(x, 10.0, None, m.use_graph, False)
        h, w = H // 16, W // 16
        n = C * h * w
        dev = x.device
        perm = torch.empty((B, ns, n), dtype=torch.int32, device=dev)
        layer = torch.empty((B, h, w, d), dtype=torch.uint8, device=dev)
        if schedule is not None:
            levels, index = schedule
            table, stage_map, n_stages = schedule_buffers(B, h * w, dev)
            fill_schedule(table, stage_map, n_stages, levels, index, h * w, C)
            stage = torch.empty_like(layer)
            ops.variance_layers_table(plan.std_p, table, layer, n_slice=ns)
            ops.stage_ids(layer, stage_map, n_stages, stage)
            ops.variance_rank_staged(plan.std_p, stage, perm, n_slice=ns, workspace=ops.rank_workspace(plan.std_p, ns, dev))
            layer = stage                                                    # the marks count stage ids
        else:
            ops.variance_rank(plan.std_p, perm, n_slice=ns, workspace=ops.rank_workspace(plan.std_p, ns, dev))
        r_sym, r_idx = torch.empty_like(perm), torch.empty_like(perm)
        ops.rank_gather(perm, ns, plan.sym.window(d, d), r_sym, plan.idx.window(d, d), r_idx)
        if schedule is None:
            ops.variance_layers(plan.std_p, qs, layer, n_slice=ns)           # the masks of the marks, as every plan builds them
        count = torch.empty((len(qs), B, ns), dtype=torch.int32, device=dev)
        ops.rank_counts(layer, perm, ns, len(qs), count)
        st.update(perm=perm, std_p=plan.std_p, count=count)
        if coder == "device":
            tg, te = bs.DeviceCoderTables.of(m.gaussian_conditional, dev), bs.DeviceCoderTables.of(m.entropy_bottleneck, dev)
            if Kb > 1:
                z_str = bs.encode_window_interleaved_device(plan.z_sym, None, 1, m.N, te, Kb)[0]
                base = bs.encode_window_interleaved_device(plan.sym, plan.idx, ns, C, tg, Kb)   # [slice][image]
            else:
                z_str = bs.encode_streams_device(plan.z_sym, None, 1, m.N, te)[0]
                base = bs.encode_streams_device(plan.sym, plan.idx, ns, C, tg)                  # [slice][image]
            st.update(z_str=z_str, base=base, r_sym=r_sym, r_idx=r_idx)
            return st
        nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu().numpy()
        sym_b, idx_b, zs = nchw(plan.sym.buf[..., :d]), nchw(plan.idx.buf[..., :d]), nchw(plan.z_sym.buf)
        r_sym, r_idx = r_sym.cpu().numpy(), r_idx.cpu().numpy()
    tg, te = bs.Tables.of(m.gaussian_conditional), bs.Tables.of(m.entropy_bottleneck)
    zi = np.broadcast_to(np.arange(m.N, dtype=np.int32)[:, None, None], zs.shape[1:])
    z_jobs = [(zs[b], zi) for b in range(B)]
    z_str = bs.encode_streams(z_jobs, te) if Kb == 1 else bs.encode_interleaved_streams(z_jobs, te, lanes=Kb)
    sl = lambda a, b, i: a[b, i * C:(i + 1) * C]
    jobs = [(sl(sym_b, b, i), sl(idx_b, b, i)) for i in range(ns) for b in range(B)]
    e_jobs = [(r_sym[b, j], r_idx[b, j]) for b in range(B) for j in range(ns)]
    if K == 1 and Kb == 1:                                                                  # one call, as ever
        y_str = bs.encode_streams(jobs + e_jobs, tg)
        emb_str = y_str[ns * B:]
    else:
        y_str = bs.encode_streams(jobs, tg) if Kb == 1 else bs.encode_interleaved_streams(jobs, tg, lanes=Kb)
        emb_str = bs.encode_streams(e_jobs, tg) if K == 1 else bs.encode_interleaved_streams(e_jobs, tg, lanes=K)
    st.update(z_str=z_str, base=[y_str[i * B:(i + 1) * B] for i in range(ns)], emb_str=emb_str, r_idx=r_idx)
    return st


def _encode_finish(st: dict, count=None) -> List[dict]:
    """The second pass of :func:`encode_batch`: the marks' bytes from the marks' counts — bitstream.prefix_bytes on the host
    coder, the device encode launch (which also codes the embedded strings) on the device coder — and the containers.
    ``count``: int32 [L, B, ns], a device tensor or an array, non-decreasing in L and at most n; None: the batch's own."""
    from . import bitstream as bs
    m, B, H, W, qs, K, Kb, schedule = (st[k] for k in ("m", "B", "H", "W", "qs", "K", "Kb", "schedule"))
    ns = m.ns0
    count = st["count"] if count is None else count
    if st["coder"] == "device":
        dev = st["r_sym"].device
        count = torch.as_tensor(count, dtype=torch.int32).to(dev).contiguous()
        with torch.no_grad():
            emb_str, cut = bs.encode_embedded_device(st["r_sym"], st["r_idx"], bs.DeviceCoderTables.of(m.gaussian_conditional, dev),
                                                     K, count)                                  # stream b * ns + j
        cuts = cut.reshape(len(qs), B, ns)
        count = count.cpu().numpy().astype(np.int64)
    else:
        count = (count.cpu().numpy() if isinstance(count, torch.Tensor) else np.asarray(count)).astype(np.int64)
        emb_str, r_idx, tg = st["emb_str"], st["r_idx"], bs.Tables.of(m.gaussian_conditional)
        got = _map_threads(lambda bj: bs.prefix_bytes(emb_str[bj[0] * ns + bj[1]], r_idx[bj[0], bj[1]],
                                                      count[:, bj[0], bj[1]].tolist(), tg, lanes=K),
                           [(b, j) for b in range(B) for j in range(ns)])
        cuts = np.asarray(got, dtype=np.int64).reshape(B, ns, len(qs)).transpose(2, 0, 1)
    z_str, base = st["z_str"], st["base"]
    containers = []
    for b in range(B):
        c = {"format": FORMAT if K == 1 else FORMAT_LANES, "shape": (H // 64, W // 64), "z": [z_str[b]],
             "base": [[base[i][b]] for i in range(ns)], "embedded": [emb_str[b * ns + j] for j in range(ns)],
             "marks": {"q": list(qs), "count": [[int(count[k, b, j]) for j in range(ns)] for k in range(len(qs))],
                       "bytes": [[int(cuts[k, b, j]) for j in range(ns)] for k in range(len(qs))]}}
        if K > 1:
            c["lanes"] = K
        if schedule is not None:
            levels, index = schedule
            c["format"], c["lanes"] = FORMAT_SCHEDULED, K
            c["marks"]["stage"] = c["marks"].pop("q")
            c["schedule"] = {"levels": [float(v) for v in levels[b]], "index": index[b].copy()}
            c["side_bytes"] = 8 * len(levels[b]) + int(index[b].size)     # carried raw, as a quality map is (section 9k)
        if Kb > 1:
            c["format"], c["lanes"], c["base_lanes"] = FORMAT_BASE_LANES, K, Kb
        containers.append(c)
    return containers


def _scheduled(c) -> bool:
    """Whether a checked container is in a scheduled rank order: ``"embedded-3"``, or ``"embedded-4"`` with a schedule."""
    return c["format"] == FORMAT_SCHEDULED or (c["format"] == FORMAT_BASE_LANES and "schedule" in c)


def _base_lanes(c) -> int:
    """The lanes of z and the base strings of a checked container: its ``"base_lanes"`` for ``"embedded-4"``, otherwise 1."""
    return int(c["base_lanes"]) if c["format"] == FORMAT_BASE_LANES else 1


def _check_container(c) -> int:
    """The lanes per embedded stream of container ``c``: 1 for ``"embedded-1"``, its ``"lanes"`` for ``"embedded-2"``,
    ``"embedded-3"`` and ``"embedded-4"`` (which carry the key for K = 1 too).  An ``"embedded-4"`` container also carries
    ``"base_lanes"`` > 1 (:func:`_base_lanes`) and is scheduled exactly when it carries ``"schedule"`` (:func:`_scheduled`)."""
    from . import bitstream as bs
    if not isinstance(c, dict) or c.get("format") not in _FORMATS:
        raise ValueError(f"not an embedded container (format {FORMAT!r}, {FORMAT_LANES!r}, {FORMAT_SCHEDULED!r} or "
                         f"{FORMAT_BASE_LANES!r}): got {c.get('format') if isinstance(c, dict) else type(c).__name__!r}")
    if c["format"] == FORMAT:
        return 1
    K = bs.check_lanes(c.get("lanes"))
    if c["format"] == FORMAT_BASE_LANES:
        if "base_lanes" not in c:
            raise ValueError(f"not an embedded container: format {FORMAT_BASE_LANES!r} carries \"base_lanes\", this one lacks it")
        try:
            Kb = bs.check_lanes(c["base_lanes"])
        except ValueError as e:
            raise ValueError(f"not an embedded container: format {FORMAT_BASE_LANES!r}: base_lanes: {e}") from e
        if Kb == 1:
            raise ValueError(f"an {FORMAT_BASE_LANES!r} container carries base_lanes > 1; \"base_lanes\": 1 is format {FORMAT!r}, "
                             f"{FORMAT_LANES!r} or {FORMAT_SCHEDULED!r}")
        if "schedule" not in c:
            if "q" not in c.get("marks", ()):
                raise ValueError(f"not an embedded container: an unscheduled {FORMAT_BASE_LANES!r} container carries marks by \"q\", "
                                 "this one lacks them")
            return K
    if _scheduled(c):
        if not isinstance(c.get("schedule"), dict) or "side_bytes" not in c or "stage" not in c.get("marks", ()):
            raise ValueError(f"not an embedded container: a scheduled {c['format']!r} container carries \"schedule\", \"side_bytes\" "
                             "and marks by \"stage\", this one lacks them")
        return K
    if K == 1:
        raise ValueError(f"an {FORMAT_LANES!r} container carries lanes > 1; one lane is format {FORMAT!r}")
    return K


def truncate(container, q: Optional[float] = None, max_bytes: Optional[int] = None,
             slice_bytes: Optional[Sequence[int]] = None, stage: Optional[int] = None) -> dict:
    """A copy of ``container`` with its embedded streams cut, on the host alone (what a server or a transmitter does).
    Exactly one of: ``q`` — a marked quality: every slice is cut at that mark's bytes; ``max_bytes`` — the largest mark
    whose z + base + embedded total fits (the base alone when no mark fits, ValueError when not even the base does);
    ``slice_bytes`` — one explicit length per slice, any byte count (a length beyond what the slice holds keeps it whole);
    ``stage`` — a stage of a scheduled container (``"embedded-3"``, or ``"embedded-4"`` with a schedule), which is marked by
    stage and refuses ``q``; its ``max_bytes`` counts the schedule's ``side_bytes`` with z and the base.  ``"lanes"``,
    ``"base_lanes"`` and the schedule go through untouched."""
    _check_container(container)
    if sum(a is not None for a in (q, max_bytes, slice_bytes, stage)) != 1:
        raise ValueError("truncate: give exactly one of q, stage, max_bytes and slice_bytes")
    emb, marks = container["embedded"], container["marks"]
    ns = len(emb)
    scheduled = _scheduled(container)
    if q is not None and scheduled:
        raise ValueError(f"truncate: a scheduled container ({container['format']!r}) is marked by stage, a uniform quality is no "
                         "prefix of its order; cut it with stage=")
    if stage is not None:
        if not scheduled:
            raise ValueError(f"truncate: stage= cuts a scheduled container ({FORMAT_SCHEDULED!r}, or {FORMAT_BASE_LANES!r} with a "
                             f"schedule), this one is {container['format']!r} without one; cut it with q=")
        ks = [k for k, st in enumerate(marks["stage"]) if int(st) == int(stage)] if int(stage) == stage else []
        if not ks:
            raise ValueError(f"truncate: stage {stage} is not marked in this container (stages {list(marks['stage'])})")
        q, row = f"stage {int(stage)}", marks["bytes"][ks[0]]
    if slice_bytes is not None:
        cut = [int(v) for v in slice_bytes]
        if len(cut) != ns or min(cut) < 0:
            raise ValueError(f"truncate: slice_bytes takes {ns} lengths >= 0, got {list(slice_bytes)}")
    elif stage is not None:
        cut = [int(v) for v in row]
    elif q is not None:
        ks = [k for k, mq in enumerate(marks["q"]) if float(mq) == float(q)]
        if not ks:
            raise ValueError(f"truncate: quality {q} is not marked in this container (marks {list(marks['q'])}); cut at explicit "
                             "lengths with slice_bytes, or decode the quality from a longer prefix")
        cut = [int(v) for v in marks["bytes"][ks[0]]]
    else:
        fixed = sum(container_bytes(container)[:2]) + (int(container["side_bytes"]) if scheduled else 0)
        if fixed > max_bytes:
            raise ValueError(f"truncate: z and the base slices{' and the schedule' if scheduled else ''} take {fixed} bytes, "
                             f"more than max_bytes = {max_bytes}")
        cut = [0] * ns
        for row in marks["bytes"]:                         # non-decreasing with the quality
            if fixed + sum(int(v) for v in row) <= max_bytes and all(int(v) <= len(s) for v, s in zip(row, emb)):
                cut = [int(v) for v in row]
    if q is not None:
        short = [j for j in range(ns) if cut[j] > len(emb[j])]
        if short:
            raise ValueError(f"truncate: slice {short[0]} holds {len(emb[short[0]])} bytes, the mark of "
                             f"{q if stage is not None else f'quality {q}'} needs "
                             f"{cut[short[0]]}: the container was already cut below it")
    out = dict(container)
    out["embedded"] = [bytes(s[:b]) for s, b in zip(emb, cut)]
    return out


def delta(longer, shorter) -> List[bytes]:
    """Per slice, the bytes of ``longer`` that follow ``shorter``: what a transmitter sends to a receiver that holds
    ``shorter`` (:meth:`EmbeddedDecoder.extend`).  On the host alone, like :func:`truncate`.  ``shorter`` must be a cut of
    ``longer`` — the same format, shape, lanes, z, base and schedule, every embedded string a prefix of ``longer``'s —;
    ValueError names the slice that is not."""
    Ka, Kb = _check_container(longer), _check_container(shorter)
    for key, what in (("format", "format"), ("shape", "shape"), ("z", "z stream"), ("base", "base slices"), ("schedule", "schedule")):
        if (key in longer) != (key in shorter) or not _same(longer.get(key), shorter.get(key)):
            if key == "base" and len(longer["base"]) == len(shorter["base"]):
                j = [_same(a, b) for a, b in zip(longer["base"], shorter["base"])].index(False)
                raise ValueError(f"delta: the base stream of slice {j} differs: the shorter container is no cut of the longer one")
            raise ValueError(f"delta: the containers differ in their {what}: the shorter one is no cut of the longer one")
    if Ka != Kb:
        raise ValueError(f"delta: the containers differ in their lanes ({Kb} and {Ka}): the shorter one is no cut of the longer one")
    if _base_lanes(longer) != _base_lanes(shorter):
        raise ValueError(f"delta: the containers differ in their base_lanes ({_base_lanes(shorter)} and {_base_lanes(longer)}): "
                         "the shorter one is no cut of the longer one")
    ea, eb = longer["embedded"], shorter["embedded"]
    if len(ea) != len(eb):
        raise ValueError(f"delta: the containers hold {len(eb)} and {len(ea)} slices: the shorter one is no cut of the longer one")
    out = []
    for j, (a, b) in enumerate(zip(ea, eb)):
        if len(b) > len(a) or bytes(a[:len(b)]) != bytes(b):
            raise ValueError(f"delta: slice {j}: the shorter container's {len(b)} bytes are no prefix of the longer one's {len(a)}")
        out.append(bytes(a[len(b):]))
    return out


# ------------------------------------------------------------------------------------------------ codestreams (section 9u)
STREAM_MAGIC = b"VAMe"
STREAM_VERSION = 1
_FIXED = struct.Struct("<BBBBHHHHI")       # format digit, flags, lanes, base_lanes, shape[0], shape[1], ns, L, bytes of z
_FLAG_SCHEDULED = 1
FRAME = Frame(STREAM_MAGIC, "an embedded codestream", "codestream", (STREAM_VERSION,), range(_FIXED.size + 8, MAX_HEADER + 1),
              f"a header takes {_FIXED.size + 8} .. {MAX_HEADER}")
_seal = FRAME.seal                         # the preamble of a header and the header


def _format_of(K: int, Kb: int, scheduled: bool) -> str:
    """The format name encode_batch gives a container of these lanes, base lanes and order."""
    return FORMAT_BASE_LANES if Kb > 1 else FORMAT_SCHEDULED if scheduled else FORMAT_LANES if K > 1 else FORMAT


def _u32_table(rows, L: int, ns: int, what: str) -> np.ndarray:
    try:
        a = np.asarray(rows, dtype=np.int64)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"to_bytes: the marks' {what} are integers [{L}][{ns}]") from e
    if a.shape != (L, ns) or (a < 0).any() or (a >= 1 << 32).any():
        raise ValueError(f"to_bytes: the marks' {what} are integers [{L}][{ns}] in 0 .. 2^32 - 1, got shape {list(a.shape)}")
    return a


def to_bytes(container) -> bytes:
    """One UNCUT container of any embedded format as one codestream: preamble, header, z, the ns base
    strings, then the embedded streams in rounds — round k holds, slice by slice, the bytes between mark k - 1 and mark k,
    a last round what follows the last mark.  Every prefix of the result from :func:`need_bytes` on is a container
    (:func:`from_bytes`), and ``from_bytes(to_bytes(c))`` equals ``c`` entry by entry.  Host only.  ValueError for a cut
    container (an embedded string shorter than its last mark's bytes) and for one the format cannot carry."""
    K = _check_container(container)
    c = container
    Kb, scheduled = _base_lanes(c), _scheduled(c)
    if _format_of(K, Kb, scheduled) != c["format"]:
        raise ValueError(f"to_bytes: lanes {K}, base_lanes {Kb}{', a schedule' if scheduled else ''} are format "
                         f"{_format_of(K, Kb, scheduled)!r}, this container says {c['format']!r}")
    keys = {"format", "shape", "z", "base", "embedded", "marks"} | ({"lanes"} if c["format"] != FORMAT else set()) \
        | ({"base_lanes"} if Kb > 1 else set()) | ({"schedule", "side_bytes"} if scheduled else set())
    if set(c) != keys:
        raise ValueError(f"to_bytes: an {c['format']!r} container{' with a schedule' if scheduled else ''} has the keys "
                         f"{sorted(keys)}, this one has {sorted(c, key=str)}")
    try:
        s0, s1 = (int(v) for v in c["shape"])
    except (TypeError, ValueError) as e:
        raise ValueError(f"to_bytes: shape is (H / 64, W / 64), got {c['shape']!r}") from e
    if tuple(c["shape"]) != (s0, s1) or not (1 <= s0 <= 0xFFFF and 1 <= s1 <= 0xFFFF):
        raise ValueError(f"to_bytes: shape is (H / 64, W / 64) with entries in 1 .. 65535, got {c['shape']!r}")
    isb = lambda s: isinstance(s, (bytes, bytearray, memoryview))
    emb, z, base = c["embedded"], c["z"], c["base"]
    if not isinstance(emb, (list, tuple)) or not 1 <= len(emb) <= 0xFFFF or not all(isb(s) for s in emb):
        raise ValueError("to_bytes: \"embedded\" is a list of 1 .. 65535 bytes objects")
    ns = len(emb)
    if not isinstance(z, (list, tuple)) or len(z) != 1 or not isb(z[0]):
        raise ValueError("to_bytes: \"z\" is a list of one bytes object")
    if not isinstance(base, (list, tuple)) or len(base) != ns or not all(isinstance(s, (list, tuple)) and len(s) == 1 and isb(s[0])
                                                                          for s in base):
        raise ValueError(f"to_bytes: \"base\" is a list of {ns} lists of one bytes object each")
    lens = np.asarray([len(z[0])] + [len(s[0]) for s in base] + [len(s) for s in emb], dtype=np.int64)
    if (lens >= 1 << 32).any():
        raise ValueError("to_bytes: a string of 2^32 bytes or more does not fit the header's length fields")
    marks = c["marks"]
    by = "stage" if scheduled else "q"
    if not isinstance(marks, dict) or set(marks) != {by, "count", "bytes"}:
        raise ValueError(f"to_bytes: the marks of this container are a dict of \"{by}\", \"count\" and \"bytes\"")
    try:
        vals = [int(v) if scheduled else float(v) for v in marks[by]]
    except (TypeError, ValueError) as e:
        raise ValueError(f"to_bytes: the marks' \"{by}\" is a list of numbers") from e
    L = len(vals)
    if not 1 <= L <= 0xFFFF or (scheduled and (vals != list(marks[by]) or min(vals) < 0 or max(vals) >= 1 << 32)):
        raise ValueError(f"to_bytes: 1 .. 65535 marks{', stages as integers in 0 .. 2^32 - 1' if scheduled else ''}, got {marks[by]!r}")
    count, cut = _u32_table(marks["count"], L, ns, "counts"), _u32_table(marks["bytes"], L, ns, "bytes")
    down = np.argwhere(np.diff(cut, axis=0) < 0)
    if len(down):
        raise ValueError(f"to_bytes: slice {int(down[0][1])}: the bytes of mark {int(down[0][0]) + 1} lie below those of the mark "
                         "before; marks never decrease")
    short = np.flatnonzero(cut[-1] > lens[1 + ns:])
    if short.size:
        j = int(short[0])
        raise ValueError(f"to_bytes: slice {j} holds {int(lens[1 + ns + j])} bytes, its last mark needs {int(cut[-1, j])}: the "
                         "container was cut; a codestream is made from the uncut container and cut as bytes")
    parts = [_FIXED.pack(_FORMATS.index(c["format"]) + 1, _FLAG_SCHEDULED if scheduled else 0, K, Kb, s0, s1, ns, L, int(lens[0])),
             lens[1:].astype("<u4").tobytes(), np.asarray(vals, dtype="<u4" if scheduled else "<f8").tobytes(),
             count.astype("<u4").tobytes(), cut.astype("<u4").tobytes()]
    if scheduled:
        sc = c["schedule"]
        try:
            lv, ix = np.asarray(sc["levels"], dtype=np.float64).reshape(-1), np.asarray(sc["index"])
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError("to_bytes: the schedule is {\"levels\": floats, \"index\": uint8 [stages, H / 16, W / 16]}") from e
        if ix.dtype != np.uint8 or ix.ndim != 3 or ix.shape[1:] != (4 * s0, 4 * s1) or not 1 <= ix.shape[0] <= 0xFFFF \
                or not 1 <= lv.size <= 0xFFFF:
            raise ValueError(f"to_bytes: the schedule's index is uint8 [stages, {4 * s0}, {4 * s1}] beside 1 .. 65535 levels, got "
                             f"{ix.dtype} {list(ix.shape)} and {lv.size} levels")
        if c["side_bytes"] != 8 * lv.size + ix.size:
            raise ValueError(f"to_bytes: side_bytes is 8 per level and 1 per index entry, {8 * lv.size + ix.size}, got {c['side_bytes']!r}")
        parts += [struct.pack("<HH", lv.size, ix.shape[0]), lv.astype("<f8").tobytes(), np.ascontiguousarray(ix).tobytes()]
    hlen = sum(len(p) for p in parts) + 8
    if hlen > MAX_HEADER:
        raise ValueError(f"to_bytes: the header would take {hlen} bytes, the limit is {MAX_HEADER}")
    parts.append(struct.pack("<Q", PREAMBLE_BYTES + hlen + int(lens.sum())))
    header = b"".join(parts)
    out = [_seal(header), bytes(z[0])] + [bytes(s[0]) for s in base]
    edge = np.concatenate([np.zeros((1, ns), dtype=np.int64), cut, lens[None, 1 + ns:]])
    out += [bytes(emb[j][int(edge[k, j]):int(edge[k + 1, j])]) for k in range(L + 1) for j in range(ns)]
    return b"".join(out)


class _Stream:
    """A parsed codestream header: the fields, and the byte arithmetic of the body that follows from them."""

    def __init__(self, d, what: str):
        """Parses ``d`` (bytes that hold at least the header, or ``FRAME.open`` says what is needed).  ValueError names what
        is wrong; nothing beyond the stated header length is read."""
        from . import bitstream as bs
        d, _, hlen, end = FRAME.open(d, what)
        self.header_end, at = end, PREAMBLE_BYTES

        def take(dtype, n):
            nonlocal at
            size = n * np.dtype(dtype).itemsize
            if at + size > end:
                raise ValueError(f"{what}: the header's fields need more than its stated {hlen} bytes: it contradicts itself")
            a = np.frombuffer(d, dtype=dtype, count=n, offset=at)
            at += size
            return a
        digit, flags, K, Kb, s0, s1, ns, L, z_len = _FIXED.unpack_from(d, at)      # hlen >= _FIXED.size + 8 (_header_end)
        at += _FIXED.size
        if not 1 <= digit <= len(_FORMATS) or flags & ~_FLAG_SCHEDULED:
            raise ValueError(f"{what}: format digit {digit} and flags {flags:#x}: not a header of version {STREAM_VERSION}")
        self.format, self.scheduled = _FORMATS[digit - 1], bool(flags & _FLAG_SCHEDULED)
        for name, v in (("lanes", K), ("base_lanes", Kb)):
            try:
                bs.check_lanes(v)
            except ValueError as e:
                raise ValueError(f"{what}: the header's {name}: {e}") from e
        if _format_of(K, Kb, self.scheduled) != self.format:
            raise ValueError(f"{what}: the header contradicts itself: lanes {K}, base_lanes {Kb}"
                             f"{', scheduled' if self.scheduled else ''} are format {_format_of(K, Kb, self.scheduled)!r}, it says "
                             f"{self.format!r}")
        if not (s0 and s1 and ns and L):
            raise ValueError(f"{what}: the header contradicts itself: shape ({s0}, {s1}), {ns} slices and {L} marks, none may be 0")
        self.lanes, self.base_lanes, self.shape, self.ns, self.L = K, Kb, (s0, s1), ns, L
        lens = take("<u4", 2 * ns).astype(np.int64)
        self.z_len, self.base_len, self.emb_len = z_len, lens[:ns], lens[ns:]
        self.values = [int(v) for v in take("<u4", L)] if self.scheduled else [float(v) for v in take("<f8", L)]
        self.count = take("<u4", L * ns).astype(np.int64).reshape(L, ns)
        self.cut = take("<u4", L * ns).astype(np.int64).reshape(L, ns)
        self.schedule = None
        if self.scheduled:
            n_lv, n_st = (int(v) for v in take("<u2", 2))
            if not (n_lv and n_st):
                raise ValueError(f"{what}: the header contradicts itself: a schedule of {n_lv} levels and {n_st} stages, none may be 0")
            lv = take("<f8", n_lv)
            self.schedule = {"levels": [float(v) for v in lv], "index": take("u1", n_st * 16 * s0 * s1).reshape(n_st, 4 * s0, 4 * s1).copy()}
            self.side_bytes = 8 * n_lv + n_st * 16 * s0 * s1
        self.total = int(take("<u8", 1)[0])
        if at != end:
            raise ValueError(f"{what}: the header's fields take {at - PREAMBLE_BYTES} of its stated {hlen} bytes: it contradicts itself")
        down = np.argwhere(np.diff(self.cut, axis=0) < 0)
        if len(down):
            k, j = int(down[0][0]) + 1, int(down[0][1])
            raise ValueError(f"{what}: the header contradicts itself: slice {j}: the bytes of mark {k}, {int(self.cut[k, j])}, lie "
                             f"below those of mark {k - 1}, {int(self.cut[k - 1, j])}")
        beyond = np.flatnonzero(self.cut[-1] > self.emb_len)
        if beyond.size:
            j = int(beyond[0])
            raise ValueError(f"{what}: the header contradicts itself: slice {j}: its last mark, {int(self.cut[-1, j])} bytes, lies "
                             f"beyond its stream's length, {int(self.emb_len[j])}")
        self.base_end = end + z_len + int(self.base_len.sum())
        if self.base_end + int(self.emb_len.sum()) != self.total:
            raise ValueError(f"{what}: the header contradicts itself: its lengths add up to {self.base_end + int(self.emb_len.sum())} "
                             f"bytes, it states a total of {self.total}")
        # the body: piece (k, j) = bytes edge[k][j] : edge[k + 1][j] of stream j, pieces in round-major order from base_end on
        self.edge = np.concatenate([np.zeros((1, ns), dtype=np.int64), self.cut, self.emb_len[None]])
        self.size = np.diff(self.edge, axis=0)                                   # [L + 1, ns]
        ends = np.cumsum(self.size.reshape(-1))
        self.start = (ends - self.size.reshape(-1)).reshape(L + 1, ns)           # offset of every piece in the body
        self.round_end = [self.base_end + int(v) for v in ends.reshape(L + 1, ns)[:L, -1]]

    def marks(self) -> dict:
        return {"stage" if self.scheduled else "q": list(self.values), "count": [[int(v) for v in row] for row in self.count],
                "bytes": [[int(v) for v in row] for row in self.cut]}

    def slice_lengths(self, n: int) -> np.ndarray:
        """int64 [ns]: the bytes of every embedded stream that the first ``n`` >= base_end bytes of the codestream hold."""
        return np.clip(n - self.base_end - self.start, 0, self.size).sum(0)

    def slices(self, d, lo, hi) -> List[bytes]:
        """Per slice j, bytes lo[j] : hi[j] of embedded stream j, gathered from the codestream ``d`` (which must hold them)."""
        out = []
        for j in range(self.ns):
            a, b, parts = int(lo[j]), int(hi[j]), []
            for k in range(self.L + 1) if a < b else ():
                s, e = int(self.edge[k, j]), int(self.edge[k + 1, j])
                u, v = max(s, a), min(e, b)
                if u < v:
                    off = self.base_end + int(self.start[k, j]) - s
                    parts.append(d[off + u:off + v])
            out.append(b"".join(parts))
        return out

    def same_batch(self, o) -> Optional[str]:
        """What keeps this image and ``o`` out of one decoder, or None."""
        for name, a, b in (("shape", self.shape, o.shape), ("lanes", self.lanes, o.lanes), ("base_lanes", self.base_lanes, o.base_lanes),
                           ("slice count", self.ns, o.ns)):
            if a != b:
                return f"its {name} is {a}, the others' {b}"
        if self.scheduled != o.scheduled:
            return "it is " + ("scheduled, the others are plain" if self.scheduled else "plain, the others are scheduled")
        if self.scheduled and self.schedule["index"].shape[0] != o.schedule["index"].shape[0]:
            return f"it has {self.schedule['index'].shape[0]} stages, the others {o.schedule['index'].shape[0]}"
        return None


def _parse(data, what: str):
    """(view, parsed header) of a codestream that holds its whole header; too few bytes are a ValueError with the need."""
    d = _view(data, what)
    return d, _Stream(d, what)


def need_bytes(data) -> int:
    """The smallest length from which :func:`from_bytes` succeeds on this codestream, as far as ``data`` (any prefix of it)
    tells: the preamble's size while that is incomplete, the header's end while the header is, then the end of the base.
    A damaged preamble or header is a ValueError."""
    d = _view(data, "need_bytes")
    end = FRAME.need_header(d, "need_bytes")
    return end if len(d) < end else _Stream(d, "need_bytes").base_end


def layout(data) -> dict:
    """Where a codestream may be cut, from its header alone (``data``: any prefix that holds the header): ``header_end``,
    ``base_end`` (the least a decoder needs), ``round_end[k]`` (the prefix that is ``truncate`` at mark k), ``total``, and the
    ``marks``, ``lanes``, ``base_lanes``, ``shape``, ``format``, ``ns`` and ``scheduled`` of the container."""
    _, s = _parse(data, "layout")
    return {"header_end": s.header_end, "base_end": s.base_end, "round_end": list(s.round_end), "total": s.total, "marks": s.marks(),
            "lanes": s.lanes, "base_lanes": s.base_lanes, "shape": s.shape, "format": s.format, "ns": s.ns, "scheduled": s.scheduled}


def _container_of(s: "_Stream", d, n: int) -> dict:
    """The container that the first ``n`` bytes of codestream ``d`` hold (base_end <= n <= total, checked by the caller)."""
    at, strings = s.header_end, []
    for ln in [s.z_len] + [int(v) for v in s.base_len]:
        strings.append(bytes(d[at:at + ln]))
        at += ln
    c = {"format": s.format, "shape": s.shape, "z": [strings[0]], "base": [[b] for b in strings[1:]],
         "embedded": s.slices(d, np.zeros(s.ns, dtype=np.int64), s.slice_lengths(n)), "marks": s.marks()}
    if s.format != FORMAT:
        c["lanes"] = s.lanes
    if s.scheduled:
        c["schedule"], c["side_bytes"] = {"levels": list(s.schedule["levels"]), "index": s.schedule["index"].copy()}, s.side_bytes
    if s.base_lanes > 1:
        c["base_lanes"] = s.base_lanes
    return c


def _check_length(s: "_Stream", n: int, what: str):
    if n < s.base_end:
        raise ValueError(f"{what}: {n} bytes end before z and the base do: {s.base_end} bytes are needed, they are decoded whole")
    check_total(n, s.total, what)


def from_bytes(data) -> dict:
    """The container that ``data`` holds: any prefix of a codestream of :func:`need_bytes` bytes or more.  Its embedded
    strings are prefixes of the original's and their lengths sum to ``len(data) - base_end`` — every byte received is used:
    a prefix that ends inside round k gives the earlier slices round k, the later ones round k - 1, and cuts one slice in
    mid-piece, which the tolerant decoder accepts.  The whole codestream gives the container it was made from, entry by
    entry.  Host only; the decoder trusts nothing: a wrong magic or version, a CRC mismatch, a header that contradicts
    itself, bytes beyond the total and too few bytes (with the number needed) are each a ValueError."""
    d, s = _parse(data, "from_bytes")
    _check_length(s, len(d), "from_bytes")
    return _container_of(s, d, len(d))


class EmbeddedDecoder:
    """Decodes a batch of embedded containers of one shape, whole or truncated, each image cut at its own place.  The base
    slices and the progressive (mu, sigma) chain run once, the rank order comes from the decoder's own sigma, and the
    embedded streams are prefix-decoded once (bitstream.decode_prefix_streams): :meth:`available` says how many leading
    elements of every slice are present.  A decoded quality equals ``forward_single_quality(x, q)`` bit for bit.

    The lanes per embedded stream are read from the containers (``"embedded-2"``: their ``"lanes"``); a batch that mixes
    them is refused.  So are the lanes of z and the base (``"embedded-4"``: their ``"base_lanes"``; 1
    without the key): those strings are needed whole, and one that decodes fewer than its elements, or fails with a status,
    is a ValueError naming the image and "z" or the slice — from the tolerant decode on the host coder, from status 1 of
    vam_rans_interleaved_decode_nhwc_device on the device.  ``coder`` (None: ``model.coder``): "host" prefix-decodes on the host's threads from a host copy of
    the ranked indexes; "device"  decodes z and the base slices with the device coder, uploads the
    embedded strings once and prefix-decodes them with ONE launch into the plan's ranked symbols; the counts come back
    with the status codes in one read, and the ranked indexes stay on the device unless :meth:`bits` asks for them.
    Either coder reads either coder's containers.

    Scheduled containers (``"embedded-3"``) bring their schedule: the plan rebuilds the scheduled rank
    order from its own sigma, :meth:`decode` and :meth:`available` work unchanged, :meth:`decode_stages` decodes stages, and
    :meth:`decode_qualities` and :meth:`bits` are refused — a uniform quality is no prefix of a scheduled order.  A batch
    mixes neither scheduled with plain containers nor different stage counts.

    ``resumable=True`` makes the decoder a receiver whose bytes keep arriving: the prefix decode goes
    through the resume path from fresh checkpoints, which the decoder owns next to its ranked symbols (device tensors on the
    device coder, numpy arrays on the host coder), and :meth:`extend` hands it the bytes that follow and decodes only the
    new elements.  With the default nothing changes."""

    def __init__(self, model, containers, coder: Optional[str] = None, resumable: bool = False):
        _check_model(model)
        cs = list(containers)
        if not cs:
            raise ValueError("EmbeddedDecoder: no containers")
        lanes = [_check_container(c) for c in cs]
        if any(k != lanes[0] for k in lanes):
            raise ValueError(f"EmbeddedDecoder: every container must have the same lanes per embedded stream, got "
                             f"{sorted(set(lanes))}; decode them separately")
        self.lanes, self.coder = lanes[0], P._check_coder(model, coder)
        base_lanes = [_base_lanes(c) for c in cs]
        if any(k != base_lanes[0] for k in base_lanes):
            raise ValueError(f"EmbeddedDecoder: every container must have the same base_lanes (the lanes of z and the base slices; "
                             f"1 without the key), got {sorted(set(base_lanes))}; decode them separately")
        self.base_lanes = base_lanes[0]
        sched = [_scheduled(c) for c in cs]
        if any(sched) and not all(sched):
            raise ValueError(f"EmbeddedDecoder: a batch holds scheduled ({FORMAT_SCHEDULED!r}, or {FORMAT_BASE_LANES!r} with a "
                             "schedule) or plain containers, not both (their rank orders differ); decode them separately")
        self.scheduled = sched[0]
        shape = tuple(cs[0]["shape"])
        for c in cs[1:]:
            if tuple(c["shape"]) != shape:
                raise ValueError(f"EmbeddedDecoder: every container must have the same shape, got {shape} and "
                                 f"{tuple(c['shape'])}; decode them separately")
        self.m, self.containers, self.B = model, cs, len(cs)
        from .control import _prepare
        _prepare(model, policy=False)
        hz, wz = int(shape[0]), int(shape[1])
        self.H, self.W = 64 * hz, 64 * wz
        _check_shape(model, self.B, self.H, self.W, "EmbeddedDecoder")
        ns = model.ns0
        if any(len(c["embedded"]) != ns or len(c["base"]) != ns for c in cs):
            raise ValueError(f"EmbeddedDecoder: a container of this model has {ns} base and {ns} embedded streams")
        self.schedule = _schedule_of(cs) if self.scheduled else None      # (levels, index [B, L, h, w])
        self.n_stages = int(self.schedule[1].shape[1]) if self.scheduled else 0
        self.dp = model._emb_dec_plan(self.B, hz, wz, self.coder, scheduled=self.scheduled)
        self._stage_count = None                            # (device, host) int [L, B, ns]: #(stage id <= k) per segment
        self._avail: Optional[np.ndarray] = None
        self.resumable = bool(resumable)
        self._ck = None                                     # resumable: bitstream.Checkpoints of the B * ns embedded streams
        self._pos = np.zeros(self.B * ns, dtype=np.int64)   # resumable: the host's copy of every stream's word position
        self.extend_bytes = 0                               # payload bytes the last extend handed to the coder
        self.idx_r: Optional[np.ndarray] = None             # host copy of the ranked indexes (device coder: only for bits())
        with torch.no_grad():
            self._front()

    def _front(self):
        from . import bitstream as bs
        cs, ns, dp = self.containers, self.m.ns0, self.dp
        if self.scheduled:
            dp.fill_schedule(*self.schedule)                # before the chain that reads it, on the same stream
            self._stage_count = None
        up = dp.front([[c["base"][i][0] for c in cs] for i in range(ns)], [c["z"][0] for c in cs], lanes=self.base_lanes,
                      interleaved=self.base_lanes > 1)
        dp.owner = self
        if self.coder == "device":
            return self._front_device(up)
        if self._avail is None:                             # the host's one pass over the embedded streams
            self.idx_r = dp.idx_r.cpu().numpy()             # [B, ns, n]
            self.ranked = np.zeros(self.idx_r.shape, dtype=np.int32)
            if self.resumable:
                self._ck = bs.Checkpoints.fresh(self.B * ns, self.lanes)
                self._resume_host()
            else:
                jobs = [(c["embedded"][j], self.idx_r[b, j], self.ranked[b, j]) for b, c in enumerate(cs) for j in range(ns)]
                got = bs.decode_prefix_streams(jobs, bs.Tables.of(self.m.gaussian_conditional), lanes=self.lanes)
                self._avail = np.asarray(got, dtype=np.int64).reshape(self.B, ns)
        with dp.runner.on_stream():
            dp.ranked.copy_(torch.from_numpy(self.ranked))

    def _front_device(self, up):
        """The embedded strings go up once and ONE launch prefix-decodes them from the plan's ranked indexes into its ranked
        symbols; this decoder keeps its own copy of them for when another decoder has used the plans since."""
        from . import _lib as L
        from . import bitstream as bs
        cs, ns, dp, B = self.containers, self.m.ns0, self.dp, self.B
        with dp.runner.on_stream():
            if self._avail is None and self.resumable:
                self._ck = bs.Checkpoints.fresh(B * ns, self.lanes, dp.device)
                self._meta = torch.zeros((3, B * ns), dtype=torch.int32, device=dp.device)
                self._ck.pos = self._meta[2]                # the kernel's pos comes back with the one read of meta
                self.ranked = torch.zeros_like(dp.ranked)
                got = self._resume_device()
            elif self._avail is None:
                emb = bs.upload_streams([c["embedded"][j] for c in cs for j in range(ns)], dp.device)
                meta = torch.empty((2, B * ns), dtype=torch.int32, device=dp.device)
                bs.decode_embedded_uploaded(emb, 0, dp.idx_r, dp.ranked, bs.DeviceCoderTables.of(self.m.gaussian_conditional, dp.device),
                                            self.lanes, meta)
                self.ranked = dp.ranked.clone()
                got = meta.cpu().numpy()                    # the one read: available counts and status codes
            else:
                dp.ranked.copy_(self.ranked)
                got = None
            try:
                bs.check_status(up, B, "EmbeddedDecoder", lambda k: f"z stream (image {k})" if k < B else
                                f"base stream (image {k % B}, slice {k // B - 1})")
            except L.VamError as e:
                if self.base_lanes == 1:
                    raise
                raise ValueError(f"{e} (z and the base of an {FORMAT_BASE_LANES!r} container are needed whole)") from e
        if got is not None:
            bad = np.flatnonzero(got[1])
            if bad.size:
                k = int(bad[0])
                raise L.VamError(f"EmbeddedDecoder: embedded stream (image {k // ns}, slice {k % ns}): "
                                 f"{bs.status_text(int(got[1][k]))}")
            self._avail = got[0].astype(np.int64).reshape(B, ns)

    def _tails(self) -> List[bytes]:
        """Per embedded stream (image-major) the bytes its container holds from byte 4 * pos on."""
        ns = self.m.ns0
        return [c["embedded"][j][4 * int(self._pos[b * ns + j]):] for b, c in enumerate(self.containers) for j in range(ns)]

    def _raise_status(self, status: np.ndarray):
        from . import _lib as L
        from . import bitstream as bs
        bad = np.flatnonzero(status)
        if bad.size:
            k, ns = int(bad[0]), self.m.ns0
            raise L.VamError(f"EmbeddedDecoder: embedded stream (image {k // ns}, slice {k % ns}): "
                             f"{bs.status_text(int(status[k]))}")

    def _resume_host(self):
        """The resume call on the thread pool, every stream from its bytes at 4 * pos, into the host's ranked symbols."""
        from . import _lib as L
        from . import bitstream as bs
        ns, tails = self.m.ns0, self._tails()
        jobs = [(tails[k], self.idx_r[k // ns, k % ns], self.ranked[k // ns, k % ns]) for k in range(self.B * ns)]
        status = np.zeros(self.B * ns, dtype=np.int32)
        self.extend_bytes = sum(len(t) for t in tails)
        try:
            got = bs.resume_prefix_streams(jobs, bs.Tables.of(self.m.gaussian_conditional), self._ck, lanes=self.lanes, status=status)
        except L.VamError:
            self._pos[:] = self._ck.pos
            self._raise_status(status)
            raise
        self._pos[:] = self._ck.pos
        self._avail = np.asarray(got, dtype=np.int64).reshape(self.B, ns)

    def _resume_device(self) -> np.ndarray:
        """ONE upload of every stream's bytes from 4 * pos on, ONE launch into the decoder's own ranked symbols, ONE read of
        meta (available, status, pos); then the plan's ranked symbols are refreshed on the device.  Returns meta."""
        from . import bitstream as bs
        dp, tails = self.dp, self._tails()
        self.extend_bytes = sum(len(t) for t in tails)
        up = bs.upload_streams(tails, dp.device)
        bs.resume_embedded_uploaded(up, 0, dp.idx_r, self.ranked, bs.DeviceCoderTables.of(self.m.gaussian_conditional, dp.device),
                                    self.lanes, self._ck, self._meta)
        dp.ranked.copy_(self.ranked)
        got = self._meta.cpu().numpy()
        self._pos[:] = got[2]
        return got

    def extend(self, more) -> np.ndarray:
        """Hand a resumable decoder the bytes that follow what it holds: ``more`` has one entry per container, each a
        sequence of ns ``bytes`` objects (``b""`` allowed), e.g. :func:`delta`'s.  Only the elements the new bytes reach are
        entropy-decoded, from each stream's checkpoint.  Returns the new :meth:`available`.  Afterwards the decoder is
        indistinguishable from a fresh one on the concatenated containers, which ``self.containers`` then holds.
        Host coder: the resume call on the thread pool, then the device copy of the ranked symbols is refreshed.  Device
        coder: one host-to-device copy of every stream's bytes from its last whole decoded group on, one launch, one read of
        (available, status, pos); no symbols or indexes cross to the host.  ``self.extend_bytes``: the payload bytes handed to
        the coder."""
        ns = self.m.ns0
        if not self.resumable:
            raise ValueError("EmbeddedDecoder.extend: this decoder keeps no checkpoints; build it with resumable=True")
        try:
            more = [list(row) for row in more]
        except TypeError as e:
            raise ValueError(f"EmbeddedDecoder.extend: expected {self.B} sequences of {ns} bytes objects") from e
        if len(more) != self.B or any(len(row) != ns for row in more):
            raise ValueError(f"EmbeddedDecoder.extend: expected {self.B} entries of {ns} slices each, got "
                             f"{[len(row) for row in more]}")
        for b, row in enumerate(more):
            for j, s in enumerate(row):
                if not isinstance(s, (bytes, bytearray, memoryview)):
                    raise ValueError(f"EmbeddedDecoder.extend: image {b}, slice {j}: expected bytes, got {type(s).__name__}")
        cs = []
        for c, row in zip(self.containers, more):
            c = dict(c)
            c["embedded"] = [bytes(old) + bytes(s) for old, s in zip(c["embedded"], row)]
            cs.append(c)
        with torch.no_grad():
            self._own()
            self.containers = cs
            if self.coder == "device":
                with self.dp.runner.on_stream():
                    got = self._resume_device()
                self._raise_status(got[1])
                self._avail = got[0].astype(np.int64).reshape(self.B, ns)
            else:
                self._resume_host()
                with self.dp.runner.on_stream():
                    self.dp.ranked.copy_(torch.from_numpy(self.ranked))
        return self.available()

    def _idx_r(self) -> np.ndarray:
        if self.idx_r is None:
            self._own()
            self.idx_r = self.dp.idx_r.cpu().numpy()
        return self.idx_r

    def _own(self):
        if self.dp.owner is not self:                       # another decoder ran on the same plans since
            self._front()

    def available(self) -> np.ndarray:
        """int [B][ns]: the leading elements (in rank order) of every slice that the held bytes decode."""
        return self._avail.copy()

    def _result(self, t, i):
        return {"x_hat": t.x_hat[i * self.B:(i + 1) * self.B].clone(), "y_hat": t.level(t.y_prog, i).torch_nchw().clone()}

    def decode(self) -> dict:
        """{"x_hat", "y_hat"} from everything present, as one level: an element of rank r < available is dequantised, the
        others take mu."""
        with torch.no_grad():
            self._own()
            t = self.dp.tail_counts(self._avail.astype(np.int32)[None], self.m.use_graph)
            return self._result(t, 0)

    def _counts(self, qs: Sequence[float]):
        """Device counts [len(qs), B, ns] of the non-decreasing qualities ``qs`` from the decoder's own sigma."""
        from . import _lib as L
        G = L.VAM_MAX_LAYER_LEVELS
        parts = [self.dp.quality_counts(qs[i:i + G]) for i in range(0, len(qs), G)]
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def _check_present(self, qs, count: np.ndarray):
        for k, q in enumerate(qs):
            short = np.argwhere(count[k] > self._avail)
            if len(short):
                b, j = (int(v) for v in short[0])
                raise ValueError(f"EmbeddedDecoder: quality {q} needs {int(count[k, b, j])} elements of slice {j} of image {b}, "
                                 f"its container holds {int(self._avail[b, j])}")

    def _refuse_scheduled(self, what: str):
        if self.scheduled:
            raise ValueError(f"EmbeddedDecoder.{what}: these containers are scheduled ({self.containers[0]['format']!r}); a uniform quality is "
                             "no prefix of a scheduled rank order, decode stages with decode_stages")

    def decode_stages(self, ks: Sequence[int]) -> List[dict]:
        """{"x_hat", "y_hat"} of the batch per stage of ``ks`` (any stages 0 .. L-1 in any order) of a scheduled decoder:
        stage k equals ``forward_quality_map(x, S[k])`` bit for bit.  The counts come from the decoder's own sigma and the
        containers' schedule (vam_rank_counts on the stage ids); ValueError when a container holds too little for a stage."""
        from .control import sweep_groups
        if not self.scheduled:
            raise ValueError("EmbeddedDecoder.decode_stages: these containers carry no schedule; decode qualities with "
                             "decode_qualities")
        ks = list(ks)
        if not ks or any(isinstance(k, bool) or int(k) != k or not 0 <= int(k) < self.n_stages for k in ks):
            raise ValueError(f"stages must be integers in 0..{self.n_stages - 1}, got {ks}")
        ks = [int(k) for k in ks]
        with torch.no_grad():
            self._own()
            dp, use_graph = self.dp, self.m.use_graph
            if self._stage_count is None:
                count = dp.stage_counts(self.n_stages)
                self._stage_count = (count, count.cpu().numpy())
            count, host = self._stage_count
            for k in sorted(set(ks)):
                short = np.argwhere(host[k] > self._avail)
                if len(short):
                    b, j = (int(v) for v in short[0])
                    raise ValueError(f"EmbeddedDecoder: stage {k} needs {int(host[k, b, j])} elements of slice {j} of image {b}, "
                                     f"its container holds {int(self._avail[b, j])}")
            out: List[Optional[dict]] = [None] * len(ks)
            pos = sorted(range(len(ks)), key=lambda g: ks[g])              # the counts never decrease with the stage
            count = count[[ks[g] for g in pos]].contiguous()
            for _, _, groups in sweep_groups(len(pos), self.B, self.H, self.W):
                for l0, l1 in groups:
                    t = dp.tail_counts(count[l0:l1], use_graph)
                    for i, g in enumerate(pos[l0:l1]):
                        out[g] = self._result(t, i)
        return out

    def decode_marks(self, ks: Sequence[int]) -> List[dict]:
        """{"x_hat", "y_hat"} of the batch per mark of ``ks`` (any marks 0 .. L-1 in any order), every slice at the element
        count the container's OWN mark states (``marks["count"][k]``), not at a count derived from the decoder's sigma.  On an
        ordinary container mark k equals ``decode_qualities([q_k])`` bit for bit, on a scheduled one ``decode_stages([k])``;
        the marks of a tile of a picture with picture-wide marks state the picture's counts, which no
        quality of the tile alone gives.  ValueError when a container holds too little for a mark."""
        from .control import sweep_groups
        ks = list(ks)
        rows = [np.asarray(c["marks"]["count"], dtype=np.int64).reshape(-1, self.m.ns0) for c in self.containers]
        n_marks = min(r.shape[0] for r in rows)
        if not ks or any(isinstance(k, bool) or int(k) != k or not 0 <= int(k) < n_marks for k in ks):
            raise ValueError(f"marks must be integers in 0..{n_marks - 1} (the marks every container carries), got {ks}")
        ks = [int(k) for k in ks]
        pos = sorted(range(len(ks)), key=lambda g: ks[g])                  # a container's counts never decrease with the mark
        host = np.stack([np.stack([r[ks[g]] for r in rows]) for g in pos])  # [len(ks), B, ns]
        if (np.diff(host, axis=0) < 0).any() or (host < 0).any():
            raise ValueError("EmbeddedDecoder.decode_marks: a container's mark counts decrease with the mark or are negative")
        for i, g in enumerate(pos):
            short = np.argwhere(host[i] > self._avail)
            if len(short):
                b, j = (int(v) for v in short[0])
                raise ValueError(f"EmbeddedDecoder: mark {ks[g]} needs {int(host[i, b, j])} elements of slice {j} of image {b}, "
                                 f"its container holds {int(self._avail[b, j])}")
        with torch.no_grad():
            self._own()
            out: List[Optional[dict]] = [None] * len(ks)
            count = host.astype(np.int32)
            for _, _, groups in sweep_groups(len(pos), self.B, self.H, self.W):
                for l0, l1 in groups:
                    t = self.dp.tail_counts(count[l0:l1], self.m.use_graph)
                    for i, g in enumerate(pos[l0:l1]):
                        out[g] = self._result(t, i)
        return out

    def decode_qualities(self, qs: Sequence[float]) -> List[dict]:
        """{"x_hat", "y_hat"} of the batch per quality of ``qs`` (any qualities >= 0 in any order, marked or not; 0 is the
        base, g_s[0] on y_hat_base).  The counts come from the decoder's own sigma; ValueError when a container holds too
        little for one of them."""
        from .control import sweep_groups
        self._refuse_scheduled("decode_qualities")
        qs = [float(q) for q in qs]
        if not qs or any(not (q >= 0.0) or math.isinf(q) for q in qs):
            raise ValueError(f"qualities must be finite and >= 0, got {qs}")
        with torch.no_grad():
            self._own()
            out: List[Optional[dict]] = [None] * len(qs)
            dp, use_graph = self.dp, self.m.use_graph
            pos = sorted((g for g, q in enumerate(qs) if q > 0), key=lambda g: qs[g])
            if pos:
                sq = [qs[g] for g in pos]
                count = self._counts(sq)
                self._check_present(sq, count.cpu().numpy())
            if len(pos) < len(qs):
                dp.base(use_graph)
                for g, q in enumerate(qs):
                    if q == 0:
                        out[g] = {"x_hat": dp.x_hat.clone(), "y_hat": dp.yb.torch_nchw().clone()}
            for _, _, groups in sweep_groups(len(pos), self.B, self.H, self.W):
                for l0, l1 in groups:
                    t = dp.tail_counts(count[l0:l1], use_graph)
                    for i, g in enumerate(pos[l0:l1]):
                        out[g] = self._result(t, i)
        return out

    def bits(self, q: float) -> List[float]:
        """Each image's bits up to quality ``q``: z, the base and, per slice, the shortest prefix that decodes the elements
        of that quality's mask (0 = the base alone)."""
        from . import bitstream as bs
        self._refuse_scheduled("bits")
        q = float(q)
        if not (q >= 0.0) or math.isinf(q):
            raise ValueError(f"qualities must be finite and >= 0, got {q}")
        fixed = [8.0 * sum(container_bytes(c)[:2]) for c in self.containers]
        if q == 0:
            return fixed
        ns = self.m.ns0
        with torch.no_grad():
            self._own()
            count = self._counts([q]).cpu().numpy()
        self._check_present([q], count)
        tg = bs.Tables.of(self.m.gaussian_conditional)
        idx_r = self._idx_r()
        cut = _map_threads(lambda bj: bs.prefix_bytes(self.containers[bj[0]]["embedded"][bj[1]], idx_r[bj[0], bj[1]],
                                                      [int(count[0, bj[0], bj[1]])], tg, lanes=self.lanes)[0],
                           [(b, j) for b in range(self.B) for j in range(ns)])
        return [fixed[b] + 8.0 * sum(cut[b * ns:(b + 1) * ns]) for b in range(self.B)]


class StreamDecoder:
    """A receiver of codestreams: ``n_images`` images of one batch, each arriving as raw bytes in chunks
    that may end anywhere — inside the header, inside a word.  :meth:`feed` keeps every image's bytes and parses its header
    as soon as it is complete; when ALL images hold z and the base whole it builds one
    ``EmbeddedDecoder(model, [from_bytes(...)], coder, resumable=True)``, and from then on every feed turns the new bytes into
    per-slice deltas by the header's arithmetic (no transmitter-side :func:`delta`) and calls
    :meth:`EmbeddedDecoder.extend`: nothing is entropy-decoded twice.  After any sequence of feeds :meth:`decode`,
    :meth:`available` and the inner decoder equal, bit for bit, a fresh ``EmbeddedDecoder`` on ``from_bytes`` of everything
    fed so far, on both coders.  The images must agree in shape, lanes, base_lanes, schedule-or-not and stage count; the one
    that does not is refused, by its number, at the feed that completes its header.  A refused feed changes nothing: it is
    checked as a whole before anything is kept, and when the feed that completes z and the base makes ``EmbeddedDecoder``
    raise (a damaged base string, a coder status) its bytes are dropped again, so the decoder stays not ready and says so.
    Only :meth:`EmbeddedDecoder.extend` of a ready decoder keeps the bytes it was handed when it raises a coder status, as it
    does on its own."""

    def __init__(self, model, n_images: int, coder: Optional[str] = None):
        _check_model(model)
        if isinstance(n_images, bool) or not isinstance(n_images, (int, np.integer)) or n_images < 1:
            raise ValueError(f"StreamDecoder: n_images is an integer >= 1, got {n_images!r}")
        self.m, self.B, self.coder = model, int(n_images), P._check_coder(model, coder)
        self._buf = [bytearray() for _ in range(self.B)]
        self._hdr: List[Optional[_Stream]] = [None] * self.B
        self._held: List[Optional[np.ndarray]] = [None] * self.B      # per image the bytes of every slice the inner decoder holds
        self.decoder: Optional[EmbeddedDecoder] = None
        self.extend_bytes = 0                               # payload bytes the last feed handed to the coder

    @property
    def ready(self) -> bool:
        """Whether every image held z and the base at the last feed: there is a picture to decode."""
        return self.decoder is not None

    def need(self) -> List[int]:
        """Per image the bytes it still lacks before the first picture, as far as its bytes tell (:func:`need_bytes`)."""
        return [max(0, (h.base_end if h is not None else need_bytes(bytes(b))) - len(b)) for h, b in zip(self._hdr, self._buf)]

    def feed(self, chunks) -> Optional[np.ndarray]:
        """``chunks``: one bytes-like object per image, ``b""`` allowed, each the bytes that follow what the image was fed
        before.  Returns :meth:`available`, or None while an image still lacks part of its header, z or base."""
        try:
            chunks = list(chunks)
        except TypeError as e:
            raise ValueError(f"StreamDecoder.feed: expected {self.B} bytes-like objects, one per image") from e
        if len(chunks) != self.B:
            raise ValueError(f"StreamDecoder.feed: expected {self.B} chunks, one per image, got {len(chunks)}")
        chunks = [chunk_view(ch, f"StreamDecoder.feed: image {b}") for b, ch in enumerate(chunks)]
        hdr, before = list(self._hdr), (list(self._hdr), [len(buf) for buf in self._buf])
        for b, ch in enumerate(chunks):                     # everything is checked before anything is kept
            if hdr[b] is None:
                d = memoryview(bytes(self._buf[b]) + bytes(ch))
                if FRAME.whole(d, f"StreamDecoder.feed: image {b}"):
                    hdr[b] = _Stream(d, f"StreamDecoder.feed: image {b}")
                    if hdr[b].ns != self.m.ns0:
                        raise ValueError(f"StreamDecoder.feed: image {b}: its codestream holds {hdr[b].ns} slices, a container of this "
                                         f"model has {self.m.ns0}")
                    other = next((h for a, h in enumerate(hdr) if h is not None and a != b), None)
                    why = hdr[b].same_batch(other) if other is not None else None
                    if why:
                        raise ValueError(f"StreamDecoder.feed: image {b} does not belong to this batch: {why}; decode it separately")
            if hdr[b] is not None:
                check_total(len(self._buf[b]) + len(ch), hdr[b].total, f"StreamDecoder.feed: image {b}", per_image=True)
        self._hdr = hdr
        for buf, ch in zip(self._buf, chunks):
            buf += ch
        self.extend_bytes = 0
        if any(h is None or len(buf) < h.base_end for h, buf in zip(hdr, self._buf)):
            return None
        now = [h.slice_lengths(len(buf)) for h, buf in zip(hdr, self._buf)]
        if self.decoder is None:
            views = [memoryview(buf) for buf in self._buf]
            try:
                cs = [_container_of(h, d, len(d)) for h, d in zip(hdr, views)]
            finally:
                for d in views:
                    d.release()
            try:
                self.decoder = EmbeddedDecoder(self.m, cs, self.coder, resumable=True)
            except Exception:                               # a damaged z or base, a coder status: this feed is not kept either
                self._hdr = before[0]
                for buf, n in zip(self._buf, before[1]):
                    del buf[n:]
                raise
            self._held = now
            self.extend_bytes = self.decoder.extend_bytes
        elif any((a != b).any() for a, b in zip(now, self._held)):
            views = [memoryview(buf) for buf in self._buf]
            try:
                more = [h.slices(d, lo, hi) for h, d, lo, hi in zip(hdr, views, self._held, now)]
            finally:
                for d in views:
                    d.release()
            self._held = now                                # extend keeps the bytes even when it raises a coder status
            self.decoder.extend(more)
            self.extend_bytes = self.decoder.extend_bytes
        return self.available()

    def available(self) -> Optional[np.ndarray]:
        """int [B][ns] as :meth:`EmbeddedDecoder.available`; None while not ready."""
        return self.decoder.available() if self.ready else None

    def _inner(self, what: str) -> "EmbeddedDecoder":
        if not self.ready:
            need = self.need()
            b = next((k for k, v in enumerate(need) if v), 0)
            raise ValueError(f"StreamDecoder.{what}: nothing to decode yet: image {b} lacks {need[b]} bytes of its header, z "
                             "and base")
        return self.decoder

    def decode(self) -> dict:
        return self._inner("decode").decode()

    def decode_stages(self, ks: Sequence[int]) -> List[dict]:
        return self._inner("decode_stages").decode_stages(ks)

    def decode_qualities(self, qs: Sequence[float]) -> List[dict]:
        return self._inner("decode_qualities").decode_qualities(qs)
