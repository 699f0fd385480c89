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
"""
from __future__ import annotations

import math
import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import progressive as P
from .progressive import Q_LIST

FORMAT = "embedded-1"
FORMAT_LANES = "embedded-2"          # embedded streams on K > 1 interleaved lanes; carries "lanes": K
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


def encode_batch(model, x, marks: Sequence[float] = Q_LIST, save_path=None, coder: Optional[str] = None, lanes: int = 1) -> List[dict]:
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
    from the argument only, never from ``model.coder_lanes``.  K = 1 is format ``"embedded-1"`` with no new key."""
    from . import _lib as L
    from . import bitstream as bs
    from . import ops
    from .models import EMPTY_SCALE_TABLE
    _check_model(model)
    qs = P.check_q_list(marks)
    coder, K = P._check_coder(model, coder), bs.check_lanes(lanes)
    m = model
    B, _, H, W = x.shape
    d, C, ns = m.division_dimension[0], m.dim_chunk, m.ns0
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
        ops.variance_rank(plan.std_p, perm, n_slice=ns, workspace=ops.rank_workspace(plan.std_p, ns, dev))
        r_sym, r_idx = torch.empty_like(perm), torch.empty_like(perm)
        ops.rank_gather(perm, ns, plan.sym.window(d, d), r_sym, plan.idx.window(d, d), r_idx)
        layer = torch.empty((B, h, w, d), dtype=torch.uint8, device=dev)
        ops.variance_layers(plan.std_p, qs, layer, n_slice=ns)               # the masks of the marks, as every plan builds them
        count = torch.empty((len(qs), B, ns), dtype=torch.int32, device=dev)
        ops.rank_counts(layer, perm, ns, len(qs), count)
        if coder == "device":
            tg, te = bs.DeviceCoderTables.of(m.gaussian_conditional, dev), bs.DeviceCoderTables.of(m.entropy_bottleneck, dev)
            z_str = bs.encode_streams_device(plan.z_sym, None, 1, m.N, te)[0]
            base = bs.encode_streams_device(plan.sym, plan.idx, ns, C, tg)                      # [slice][image]
            emb_str, cut = bs.encode_embedded_device(r_sym, r_idx, tg, K, count)                # stream b * ns + j
            cuts = cut.reshape(len(qs), B, ns)
            count = count.cpu().numpy().astype(np.int64)
        else:
            nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu().numpy()
            sym_b, idx_b, zs = nchw(plan.sym.buf[..., :d]), nchw(plan.idx.buf[..., :d]), nchw(plan.z_sym.buf)
            r_sym, r_idx, count = r_sym.cpu().numpy(), r_idx.cpu().numpy(), count.cpu().numpy().astype(np.int64)
    if coder == "host":
        tg, te = bs.Tables.of(m.gaussian_conditional), bs.Tables.of(m.entropy_bottleneck)
        zi = np.broadcast_to(np.arange(m.N, dtype=np.int32)[:, None, None], zs.shape[1:])
        z_str = bs.encode_streams([(zs[b], zi) for b in range(B)], te)
        sl = lambda a, b, i: a[b, i * C:(i + 1) * C]
        jobs = [(sl(sym_b, b, i), sl(idx_b, b, i)) for i in range(ns) for b in range(B)]
        e_jobs = [(r_sym[b, j], r_idx[b, j]) for b in range(B) for j in range(ns)]
        if K == 1:                                                                              # one call, as ever
            y_str = bs.encode_streams(jobs + e_jobs, tg)
            emb_str = y_str[ns * B:]
        else:
            y_str = bs.encode_streams(jobs, tg)
            emb_str = bs.encode_interleaved_streams(e_jobs, tg, lanes=K)
        base = [y_str[i * B:(i + 1) * B] for i in range(ns)]
        got = _map_threads(lambda bj: bs.prefix_bytes(emb_str[bj[0] * ns + bj[1]], r_idx[bj[0], bj[1]],
                                                      count[:, bj[0], bj[1]].tolist(), tg, lanes=K),
                           [(b, j) for b in range(B) for j in range(ns)])
        cuts = np.asarray(got, dtype=np.int64).reshape(B, ns, len(qs)).transpose(2, 0, 1)
    containers = []
    for b in range(B):
        c = {"format": FORMAT if K == 1 else FORMAT_LANES, "shape": (H // 64, W // 64), "z": [z_str[b]],
             "base": [[base[i][b]] for i in range(ns)], "embedded": [emb_str[b * ns + j] for j in range(ns)],
             "marks": {"q": list(qs), "count": [[int(count[k, b, j]) for j in range(ns)] for k in range(len(qs))],
                       "bytes": [[int(cuts[k, b, j]) for j in range(ns)] for k in range(len(qs))]}}
        if K > 1:
            c["lanes"] = K
        containers.append(c)
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        for b, c in enumerate(containers):
            with open(os.path.join(save_path, "embedded.pkl" if B == 1 else f"embedded_{b}.pkl"), "wb") as f:
                pickle.dump(c, f)
    return containers


def _check_container(c) -> int:
    """The lanes per embedded stream of container ``c``: 1 for ``"embedded-1"``, its ``"lanes"`` for ``"embedded-2"``."""
    from . import bitstream as bs
    if not isinstance(c, dict) or c.get("format") not in (FORMAT, FORMAT_LANES):
        raise ValueError(f"not an embedded container (format {FORMAT!r} or {FORMAT_LANES!r}): got "
                         f"{c.get('format') if isinstance(c, dict) else type(c).__name__!r}")
    if c["format"] == FORMAT:
        return 1
    K = bs.check_lanes(c.get("lanes"))
    if K == 1:
        raise ValueError(f"an {FORMAT_LANES!r} container carries lanes > 1; one lane is format {FORMAT!r}")
    return K


def truncate(container, q: Optional[float] = None, max_bytes: Optional[int] = None,
             slice_bytes: Optional[Sequence[int]] = None) -> dict:
    """A copy of ``container`` with its embedded streams cut, on the host alone (what a server or a transmitter does).
    Exactly one of: ``q`` — a marked quality: every slice is cut at that mark's bytes; ``max_bytes`` — the largest mark
    whose z + base + embedded total fits (the base alone when no mark fits, ValueError when not even the base does);
    ``slice_bytes`` — one explicit length per slice, any byte count (a length beyond what the slice holds keeps it whole)."""
    _check_container(container)
    if sum(a is not None for a in (q, max_bytes, slice_bytes)) != 1:
        raise ValueError("truncate: give exactly one of q, max_bytes and slice_bytes")
    emb, marks = container["embedded"], container["marks"]
    ns = len(emb)
    if slice_bytes is not None:
        cut = [int(v) for v in slice_bytes]
        if len(cut) != ns or min(cut) < 0:
            raise ValueError(f"truncate: slice_bytes takes {ns} lengths >= 0, got {list(slice_bytes)}")
    elif q is not None:
        ks = [k for k, mq in enumerate(marks["q"]) if float(mq) == float(q)]
        if not ks:
            raise ValueError(f"truncate: quality {q} is not marked in this container (marks {list(marks['q'])}); cut at explicit "
                             "lengths with slice_bytes, or decode the quality from a longer prefix")
        cut = [int(v) for v in marks["bytes"][ks[0]]]
    else:
        fixed = sum(container_bytes(container)[:2])
        if fixed > max_bytes:
            raise ValueError(f"truncate: z and the base slices take {fixed} bytes, more than max_bytes = {max_bytes}")
        cut = [0] * ns
        for row in marks["bytes"]:                         # non-decreasing with the quality
            if fixed + sum(int(v) for v in row) <= max_bytes and all(int(v) <= len(s) for v, s in zip(row, emb)):
                cut = [int(v) for v in row]
    if q is not None:
        short = [j for j in range(ns) if cut[j] > len(emb[j])]
        if short:
            raise ValueError(f"truncate: slice {short[0]} holds {len(emb[short[0]])} bytes, the mark of quality {q} needs "
                             f"{cut[short[0]]}: the container was already cut below it")
    out = dict(container)
    out["embedded"] = [bytes(s[:b]) for s, b in zip(emb, cut)]
    return out


class EmbeddedDecoder:
    """Decodes a batch of embedded containers of one shape, whole or truncated, each image cut at its own place.  The base
    slices and the progressive (mu, sigma) chain run once, the rank order comes from the decoder's own sigma, and the
    embedded streams are prefix-decoded once (bitstream.decode_prefix_streams): :meth:`available` says how many leading
    elements of every slice are present.  A decoded quality equals ``forward_single_quality(x, q)`` bit for bit.

    The lanes per embedded stream are read from the containers (``"embedded-2"``: their ``"lanes"``); a batch that mixes
    them is refused.  ``coder`` (None: ``model.coder``): "host" prefix-decodes on the host's threads from a host copy of
    the ranked indexes; "device"  decodes z and the base slices with the device coder, uploads the
    embedded strings once and prefix-decodes them with ONE launch into the plan's ranked symbols; the counts come back
    with the status codes in one read, and the ranked indexes stay on the device unless :meth:`bits` asks for them.
    Either coder reads either coder's containers."""

    def __init__(self, model, containers, coder: Optional[str] = None):
        _check_model(model)
        cs = list(containers)
        if not cs:
            raise ValueError("EmbeddedDecoder: no containers")
        lanes = [_check_container(c) for c in cs]
        if any(k != lanes[0] for k in lanes):
            raise ValueError(f"EmbeddedDecoder: every container must have the same lanes per embedded stream, got "
                             f"{sorted(set(lanes))}; decode them separately")
        self.lanes, self.coder = lanes[0], P._check_coder(model, coder)
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
        self.dp = model._emb_dec_plan(self.B, hz, wz, self.coder)
        self._avail: Optional[np.ndarray] = None
        self.idx_r: Optional[np.ndarray] = None             # host copy of the ranked indexes (device coder: only for bits())
        with torch.no_grad():
            self._front()

    def _front(self):
        from . import bitstream as bs
        cs, ns, dp = self.containers, self.m.ns0, self.dp
        up = dp.front([[c["base"][i][0] for c in cs] for i in range(ns)], [c["z"][0] for c in cs])
        dp.owner = self
        if self.coder == "device":
            return self._front_device(up)
        if self._avail is None:                             # the host's one pass over the embedded streams
            self.idx_r = dp.idx_r.cpu().numpy()             # [B, ns, n]
            self.ranked = np.zeros(self.idx_r.shape, dtype=np.int32)
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
            if self._avail is None:
                emb = bs.upload_streams([c["embedded"][j] for c in cs for j in range(ns)], dp.device)
                meta = torch.empty((2, B * ns), dtype=torch.int32, device=dp.device)
                bs.decode_embedded_uploaded(emb, 0, dp.idx_r, dp.ranked, bs.DeviceCoderTables.of(self.m.gaussian_conditional, dp.device),
                                            self.lanes, meta)
                self.ranked = dp.ranked.clone()
                got = meta.cpu().numpy()                    # the one read: available counts and status codes
            else:
                dp.ranked.copy_(self.ranked)
                got = None
            bs.check_status(up, B, "EmbeddedDecoder", lambda k: f"z stream (image {k})" if k < B else
                            f"base stream (image {k % B}, slice {k // B - 1})")
        if got is not None:
            bad = np.flatnonzero(got[1])
            if bad.size:
                k = int(bad[0])
                raise L.VamError(f"EmbeddedDecoder: embedded stream (image {k // ns}, slice {k % ns}): "
                                 f"{bs.status_text(int(got[1][k]))}")
            self._avail = got[0].astype(np.int64).reshape(B, ns)

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

    def decode_qualities(self, qs: Sequence[float]) -> List[dict]:
        """{"x_hat", "y_hat"} of the batch per quality of ``qs`` (any qualities >= 0 in any order, marked or not; 0 is the
        base, g_s[0] on y_hat_base).  The counts come from the decoder's own sigma; ValueError when a container holds too
        little for one of them."""
        from .control import sweep_groups
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
