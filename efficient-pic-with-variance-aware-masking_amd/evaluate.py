"""Evaluation drivers and metric helpers (inference half): the counterparts of
``test_epoch`` / ``compress_with_ac`` (reference training/step.py:206-243,259-358) and of
``compute_psnr`` / ``compute_padding`` (utility/functions.py:172-174,191-219) on top of the HIP model.
Rates come from the in-kernel ``log2`` accumulators (a13), squared errors from ``vam_sqdiff_sum`` (``vam_sqdiff_sum_levels``
per level and image for a rate sweep, :func:`rd_sweep`).
"""
from __future__ import annotations

import math
import time
from typing import Iterable, List, Optional, Sequence

import torch

from . import ops


def compute_padding(in_h: int, in_w: int, *, out_h=None, out_w=None, min_div=1):
    """utility/functions.py:191-219: (left, right, top, bottom) pad and un-pad tuples to a multiple of min_div."""
    if out_h is None:
        out_h = (in_h + min_div - 1) // min_div * min_div
    if out_w is None:
        out_w = (in_w + min_div - 1) // min_div * min_div
    if out_h % min_div != 0 or out_w % min_div != 0:
        raise ValueError(f"Padded output height and width are not divisible by min_div={min_div}.")
    left = (out_w - in_w) // 2
    right = out_w - in_w - left
    top = (out_h - in_h) // 2
    bottom = out_h - in_h - top
    return (left, right, top, bottom), (-left, -right, -top, -bottom)


def pad_image(x: torch.Tensor, min_div: int = 64):
    """test/utils.py:7-13: zero-pad to a multiple of 64 (6 stride-2 stages); returns (x_padded, unpad)."""
    pad, unpad = compute_padding(x.size(2), x.size(3), min_div=min_div)
    return torch.nn.functional.pad(x, pad, mode="constant", value=0), unpad


def compute_psnr(a: torch.Tensor, b: torch.Tensor) -> float:
    """utility/functions.py:172-174: -10 log10(mean((a-b)^2)) over the whole tensor pair."""
    a, b = a.contiguous(), b.contiguous()
    acc = torch.zeros(1, dtype=torch.float64, device=a.device)
    ops.sqdiff_sum(a, b, acc)
    return -10.0 * math.log10(acc.item() / a.numel())


def estimated_bpp(out: dict, num_pixels: int) -> float:
    """training/loss.py:217-228 (RateLoss): (sum log2 lik_y + sum log2 lik_z) / (-pixels)."""
    return -out["log2_likelihood_sum"].sum().item() / num_pixels


def _sweeps(model) -> bool:
    """Does ``model`` evaluate a quality list in one sweep (VarianceMaskingPIC.forward_qualities)?"""
    f = getattr(model, "_sweep_eligible", None)
    return bool(f is not None and f())


def _rd_sums(model, x: torch.Tensor, qualities: Sequence[float], mask_pol: str = "point-based-std"):
    """Per (quality, image) float64 device tensors [L, B]: the sum of log2 likelihoods (y and z) and the sum of squared
    errors of the reconstruction.  No host synchronisation."""
    dev = next(model.parameters()).device
    x = x.to(dev).contiguous()
    nq, B = len(qualities), x.shape[0]
    ls = torch.zeros((nq, B), dtype=torch.float64, device=dev)
    sq = torch.zeros((nq, B), dtype=torch.float64, device=dev)
    if not _sweeps(model):
        for k, q in enumerate(qualities):
            out = model.forward_single_quality(x, q, mask_pol, training=False)
            ls[k] = out["log2_likelihood_sum"].sum(0)
            ops.sqdiff_sum_levels(x, out["x_hat"].contiguous(), sq[k:k + 1])
        return ls, sq

    def emit(i0, i1, sw, t, ks):
        fp, xb = sw.fp, x[i0:i1]
        if t is None:                      # the base reconstruction, once for every 0 of the list
            acc = torch.zeros((1, i1 - i0), dtype=torch.float64, device=dev)
            ops.sqdiff_sum_levels(xb, fp.x_hat, acc)
            tot = fp.log2sum.sum(0)
            for k in ks:
                sq[k, i0:i1] = acc[0]
                ls[k, i0:i1] = tot
            return
        acc = torch.zeros((len(ks), i1 - i0), dtype=torch.float64, device=dev)
        ops.sqdiff_sum_levels(xb, t.x_hat, acc)                    # every level of the group in one launch
        tot = (fp.log2sum[0].unsqueeze(0) + t.log2sum) + fp.log2sum[1].unsqueeze(0)
        for g, k in enumerate(ks):
            sq[k, i0:i1] = acc[g]
            ls[k, i0:i1] = tot[g]
    model._sweep(x, list(qualities), mask_pol, emit)
    return ls, sq


def rd_sweep(model, x: torch.Tensor, qualities: Sequence[float]):
    """Rate and distortion of every image of ``x`` at every quality: (bpp, psnr), float64 [L, B] host tensors, with the
    definitions of :func:`estimated_bpp` and :func:`compute_psnr` applied to each image on its own.  Eligible models run
    one sweep (forward_qualities' plan); the host synchronises once, at the end."""
    with torch.no_grad():
        ls, sq = _rd_sums(model, x, qualities)
        hw = x.shape[2] * x.shape[3]
        vals = torch.stack([ls, sq]).cpu()
    return -vals[0] / hw, -10.0 * torch.log10(vals[1] / (x[0].numel()))


def rate_curve(model, x: torch.Tensor, qualities: Sequence[float]):
    """Estimated bpp of every image of ``x`` at every quality, float64 [L, B] on the host, without reconstructing anything
    (VarianceMaskingPIC.rate_curve): equal to :func:`rd_sweep`'s bpp."""
    dev = next(model.parameters()).device
    return model.rate_curve(x.to(dev).contiguous(), qualities)["bpp"].cpu()


def _rd_sums_per_image(model, x: torch.Tensor, Q: torch.Tensor, mask_pol: str = "point-based-std"):
    """:func:`_rd_sums` with image b of row t at quality Q[t][b] (host float64 [T, B]), on the per-image sweep: one front
    end per sub-batch, the base once for the entries equal to 0, the per-image tails for the others.  No host
    synchronisation."""
    dev = next(model.parameters()).device
    T, B = Q.shape
    ls = torch.zeros((T, B), dtype=torch.float64, device=dev)
    sq = torch.zeros((T, B), dtype=torch.float64, device=dev)
    is0 = (Q == 0).to(dev)

    def emit(i0, i1, sw, t, ks):
        fp, xb = sw.fp, x[i0:i1]
        n = 1 if t is None else len(ks)
        acc = torch.zeros((n, i1 - i0), dtype=torch.float64, device=dev)
        ops.sqdiff_sum_levels(xb, fp.x_hat if t is None else t.x_hat, acc)
        if t is None:
            tot = fp.log2sum.sum(0).unsqueeze(0)
        else:
            tot = (fp.log2sum[0].unsqueeze(0) + t.log2sum) + fp.log2sum[1].unsqueeze(0)
        for g, k in enumerate(ks):
            take = is0[k, i0:i1] if t is None else ~is0[k, i0:i1]
            g_ = 0 if t is None else g
            sq[k, i0:i1] = torch.where(take, acc[g_], sq[k, i0:i1])
            ls[k, i0:i1] = torch.where(take, tot[g_], ls[k, i0:i1])
    model._sweep(x, Q.tolist(), mask_pol, emit, per_image=True)
    return ls, sq


def rd_at_qualities(model, x: torch.Tensor, Q):
    """Rate and distortion of image b at quality Q[t][b]: (bpp, psnr), float64 [T, B] host tensors (``Q``: [T, B], or B
    values for T = 1; zeros and positives may mix freely), equal to :func:`rd_sweep` on each image alone with its column
    of Q up to the float64 summation order.  Eligible models run the per-image sweep (VarianceMaskingPIC.
    forward_qualities_per_image's plans) and synchronise once; the others loop over the images."""
    dev = next(model.parameters()).device
    x = x.to(dev).contiguous()
    Q = torch.as_tensor(Q, dtype=torch.float64).cpu()
    if Q.dim() == 1:
        Q = Q.unsqueeze(0)
    if Q.dim() != 2 or Q.shape[1] != x.shape[0]:
        raise ValueError(f"Q is [T, {x.shape[0]}] (or one row of {x.shape[0]}), got shape {tuple(Q.shape)}")
    if not bool((Q >= 0).all()):
        raise ValueError("qualities must be >= 0 (and not NaN)")
    if not _sweeps(model):
        bpp, psnr = torch.zeros_like(Q), torch.zeros_like(Q)
        for b in range(x.shape[0]):
            r, p_ = rd_sweep(model, x[b:b + 1], Q[:, b].tolist())
            bpp[:, b], psnr[:, b] = r[:, 0], p_[:, 0]
        return bpp, psnr
    with torch.no_grad():
        ls, sq = _rd_sums_per_image(model, x, Q)
        hw = x.shape[2] * x.shape[3]
        vals = torch.stack([ls, sq]).cpu()
    return -vals[0] / hw, -10.0 * torch.log10(vals[1] / (x[0].numel()))


# ----------------------------------------------------------------------------- quality maps
def latent_quality_map(pixel_map) -> torch.Tensor:
    """A quality map on the latent grid from one on the pixels: [B, H, W] or [B, 1, H, W] -> float64 [B, H/16, W/16], the
    MAXIMUM over each 16 x 16 block, so a block that touches a region gets the region's quality."""
    pm = torch.as_tensor(pixel_map).detach().to("cpu", torch.float64)
    if pm.dim() == 4 and pm.shape[1] == 1:
        pm = pm[:, 0]
    if pm.dim() != 3 or pm.shape[1] % 16 or pm.shape[2] % 16:
        raise ValueError(f"pixel map: [B, H, W] or [B, 1, H, W] with H, W multiples of 16, got shape {list(pm.shape)}")
    B, H, W = pm.shape
    return pm.reshape(B, H // 16, 16, W // 16, 16).amax(dim=(2, 4))


def quality_map_from_boxes(B: int, H: int, W: int, background: float, boxes) -> torch.Tensor:
    """The latent quality map [B, H/16, W/16] of images H x W at quality ``background`` with pixel boxes
    ``(b, y0, x0, y1, x1, q)`` (rows y0..y1-1, columns x0..x1-1 of image b at quality q; later boxes win where boxes
    overlap).  The pixel map goes through :func:`latent_quality_map`."""
    pm = torch.full((B, H, W), float(background), dtype=torch.float64)
    for b, y0, x0, y1, x1, q in boxes:
        if not (0 <= b < B and 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W):
            raise ValueError(f"box {(b, y0, x0, y1, x1, q)} lies outside {B} images of {H}x{W}")
        pm[b, y0:y1, x0:x1] = float(q)
    return latent_quality_map(pm)


def _region_sets(region, B: int, H: int, W: int, dev):
    """[None] (all pixels) and, with a boolean pixel ``region`` [B, H, W] or [B, 1, H, W], the region and its complement."""
    if region is None:
        return [None]
    r = torch.as_tensor(region).to(dev)
    r = (r[:, 0] if r.dim() == 4 else r).bool()
    if tuple(r.shape) != (B, H, W):
        raise ValueError(f"region: a boolean [B, H, W] or [B, 1, H, W] for images {[B, H, W]}, got {list(r.shape)}")
    return [None, r, ~r]


def _sqdiff_sets(x, x_hat, sets):
    """(sq, n) float64 [len(sets), B] on the device: per image the squared error summed over each pixel set of
    :func:`_region_sets` and the number of values in it (compute_psnr's two terms)."""
    B = x.shape[0]
    sq = torch.zeros((len(sets), B), dtype=torch.float64, device=x.device)
    n = torch.full((len(sets), B), float(x[0].numel()), dtype=torch.float64, device=x.device)
    for k, r in enumerate(sets):
        if r is None:
            ops.sqdiff_sum_levels(x, x_hat, sq[k:k + 1])
        else:                                      # outside the set both tensors are 0: only its pixels are summed
            m = r.unsqueeze(1).to(x.dtype)
            ops.sqdiff_sum_levels((x * m).contiguous(), (x_hat * m).contiguous(), sq[k:k + 1])
            n[k] = 3.0 * r.flatten(1).sum(1).double()
    return sq, n


def rd_quality_map(model, x: torch.Tensor, qmap, region=None):
    """Rate and distortion of ``forward_quality_map(x, qmap)`` per image: {"bpp", "psnr"} float64 [B] host tensors
    (:func:`estimated_bpp` and :func:`compute_psnr` applied to each image on its own) and, with a boolean pixel ``region``
    [B, H, W] or [B, 1, H, W], {"psnr_in", "psnr_out"}: compute_psnr's definition on the pixels inside and outside the region
    (NaN for an image whose set is empty)."""
    dev = next(model.parameters()).device
    x = x.to(dev).contiguous()
    B, _, H, W = x.shape
    with torch.no_grad():
        out = model.forward_quality_map(x, qmap)
        x_hat = out["x_hat"].contiguous()
        sets = _region_sets(region, B, H, W, dev)
        sq, n = _sqdiff_sets(x, x_hat, sets)
        vals = torch.cat([out["log2_likelihood_sum"].sum(0, keepdim=True), sq, n]).cpu()
    ns = len(sets)
    psnr = -10.0 * torch.log10(vals[1:1 + ns] / vals[1 + ns:])
    res = {"bpp": -vals[0] / (H * W), "psnr": psnr[0]}
    if region is not None:
        res.update({"psnr_in": psnr[1], "psnr_out": psnr[2]})
    return res


def rd_at_rates(model, x: torch.Tensor, target_bpps):
    """Rate and distortion at target rates: the qualities are resolved once for the batch (VarianceMaskingPIC.
    qualities_for_bpp: per image the largest quality whose estimated rate fits each target), then every image is
    evaluated at its own qualities in the same batch (:func:`rd_at_qualities`).  ``target_bpps``: T floats or
    a [T, B] tensor.  Returns (bpp, psnr, quality, reached), [T, B] host tensors; where ``reached`` is False (even the
    base exceeds the budget) the row holds the base (quality 0)."""
    dev = next(model.parameters()).device
    x = x.to(dev).contiguous()
    sol = model.qualities_for_bpp(x, target_bpps)
    q = sol["quality"]
    bpp, psnr = rd_at_qualities(model, x, q)
    return bpp, psnr, q, sol["reached"]


def rd_at_sizes(model, x: torch.Tensor, target_bytes):
    """Coded size and distortion at byte budgets, the analogue of :func:`rd_at_rates`: the qualities are resolved once for
    the batch (VarianceMaskingPIC.qualities_for_bytes: per image the largest quality whose compress strings are guaranteed
    to fit each budget), then every image is evaluated at its own qualities in the same batch.  ``target_bytes``: T numbers or a [T, B]
    tensor.  Returns (bytes, psnr, quality, reached), [T, B] host tensors: ``bytes`` the guaranteed upper size at that
    quality; where ``reached`` is False (even the base exceeds the budget) the row holds the base (quality 0)."""
    dev = next(model.parameters()).device
    x = x.to(dev).contiguous()
    sol = model.qualities_for_bytes(x, target_bytes)
    q = sol["quality"]
    return sol["bytes"], rd_at_qualities(model, x, q)[1], q, sol["reached"]


def _checkpoint_for(model, x, p):
    """training/step.py:13-29 extract_quality_ref + ExtractChekpointRepr (REM models only)."""
    levels = getattr(model, "check_levels", None)
    if not levels or p <= levels[0]:
        return None
    q_ref = max(l for l in levels if l < p)
    return model.ExtractChekpointRepr(x, quality=q_ref, rc=False)


def test_epoch(batches: Iterable[torch.Tensor], model, pr_list: Sequence[float], rems: bool = False):
    """training/step.py:206-243: likelihood-estimated (bpp, PSNR) averaged over the batches, per quality."""
    bpp = [[] for _ in pr_list]
    psnr = [[] for _ in pr_list]
    sweep = not rems and _sweeps(model)
    with torch.no_grad():
        for d in batches:
            n_pix = d.shape[0] * d.shape[2] * d.shape[3]
            if sweep:                      # one front end for the whole list; the same formulas over the batch's sums
                ls, sq = _rd_sums(model, d, pr_list)
                vals = torch.stack([ls.sum(1), sq.sum(1)]).cpu()
                for j in range(len(pr_list)):
                    bpp[j].append(-float(vals[0, j]) / n_pix)
                    psnr[j].append(-10.0 * math.log10(float(vals[1, j]) / d.numel()))
                continue
            for j, p in enumerate(pr_list):
                ck = _checkpoint_for(model, d, p) if rems else None
                out = model.forward_single_quality(d, quality=p, training=False, **({"checkpoint_ref": ck} if rems else {}))
                bpp[j].append(estimated_bpp(out, n_pix))
                psnr[j].append(compute_psnr(d, out["x_hat"]))
    return [sum(v) / len(v) for v in bpp], [sum(v) / len(v) for v in psnr]


def compress_with_ac(model, images: Iterable[torch.Tensor], pr_list: Sequence[float], rems: bool = False,
                     with_msssim: bool = False):
    """training/step.py:259-358: real codec evaluation — compress + decompress every (unpadded) image at every
    quality; bpp = 8 * bytes / pixels of the ORIGINAL image, PSNR on the cropped reconstruction.
    Returns (bpp, psnr, enc_seconds, dec_seconds) lists per quality, plus the MS-SSIM in dB
    (-10 log10(1 - ms_ssim), step.py:323-324) as a fifth list when ``with_msssim``."""
    nq = len(pr_list)
    bpp, psnr, t_enc, t_dec = [[] for _ in range(nq)], [[] for _ in range(nq)], [[] for _ in range(nq)], [[] for _ in range(nq)]
    mssim = [[] for _ in range(nq)]
    with torch.no_grad():
        for x in images:
            xp, unpad = pad_image(x)
            for j, p in enumerate(pr_list):
                ck = _checkpoint_for(model, xp, p) if rems else None
                t0 = time.perf_counter()
                enc = model.compress(xp, quality=p, checkpoint_rep=ck)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                dec = model.decompress(enc["strings"], enc["shape"], quality=p, checkpoint_rep=ck)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                x_hat = torch.nn.functional.pad(dec["x_hat"], unpad)
                n_bytes = sum(len(s) for sl in enc["strings"][0] for s in sl) + sum(len(s) for s in enc["strings"][1])
                bpp[j].append(8.0 * n_bytes / (x.shape[0] * x.shape[2] * x.shape[3]))
                psnr[j].append(compute_psnr(x, x_hat))
                if with_msssim:
                    mssim[j].append(-10.0 * math.log10(max(1.0 - compute_msssim(x, x_hat), 1e-12)))
                t_enc[j].append(t1 - t0)
                t_dec[j].append(t2 - t1)
    avg = lambda rows: [sum(v) / len(v) for v in rows]
    if with_msssim:
        return avg(bpp), avg(psnr), avg(t_enc), avg(t_dec), avg(mssim)
    return avg(bpp), avg(psnr), avg(t_enc), avg(t_dec)


def progressive_rd(model, images: Sequence[torch.Tensor], q_list: Sequence[float], coder: Optional[str] = None, lanes: int = 1):
    """The demo's progressive printout (reference demo.py with src/test/functions_encode.py / functions_decode.py) for a
    list of images on the batched container (progressive.encode_batch / ProgressiveDecoder): images of one shape are
    padded as :func:`compress_with_ac` pads them and coded as one batch; every level 0..len(q_list) is decoded.  Returns
    one dict per level: q (0 for the base), bpp (8 * the container's bytes up to the level / pixels of the ORIGINAL image),
    psnr (of the cropped decode), enc_s and dec_s (seconds per image: the encode once, the decode of that level), each
    the mean over the images, plus the per-image "bpp_all" / "psnr_all".  ``coder`` (None: model.coder) and ``lanes`` go to
    encode_batch and the decoder as given."""
    from . import progressive as P
    images = [x if x.dim() == 4 else x.unsqueeze(0) for x in images]
    nl = len(q_list) + 1
    rows = [{"q": 0.0 if k == 0 else float(q_list[k - 1]), "bpp_all": [None] * len(images), "psnr_all": [None] * len(images),
             "enc_s": 0.0, "dec_s": 0.0} for k in range(nl)]
    by_shape = {}
    for i, x in enumerate(images):
        by_shape.setdefault(tuple(x.shape[1:]), []).append(i)
    with torch.no_grad():
        for ids in by_shape.values():
            xs = torch.cat([images[i] for i in ids], 0)
            xp, unpad = pad_image(xs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            containers, _ = P.encode_batch(model, xp, q_list, coder=coder, lanes=lanes)
            t1 = time.perf_counter()
            dec = P.ProgressiveDecoder(model, containers, coder=coder)
            for k in range(nl):
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                out = dec.decode(k)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                x_hat = torch.nn.functional.pad(out["x_hat"], unpad)
                rows[k]["enc_s"] += (t1 - t0)
                rows[k]["dec_s"] += (t3 - t2) if k else (t3 - t1)       # level 0 includes the base decode
                for n, (i, c) in enumerate(zip(ids, containers)):
                    x = images[i]
                    rows[k]["bpp_all"][i] = P.bits_up_to(c, k) / (x.shape[0] * x.shape[2] * x.shape[3])
                    rows[k]["psnr_all"][i] = compute_psnr(x, x_hat[n:n + 1])
    for r in rows:
        r["bpp"] = sum(r["bpp_all"]) / len(images)
        r["psnr"] = sum(r["psnr_all"]) / len(images)
        r["enc_s"] /= len(images)
        r["dec_s"] /= len(images)
    return rows


def embedded_rd(model, images: Sequence[torch.Tensor], qualities: Sequence[float], coder=None, lanes: int = 1, base_lanes: int = 1):
    """:func:`progressive_rd`'s printout for the embedded format (embedded.encode_batch / EmbeddedDecoder, DESIGN section
    9m): images of one shape are padded and coded as one batch, ONCE and without a quality list of their own; the base and
    then every quality of ``qualities`` (any values >= 0, marked or not) is decoded from the same streams.  Returns one
    dict per level, the base first: q, bpp (8 * the bytes a receiver needs for that quality — z, the base and the shortest
    prefix of every slice — / pixels of the ORIGINAL image), psnr (of the cropped decode), enc_s and dec_s (seconds per
    image: the encode once, the decode of that level), each the mean over the images, plus "bpp_all" / "psnr_all".
    ``coder``, ``lanes`` and ``base_lanes`` are passed on to embedded.encode_batch, ``coder`` to the decoder too (DESIGN sections
    9q and 9t)."""
    from . import embedded as EB
    images = [x if x.dim() == 4 else x.unsqueeze(0) for x in images]
    levels = [0.0] + [float(q) for q in qualities]
    rows = [{"q": q, "bpp_all": [None] * len(images), "psnr_all": [None] * len(images), "enc_s": 0.0, "dec_s": 0.0}
            for q in levels]
    by_shape = {}
    for i, x in enumerate(images):
        by_shape.setdefault(tuple(x.shape[1:]), []).append(i)
    with torch.no_grad():
        for ids in by_shape.values():
            xs = torch.cat([images[i] for i in ids], 0)
            xp, unpad = pad_image(xs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            containers = EB.encode_batch(model, xp, coder=coder, lanes=lanes, base_lanes=base_lanes)
            t1 = time.perf_counter()
            dec = EB.EmbeddedDecoder(model, containers, coder=coder)
            for k, q in enumerate(levels):
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                out = dec.decode_qualities([q])[0]
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                x_hat = torch.nn.functional.pad(out["x_hat"], unpad)
                bits = dec.bits(q)
                rows[k]["enc_s"] += (t1 - t0)
                rows[k]["dec_s"] += (t3 - t2) if k else (t3 - t1)       # the base includes the base and prefix decode
                for n, i in enumerate(ids):
                    x = images[i]
                    rows[k]["bpp_all"][i] = bits[n] / (x.shape[0] * x.shape[2] * x.shape[3])
                    rows[k]["psnr_all"][i] = compute_psnr(x, x_hat[n:n + 1])
    for r in rows:
        r["bpp"] = sum(r["bpp_all"]) / len(images)
        r["psnr"] = sum(r["psnr_all"]) / len(images)
        r["enc_s"] /= len(images)
        r["dec_s"] /= len(images)
    return rows


def tiled_rd(model, image: torch.Tensor, qualities: Sequence[float], tile: int = 256, overlap: int = 32, coder=None, lanes: int = 1,
             base_lanes: int = 1, group: Optional[int] = None, allocation: str = "tile"):
    """:func:`embedded_rd` for ONE picture of any size coded in tiles (tiled.encode / PictureDecoder): the
    picture, fp32 [3, H, W] or [1, 3, H, W], is coded ONCE with ``qualities`` (non-decreasing, as marks) as its marks, and
    mark k is decoded from ``data[:round_end[k]]``, the prefix that holds every tile at exactly that mark.  One dict per
    quality: q, bytes (``round_end[k]``: picture header, every tile's head and the rounds up to k), bpp (8 * bytes / (H W),
    the true size), psnr against the original (:func:`compute_psnr`; nothing is padded or cropped), enc_s (the one encode) and
    dec_s (parsing that prefix and decoding the whole picture at q).  Quality q keeps a quantile PER TILE, so these rows are
    not those of the untiled forward; and nothing here measures the seams.

    ``allocation`` = "picture" (DESIGN section 9w): the marks are picture-wide (``tiled.encode(allocation="picture")``) and mark
    k is decoded with ``decode(mark=k)``.  Every row also carries ``allocation`` and ``kept_min`` / ``kept_max``: the smallest
    and largest fraction of its progressive elements that a tile keeps at that mark, from the counts in the tiles' heads —
    the spread that a picture-wide threshold opens between flat and busy tiles."""
    from . import tiled as TL
    x = image if image.dim() == 4 else image.unsqueeze(0)
    qs = [float(q) for q in qualities]
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = TL.encode(model, x, tile=tile, overlap=overlap, marks=qs, coder=coder, lanes=lanes, base_lanes=base_lanes, group=group,
                         allocation=allocation)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return _tiled_rows(model, x, data, qs, coder, group, allocation, t1 - t0)


def _tiled_rows(model, x, data, qs, coder, group, allocation: str, enc_s: float):
    """The rows of :func:`tiled_rd` for the coded picture ``data`` whose marks are ``qs``: mark k decoded from
    ``data[:round_end[k]]``, and the kept fractions from the counts in the tiles' heads."""
    import numpy as np
    from . import embedded as EB
    from . import tiled as TL
    H, W = int(x.shape[2]), int(x.shape[3])
    rows = []
    lay = TL.layout(data)
    ends = lay["round_end"]
    heads = [data[o:o + n] for row in lay["head"] for o, n in row if n]
    count = np.asarray([EB.layout(h)["marks"]["count"] for h in heads], dtype=np.float64)            # [tiles, marks, ns]
    kept = count.sum(-1) / (lay["ns"] * model.dim_chunk * (lay["th"] // 16) * (lay["tw"] // 16))    # [tiles, marks]
    for k, q in enumerate(qs):
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dec = TL.PictureDecoder(model, data[:ends[k]], coder=coder, group=group)
        x_hat = dec.decode(mark=k) if allocation == "picture" else dec.decode(q=q)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        rows.append({"q": q, "bytes": int(ends[k]), "bpp": 8.0 * ends[k] / (H * W), "psnr": compute_psnr(x, x_hat.unsqueeze(0)),
                     "enc_s": enc_s, "dec_s": t3 - t2, "allocation": allocation, "kept_min": float(kept[:, k].min()),
                     "kept_max": float(kept[:, k].max())})
    return rows


def tiled_rd_at_sizes(model, image: torch.Tensor, budgets, tile: int = 256, overlap: int = 32, coder=None, lanes: int = 1,
                      q_tol: float = 1e-3, base_lanes: int = 1, group: Optional[int] = None):
    """:func:`tiled_rd` at byte budgets instead of qualities (``tiled.encode(allocation="picture", max_bytes=budgets)``,
    DESIGN section 9ze): the picture is coded ONCE with its rounds placed at the budgets, and mark k is decoded from
    ``data[:round_end[k]]`` with ``decode(mark=k)``.  One dict per budget: tiled_rd's keys, where "q" is the quality the
    search solved and "bytes" = ``round_end[k]`` <= the budget, and "budget" itself."""
    from . import tiled as TL
    x = image if image.dim() == 4 else image.unsqueeze(0)
    budgets = TL.check_budgets(budgets, "tiled_rd_at_sizes")
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = TL.encode(model, x, tile=tile, overlap=overlap, coder=coder, lanes=lanes, base_lanes=base_lanes, group=group,
                         allocation="picture", max_bytes=budgets, q_tol=q_tol)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rows = _tiled_rows(model, x, data, [q for q, _ in TL.budget_marks(data)], coder, group, "picture", t1 - t0)
    for r, N in zip(rows, budgets):
        r["budget"] = N
    return rows


def tiled_stream_rd(model, image: torch.Tensor, cuts: Optional[Sequence[int]] = None, window=None, tile: int = 256, overlap: int = 32,
                    marks: Optional[Sequence[float]] = None, coder=None, lanes: int = 1, base_lanes: int = 1,
                    group: Optional[int] = None, allocation: str = "tile", schedule=None, cache_tiles: Optional[int] = None):
    """Rate and distortion of ONE picture codestream as a receiver sees it arrive (tiled.PictureStream):
    the picture is coded once (``tiled.encode`` with the encode options given), then ONE ``PictureStream`` is fed up to each
    byte position of ``cuts`` (ascending, from ``need_bytes`` on; None: ``need_bytes`` and every ``round_end``) and
    ``view(window)`` is taken after each feed.  One dict per cut: bytes, bpp (8 * bytes / (H W)), psnr of the view against
    the same window of the picture, ``tiles`` (the tiles of the window) and ``decoded`` (those that ran the network for this
    cut: the tiles whose own bytes grew since the cut before), and dec_s (the feed and the view).  ``cache_tiles`` defaults to
    the tiles of the window."""
    from . import tiled as TL
    x = image if image.dim() == 4 else image.unsqueeze(0)
    H, W = int(x.shape[2]), int(x.shape[3])
    rows = []
    with torch.no_grad():
        data = TL.encode(model, x, tile=tile, overlap=overlap, marks=marks, coder=coder, lanes=lanes, base_lanes=base_lanes, group=group,
                         allocation=allocation, schedule=schedule)
        lay = TL.layout(data)
        cuts = sorted({lay["need_bytes"], *lay["round_end"]}) if cuts is None else [int(n) for n in cuts]
        if any(b < a for a, b in zip(cuts, cuts[1:])) or (cuts and not lay["need_bytes"] <= cuts[0]) or (cuts and cuts[-1] > len(data)):
            raise ValueError(f"tiled_stream_rd: cuts are ascending byte positions in {lay['need_bytes']} (need_bytes) .. {len(data)}, "
                             f"got {cuts}")
        y0, x0, h, w = TL._window(lay, window, "tiled_stream_rd")
        want = x[:, :, y0:y0 + h, x0:x0 + w]
        n_tiles = len(TL.tiles_for(lay, (y0, x0, h, w)))
        stream = TL.PictureStream(model, coder=coder, group=group, cache_tiles=max(n_tiles, 1) if cache_tiles is None else cache_tiles)
        at = 0
        for n in cuts:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stream.feed(data[at:n])
            x_hat = stream.view((y0, x0, h, w))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            at = n
            rows.append({"bytes": n, "bpp": 8.0 * n / (H * W), "psnr": compute_psnr(want, x_hat.unsqueeze(0)),
                         "decoded": len(stream.last_decoded), "tiles": len(stream.last_tiles), "dec_s": t1 - t0})
    return rows


def pyramid_rd(model, image: torch.Tensor, qualities: Sequence[float], levels: Optional[int] = None, tile: int = 256, overlap: int = 32,
               coder=None, lanes: int = 1, base_lanes: int = 1, group: Optional[int] = None):
    """:func:`tiled_rd` for a resolution pyramid (pyramid.encode / PyramidDecoder): the picture is coded
    ONCE with ``qualities`` (non-decreasing, as marks) as the marks of every level.  One dict per level and quality: level,
    shape (H_k, W_k), q, bytes (the pyramid header plus that level's own ``round_end`` for the mark: the prefix of that level's
    codestream that holds every tile exactly at the mark, sent alone), bpp (8 * bytes / (H W) over the
    TRUE level-0 size), psnr of the level's decode against the REDUCED original (``ops.picture_halve`` of the picture, k
    times), enc_s (the one encode of all levels), dec_s (parsing that prefix of the level and decoding it whole at q) and
    total_over_level0: the pyramid's total bytes over level 0's alone."""
    from . import ops
    from . import pyramid as PY
    from . import tiled as TL
    x = image if image.dim() == 4 else image.unsqueeze(0)
    H, W = int(x.shape[2]), int(x.shape[3])
    qs = [float(q) for q in qualities]
    rows = []
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = PY.encode(model, x, levels=levels, tile=tile, overlap=overlap, marks=qs, coder=coder, lanes=lanes, base_lanes=base_lanes,
                         group=group)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lay = PY.layout(data)
        ratio = lay["total"] / lay["levels"][0]["length"]
        want = x[0].contiguous()
        for lv in lay["levels"]:
            k = lv["level"]
            if k:
                want = ops.picture_halve(want)
            stream = PY.level_stream(data, k)
            for j, q in enumerate(qs):
                end = lv["layout"]["round_end"][j]
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                x_hat = TL.PictureDecoder(model, stream[:end], coder=coder, group=group).decode(q=q)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                n = lay["header_end"] + int(end)
                rows.append({"level": k, "shape": tuple(lv["shape"]), "q": q, "bytes": n, "bpp": 8.0 * n / (H * W),
                             "psnr": compute_psnr(want.unsqueeze(0), x_hat.unsqueeze(0)), "enc_s": t1 - t0, "dec_s": t3 - t2,
                             "total_over_level0": ratio})
    return rows


def pyramid_fill_rd(model, image: torch.Tensor, cuts: Sequence[int], levels: Optional[int] = None, tile: int = 256, overlap: int = 32,
                    marks: Optional[Sequence[float]] = None, coder=None, lanes: int = 1, base_lanes: int = 1, group: Optional[int] = None,
                    cache_tiles: Optional[int] = None):
    """Bytes received against the quality of the FILLED level-0 view (``PyramidStream.view(fill=True)``):
    the picture is coded once as a pyramid, and one receiver is fed from cut to cut (``cuts``: byte counts in ascending order,
    each at least ``pyramid.need_bytes`` of the stream, those beyond its total meaning all of it).  One dict per cut: bytes,
    bpp (8 * bytes / (H W)), psnr of the filled level-0 view against the picture, sharp (the share of level-0 pixels all of
    whose tiles have arrived), chain (per level of the view, finest first: (level, tiles composed sharp, tiles that ran the
    network), as counts) and dec_s (feeding the bytes and the view).  ``cache_tiles`` defaults to every tile of a level."""
    import numpy as np
    from . import pyramid as PY
    from . import tiled as TL
    x = image if image.dim() == 4 else image.unsqueeze(0)
    H, W = int(x.shape[2]), int(x.shape[3])
    cuts = [int(n) for n in cuts]
    if not cuts or any(b < a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"pyramid_fill_rd: cuts are one or more byte counts in ascending order, got {list(cuts)}")
    rows = []
    with torch.no_grad():
        data = PY.encode(model, x, levels=levels, tile=tile, overlap=overlap, marks=marks, coder=coder, lanes=lanes, base_lanes=base_lanes,
                         group=group)
        need = PY.need_bytes(data)
        if cuts[0] < need:
            raise ValueError(f"pyramid_fill_rd: a cut of {cuts[0]} bytes: nothing decodes before need_bytes = {need}")
        g = TL.grid(H, W, tile, overlap)
        stream = PY.PyramidStream(model, coder=coder, group=group, cache_tiles=g["R"] * g["C"] if cache_tiles is None else cache_tiles)
        want = x[:1].contiguous()
        for n in (min(n, len(data)) for n in cuts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stream.feed(data[len(stream.data):n])
            x_hat = stream.view(level=0, fill=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ready = stream.streams[0].tile_ready
            sharp = np.zeros((H, W), dtype=bool)
            if ready is not None:
                sharp[:] = True
                for r, c in zip(*np.nonzero(~ready)):          # a tile that has not arrived takes its whole extent with it
                    sharp[r * g["Sy"]:r * g["Sy"] + g["th"], c * g["Sx"]:c * g["Sx"] + g["tw"]] = False
            rows.append({"bytes": n, "bpp": 8.0 * n / (H * W), "psnr": compute_psnr(want, x_hat.unsqueeze(0)), "sharp": float(sharp.mean()),
                         "chain": [(k, len(a), len(b)) for k, a, b in stream.last_chain], "dec_s": t1 - t0})
    return rows


def session_rd(model, image: torch.Tensor, tour: Sequence[dict], levels: Optional[int] = None, tile: int = 256, overlap: int = 32,
               marks: Optional[Sequence[float]] = None, coder=None, lanes: int = 1, base_lanes: int = 1, group: Optional[int] = None,
               allocation: str = "tile", schedule=None, cache_tiles: Optional[int] = None):
    """Bytes sent against the quality of the viewport along a viewing session (``session.Server`` / ``session.Client``, DESIGN
    section 9zd): the picture is coded ONCE as a pyramid, and one server and one client follow ``tour``, a list of
    ``dict(rect, out_hw, unit=1, rounds=None)``.  The session opens with ``Server.open()``, the picture's headers alone, merged
    before the tour and counted in bytes_total, in no step.  Per step the server's increment for the viewport is merged and
    the viewport is viewed filled, at the last mark (stage, for a schedule) that ``rounds`` holds whole, from everything held
    when ``rounds`` is 0.  One dict per step: bytes (this message), bytes_total (all messages so far, the opening one
    included), bytes_stateless (the length of ``pyramid.extract_viewport`` for the same request), tiles and decoded (of the
    viewport's level: composed, and run through the network), dec_s (the merge plus the viewport) and psnr against the same
    viewport of the original: ``ops.picture_halve`` k* times, then ``ops.picture_resample``.  ``cache_tiles`` defaults to every
    tile of level 0."""
    from . import ops
    from . import pyramid as PY
    from . import session as SS
    from . import tiled as TL
    x = image if image.dim() == 4 else image.unsqueeze(0)
    H, W = int(x.shape[2]), int(x.shape[3])
    rows = []
    with torch.no_grad():
        kw = dict(schedule=schedule) if schedule is not None else dict(marks=marks, allocation=allocation)
        data = PY.encode(model, x, levels=levels, tile=tile, overlap=overlap, coder=coder, lanes=lanes, base_lanes=base_lanes, group=group, **kw)
        lay = PY.layout(data)
        n_marks = len(lay["levels"][0]["layout"]["marks"])
        g = TL.grid(H, W, tile, overlap)
        server = SS.Server(data)
        client = SS.Client(model, coder=coder, group=group, cache_tiles=g["R"] * g["C"] if cache_tiles is None else cache_tiles)
        opening = server.open()
        client.merge(opening)
        originals, total = [x[0].contiguous()], len(opening)
        for step in tour:
            rect, out_hw, unit, rounds = step["rect"], step["out_hw"], step.get("unit", 1), step.get("rounds")
            stateless = len(PY.extract_viewport(data, rect, out_hw, unit, rounds))
            m = n_marks - 1 if rounds is None else min(int(rounds), n_marks) - 1
            how = {} if m < 0 else {"stage": m} if schedule is not None else {"mark": m}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            message = server.viewport(rect, out_hw, unit, rounds)
            client.merge(message)
            x_hat = client.viewport(rect, out_hw, unit, fill=True, **how)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            full, out_hw, unit, k, win = PY._viewport_plan("session_rd", rect, out_hw, unit, None, None, H, W, lay["n_levels"])
            while len(originals) <= k:
                originals.append(ops.picture_halve(originals[-1]))
            y0, x0, h, w = win
            want = ops.picture_resample(originals[k][:, y0:y0 + h, x0:x0 + w].contiguous(), win, lay["levels"][k]["shape"], k, full, unit, out_hw)
            total += len(message)
            rows.append({"bytes": len(message), "bytes_total": total, "bytes_stateless": stateless, "tiles": len(client.last_tiles),
                         "decoded": len(client.last_decoded), "dec_s": t1 - t0, "psnr": compute_psnr(want.unsqueeze(0), x_hat.unsqueeze(0))})
    return rows


def embedded_stream_rd(model, images: Sequence[torch.Tensor], byte_budgets: Sequence[int], coder=None, lanes: int = 1,
                       base_lanes: int = 1):
    """Rate and distortion of a codestream (embedded.to_bytes) cut at real byte budgets: images of ONE
    shape are padded and coded as one batch, once; every image's codestream is cut at ``data[:n]`` for each n of
    ``byte_budgets`` (ascending; every n at least the largest ``need_bytes`` of the batch, a ValueError says which is not)
    and ONE embedded.StreamDecoder is fed from budget to budget.  One dict per budget, with a list per image: "budget",
    "bytes" (min(n, the image's total): all of them are decoded), "bpp" (8 * bytes / pixels of the original image), "psnr"
    (of the cropped decode) and "available" (decoded elements); beside them what ``truncate(container, max_bytes=n)`` makes
    of the same n — "truncate_bytes" (z, base and the embedded bytes of the largest mark that fits; it counts no header),
    "unused" (n - truncate_bytes, the slack a mark leaves) and "truncate_psnr" — and "header_bytes" of the codestream."""
    from . import embedded as EB
    images = [x if x.dim() == 4 else x.unsqueeze(0) for x in images]
    budgets = [int(n) for n in byte_budgets]
    if not budgets or any(b < a for a, b in zip(budgets, budgets[1:])):
        raise ValueError(f"embedded_stream_rd: byte_budgets are one or more byte counts in ascending order, got {list(byte_budgets)}")
    if len({tuple(x.shape[1:]) for x in images}) != 1 or any(x.shape[0] != 1 for x in images):
        raise ValueError("embedded_stream_rd: the images of one call are single images of one shape")
    rows = []
    with torch.no_grad():
        xp, unpad = pad_image(torch.cat(images, 0))
        cs = EB.encode_batch(model, xp, coder=coder, lanes=lanes, base_lanes=base_lanes)
        data = [EB.to_bytes(c) for c in cs]
        lay = [EB.layout(d) for d in data]
        need = max(v["base_end"] for v in lay)
        if budgets[0] < need:
            raise ValueError(f"embedded_stream_rd: a budget of {budgets[0]} bytes decodes nothing: {need} bytes are needed for header, "
                             "z and base")
        pixels = [x.shape[2] * x.shape[3] for x in images]
        psnr = lambda out: [compute_psnr(x, torch.nn.functional.pad(out["x_hat"], unpad)[i:i + 1]) for i, x in enumerate(images)]
        dec, sent, marked = EB.StreamDecoder(model, len(images), coder=coder), [0] * len(images), {}
        for n in budgets:
            upto = [min(n, v["total"]) for v in lay]
            avail = dec.feed([d[a:b] for d, a, b in zip(data, sent, upto)])
            sent = upto
            row = {"budget": n, "bytes": upto, "bpp": [8.0 * b / p for b, p in zip(upto, pixels)], "psnr": psnr(dec.decode()),
                   "available": [int(v) for v in avail.sum(1)], "header_bytes": [v["header_end"] for v in lay]}
            cut = [EB.truncate(c, max_bytes=n) for c in cs]
            key = tuple(len(s) for c in cut for s in c["embedded"])
            if key not in marked:                           # budgets that buy the same marks share one decode
                marked[key] = psnr(EB.EmbeddedDecoder(model, cut, coder=coder).decode())
            row.update(truncate_bytes=[sum(EB.container_bytes(c)) for c in cut], truncate_psnr=marked[key])
            row["unused"] = [n - v for v in row["truncate_bytes"]]
            rows.append(row)
    return rows


def roi_schedule(B: int, H: int, W: int, boxes, roi_qualities: Sequence[float], background_qualities: Sequence[float]):
    """A region-of-interest schedule for embedded.encode_batch(schedule=...): a list of latent quality
    maps [B, H/16, W/16].  ``boxes``: pixel boxes ``(b, y0, x0, y1, x1)`` of the region.  First the region climbs through
    ``roi_qualities`` over the background at ``background_qualities[0]``, then the background climbs through the rest of
    ``background_qualities`` under the region at ``roi_qualities[-1]``.  Both lists non-decreasing; a stage at which the
    background would pass the region is refused by embedded.check_schedule's monotonicity (the block-maximum rule of
    :func:`latent_quality_map` gives a block that touches the region the larger of the two)."""
    rq, bq = [float(q) for q in roi_qualities], [float(q) for q in background_qualities]
    if not rq or not bq:
        raise ValueError("roi_schedule: roi_qualities and background_qualities need at least one quality each")
    stages = [(r, bq[0]) for r in rq] + [(rq[-1], g) for g in bq[1:]]
    return [quality_map_from_boxes(B, H, W, g, [tuple(box[:5]) + (r,) for box in boxes]) for r, g in stages]


def embedded_roi_rd(model, images: torch.Tensor, schedule, region, coder=None, lanes: int = 1, base_lanes: int = 1):
    """Rate and distortion per stage of a scheduled embedded stream: ``images`` [B, 3, H, W] (H, W
    multiples of 64) are coded ONCE with embedded.encode_batch(schedule=...), and every stage is decoded from the same
    containers.  One dict per stage: "stage", "bytes" (per image: z, the base, the schedule's side bytes and the stage's
    mark of every slice — what a receiver needs for it), "bpp" (8 * bytes / pixels), and "psnr", "psnr_in", "psnr_out"
    (float64 [B] host tensors; :func:`rd_quality_map`'s definition on all pixels and on the pixels inside and outside the
    boolean pixel ``region`` [B, H, W] or [B, 1, H, W]).  ``coder``, ``lanes`` and ``base_lanes`` go to encode_batch."""
    from . import embedded as EB
    dev = next(model.parameters()).device
    x = images.to(dev).contiguous()
    B, _, H, W = x.shape
    sets = _region_sets(region, B, H, W, dev)
    if len(sets) != 3:
        raise ValueError("embedded_roi_rd: region is a boolean [B, H, W] or [B, 1, H, W]")
    rows = []
    with torch.no_grad():
        containers = EB.encode_batch(model, x, schedule=schedule, coder=coder, lanes=lanes, base_lanes=base_lanes)
        dec = EB.EmbeddedDecoder(model, containers, coder=coder)
        for k in range(dec.n_stages):
            x_hat = dec.decode_stages([k])[0]["x_hat"].contiguous()
            sq, n = _sqdiff_sets(x, x_hat, sets)
            psnr = (-10.0 * torch.log10(sq / n)).cpu()
            nbytes = [sum(EB.container_bytes(c)[:2]) + int(c["side_bytes"]) + sum(int(v) for v in c["marks"]["bytes"][k])
                      for c in containers]
            rows.append({"stage": k, "bytes": nbytes, "bpp": [8.0 * v / (H * W) for v in nbytes],
                         "psnr": psnr[0], "psnr_in": psnr[1], "psnr_out": psnr[2]})
    return rows


def picture_roi_schedule(H: int, W: int, boxes, roi_qualities: Sequence[float], background_qualities: Sequence[float], device):
    """:func:`roi_schedule`'s stage ladder as a PICTURE-wide schedule for ``tiled.encode(schedule=)``: fp32
    [L, H, W] on ``device``, at pixel resolution, any H and W.  ``boxes``: pixel boxes ``(y0, x0, y1, x1)`` of the region
    (rows y0..y1-1, columns x0..x1-1).  First the region climbs through ``roi_qualities`` over the background at
    ``background_qualities[0]``, then the background climbs through the rest of ``background_qualities`` under the region at
    ``roi_qualities[-1]``; L = len(roi_qualities) + len(background_qualities) - 1.  Built with torch fills on the device."""
    rq, bq = [float(q) for q in roi_qualities], [float(q) for q in background_qualities]
    if not rq or not bq:
        raise ValueError("picture_roi_schedule: roi_qualities and background_qualities need at least one quality each")
    boxes = [tuple(int(v) for v in box[:4]) for box in boxes]
    for y0, x0, y1, x1 in boxes:
        if not (0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W):
            raise ValueError(f"picture_roi_schedule: box {(y0, x0, y1, x1)} lies outside the picture of {H}x{W}")
    stages = [(r, bq[0]) for r in rq] + [(rq[-1], g) for g in bq[1:]]
    S = torch.empty((len(stages), H, W), dtype=torch.float32, device=device)
    for k, (r, g) in enumerate(stages):
        S[k].fill_(g)
        for y0, x0, y1, x1 in boxes:
            S[k, y0:y1, x0:x1].fill_(r)
    return S


def tiled_roi_rd(model, image: torch.Tensor, schedule, region, tile: int = 256, overlap: int = 32, coder=None, lanes: int = 1,
                 base_lanes: int = 1, group: Optional[int] = None):
    """:func:`embedded_roi_rd` for ONE picture of any size coded in scheduled tiles (tiled.encode(schedule=) /
    PictureDecoder.decode(stage=)): the picture, fp32 [3, H, W] or [1, 3, H, W], is coded ONCE with the
    picture-wide ``schedule`` fp32 [L, H, W], and stage k is decoded from ``data[:round_end[k]]``, the prefix that holds every
    tile exactly at that stage.  One dict per stage: "stage", "bytes" (``round_end[k]``: picture header, every tile's head —
    its schedule included — and the rounds up to k), "bpp" (8 * bytes / (H W), the true size), and "psnr", "psnr_in",
    "psnr_out": :func:`compute_psnr`'s definition on all pixels and on the pixels inside and outside the boolean pixel
    ``region`` [H, W] (NaN for an empty set); "enc_s" (the one encode) and "dec_s"."""
    from . import tiled as TL
    x = (image if image.dim() == 4 else image.unsqueeze(0)).contiguous()
    H, W = int(x.shape[2]), int(x.shape[3])
    r = torch.as_tensor(region)
    if r.dim() != 2 or tuple(r.shape) != (H, W):
        raise ValueError(f"tiled_roi_rd: region is a boolean [H, W] = {[H, W]}, got {list(r.shape)}")
    sets = _region_sets(r.unsqueeze(0), 1, H, W, x.device)
    rows = []
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = TL.encode(model, x, tile=tile, overlap=overlap, coder=coder, lanes=lanes, base_lanes=base_lanes, group=group,
                         schedule=schedule)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lay = TL.layout(data)
        for k in range(lay["stages"]):
            end = lay["round_end"][k]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            x_hat = TL.PictureDecoder(model, data[:end], coder=coder, group=group).decode(stage=k)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            sq, n = _sqdiff_sets(x, x_hat.unsqueeze(0).contiguous(), sets)
            psnr = (-10.0 * torch.log10(sq / n)).cpu()
            rows.append({"stage": k, "bytes": int(end), "bpp": 8.0 * end / (H * W), "psnr": float(psnr[0, 0]),
                         "psnr_in": float(psnr[1, 0]), "psnr_out": float(psnr[2, 0]), "enc_s": t1 - t0, "dec_s": t3 - t2})
    return rows


def valid_epoch(epoch: int, test_dataloader: Iterable[torch.Tensor], criterion, model, pr_list: Sequence[float] = (0.05,),
                rems: Optional[Sequence[float]] = None):
    """training/step.py:136-202 (without wandb): mean criterion loss over batches x qualities — what drives the
    ReduceLROnPlateau scheduler of train.py:130,279.  ``rems`` = the check levels (REM models) or None."""
    from .finetune import extract_quality_ref
    model.eval()
    device = next(model.parameters()).device
    tot = {"loss": 0.0, "bpp": 0.0, "mse": 0.0, "psnr": 0.0}
    n = 0
    sweep = not rems and _sweeps(model)
    with torch.no_grad():
        for d in test_dataloader:
            d = d.to(device)
            outs = model.forward_qualities(d, list(pr_list), mask_pol="point-based-std") if sweep else None
            for j, p in enumerate(pr_list):
                if sweep:
                    out = outs[j]
                elif rems is None:
                    out = model.forward_single_quality(d, quality=p, training=False)
                else:
                    q_ref = extract_quality_ref(p, rems)
                    ck = None if q_ref is None else model.ExtractChekpointRepr(d, quality=q_ref, rc=False)
                    out = model.forward_single_quality(d, quality=p, training=False, checkpoint_ref=ck)
                crit = criterion(out, d)
                psnr = compute_psnr(d, out["x_hat"])
                tot["loss"] += float(crit["loss"])
                tot["bpp"] += float(crit["bpp_loss"])
                tot["mse"] += 10.0 ** (-psnr / 10.0)
                tot["psnr"] += psnr
                n += 1
    n = max(n, 1)
    return tot["loss"] / n, {k: v / n for k, v in tot.items()}


def read_image(filepath) -> torch.Tensor:
    """utility/functions.py:62-66: RGB image file -> float32 [3,H,W] in [0,1] (what torchvision's ToTensor does to
    an 8-bit image: value / 255, HWC -> CHW)."""
    import numpy as np
    from PIL import Image
    img = Image.open(filepath).convert("RGB")
    a = np.asarray(img, dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1).to(torch.float32).div(255.0)


def write_image(x: torch.Tensor, filepath):
    """Inverse of :func:`read_image` for a [3,H,W] or [1,3,H,W] tensor in [0,1] (demo.py saves reconstructions)."""
    import numpy as np
    from PIL import Image
    if x.dim() == 4:
        x = x[0]
    a = (x.detach().clamp(0, 1).mul(255.0).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy())
    Image.fromarray(np.ascontiguousarray(a), mode="RGB").save(filepath)


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def compute_msssim(a: torch.Tensor, b: torch.Tensor, data_range: float = 1.0) -> float:
    """utility/functions.py:176-177: ``ms_ssim(a, b, data_range=1.)`` of pytorch_msssim 0.2.1 — 11-tap Gaussian
    (sigma 1.5), 5 scales, default weights, mean over images and channels — on the GPU (``vam_ssim_level``,
    ``vam_avgpool2``).  NCHW fp32 CUDA tensors; the smaller side must exceed 160 pixels."""
    from . import _lib as L
    L.require_gpu()
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f"expected two [B,C,H,W] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if min(a.shape[2:]) <= (11 - 1) * 2 ** 4:
        raise ValueError("image too small for 5 scales with an 11-tap window (smaller side must exceed 160)")
    lib = L.load()
    x, y = a.detach().float().contiguous(), b.detach().float().contiguous()
    B, C_, H, W = x.shape
    planes = B * C_
    coords = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    win = (g / g.sum()).to(x.device)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vals = []
    for lvl in range(5):
        sums = torch.zeros((2, planes), dtype=torch.float64, device=x.device)
        L.check(lib.vam_ssim_level(x.data_ptr(), y.data_ptr(), planes, H, W, win.data_ptr(), c1, c2, sums[0].data_ptr(),
                                   sums[1].data_ptr(), ops.stream_ptr()), "vam_ssim_level")
        mean = sums / float((H - 10) * (W - 10))
        vals.append(torch.relu(mean[1] if lvl < 4 else mean[0]))
        if lvl < 4:
            ph, pw = H % 2, W % 2
            Ho, Wo = (H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1
            nx = torch.empty((B, C_, Ho, Wo), dtype=torch.float32, device=x.device)
            ny = torch.empty_like(nx)
            L.check(lib.vam_avgpool2(x.data_ptr(), nx.data_ptr(), planes, H, W, ph, pw, ops.stream_ptr()), "vam_avgpool2")
            L.check(lib.vam_avgpool2(y.data_ptr(), ny.data_ptr(), planes, H, W, ph, pw, ops.stream_ptr()), "vam_avgpool2")
            x, y, H, W = nx, ny, Ho, Wo
    w = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64, device=x.device).reshape(-1, 1)
    return float(torch.prod(torch.stack(vals, 0) ** w, dim=0).mean())


def msssim_per_image(a: torch.Tensor, b: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """MS-SSIM of each image of ``b`` against ``a`` ([B,C,H,W] CUDA tensors): [B] float64, the mean over channels, from the
    LDS-tiled forward of the training loss (ops.msssim_forward, csrc/msssim.hip) — deterministic, no host synchronisation.
    The function of :func:`compute_msssim` (whose mean over the batch it reproduces up to summation order); a plane with a
    non-positive level mean counts as 0."""
    from . import _lib as L
    L.require_gpu()
    ops._msssim_check(a, b)
    val, _, _ = ops.msssim_forward(a.detach().float().contiguous(), b.detach().float().contiguous(), data_range)
    return val
