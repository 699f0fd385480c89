#!/usr/bin/env python3
"""Per-image qualities in one batch against the per-image loops they replace, one GPU, same model, same
inputs, hipGraph on.  Each part is warmed, then the two paths alternate, each timed from a device synchronisation to the
next; medians are reported.  Every part asserts that the two paths give the same results; no time is asserted.

  (a) ``evaluate.rd_at_rates(x, 4 targets)`` against the loop it ran before: the qualities resolved once, then one
      ``rd_sweep(x[b:b+1], q[:, b])`` per image (written here from the public API);
  (b) ``compress_per_image(x, q)`` against B calls of ``compress(x[b:b+1], q_b)``, both at the qualities
      ``qualities_for_bytes`` returns for one budget per image;
  (c) the hipGraphs each path of (b) captures over 5 successive batches of budgets (so: of different qualities), from a
      model without plans, and the graphs it retires.

Prints one JSON line.

    python scripts/bench_per_image.py [--warmup 1] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = [("32x256x256", 32, 256, 256), ("8x256x256", 8, 256, 256)]
FRACTIONS = (0.2, 0.4, 0.6, 0.8)
BATCH_FRACTIONS = (0.3, 0.4, 0.5, 0.6, 0.7)      # (c): five batches of budgets


def rd_at_rates_loop(net, x, targets):
    """evaluate.rd_at_rates as it ran before the per-image sweep: every image evaluated on its own."""
    from vampic import evaluate as EV
    sol = net.qualities_for_bpp(x, targets)
    q = sol["quality"]
    bpp, psnr = torch.zeros_like(q), torch.zeros_like(q)
    for b in range(x.shape[0]):
        r, p_ = EV.rd_sweep(net, x[b:b + 1], q[:, b].tolist())
        bpp[:, b], psnr[:, b] = r[:, 0], p_[:, 0]
    return bpp, psnr, q, sol["reached"]


def compress_loop(net, x, qs):
    return [net.compress(x[b:b + 1], q)["strings"] for b, q in enumerate(qs)]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _timed(fns, warmup, reps):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t[key].append(1e3 * (time.perf_counter() - t0))
            del out
    return {k: round(statistics.median(v), 2) for k, v in t.items()}, {k: [round(x, 2) for x in v] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import evaluate as EV, ops
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    captures = [0]
    capture = ops.Graph.capture

    def counted(self, fn):
        captures[0] += 1
        return capture(self, fn)
    ops.Graph.capture = counted
    closes = [0]
    close = ops.Graph.close

    def counted_close(self):
        closes[0] += 1 if self.exec else 0
        return close(self)
    ops.Graph.close = counted_close

    res = {"metric": "per-image qualities in one batch (ms per call, median)", "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "reps": a.reps, "rd_at_rates": {}, "compress": {}, "graphs": {}}
    with torch.no_grad():
        for name, B, H, W in CASES:
            x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
            # (a) rate and distortion at four target rates per image
            ends = EV.rate_curve(net, x, [0, 10])
            tg = torch.stack([ends[0] + f * (ends[1] - ends[0]) for f in FRACTIONS])
            new = lambda: EV.rd_at_rates(net, x, tg)
            old = lambda: rd_at_rates_loop(net, x, tg)
            n_, o_ = new(), old()
            assert torch.equal(n_[2], o_[2]) and torch.equal(n_[3], o_[3]), "resolved qualities differ"
            d_bpp, d_psnr = _rel(n_[0], o_[0]), _rel(n_[1], o_[1])
            assert d_bpp <= 1e-12 and d_psnr <= 1e-12, (d_bpp, d_psnr)
            med, runs = _timed({"per_image_loop": old, "rd_at_rates": new}, a.warmup, a.reps)
            res["rd_at_rates"][name] = dict(med, targets=len(FRACTIONS), ratio=round(med["rd_at_rates"] / med["per_image_loop"], 4),
                                            max_rel_bpp=d_bpp, max_rel_psnr=d_psnr, runs=runs)
            # (b) one byte budget per image: the batch in one call against one compress per image
            size = net.coded_size_curve(x, [0, 10])["bytes_hi"].double()
            qs = net.qualities_for_bytes(x, (size[0] + 0.5 * (size[1] - size[0])).unsqueeze(0))["quality"][0].tolist()
            batch = lambda: [it["strings"] for it in net.compress_per_image(x, qs)]
            loop = lambda: compress_loop(net, x, qs)
            same = batch() == loop()
            assert same, "compress_per_image and compress differ"
            med, runs = _timed({"compress_loop": loop, "compress_per_image": batch}, a.warmup, a.reps)
            res["compress"][name] = dict(med, ratio=round(med["compress_per_image"] / med["compress_loop"], 4), identical=same,
                                         distinct_qualities=len(set(qs)), runs=runs)
            # (c) graphs captured and retired over five batches of different qualities, each path from a model without plans
            vecs = [net.qualities_for_bytes(x, (size[0] + f * (size[1] - size[0])).unsqueeze(0))["quality"][0].tolist()
                    for f in BATCH_FRACTIONS]
            counts = {}
            for key, fn in (("compress_per_image", lambda q: [it["strings"] for it in net.compress_per_image(x, q)]),
                            ("compress_loop", lambda q: compress_loop(net, x, q))):
                net._drop_plans()
                c0, r0 = captures[0], closes[0]
                outs = [fn(q) for q in vecs]
                counts[key] = {"captured": captures[0] - c0, "given_up": closes[0] - r0}
                counts[key + "_out"] = outs
            assert counts.pop("compress_per_image_out") == counts.pop("compress_loop_out"), "the five batches differ"
            res["graphs"][name] = dict(counts, batches=len(vecs))
            net._drop_plans()
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
