#!/usr/bin/env python3
"""Rate sweep against the per-quality loop: ``VarianceMaskingPIC.forward_qualities(x, qs)`` against
``[forward_single_quality(x, q) for q in qs]`` on one GPU, same model, same inputs, hipGraph on.  Each size is warmed,
then the two paths alternate (loop, sweep, loop, sweep, ...), each timed from a device synchronisation to the next; the
medians are reported.  At every size the outputs of the two paths are checked equal (tensors bit for bit, the float64
rate sums to 1e-12).  Prints one JSON line.

    python scripts/bench_sweep.py [--warmup 2] [--reps 5]
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

QS15 = [0, 0.05, 0.1, 0.25, 0.5, 0.6, 0.75, 1, 1.25, 2, 2.5, 3, 3.5, 5, 10]
QS7 = [0.76, 1, 1.25, 2, 3, 5, 10]
CASES = [("32x256x256/15", 32, 256, 256, QS15), ("32x256x256/7", 32, 256, 256, QS7), ("1x512x768/15", 1, 512, 768, QS15)]


def _equal(got, want) -> bool:
    for g, w in zip(got, want):
        for k, v in w.items():
            if k == "log2_likelihood_sum":
                if float((g[k] - v).abs().max() / v.abs().max()) >= 1e-12:
                    return False
            elif k == "likelihoods":
                if not all(torch.equal(g[k][kk], v[kk]) for kk in v):
                    return False
            elif torch.is_tensor(v) and not torch.equal(g[k], v):
                return False
    return len(got) == len(want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from bench import build_model
    import vampic
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    res = {"metric": "rate sweep vs per-quality loop (ms per list, median)", "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "reps": a.reps, "cases": {}}
    for name, B, H, W, qs in CASES:
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        loop = lambda: [net.forward_single_quality(x, q, training=False) for q in qs]
        sweep = lambda: net.forward_qualities(x, qs)
        with torch.no_grad():
            ok = _equal(sweep(), loop())
            for _ in range(a.warmup):
                loop()
                sweep()
            t = {"loop": [], "sweep": []}
            for _ in range(a.reps):
                for key, fn in (("loop", loop), ("sweep", sweep)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize()
                    t[key].append(1e3 * (time.perf_counter() - t0))
                    del out
        ml, ms = statistics.median(t["loop"]), statistics.median(t["sweep"])
        res["cases"][name] = {"levels": len(qs), "loop_ms": round(ml, 2), "sweep_ms": round(ms, 2), "ratio": round(ms / ml, 3),
                              "loop_runs_ms": [round(v, 2) for v in t["loop"]], "sweep_runs_ms": [round(v, 2) for v in t["sweep"]],
                              "outputs_equal": ok}
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
