#!/usr/bin/env python3
"""Rate control against what it replaces, one GPU, same model, same inputs, hipGraph on.  Each part is
warmed, then the two paths alternate, each timed from a device synchronisation to the next; medians are reported.

  (a) ``rate_curve(x, qs)`` against ``forward_qualities(x, qs)`` over the reference ``test_epoch`` list (the rates of the
      two are checked equal to 1e-12);
  (b) ``qualities_for_bpp(x, 4 targets)`` against a plain bisection over ``forward_single_quality`` to the same q_tol,
      written here from the public API only (both answers are checked against the solver's contract);
  (c) for one 512x768 image, the coded bytes of the container ``progressive.q_list_for_bpps`` leads to, beside the targets
      (reported, not asserted: the estimate is a likelihood sum, the container is range-coded bytes).

Prints one JSON line.

    python scripts/bench_rate.py [--warmup 2] [--reps 5]
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
CASES = [("32x256x256", 32, 256, 256), ("1x512x768", 1, 512, 768)]
SOLVER_IMAGES = 8        # (b) runs on the first 8 images of a case: the bisection is 14 probes per image and target
FRACTIONS = (0.2, 0.4, 0.6, 0.8)
Q_TOL = 1e-3


def _bpp(net, x, q):
    out = net.forward_single_quality(x, q, training=False)
    return (-out["log2_likelihood_sum"].sum(0) / (x.shape[2] * x.shape[3])).cpu()


def bisect(net, x, targets, q_tol=Q_TOL):
    """What a user does without qualities_for_bpp: per image and target a bisection on q over forward_single_quality
    (the brackets differ per image, so every probe is one image).  hipGraph is off for the probes: each one is a new
    quality, whose graph would be captured and never replayed.  ``targets`` [T, B]; returns the largest probed q within
    budget (0 where not even the base fits), [T, B]."""
    T, B = targets.shape
    out = torch.zeros((T, B), dtype=torch.float64)
    graph, net.use_graph = net.use_graph, False
    try:
        for b in range(B):
            xb = x[b:b + 1]
            r0, r10 = float(_bpp(net, xb, 0.0)), float(_bpp(net, xb, 10.0))
            for t in range(T):
                tg = float(targets[t, b])
                if r0 > tg or r10 <= tg:
                    out[t, b] = 10.0 if r10 <= tg else 0.0
                    continue
                lo, hi = 0.0, 10.0
                while hi - lo > q_tol:
                    mid = 0.5 * (lo + hi)
                    if float(_bpp(net, xb, mid)) <= tg:
                        lo = mid
                    else:
                        hi = mid
                out[t, b] = lo
    finally:
        net.use_graph = graph
    return out


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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import progressive as PR
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    res = {"metric": "rate control (ms per call, median)", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "reps": a.reps, "q_tol": Q_TOL, "curve": {}, "solver": {}}
    with torch.no_grad():
        for name, B, H, W in CASES:
            x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
            # (a) the rate of the test_epoch list
            curve = lambda: net.rate_curve(x, QS15)["log2_likelihood_sum"]
            sweep = lambda: torch.stack([o["log2_likelihood_sum"] for o in net.forward_qualities(x, QS15)])
            front = lambda: net.rate_curve(x, [0])["log2_likelihood_sum"]
            c, s = curve(), sweep()
            ok = float((c - s).abs().max() / s.abs().max()) < 1e-12
            med, runs = _timed({"sweep": sweep, "rate_curve": curve, "front_only": front}, a.warmup, a.reps)
            res["curve"][name] = dict(med, levels=len(QS15), ratio=round(med["rate_curve"] / med["sweep"], 3), rates_equal=ok, runs=runs)
            # (b) the qualities of four budgets per image
            xs = x[:SOLVER_IMAGES]
            r0, r10 = _bpp(net, xs, 0.0), _bpp(net, xs, 10.0)
            tg = torch.stack([r0 + f * (r10 - r0) for f in FRACTIONS])
            solve = lambda: net.qualities_for_bpp(xs, tg, q_tol=Q_TOL)["quality"]
            plain = lambda: bisect(net, xs, tg)
            qs, qb = solve(), plain()
            med, runs = _timed({"bisection": plain, "solver": solve}, 1, max(1, a.reps // 2))
            res["solver"][name] = dict(med, images=xs.shape[0], targets=len(FRACTIONS), ratio=round(med["solver"] / med["bisection"], 4),
                                       max_abs_q_difference=float((qs - qb).abs().max()), runs=runs)
            net._drop_plans()
            torch.cuda.empty_cache()
        # (c) a container built for target rates: estimated against coded
        x = vampic.synth.synth_image(1, 512, 768, seed=0).to(dev)
        net.update()
        r0, r10 = float(_bpp(net, x, 0.0)), float(_bpp(net, x, 10.0))
        tg = [r0 + f * (r10 - r0) for f in FRACTIONS]
        q_list = PR.q_list_for_bpps(net, x, tg)
        containers, _ = PR.encode_batch(net, x, q_list)
        est = net.rate_curve(x, q_list)["bpp"][:, 0].tolist()
        coded = [PR.bits_up_to(containers[0], k) / (512 * 768) for k in range(1, len(q_list) + 1)]
        res["container_1x512x768"] = {"target_bpp": [round(t, 5) for t in tg], "q_list": [round(q, 5) for q in q_list],
                                      "estimated_bpp": [round(v, 5) for v in est], "coded_bpp": [round(v, 5) for v in coded],
                                      "coded_over_estimated": [round(c / e, 5) for c, e in zip(coded, est)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
