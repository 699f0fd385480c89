#!/usr/bin/env python3
"""Coded-size control against what it replaces, one GPU, same model, same inputs, hipGraph on.  Each part
is warmed, then the two paths alternate, each timed from a device synchronisation to the next; medians are reported.

  (a) ``coded_size_curve(x, qs)`` over the reference ``test_epoch`` list (15 qualities) against 15 real ``compress(x, q)``
      calls (every actual size is checked to lie within [bytes_lo, bytes_hi]);
  (b) ``qualities_for_bytes(x, 4 targets)`` against a plain bisection over the real ``compress`` to the same q_tol, written
      here from the public API only (the solver's answers are checked against the real compress);
  (c) ``progressive.container_sizes(x, Q_LIST)`` against ``progressive.encode_batch(x, Q_LIST)`` (every group of streams is
      checked to lie within its bounds).

Prints one JSON line.

    python scripts/bench_size.py [--warmup 2] [--reps 5]
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
SOLVER_IMAGES = 8        # (b) and (c) run on the first 8 images of a case
FRACTIONS = (0.2, 0.4, 0.6, 0.8)
Q_TOL = 1e-3


def _size(net, xb, q):
    out = net.compress(xb, q)
    return sum(len(s) for part in out["strings"][0] for s in part) + sum(len(s) for s in out["strings"][1])


def compress_sizes(net, x, qs):
    """What a user does without coded_size_curve: one real compress per quality; [len(qs), B] bytes."""
    out = torch.zeros((len(qs), x.shape[0]), dtype=torch.int64)
    for k, q in enumerate(qs):
        r = net.compress(x, q)
        for b in range(x.shape[0]):
            out[k, b] = sum(len(part[b]) for part in r["strings"][0]) + len(r["strings"][1][b])
    return out


def bisect(net, x, targets, q_tol=Q_TOL):
    """Per image and target a bisection on q over the real compress (the brackets differ per image, so every probe is one
    image).  hipGraph is off for the probes: each one is a new quality.  ``targets`` [T, B]; returns the largest probed q
    within budget (0 where not even the base fits), [T, B]."""
    T, B = targets.shape
    out = torch.zeros((T, B), dtype=torch.float64)
    graph, net.use_graph = net.use_graph, False
    try:
        for b in range(B):
            xb = x[b:b + 1]
            r0, r10 = _size(net, xb, 0.0), _size(net, xb, 10.0)
            for t in range(T):
                tg = float(targets[t, b])
                if r0 > tg or r10 <= tg:
                    out[t, b] = 10.0 if r10 <= tg else 0.0
                    continue
                lo, hi = 0.0, 10.0
                while hi - lo > q_tol:
                    mid = 0.5 * (lo + hi)
                    if _size(net, xb, mid) <= tg:
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
    net.update()
    res = {"metric": "coded-size control (ms per call, median)", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "reps": a.reps, "q_tol": Q_TOL, "curve": {}, "solver": {}, "container": {}}
    with torch.no_grad():
        for name, B, H, W in CASES:
            x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
            # (a) the sizes of the test_epoch list
            curve = lambda: net.coded_size_curve(x, QS15)
            loop = lambda: compress_sizes(net, x, QS15)
            front = lambda: net.coded_size_curve(x, [0])
            c, s = curve(), loop()
            ok = bool(((c["bytes_lo"] <= s) & (s <= c["bytes_hi"])).all())
            med, runs = _timed({"compress_loop": loop, "coded_size_curve": curve, "front_only": front}, a.warmup, a.reps)
            res["curve"][name] = dict(med, levels=len(QS15), ratio=round(med["coded_size_curve"] / med["compress_loop"], 4),
                                      actual_within_bounds=ok, max_width_bytes=int((c["bytes_hi"] - c["bytes_lo"]).max()), runs=runs)
            # (b) the qualities of four byte budgets per image
            xs = x[:SOLVER_IMAGES]
            ends = net.coded_size_curve(xs, [0, 10])["bytes_hi"].double()
            tg = torch.stack([ends[0] + f * (ends[1] - ends[0]) for f in FRACTIONS])
            solve = lambda: net.qualities_for_bytes(xs, tg, q_tol=Q_TOL)["quality"]
            plain = lambda: bisect(net, xs, tg)
            qs, qb = solve(), plain()
            fits = all(_size(net, xs[b:b + 1], float(qs[t, b])) <= float(tg[t, b]) for t in range(len(FRACTIONS)) for b in range(xs.shape[0]))
            med, runs = _timed({"bisection": plain, "solver": solve}, 1, max(1, a.reps // 2))
            res["solver"][name] = dict(med, images=xs.shape[0], targets=len(FRACTIONS), ratio=round(med["solver"] / med["bisection"], 4),
                                       max_abs_q_difference=float((qs - qb).abs().max()), solver_fits_every_budget=fits, runs=runs)
            # (c) the sizes of a container against writing it
            sizes = lambda: PR.container_sizes(net, xs, PR.Q_LIST)
            encode = lambda: PR.encode_batch(net, xs, PR.Q_LIST)[0]
            sz, cs = sizes(), encode()
            ok = all(s_["progressive"][k][0] <= sum(len(v) for v in c_["progressive"][k]) <= s_["progressive"][k][1]
                     for s_, c_ in zip(sz, cs) for k in range(len(PR.Q_LIST)))
            ok = ok and all(s_["base"][0] <= sum(len(v[0]) for v in c_["base"]) <= s_["base"][1] and
                            s_["z"][0] <= len(c_["z"][0]) <= s_["z"][1] for s_, c_ in zip(sz, cs))
            med, runs = _timed({"encode_batch": encode, "container_sizes": sizes}, a.warmup, a.reps)
            res["container"][name] = dict(med, images=xs.shape[0], layers=len(PR.Q_LIST), actual_within_bounds=ok,
                                          ratio=round(med["container_sizes"] / med["encode_batch"], 4), runs=runs)
            net._drop_plans()
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
