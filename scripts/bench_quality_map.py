#!/usr/bin/env python3
"""A quality map against per-image qualities, one GPU, same model, same input, hipGraph on:
``forward_quality_map`` with a centre-box map (q_roi inside, q_bg outside) against ``forward_per_image`` at q_roi for every
image, at 32x3x256x256.  The two plans differ in the last pass of ONE mask launch.  Both are warmed, then they alternate, each
timed from a device synchronisation to the next; medians are reported.  A constant map is checked against
``forward_per_image`` first (identical tensors); no time is asserted.  Also timed: ``quality_map_rate`` and
``quality_map_for_bpp`` (one target per image) for the same floor map.

Prints one JSON line.

    python scripts/bench_quality_map.py [--warmup 2] [--reps 9]
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

B, H, W = 32, 256, 256
Q_ROI, Q_BG = 8.0, 1.0


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
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import evaluate as EV
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
    box = [(b, H // 4, W // 4, 3 * H // 4, 3 * W // 4, Q_ROI) for b in range(B)]
    qmap = EV.quality_map_from_boxes(B, H, W, Q_BG, box)
    floor = EV.quality_map_from_boxes(B, H, W, 0.0, box)
    const = torch.full_like(qmap, Q_ROI)
    res = {"metric": "quality map against per-image qualities (ms per call, median)", "device": torch.cuda.get_device_name(0),
           "case": f"{B}x3x{H}x{W}", "q_roi": Q_ROI, "q_bg": Q_BG, "warmup": a.warmup, "reps": a.reps}
    with torch.no_grad():
        one, ref = net.forward_quality_map(x, const), net.forward_per_image(x, [Q_ROI] * B)
        same = all(torch.equal(one[k], ref[k]) for k in ("x_hat", "y_hat", "mask"))
        assert same, "a constant map and forward_per_image differ"
        fns = {"forward_per_image": lambda: net.forward_per_image(x, [Q_ROI] * B),
               "forward_quality_map": lambda: net.forward_quality_map(x, qmap)}
        med, runs = _timed(fns, a.warmup, a.reps)
        res["forward"] = dict(med, ratio=round(med["forward_quality_map"] / med["forward_per_image"], 4), constant_map_identical=same,
                              runs=runs)
        ends = torch.stack([net.quality_map_rate(x, floor)["bpp"], net.quality_map_rate(x, const.fill_(10.0))["bpp"]]).cpu()
        target = (0.5 * (ends[0] + ends[1])).unsqueeze(0)
        fns = {"quality_map_rate": lambda: net.quality_map_rate(x, qmap),
               "quality_map_for_bpp": lambda: net.quality_map_for_bpp(x, floor, target)}
        med, runs = _timed(fns, a.warmup, a.reps)
        sol = net.quality_map_for_bpp(x, floor, target)
        res["rate"] = dict(med, reached=int(sol["reached"].sum()), q_min=round(float(sol["quality"].min()), 4),
                           q_max=round(float(sol["quality"].max()), 4), runs=runs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
