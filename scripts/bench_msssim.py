#!/usr/bin/env python3
"""The MS-SSIM distortion on one GPU:

  loss   ``ops.ms_ssim`` forward and forward + backward at 64x3x256x256 (two levels x 32 images, what a first_train step
         hands the criterion), in ms per call, beside five ``vam_ssim_level`` launches on the same pyramid (the
         evaluation metric's direct 121-tap kernel, forward only, no pooling) for scale;
  train  a first_train step (32x3x256x256, qualities [0, 10], Adam) with ``metric="mse"`` against ``metric="ms-ssim"``.

Each measurement runs in a child process of its own under its own time limit; the first one that fails or runs out of time
ends the run (nothing more is started on the GPU).  Medians are reported; no time is asserted.  Prints one JSON line.

    python scripts/bench_msssim.py [--warmup 2] [--reps 9] [--steps 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L_, B, H, W = 2, 32, 256, 256
LIMITS = {"loss": 180, "train-mse": 420, "train-ms-ssim": 420}          # seconds per child


def _median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(t), 3), [round(v, 3) for v in t]


def step_loss(a):
    import torch
    import vampic
    from vampic import _lib as L, ops
    lib = L.load()
    x = vampic.synth.synth_image(B, H, W, seed=0).cuda()
    gen = torch.Generator().manual_seed(1)
    x_hat = (x.cpu().unsqueeze(0) + torch.tensor([0.1, 0.03]).reshape(2, 1, 1, 1, 1) * torch.randn((L_, B, 3, H, W), generator=gen)).cuda()
    tgt = x.unsqueeze(0).expand(L_, B, 3, H, W).reshape(L_ * B, 3, H, W).contiguous()
    y = x_hat.reshape(L_ * B, 3, H, W).requires_grad_(True)

    def fwd():
        with torch.no_grad():
            return ops.ms_ssim(tgt, y)

    def fwd_bwd():
        y.grad = None
        ops.ms_ssim(tgt, y).sum().backward()

    # the evaluation metric's kernel on the same five levels (pyramid built once, outside the timing)
    planes = L_ * B * 3
    _, _, state = ops.msssim_forward(tgt, y.detach(), keep_pyramid=True)
    pyramid, win = state[0], ops._msssim_window(x.device)
    sums = torch.zeros((5, 2, planes), dtype=torch.float64, device=x.device)

    def old_levels():
        for lvl, (xl, yl, h, w) in enumerate(pyramid):
            L.check(lib.vam_ssim_level(xl.data_ptr(), yl.data_ptr(), planes, h, w, win.data_ptr(), 1e-4, 9e-4, sums[lvl, 0].data_ptr(),
                                       sums[lvl, 1].data_ptr(), ops.stream_ptr()), "vam_ssim_level")

    res = {"case": f"{L_ * B}x3x{H}x{W}"}
    for key, fn in (("forward_ms", fwd), ("forward_backward_ms", fwd_bwd), ("five_vam_ssim_level_launches_ms", old_levels)):
        res[key], res[key + "_runs"] = _median_ms(fn, a.warmup, a.reps)
    res["ms_ssim_mean"] = round(float(fwd().mean()), 6)
    return res


def step_train(a, metric):
    import torch
    import vampic
    from vampic import finetune as ft
    from vampic.checkpoint import configure_optimizers
    from bench import build_model
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net = net.train()
    ft.first_train_setup(net)
    opt, _ = configure_optimizers(net, argparse.Namespace(learning_rate=1e-4, aux_learning_rate=1e-3, training_type="first_train"))
    crit = ft.ScalableRateDistortionLoss(lmbda_list=[0.0055, 0.04], device=dev, metric=metric)
    x = vampic.synth.synth_image(B, H, W, seed=300).to(dev)
    last = {}

    def step():
        last["crit"] = ft.first_train_step(net, crit, x, opt, [0, 10])

    ms, runs = _median_ms(step, max(a.warmup, 1), a.steps)
    return {"case": f"first_train step, {B}x3x{H}x{W}, qualities [0, 10]", "metric": metric, "ms_per_step": ms, "runs": runs,
            "loss": round(float(last["crit"]["loss"]), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step", choices=list(LIMITS), default=None, help="run one measurement in this process (what the driver starts)")
    a = ap.parse_args()
    if a.step is not None:
        res = step_loss(a) if a.step == "loss" else step_train(a, a.step[len("train-"):])
        print(json.dumps(res))
        return 0
    out = {"metric": "MS-SSIM distortion: loss and first_train step (ms, median)", "warmup": a.warmup, "reps": a.reps, "steps": a.steps}
    for name, limit in LIMITS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--warmup", str(a.warmup), "--reps", str(a.reps),
               "--steps", str(a.steps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[name] = {"error": f"no result within {limit} s"}
            break
        if p.returncode != 0:
            out[name] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            break
        out[name] = json.loads(p.stdout.strip().splitlines()[-1])
    ok = all("error" not in out.get(k, {"error": "not run"}) for k in LIMITS)
    if ok:
        out["first_train_ms_ssim_over_mse"] = round(out["train-ms-ssim"]["ms_per_step"] / out["train-mse"]["ms_per_step"], 4)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
