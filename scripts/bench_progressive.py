#!/usr/bin/env python3
"""Progressive containers: the eager harness (progressive.encode / progressive.decode, one image at a time, every level
decoded as the demo decodes it) against the batched path on the fused plans (progressive.encode_batch /
ProgressiveDecoder.decode_levels) on one GPU, same model, same inputs, hipGraph on.  Each case is
warmed, then the two paths alternate (eager, batched, eager, ...), each phase timed from a device synchronisation to the
next; medians are reported.  "encode" is the container of every image, "decode" every level 0..L of every image.  The
host coder's share of each phase (bitstream.encode / decode / encode_streams / decode_streams, wall time on the calling
thread) is reported beside it.  Prints one JSON line.

    python scripts/bench_progressive.py [--warmup 1] [--reps 3]
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

DEMO_Q = [0.01, 0.05, 0.1, 0.25, 0.5, 0.6, 0.7, 0.8, 0.9, 1, 2, 3, 4, 4.5, 10]       # reference test/parser.py:20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import bitstream as bs, progressive as P
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    coder = [0.0]

    def timed(fn):
        def run(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                coder[0] += time.perf_counter() - t0
        return run
    for name in ("encode", "decode", "encode_streams", "decode_streams"):
        setattr(bs, name, timed(getattr(bs, name)))

    def eager_enc(x, qs):
        return [P.encode(net, x[b:b + 1], q_list=qs)[0] for b in range(x.shape[0])]

    def eager_dec(cs, qs):
        outs = []
        for c in cs:                                                 # the demo's loop over the levels of one image
            d0 = P.decode(net, c, q_ind=0)
            st, last = {}, d0
            for k in range(1, len(qs) + 1):
                last = P.decode(net, c, q_ind=k, z_data=st.get("z"), res_base=d0["res_base"], entropy_data=st.get("e"))
                st = {"z": last["z_data"], "e": last["entropy_data"]}
            outs.append(last["x_hat"])
        return torch.cat(outs, 0)

    def batch_enc(x, qs):
        return P.encode_batch(net, x, qs)[0]

    def batch_dec(cs, qs):
        return P.ProgressiveDecoder(net, cs).decode_levels(list(range(len(qs) + 1)))[-1]["x_hat"]

    res = {"metric": "progressive container: eager harness vs batched plans (ms, median)", "device": torch.cuda.get_device_name(0),
           "coder_threads": bs.coder_threads(), "warmup": a.warmup, "reps": a.reps, "cases": {}}
    for case, B, H, W, qs in (("1x512x768/15", 1, 512, 768, DEMO_Q), ("8x256x256/14", 8, 256, 256, P.Q_LIST)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        paths = {"eager": (eager_enc, eager_dec), "batched": (batch_enc, batch_dec)}
        t = {f"{p}_{ph}": [] for p in paths for ph in ("enc", "enc_coder", "dec", "dec_coder")}
        same = None
        with torch.no_grad():
            for rep in range(a.warmup + a.reps):
                last = {}
                for p, (enc, dec) in paths.items():
                    torch.cuda.synchronize()
                    coder[0] = 0.0
                    t0 = time.perf_counter()
                    cs = enc(x, qs)
                    torch.cuda.synchronize()
                    t1, c1 = time.perf_counter(), coder[0]
                    coder[0] = 0.0
                    last[p] = dec(cs, qs)
                    torch.cuda.synchronize()
                    t2, c2 = time.perf_counter(), coder[0]
                    if rep >= a.warmup:
                        for k, v in (("enc", t1 - t0), ("enc_coder", c1), ("dec", t2 - t1), ("dec_coder", c2)):
                            t[f"{p}_{k}"].append(1e3 * v)
                same = float((last["eager"].clamp(0, 1) - last["batched"]).abs().max())
        med = {k: round(statistics.median(v), 1) for k, v in t.items()}
        med.update(levels=len(qs), encode_ratio=round(med["batched_enc"] / med["eager_enc"], 3),
                   decode_ratio=round(med["batched_dec"] / med["eager_dec"], 3), max_abs_xhat_diff_last_level=same)
        res["cases"][case] = med
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
