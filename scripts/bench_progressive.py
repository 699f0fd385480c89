#!/usr/bin/env python3
"""Progressive containers: the eager harness (progressive.encode / progressive.decode, one image at a time, every level
decoded as the demo decodes it) against the batched path on the fused plans (progressive.encode_batch /
ProgressiveDecoder.decode_levels) on one GPU, same model, same inputs, hipGraph on (DESIGN sections 9g, 9p).  Each case is
warmed, then the paths alternate (eager, batched, eager, ...), each phase timed from a device synchronisation to the
next; medians are reported.  "encode" is the container of every image, "decode" every level 0..L of every image.  The
host coder's share of each phase (bitstream.encode / decode / encode_streams / decode_streams, wall time on the calling
thread) is reported beside it.  Prints one JSON line.

``--coder host device`` and ``--lanes K ...`` add the batched path with every (coder, lanes) pair to the alternation on the
same build (keys ``<coder>_k<K>_*``; ``batched_*`` is host, K = 1, the default call).  For those a phase is also timed with
HIP events on the caller's stream, the coder's own share is reported as in bench_coder.py (host: wall time inside the
bitstream calls on the calling thread; device: HIP events around the coder's launches), and a third phase times every
level request of a fresh decoder on its own (``levels_wall``: the decoder with its front end, then decode(0), decode(1),
...).  The containers must be identical between the coders at equal K and every level's x_hat identical across all
variants (asserted); no time is asserted.  ``--skip-eager`` leaves the eager harness out.

    python scripts/bench_progressive.py [--warmup 1] [--reps 3] [--coder host device] [--lanes 1 64] [--skip-eager]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEMO_Q = [0.01, 0.05, 0.1, 0.25, 0.5, 0.6, 0.7, 0.8, 0.9, 1, 2, 3, 4, 4.5, 10]       # reference test/parser.py:20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--coder", nargs="+", default=["host"], choices=["host", "device"])
    ap.add_argument("--lanes", type=int, nargs="+", default=[1])
    ap.add_argument("--skip-eager", action="store_true")
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import _lib as L, bitstream as bs, progressive as P
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    lib = L.load()
    coder, pairs, depth, main_thread = [0.0], [], [0], threading.get_ident()

    def timed(fn):                       # host coder: wall time of the outermost call on the calling thread
        def run(*args, **kw):
            if threading.get_ident() != main_thread or depth[0]:
                return fn(*args, **kw)
            depth[0] += 1
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                depth[0] -= 1
                coder[0] += time.perf_counter() - t0
        return run
    for name in ("encode", "decode", "encode_streams", "decode_streams", "encode_lanes", "decode_lanes"):
        setattr(bs, name, timed(getattr(bs, name)))

    def evented(fn):                     # device coder: events around the launch, on the stream it goes to
        def run(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            pairs.append((e0, e1))
            return rc
        return run
    for name in ("vam_rans_encode_device", "vam_rans_pack_device", "vam_rans_decode_device", "vam_rans_lanes_encode_device",
                 "vam_rans_lanes_decode_device", "vam_rans_layers_encode_device", "vam_rans_layers_decode_device"):
        setattr(lib, name, evented(getattr(lib, name)))

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

    variants = [("batched" if (c, K) == ("host", 1) else f"{c}_k{K}", c, K) for K in a.lanes for c in a.coder]
    plain = [v[0] for v in variants] == ["batched"]                 # the default call: the report of the eager comparison alone

    def phase(fn, is_device):
        """(result, wall ms, events ms, coder ms) of one phase, from a device synchronisation to the next."""
        torch.cuda.synchronize()
        coder[0] = 0.0
        del pairs[:]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        return out, wall, e0.elapsed_time(e1), (sum(p.elapsed_time(q_) for p, q_ in pairs) if is_device else 1e3 * coder[0])

    res = {"metric": "progressive container: eager harness vs batched plans, host coder vs device coder (ms, median)",
           "device": torch.cuda.get_device_name(0), "coder_threads": bs.coder_threads(), "warmup": a.warmup, "reps": a.reps,
           "variants": [v[0] for v in variants], "cases": {}}
    for case, B, H, W, qs in (("1x512x768/15", 1, 512, 768, DEMO_Q), ("8x256x256/14", 8, 256, 256, P.Q_LIST)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        levels = list(range(len(qs) + 1))
        names = ([] if a.skip_eager else ["eager"]) + [v[0] for v in variants]
        t = {f"{p}_{ph}": [] for p in names for ph in ("enc", "enc_events", "enc_coder", "dec", "dec_events", "dec_coder")}
        per_level = {v[0]: [] for v in variants}
        same, made = None, {}
        with torch.no_grad():
            for rep in range(a.warmup + a.reps):
                row, outs = {}, {}
                if not a.skip_eager:
                    cs, *enc_t = phase(lambda: eager_enc(x, qs), False)
                    eager_last, *dec_t = phase(lambda: eager_dec(cs, qs), False)
                    row["eager"] = enc_t + dec_t
                for label, c, K in variants:
                    cs, *enc_t = phase(lambda: P.encode_batch(net, x, qs, coder=c, lanes=K)[0], c == "device")
                    outs[label], *dec_t = phase(lambda: [o["x_hat"] for o in P.ProgressiveDecoder(net, cs, coder=c).decode_levels(levels)],
                                                c == "device")
                    row[label], made[(c, K)] = enc_t + dec_t, cs
                    if not plain:                # a fresh decoder, every level request on its own
                        lv, dec = [], None
                        for k in levels:
                            def one(k=k):
                                nonlocal dec
                                dec = P.ProgressiveDecoder(net, cs, coder=c) if dec is None else dec
                                return dec.decode(k)
                            lv.append(phase(one, c == "device")[1])
                        if rep >= a.warmup:
                            per_level[label].append(lv)
                if rep >= a.warmup:
                    for p, v in row.items():
                        for k, ms in zip(("enc", "enc_events", "enc_coder", "dec", "dec_events", "dec_coder"), v):
                            t[f"{p}_{k}"].append(ms)
                ref = outs[variants[0][0]]
                for label, _, _ in variants[1:]:
                    assert all(torch.equal(u, v) for u, v in zip(ref, outs[label])), f"{case}: a level's x_hat of {label} differs"
                for K in a.lanes:
                    assert len(a.coder) < 2 or made[("host", K)] == made[("device", K)], f"{case}: the containers differ at {K} lanes"
                if not a.skip_eager:
                    same = float((eager_last.clamp(0, 1) - ref[-1]).abs().max())
        med = {k: round(statistics.median(v), 1 if plain else 2) for k, v in t.items()}
        if plain:                                # the keys of the eager comparison, as they have always been
            med = {k: v for k, v in med.items() if not k.endswith("_events")}
        else:
            size = lambda cs: sum(len(c["z"][0]) + sum(len(s[0]) for s in c["base"]) + sum(len(s) for l_ in c["progressive"] for s in l_)
                                  for c in cs)
            for label, c, K in variants:
                lv = [round(statistics.median(col), 2) for col in zip(*per_level[label])]
                med.update({f"{label}_levels_wall": lv, f"{label}_levels_wall_sum": round(sum(lv), 2),
                            f"{label}_container_bytes_per_image": round(size(made[(c, K)]) / B, 1)})
            first = variants[0][0]
            for label, _, _ in variants[1:]:
                med.update({f"{label}_encode_ratio_vs_{first}": round(med[f"{label}_enc"] / med[f"{first}_enc"], 3),
                            f"{label}_decode_ratio_vs_{first}": round(med[f"{label}_dec"] / med[f"{first}_dec"], 3)})
            med.update(containers_identical_at_equal_lanes=True, x_hat_identical_at_every_level=True,
                       streams_per_image=net.ns0 * (len(qs) + 1) + 1)
        med["levels"] = len(qs)
        if not a.skip_eager:
            first = variants[0][0]
            med.update(encode_ratio=round(med[f"{first}_enc"] / med["eager_enc"], 3),
                       decode_ratio=round(med[f"{first}_dec"] / med["eager_dec"], 3), max_abs_xhat_diff_last_level=same)
        res["cases"][case] = med
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
