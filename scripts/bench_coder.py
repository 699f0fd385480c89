#!/usr/bin/env python3
"""The rANS coder on the device against the host coder (DESIGN sections 9n, 9o): ``compress`` and ``decompress`` at q = 2.5
with ``model.coder`` "host" and "device" on one GPU, same build, same model, same inputs, hipGraph on.  The host coder is
the baseline.  Each case is warmed, then the coders alternate; a call is timed twice: wall time from a device
synchronisation to the next, and HIP events on the caller's stream around the call.  Medians are reported.  Beside each
time: the coder's own share — host: wall time inside the bitstream calls on the calling thread; device: HIP events around
the vam_rans_encode_device / vam_rans_pack_device / vam_rans_decode_device launches — and the bytes copied each way for the
coder (host: the symbol and index tensors; device: lengths, status and coded bytes down, the strings with their offset
table up).  The strings of the two coders and x_hat must be identical (asserted); no time is asserted.  Prints one JSON
line.

``--lanes K [K ...]`` adds the device coder with ``model.coder_lanes`` = K to the alternation (keys ``device_k<K>_*``), the
coded bytes per image at every K against K = 1 and the overhead per stream against the 4 K + 8 (K - 1) bytes of the header
and the extra final states; x_hat must be identical across all of them and the strings identical to the host coder's at
the same K (asserted; the host's K > 1 strings are coded once per case, outside the timing).

    python scripts/bench_coder.py [--warmup 2] [--reps 10] [--lanes 8 64]
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

Q = 2.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lanes", type=int, nargs="*", default=[], help="also run the device coder with these coder_lanes")
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import _lib as L, bitstream as bs
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    lib = L.load()
    host_s, pairs, moved = [0.0], [], {"down": 0, "up": 0}

    def timed(fn):                       # host coder: wall time on the calling thread
        def run(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                host_s[0] += time.perf_counter() - t0
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
                 "vam_rans_lanes_decode_device"):
        setattr(lib, name, evented(getattr(lib, name)))

    enc_dev, upload = bs.encode_streams_device, bs.upload_streams

    def counted_encode(*args, **kw):
        out = enc_dev(*args, **kw)
        moved["down"] += 8 * sum(len(row) for row in out) + sum(len(s) for row in out for s in row)
        return out

    def counted_upload(strings, device, lanes=1):
        up = upload(strings, device, lanes)
        moved["up"] += up.buf.numel()
        return up
    bs.encode_streams_device, bs.upload_streams = counted_encode, counted_upload

    res = {"metric": "compress / decompress at q = 2.5, host coder vs device coder (ms, median)",
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "lanes": a.lanes, "cases": {}}
    configs = [("host", "host", 1), ("device", "device", 1)] + [(f"device_k{K}", "device", K) for K in a.lanes]
    for case, B, H, W in (("32x3x256x256", 32, 256, 256), ("8x3x256x256", 8, 256, 256), ("1x3x512x768", 1, 512, 768)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        h, w, n_sl, C, M_, N = H // 16, W // 16, net.ns1, net.dim_chunk, net.ns1 * net.dim_chunk, net.N
        t = {f"{c}_{k}": [] for c, _, _ in configs
             for k in ("enc_wall", "enc_events", "enc_coder", "dec_wall", "dec_events", "dec_coder")}
        last, host_at = {}, {}
        with torch.no_grad():
            net.coder = "host"
            for K in a.lanes:                        # the host coder's strings at every K: coded once, not timed
                net.coder_lanes = K
                host_at[K] = net.compress(x, quality=Q)["strings"]
            for rep in range(a.warmup + a.reps):
                for label, coder, K in configs:
                    net.coder, net.coder_lanes = coder, K
                    row = {}
                    for phase in ("enc", "dec"):
                        torch.cuda.synchronize()
                        host_s[0], moved["down"], moved["up"] = 0.0, 0, 0
                        del pairs[:]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        e0.record()
                        if phase == "enc":
                            enc = net.compress(x, quality=Q)
                        else:
                            dec = net.decompress(enc["strings"], enc["shape"], quality=Q)["x_hat"]
                        e1.record()
                        torch.cuda.synchronize()
                        row[f"{phase}_wall"] = 1e3 * (time.perf_counter() - t0)
                        row[f"{phase}_events"] = e0.elapsed_time(e1)
                        row[f"{phase}_coder"] = 1e3 * host_s[0] if coder == "host" else sum(p.elapsed_time(q_) for p, q_ in pairs)
                        row[f"{phase}_bytes"] = dict(moved)
                    if rep >= a.warmup:
                        for k in ("enc_wall", "enc_events", "enc_coder", "dec_wall", "dec_events", "dec_coder"):
                            t[f"{label}_{k}"].append(row[k])
                    last[label] = (enc["strings"], dec, row["enc_bytes"], row["dec_bytes"])
                assert last["host"][0] == last["device"][0], f"{case}: the coders' strings differ"
                for label, _, K in configs[1:]:
                    assert torch.equal(last["host"][1], last[label][1]), f"{case}: x_hat of {label} differs from the host coder's"
                    assert K == 1 or last[label][0] == host_at[K], f"{case}: the coders' strings differ at {K} lanes"
        med = {k: round(statistics.median(v), 2) for k, v in t.items()}
        n_streams = (n_sl + 1) * B
        size = lambda strings: sum(len(s) for row in strings[0] for s in row) + sum(len(s) for s in strings[1])
        coded = size(last["host"][0])
        for label, _, K in configs[2:]:
            med.update({f"{label}_encode_ratio": round(med[f"{label}_enc_wall"] / med["host_enc_wall"], 3),
                        f"{label}_decode_ratio": round(med[f"{label}_dec_wall"] / med["host_dec_wall"], 3),
                        f"{label}_bytes_per_image": round(size(last[label][0]) / B, 1),
                        f"{label}_overhead_per_stream": round((size(last[label][0]) - coded) / n_streams, 2),
                        f"{label}_overhead_expected": 4 * K + 8 * (K - 1),
                        f"{label}_enc_bytes_down": last[label][2]["down"], f"{label}_dec_bytes_up": last[label][3]["up"],
                        f"{label}_dec_bytes_down": 4 * n_streams * K})
        med["bytes_per_image"] = round(coded / B, 1)
        med.update(streams=n_streams, coded_bytes=coded, strings_identical=True, x_hat_identical=True,
                   encode_ratio=round(med["device_enc_wall"] / med["host_enc_wall"], 3),
                   decode_ratio=round(med["device_dec_wall"] / med["host_dec_wall"], 3),
                   # host coder: sym, idx [B,h,w,M] and z symbols [B,h/4,w/4,N] down; per slice the indexes down, the symbols up
                   host_enc_bytes_down=4 * B * (2 * h * w * M_ + (h // 4) * (w // 4) * N),
                   host_dec_bytes_down=4 * B * h * w * M_, host_dec_bytes_up=4 * B * (h * w * M_ + (h // 4) * (w // 4) * N),
                   device_enc_bytes_down=last["device"][2]["down"], device_dec_bytes_up=last["device"][3]["up"],
                   device_dec_bytes_down=4 * n_streams)
        res["cases"][case] = med
        net._drop_plans()
        torch.cuda.empty_cache()
    net.coder, net.coder_lanes = "host", 1
    print(json.dumps(res))


if __name__ == "__main__":
    main()
