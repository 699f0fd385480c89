#!/usr/bin/env python3
"""Embedded streams (embedded.encode_batch / EmbeddedDecoder) against the layered container
(progressive.encode_batch / ProgressiveDecoder, section 9g) on one GPU, same model, same inputs, hipGraph on, at section
9g's two inputs.  Each case is warmed, then the two formats alternate (layered, embedded, layered, ...), each phase timed
from a device synchronisation to the next; medians are reported.  "encode" is the container of every image, "decode" the
base and every quality of the list for every image.  The coder's share of each phase (host: the bitstream calls, wall time
on the calling thread; device: HIP events around the device coder's calls, the embedded launches also on their own) is
reported beside it, and the bytes per image: the embedded streams at full length against the
layered container's progressive streams.  x_hat of every level must be identical between the two formats (asserted); no
time is asserted.  Prints one JSON line.

``--coder`` and ``--lanes`` add one embedded cell per (coder, lanes per embedded stream) to the same
alternation: encode ms, decode ms and bytes per image under "cells", next to the host K = 1 cell of the same run, which is
the "embedded" path above.  x_hat of every level is asserted identical for every cell.

``--schedule roi`` measures scheduled streams instead: a centre box climbs through 3 stages to
q = 10 over background 0, then the background climbs through 3 stages.  Per (coder, lanes) cell the scheduled encode and the
decode of all 6 stages alternate with the plain embedded encode and the decode of as many marks, same run, same inputs;
before timing, x_hat of every stage is asserted identical to ``forward_quality_map`` of that stage's map.  The plain cells
are the same calls the default mode times.

``--resume S`` measures a receiver whose bytes keep arriving: every container is received in S equal
byte steps.  Per (coder, lanes) cell, (a) a fresh EmbeddedDecoder on the prefix of every step, the only way without
checkpoints, alternates with (b) ONE resumable decoder and ``extend`` per step, same run, same containers; each step ends
with ``decode()``.  Per step and in total: the wall time and the entropy-decode share of the embedded streams (host: the
bitstream call, wall time; device: HIP events around the launch).  x_hat of every step is asserted identical
between (a) and (b); no time is asserted.

``--base-lanes 1 8 64`` measures z and the base slices as interleaved strings on Kb lanes
(``encode_batch(..., base_lanes=Kb)``, format "embedded-4") next to today's K = 1 strings.  One cell per (coder, lanes, Kb),
the cells alternating on one build at the two inputs above: encode and decode wall time (decode = the decoder, the base and
every mark), the coder's share (host: the bitstream calls, wall time; device: HIP events around the device coder's calls),
within it the z + base part (device: events around those launches alone; host decode: the wall time of the strict / K = 1
string decodes; host encode: not separable where one call codes base and embedded streams), and the bytes of z + base per
image.  In the same run the layered container's device front end — ``progressive`` with ``coder="device"`` and ``lanes`` =
Kb, a LANE-SPLIT base (section 9o) — is timed at every Kb, which puts the two lane formats side by side.  x_hat of every
level is asserted identical across all cells; no time is asserted.

``--stream S`` measures the same receiver fed one byte string per image: every codestream
(``embedded.to_bytes``) is cut into S steps, the first up to an S-th of its body, the others an S-th of the body each.  Per
(coder, lanes) cell three paths alternate on the same prefixes: (a) a fresh EmbeddedDecoder on ``from_bytes`` of every
prefix, (b) one resumable decoder with ``delta`` + ``extend``, (c) one ``StreamDecoder`` and ``feed`` of the raw bytes; each
step ends with ``decode()``.  (c) - (b) per step is what the framing costs a receiver.  x_hat of every step is asserted
identical across the three; no time is asserted.

    python scripts/bench_embedded.py [--warmup 1] [--reps 3] [--coder host device] [--lanes 1 8 64]
                                     [--schedule roi | --resume S | --stream S | --base-lanes 1 8 64]
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

ROI_Q, BACKGROUND_Q = [1, 4, 10], [0, 0.5, 2, 5]          # --schedule roi: 3 region stages, then 3 background stages
PLAIN_MARKS = [0.5, 1, 2, 4, 5, 10]                        # as many marks for the plain path of the same run
DEMO_Q = [0.01, 0.05, 0.1, 0.25, 0.5, 0.6, 0.7, 0.8, 0.9, 1, 2, 3, 4, 4.5, 10]       # reference test/parser.py:20


def schedule_main(a, net, dev):
    """--schedule roi: scheduled against plain embedded streams, interleaved; prints one JSON line."""
    import vampic
    from vampic import bitstream as bs, embedded as EB, evaluate as EV
    res = {"metric": "scheduled vs plain embedded streams (ms, median)", "device": torch.cuda.get_device_name(0),
           "coder_threads": bs.coder_threads(), "warmup": a.warmup, "reps": a.reps, "stages": len(ROI_Q) + len(BACKGROUND_Q) - 1,
           "cases": {}}
    for case, B, H, W in (("1x512x768", 1, 512, 768), ("8x256x256", 8, 256, 256)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        S = EV.roi_schedule(B, H, W, [(b, H // 4, W // 4, 3 * H // 4, 3 * W // 4) for b in range(B)], ROI_Q, BACKGROUND_Q)
        ks = list(range(len(S)))
        assert len(S) == len(PLAIN_MARKS)
        cells = {}
        for c in a.coder:
            for K in a.lanes:
                cells[f"plain_{c}_k{K}"] = (lambda c=c, K=K: EB.encode_batch(net, x, PLAIN_MARKS, coder=c, lanes=K),
                                            lambda cs, c=c: EB.EmbeddedDecoder(net, cs, coder=c).decode_qualities(PLAIN_MARKS))
                cells[f"scheduled_{c}_k{K}"] = (lambda c=c, K=K: EB.encode_batch(net, x, schedule=S, coder=c, lanes=K),
                                                lambda cs, c=c: EB.EmbeddedDecoder(net, cs, coder=c).decode_stages(ks))
        t = {f"{p}_{ph}": [] for p in cells for ph in ("enc", "dec")}
        size = {}
        with torch.no_grad():
            want = [net.forward_quality_map(x, m)["x_hat"] for m in S]
            for p, (enc, dec) in cells.items():                                  # equality before any timing
                if p.startswith("scheduled"):
                    for k, (o, w_) in enumerate(zip(dec(enc()), want)):
                        assert torch.equal(o["x_hat"], w_), f"{case}: {p}: x_hat of stage {k} differs from forward_quality_map"
            for rep in range(a.warmup + a.reps):
                for p, (enc, dec) in cells.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    cs = enc()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    dec(cs)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if rep >= a.warmup:
                        t[f"{p}_enc"].append(1e3 * (t1 - t0))
                        t[f"{p}_dec"].append(1e3 * (t2 - t1))
                    size[p] = sum(len(s_) for c_ in cs for s_ in c_["embedded"]) / B
        med = {k: round(statistics.median(v), 1) for k, v in t.items()}
        med.update(x_hat_identical_to_forward_quality_map=True, side_bytes_per_image=cs[0].get("side_bytes"),
                   embedded_bytes_per_image={p: round(v, 1) for p, v in size.items()})
        res["cases"][case] = med
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


def resume_main(a, net, dev):
    """--resume S: a fresh decoder per step against one resumable decoder and extend, interleaved; prints one JSON line."""
    import vampic
    from vampic import bitstream as bs, embedded as EB
    S = a.resume
    share = {"host": 0.0, "events": []}

    def timed(fn):
        def run(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                share["host"] += time.perf_counter() - t0
        return run

    def evented(fn):
        def run(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return fn(*args, **kw)
            finally:
                e1.record()
                share["events"].append((e0, e1))
        return run
    for name in ("decode_prefix_streams", "resume_prefix_streams"):
        setattr(bs, name, timed(getattr(bs, name)))
    for name in ("decode_embedded_uploaded", "resume_embedded_uploaded"):
        setattr(bs, name, evented(getattr(bs, name)))

    def drain():
        ms = 1e3 * share["host"] + sum(e0.elapsed_time(e1) for e0, e1 in share["events"])
        share["host"] = 0.0
        share["events"].clear()
        return ms

    res = {"metric": "receiving a container in steps: fresh decoder per step (a) vs extend (b) (ms, median)",
           "device": torch.cuda.get_device_name(0), "coder_threads": bs.coder_threads(), "warmup": a.warmup, "reps": a.reps,
           "steps": S, "cases": {}}
    for case, B, H, W in (("1x512x768", 1, 512, 768), ("8x256x256", 8, 256, 256)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        out = {}
        with torch.no_grad():
            for c in a.coder:
                for K in a.lanes:
                    cs = EB.encode_batch(net, x, coder=c, lanes=K)
                    prefixes = [[EB.truncate(c_, slice_bytes=[len(s_) * i // S for s_ in c_["embedded"]]) for c_ in cs]
                                for i in range(1, S + 1)]
                    more = [None] + [[EB.delta(now, held) for now, held in zip(prefixes[i], prefixes[i - 1])] for i in range(1, S)]
                    t = {k: [[] for _ in range(S)] for k in ("fresh_ms", "fresh_coder_ms", "extend_ms", "extend_coder_ms")}
                    for r in range(a.warmup + a.reps):
                        hats = {}
                        for path in ("fresh", "extend"):
                            dec = None
                            for i in range(S):
                                torch.cuda.synchronize()
                                drain()
                                t0 = time.perf_counter()
                                if path == "fresh":
                                    dec = EB.EmbeddedDecoder(net, prefixes[i], coder=c)
                                elif i == 0:
                                    dec = EB.EmbeddedDecoder(net, prefixes[0], coder=c, resumable=True)
                                else:
                                    dec.extend(more[i])
                                x_hat = dec.decode()["x_hat"]
                                torch.cuda.synchronize()
                                ms = 1e3 * (time.perf_counter() - t0)
                                if r >= a.warmup:
                                    t[f"{path}_ms"][i].append(ms)
                                    t[f"{path}_coder_ms"][i].append(drain())
                                hats[path, i] = x_hat
                        for i in range(S):
                            assert torch.equal(hats["fresh", i], hats["extend", i]), f"{case}: {c} K={K}: x_hat of step {i} differs"
                    med = {k: [round(statistics.median(v), 2) for v in rows] for k, rows in t.items()}
                    med.update({f"{k}_total": round(sum(v), 2) for k, v in list(med.items())})
                    med.update(x_hat_identical=True, bytes_per_image=round(sum(len(s_) for c_ in cs for s_ in c_["embedded"]) / B, 1))
                    out[f"{c}_k{K}"] = med
        res["cases"][case] = out
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


def stream_main(a, net, dev):
    """--stream S: every image's codestream received in S byte steps; fresh decoder per step (a), delta + extend (b) and
    StreamDecoder.feed of the raw bytes (c) on the same prefixes, interleaved; prints one JSON line."""
    import vampic
    from vampic import bitstream as bs, embedded as EB
    S = a.stream
    res = {"metric": "receiving a codestream in steps: fresh decoder per step (a) vs delta + extend (b) vs StreamDecoder.feed (c) "
                     "(ms, median)", "device": torch.cuda.get_device_name(0), "coder_threads": bs.coder_threads(), "warmup": a.warmup,
           "reps": a.reps, "steps": S, "cases": {}}
    for case, B, H, W in (("1x512x768", 1, 512, 768), ("8x256x256", 8, 256, 256)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        out = {}
        with torch.no_grad():
            for c in a.coder:
                for K in a.lanes:
                    cs = EB.encode_batch(net, x, coder=c, lanes=K)
                    data = [EB.to_bytes(c_) for c_ in cs]
                    lay = [EB.layout(d) for d in data]
                    cuts = [[v["base_end"] + (v["total"] - v["base_end"]) * i // S for v in lay] for i in range(1, S + 1)]
                    t0 = time.perf_counter()
                    prefixes = [[EB.from_bytes(d[:n]) for d, n in zip(data, row)] for row in cuts]
                    demux_ms = 1e3 * (time.perf_counter() - t0) / S
                    more = [None] + [[EB.delta(now, held) for now, held in zip(prefixes[i], prefixes[i - 1])] for i in range(1, S)]
                    chunks = [[d[(cuts[i - 1][b] if i else 0):cuts[i][b]] for b, d in enumerate(data)] for i in range(S)]
                    t = {f"{p}_ms": [[] for _ in range(S)] for p in ("fresh", "extend", "feed")}
                    for r in range(a.warmup + a.reps):
                        hats = {}
                        for path in ("fresh", "extend", "feed"):
                            dec = None
                            for i in range(S):
                                torch.cuda.synchronize()
                                t0 = time.perf_counter()
                                if path == "fresh":
                                    dec = EB.EmbeddedDecoder(net, prefixes[i], coder=c)
                                elif path == "extend":
                                    if i == 0:
                                        dec = EB.EmbeddedDecoder(net, prefixes[0], coder=c, resumable=True)
                                    else:
                                        dec.extend(more[i])
                                else:
                                    dec = EB.StreamDecoder(net, B, coder=c) if i == 0 else dec
                                    dec.feed(chunks[i])
                                x_hat = dec.decode()["x_hat"]
                                torch.cuda.synchronize()
                                if r >= a.warmup:
                                    t[f"{path}_ms"][i].append(1e3 * (time.perf_counter() - t0))
                                hats[path, i] = x_hat
                        for i in range(S):
                            assert torch.equal(hats["fresh", i], hats["extend", i]) and torch.equal(hats["fresh", i], hats["feed", i]), \
                                f"{case}: {c} K={K}: x_hat of step {i} differs"
                    med = {k: [round(statistics.median(v), 2) for v in rows] for k, rows in t.items()}
                    med.update({f"{k}_total": round(sum(v), 2) for k, v in list(med.items())})
                    med.update(x_hat_identical=True, from_bytes_ms_per_prefix=round(demux_ms, 3), header_bytes=lay[0]["header_end"],
                               stream_bytes_per_image=round(sum(len(d) for d in data) / B, 1),
                               feed_minus_extend_ms_per_step=round((med["feed_ms_total"] - med["feed_ms"][0]
                                                                    - med["extend_ms_total"] + med["extend_ms"][0]) / (S - 1), 3))
                    out[f"{c}_k{K}"] = med
        res["cases"][case] = out
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


def base_lanes_main(a, net, dev):
    """--base-lanes: an interleaved base on Kb lanes against the K = 1 base, cells interleaved; prints one JSON line."""
    import vampic
    from vampic import bitstream as bs, embedded as EB, progressive as P
    acc = {"host": 0.0, "host_zb": 0.0, "coder": [], "zb": []}

    def timed(fn, *keys):
        def run(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                for k in keys:
                    acc[k] += time.perf_counter() - t0
        return run

    def evented(fn, *keys):
        def run(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return fn(*args, **kw)
            finally:
                e1.record()
                for k in keys:
                    acc[k].append((e0, e1))
        return run
    for name in ("encode_streams", "encode_interleaved_streams", "decode_prefix_streams"):
        setattr(bs, name, timed(getattr(bs, name), "host"))
    for name in ("decode", "decode_interleaved_strict"):                         # the host decoder's z and base strings
        setattr(bs, name, timed(getattr(bs, name), "host", "host_zb"))
    EB._map_threads = timed(EB._map_threads, "host")
    for name in ("encode_streams_device", "encode_window_interleaved_device", "decode_uploaded", "decode_window_interleaved_uploaded"):
        setattr(bs, name, evented(getattr(bs, name), "coder", "zb"))             # the device coder's z and base launches
    for name in ("encode_embedded_device", "decode_embedded_uploaded", "encode_layers_device"):
        setattr(bs, name, evented(getattr(bs, name), "coder"))

    def drain():
        """(coder ms, z + base ms) since the last call; after a synchronise."""
        out = (1e3 * acc["host"] + sum(e0.elapsed_time(e1) for e0, e1 in acc["coder"]),
               1e3 * acc["host_zb"] + sum(e0.elapsed_time(e1) for e0, e1 in acc["zb"]))
        acc["host"] = acc["host_zb"] = 0.0
        acc["coder"].clear()
        acc["zb"].clear()
        return out

    res = {"metric": "embedded containers: interleaved base on Kb lanes vs the K = 1 base (ms, median)",
           "device": torch.cuda.get_device_name(0), "coder_threads": bs.coder_threads(), "warmup": a.warmup, "reps": a.reps, "cases": {}}
    for case, B, H, W, qs in (("1x512x768/15", 1, 512, 768, DEMO_Q), ("8x256x256/14", 8, 256, 256, P.Q_LIST)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        cells = {f"{c}_k{K}_b{Kb}": (lambda c=c, K=K, Kb=Kb: EB.encode_batch(net, x, qs, coder=c, lanes=K, base_lanes=Kb),
                                     lambda cs, c=c: [o["x_hat"] for o in EB.EmbeddedDecoder(net, cs, coder=c).decode_qualities([0.0] + list(qs))])
                 for c in a.coder for K in a.lanes for Kb in a.base_lanes}
        front = {f"layered_device_lanes{Kb}": (lambda Kb=Kb: P.encode_batch(net, x, qs, coder="device", lanes=Kb)[0],
                                                lambda cs: [P.ProgressiveDecoder(net, cs, coder="device").decode_levels([0])[0]["x_hat"]])
                 for Kb in a.base_lanes}
        keys = ("enc", "enc_coder", "enc_zbase", "dec", "dec_coder", "dec_zbase")
        t = {f"{p}_{k}": [] for p in list(cells) + list(front) for k in keys}
        size = {}
        with torch.no_grad():
            for r in range(a.warmup + a.reps):
                last = {}
                for p, (enc, dec) in list(cells.items()) + list(front.items()):
                    torch.cuda.synchronize()
                    drain()
                    t0 = time.perf_counter()
                    cs = enc()
                    torch.cuda.synchronize()
                    t1, (c1, z1) = time.perf_counter(), drain()
                    last[p] = dec(cs)
                    torch.cuda.synchronize()
                    t2, (c2, z2) = time.perf_counter(), drain()
                    if r >= a.warmup:
                        for k, v in zip(keys, (1e3 * (t1 - t0), c1, z1, 1e3 * (t2 - t1), c2, z2)):
                            t[f"{p}_{k}"].append(v)
                    size[p] = sum(sum(len(s_) for s_ in c_["z"]) + sum(len(s_[0]) for s_ in c_["base"]) for c_ in cs) / B
                first = last[next(iter(cells))]
                for p in cells:
                    for k, (u, v) in enumerate(zip(first, last[p])):
                        assert torch.equal(u, v), f"{case}: x_hat of level {k} differs between {next(iter(cells))} and {p}"
                for p in front:                                                  # the layered container's level 0 is the base
                    assert torch.equal(first[0], last[p][0]), f"{case}: the base x_hat differs between the embedded cells and {p}"
        med = {k: round(statistics.median(v), 1) for k, v in t.items()}
        row = lambda p: dict({k + "_ms": med[f"{p}_{k}"] for k in keys}, z_base_bytes_per_image=round(size[p], 1))
        out = {"levels": len(qs), "x_hat_identical": True, "cells": {p: row(p) for p in cells}, "layered_front": {p: row(p) for p in front}}
        for p, v in out["cells"].items():
            if p.startswith("host"):
                v["enc_zbase_ms"] = None                                         # one host call codes base and embedded streams
        res["cases"][case] = out
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--coder", nargs="+", default=["host"], choices=["host", "device"])
    ap.add_argument("--lanes", nargs="+", type=int, default=[1])
    ap.add_argument("--schedule", choices=["roi"], default=None)
    ap.add_argument("--resume", type=int, default=None, metavar="S")
    ap.add_argument("--base-lanes", nargs="+", type=int, default=None, metavar="Kb")
    ap.add_argument("--stream", type=int, default=None, metavar="S")
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import bitstream as bs, embedded as EB, progressive as P
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    if sum(v is not None for v in (a.schedule, a.resume, a.base_lanes, a.stream)) > 1:
        ap.error("--schedule, --resume, --stream and --base-lanes measure different things: give one")
    if a.stream is not None:
        if a.stream < 2:
            ap.error("--stream takes S >= 2 steps")
        return stream_main(a, net, dev)
    if a.base_lanes is not None:
        return base_lanes_main(a, net, dev)
    if a.schedule:
        return schedule_main(a, net, dev)
    if a.resume is not None:
        if a.resume < 2:
            ap.error("--resume takes S >= 2 steps")
        return resume_main(a, net, dev)
    coder = [0.0]

    def timed(fn):
        def run(*args, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                coder[0] += time.perf_counter() - t0
        return run
    for name in ("encode", "decode", "encode_streams", "decode_streams", "decode_prefix_streams"):
        setattr(bs, name, timed(getattr(bs, name)))
    EB._map_threads = timed(EB._map_threads)     # prefix_bytes runs on worker threads: timed around the map
    events = {"coder": [], "emb": []}            # device coder: HIP events around its calls, read after the phase's synchronise

    def evented(fn, *keys):
        def run(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return fn(*args, **kw)
            finally:
                e1.record()
                for k in keys:
                    events[k].append((e0, e1))
        return run
    for name in ("encode_streams_device", "decode_uploaded"):
        setattr(bs, name, evented(getattr(bs, name), "coder"))
    for name in ("encode_embedded_device", "decode_embedded_uploaded"):
        setattr(bs, name, evented(getattr(bs, name), "coder", "emb"))

    def drain(key):
        ms = sum(e0.elapsed_time(e1) for e0, e1 in events[key])
        events[key].clear()
        return ms

    def layered_enc(x, qs):
        return P.encode_batch(net, x, qs)[0]

    def layered_dec(cs, qs):
        return [o["x_hat"] for o in P.ProgressiveDecoder(net, cs).decode_levels(list(range(len(qs) + 1)))]

    def embedded_enc(x, qs):
        return EB.encode_batch(net, x, qs)

    def embedded_dec(cs, qs):
        return [o["x_hat"] for o in EB.EmbeddedDecoder(net, cs).decode_qualities([0.0] + list(qs))]

    def cell(coder_, K):
        return (lambda x, qs: EB.encode_batch(net, x, qs, coder=coder_, lanes=K),
                lambda cs, qs: [o["x_hat"] for o in EB.EmbeddedDecoder(net, cs, coder=coder_).decode_qualities([0.0] + list(qs))])

    cells = [(c, K) for c in a.coder for K in a.lanes if (c, K) != ("host", 1)]
    res = {"metric": "embedded streams vs layered container (ms, median)", "device": torch.cuda.get_device_name(0),
           "coder_threads": bs.coder_threads(), "warmup": a.warmup, "reps": a.reps, "cases": {}}
    for case, B, H, W, qs in (("1x512x768/15", 1, 512, 768, DEMO_Q), ("8x256x256/14", 8, 256, 256, P.Q_LIST)):
        x = vampic.synth.synth_image(B, H, W, seed=0).to(dev)
        paths = {"layered": (layered_enc, layered_dec), "embedded": (embedded_enc, embedded_dec)}
        paths.update({f"embedded_{c}_k{K}": cell(c, K) for c, K in cells})
        t = {f"{p}_{ph}": [] for p in paths for ph in ("enc", "enc_coder", "dec", "dec_coder", "enc_emb_dev", "dec_emb_dev")}
        size = {}
        with torch.no_grad():
            for rep in range(a.warmup + a.reps):
                last = {}
                for p, (enc, dec) in paths.items():
                    torch.cuda.synchronize()
                    coder[0] = 0.0
                    t0 = time.perf_counter()
                    cs = enc(x, qs)
                    torch.cuda.synchronize()
                    m1 = drain("emb")
                    t1, c1 = time.perf_counter(), coder[0] + 1e-3 * drain("coder")
                    coder[0] = 0.0
                    last[p] = dec(cs, qs)
                    torch.cuda.synchronize()
                    m2 = drain("emb")
                    t2, c2 = time.perf_counter(), coder[0] + 1e-3 * drain("coder")
                    if rep >= a.warmup:
                        for k, v in (("enc", t1 - t0), ("enc_coder", c1), ("dec", t2 - t1), ("dec_coder", c2),
                                     ("enc_emb_dev", 1e-3 * m1), ("dec_emb_dev", 1e-3 * m2)):
                            t[f"{p}_{k}"].append(1e3 * v)
                    if p == "layered":
                        size[p] = sum(len(s) for c in cs for layer in c["progressive"] for s in layer) / B
                    else:
                        size[p] = sum(len(s) for c in cs for s in c["embedded"]) / B
                for p in paths:
                    for k, (u, v) in enumerate(zip(last["layered"], last[p])):
                        assert torch.equal(u, v), f"{case}: x_hat of level {k} differs between layered and {p}"
        med = {k: round(statistics.median(v), 1) for k, v in t.items()}
        med.update(levels=len(qs), encode_ratio=round(med["embedded_enc"] / med["layered_enc"], 3),
                   decode_ratio=round(med["embedded_dec"] / med["layered_dec"], 3), x_hat_identical=True,
                   layered_progressive_bytes_per_image=round(size["layered"], 1),
                   embedded_bytes_per_image=round(size["embedded"], 1),
                   bytes_ratio=round(size["embedded"] / size["layered"], 4))
        if cells:
            row = lambda p: {"enc_ms": med[f"{p}_enc"], "enc_coder_ms": med[f"{p}_enc_coder"], "enc_embedded_launch_ms": med[f"{p}_enc_emb_dev"],
                             "dec_ms": med[f"{p}_dec"], "dec_coder_ms": med[f"{p}_dec_coder"],
                             "dec_embedded_launch_ms": med[f"{p}_dec_emb_dev"], "bytes_per_image": round(size[p], 1)}
            med["cells"] = {"host_k1": row("embedded"), **{f"{c}_k{K}": row(f"embedded_{c}_k{K}") for c, K in cells}}
        res["cases"][case] = med
        net._drop_plans()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
