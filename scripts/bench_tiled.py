#!/usr/bin/env python3
"""Tiled picture codestreams (tiled.encode / PictureDecoder) on one GPU: one synthetic picture, by default
2048 x 3072 at the default tile 256 and overlap 32, hipGraph on.  After a warm-up every phase is timed from a device
synchronisation to the next and the median of the repetitions is reported:

* encode, the full decode, and the decode of a 512 x 512 window in the middle of the picture (wall time, ms);
* vam_tile_extract (all tiles, one launch) and vam_tile_blend (the whole picture, fp32 and uint8) alone, by HIP events over
  a run of launches, each beside a device-to-device ``copy_`` of as many output bytes: a copy is the floor for a kernel that
  only moves data;
* the stream's overhead: the picture header and the per-tile heads (each tile's own preamble, header, z and base) in bytes
  and in percent of the total; and, for the picture's top-left 1024 x 2048, the largest single image the rank order takes,
  the same numbers beside ``embedded.encode_batch`` of that crop as ONE image (its header, z and base against its total).

No time is asserted.  Prints one JSON line.

    python scripts/bench_tiled.py [--height 2048] [--width 3072] [--tile 256] [--overlap 32] [--warmup 1] [--reps 3]
                                  [--coder host|device] [--lanes 1] [--base-lanes 1]
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


def wall_ms(fn, warmup, reps):
    out = None
    times = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), out


def event_us(fn, iters=50):
    """Microseconds per call of ``fn`` on the current stream: HIP events around ``iters`` calls, after three of warm-up."""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def overhead(data, TL):
    lay = TL.layout(data)
    heads = lay["need_bytes"] - lay["header_end"]
    return {"tiles": lay["R"] * lay["C"], "header_bytes": lay["header_end"], "head_bytes": heads, "total_bytes": lay["total"],
            "overhead_pct": round(100.0 * lay["need_bytes"] / lay["total"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=3072)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--coder", default="host", choices=["host", "device"])
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--base-lanes", type=int, default=1)
    a = ap.parse_args()
    from bench import build_model
    import vampic
    from vampic import embedded as EB, evaluate as EV, ops, tiled as TL
    dev = torch.device("cuda:0")
    net, _ = build_model(dev)
    net.update()
    H, W = a.height, a.width
    g = TL.grid(H, W, a.tile, a.overlap)
    x = vampic.synth.synth_image(1, H, W, seed=1)[0].to(dev)
    kw = dict(tile=a.tile, overlap=a.overlap, coder=a.coder, lanes=a.lanes, base_lanes=a.base_lanes)
    res = {"metric": "tiled picture codestream (ms, median)", "device": torch.cuda.get_device_name(0), "picture": [H, W],
           "tile": [g["th"], g["tw"]], "overlap": g["V"], "grid": [g["R"], g["C"]], "group": TL._default_group(g["th"], g["tw"]),
           "coder": a.coder, "lanes": a.lanes, "base_lanes": a.base_lanes, "warmup": a.warmup, "reps": a.reps}
    with torch.no_grad():
        res["encode_ms"], data = wall_ms(lambda: TL.encode(net, x, **kw), a.warmup, a.reps)
        dec = TL.PictureDecoder(net, data, coder=a.coder)
        res["decode_full_ms"], full = wall_ms(dec.decode, a.warmup, a.reps)
        wh, ww = min(512, H), min(512, W)
        window = ((H - wh) // 2, (W - ww) // 2, wh, ww)
        res["decode_window_ms"], crop = wall_ms(lambda: dec.decode(window), a.warmup, a.reps)
        res["window"], res["window_tiles"] = list(window), len(dec.last_tiles)
        assert torch.equal(crop, full[:, window[0]:window[0] + wh, window[1]:window[1] + ww])
        res["psnr_full"] = round(EV.compute_psnr(x[None], full[None]), 3)
        res["bpp_full"] = round(8.0 * len(data) / (H * W), 4)
        # the kernels alone, beside a copy of as many output bytes
        coords = TL.tiles_for(g)
        n = len(coords)
        cd = torch.tensor(coords, dtype=torch.int32).to(dev)
        tiles = torch.empty((n, 3, g["th"], g["tw"]), dtype=torch.float32, device=dev)
        like = torch.empty_like(tiles)
        res["extract_us"] = round(event_us(lambda: ops.tile_extract(x, cd, tiles, g["V"])), 2)
        res["extract_copy_us"] = round(event_us(lambda: like.copy_(tiles)), 2)
        res["extract_out_bytes"] = tiles.numel() * 4
        slot = torch.arange(n, dtype=torch.int32, device=dev).view(g["R"], g["C"])
        w_lo, w_hi = (torch.from_numpy(t).to(dev) if g["V"] else None for t in TL.ramps(g["V"]))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for name, out in (("f32", torch.empty((3, H, W), dtype=torch.float32, device=dev)),
                          ("u8", torch.empty((H, W, 3), dtype=torch.uint8, device=dev))):
            src = torch.empty_like(out)
            res[f"blend_{name}_us"] = round(event_us(lambda: ops.tile_blend(tiles, slot, w_lo, w_hi, H, W, g["V"], (0, 0, H, W), out, status)), 2)
            res[f"blend_{name}_copy_us"] = round(event_us(lambda: out.copy_(src)), 2)
            res[f"blend_{name}_out_bytes"] = out.numel() * out.element_size()
        assert int(status.item()) == 0
        # the stream's overhead
        res["stream"] = overhead(data, TL)
        ch, cw = min(1024, H), min(2048, W)
        crop_x = x[:, :ch, :cw].contiguous()
        res["crop"] = {"picture": [ch, cw], "tiled": overhead(TL.encode(net, crop_x, **kw), TL)}
        if ch % 64 == 0 and cw % 64 == 0:
            one = EB.layout(EB.to_bytes(EB.encode_batch(net, crop_x[None], coder=a.coder, lanes=a.lanes, base_lanes=a.base_lanes)[0]))
            res["crop"]["one_image"] = {"head_bytes": one["base_end"], "total_bytes": one["total"],
                                        "overhead_pct": round(100.0 * one["base_end"] / one["total"], 3)}
    for k in ("encode_ms", "decode_full_ms", "decode_window_ms"):
        res[k] = round(res[k], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
