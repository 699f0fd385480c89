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

``--allocation tile picture`` adds ``"allocations"``: per allocation the encode time, the stream's size,
the picture header's bytes and, per mark, the smallest and largest fraction of its progressive elements a tile keeps; and for
"picture" the three kernels of csrc/pooled_select.hip alone on the picture's own key buffer (HIP events over 50 launches;
vam_pool_keys for the last group of tiles beside a ``copy_`` of the rows it writes), and ``decode(mark=k)`` of the picture-wide
stream beside ``decode(q=q_k)`` of the per-tile one for the middle mark.  Without the flag the line is what it always was.

``--schedule roi`` adds ``"scheduled"``: the picture coded with a picture-wide schedule of five stages
(``evaluate.picture_roi_schedule``: the box of the 512 x 512 window climbs through 0.5, 2.5, 5 over a background at 0.05, then the
background through 0.5, 2.5) — the encode time beside the unscheduled ``encode_ms`` of the same run, ``decode(stage=k)`` for
every stage beside ``decode(mark=k)`` of the unscheduled stream, vam_tile_schedule alone for all tiles in one launch (HIP events
over 50 launches) beside a ``copy_`` of as many bytes as it reads, the bytes of every stage (``round_end``) and the share of
every stage's round that lies in the tiles the box touches.

``--stream`` adds ``"receiver"``: the stream is fed to a ``tiled.PictureStream`` round by round (the heads,
then every ``round_end``); after each feed ``Canvas.refresh()`` of the whole picture and, on a second receiver, of the 512 x 512
window is timed beside a fresh ``PictureDecoder(prefix).decode(window)`` of the same bytes in the same process (whose code
path is that of the commit before the receiver); every run starts a new receiver, and the median, the smallest and the largest
of the runs are reported with the tiles that ran the network.  With ``--schedule roi`` the scheduled stream is fed, too.  It
also times vam_tile_refresh alone (HIP events over 50 launches, five times: median, min, max) for a box of one dirty tile, of
nine and of all, beside vam_tile_blend of the same box.  ``--pan`` adds ``"pan"``: on the whole stream a 512 x 512 window moves by
one tile stride at a time along the middle row of the picture and then down its middle column; per step ``view`` beside a
fresh ``decode`` of that window, and the tiles ``view`` decoded.

``--pyramid`` adds ``"pyramid"``: ``pyramid.encode`` of the picture (default levels) beside ``encode_ms``, the
``tiled.encode`` of the same run, whose code this section's commit did not touch, and beside the figure DESIGN section 9y
recorded for it; the pyramid's total bytes over level 0's; ``PyramidDecoder.decode(level=k)`` of the WHOLE picture at every level
(level 0 is the full decode); a new ``PyramidStream`` that is fed ``need_bytes`` only, timed from the feed to the first
whole-picture view (the coarsest level), beside a new ``tiled.PictureStream`` fed level 0's ``need_bytes`` and viewed whole;
and vam_picture_halve alone on the picture, both modes (HIP events over 50 launches, five times: median, min, max), beside a
``copy_`` of as many bytes as it READS.

``--pyramid --fill`` adds ``"fill"`` to it: vam_tile_compose alone on a 512 x 768 window in the middle of
the picture, fp32 and uint8, at d = 1 and d = 3 with all tiles, half of them (a checkerboard) and none available, beside
vam_tile_blend of that window and a device ``copy_`` of as many bytes as it writes -- each a few microseconds, so 200 launches
are captured into one graph and its replays are timed by HIP events (five times: median, min, max): events around single
launches would time the host's enqueue; and the first picture at level-0 resolution: a new ``PyramidStream`` fed ``need_bytes`` and viewed with
``fill=True``, beside a new one fed up to the last of level 0's heads and viewed without: bytes and wall time of each.

``--pyramid --zoom`` adds ``"zoom"`` to it: vam_picture_resample alone into a 512 x 768 viewport from level
0's support window at the scales 1, 1.5, 2 and 1/3, fp32 and uint8, beside a device ``copy_`` of as many bytes as it writes and
vam_tile_compose of the same output size, timed as ``--fill`` times its kernels; then ``PyramidDecoder.viewport`` of the whole
picture beside ``decode`` of the level it picks, a level-0 rect at scale 1.5 beside ``decode`` of its support window, and pan
steps of that rect on a warm ``PyramidStream``: wall time and the tiles that ran the network.

``--pyramid --session`` adds ``"session"`` to it: one ``session.Server`` and one ``session.Client`` follow a tour
of 512 x 768 viewports after the session's opening message (``Server.open()``, the headers; ``open_bytes``, in no step and not
in ``sum_bytes``) -- the whole picture, a zoom to a level-0 rect in the middle, eight pan steps of (+64, -96) pixels, all
rounds instead of the first two, and a zoom out to the whole picture.  Per step: the bytes of the server's increment beside
the length of ``pyramid.extract_viewport`` for the same request, the tiles composed and those that ran the network, and the
wall time of merging the message and viewing the viewport (filled, at the mark the rounds hold) beside a fresh
``PyramidDecoder`` on the stateless extract showing the same viewport; every run starts a new server and client.

``--budget N [N ...]`` adds ``"budget"``: ``tiled.encode(allocation="picture", max_bytes=[N ...])`` beside
``encode(allocation="picture", marks=)`` at the qualities it solved, whose code that section's commit did not touch ([median,
min, max] ms each; the two streams must be identical); ``tiled.solve_budgets`` alone inside such an encode with its passes,
launches and read-backs; the ``cut`` buffer's size; and vam_rans_interleaved_cut_table_device alone on the last group of tiles
beside vam_rans_interleaved_encode_device on the same buffers with the solved marks, at 1 and 64 lanes (HIP events over 50
launches, three times each).

No time is asserted.  Prints one JSON line.

    python scripts/bench_tiled.py [--height 2048] [--width 3072] [--tile 256] [--overlap 32] [--warmup 1] [--reps 3]
                                  [--coder host|device] [--lanes 1] [--base-lanes 1] [--allocation tile picture]
                                  [--schedule roi] [--stream] [--pan] [--pyramid [--fill] [--zoom] [--session]]
                                  [--budget BYTES [BYTES ...]] [--q-tol 1e-3]
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


def graph_us(fn, iters=200, replays=5):
    """Microseconds per call of ``fn`` with the host out of the way: ``iters`` calls captured into one graph, which is
    replayed ``replays`` times between two HIP events after one replay of warm-up.  For kernels of a few microseconds, where
    ``event_us`` would measure how fast the host enqueues."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (iters * replays)


def overhead(data, TL):
    lay = TL.layout(data)
    heads = lay["need_bytes"] - lay["header_end"]
    return {"tiles": lay["R"] * lay["C"], "header_bytes": lay["header_end"], "head_bytes": heads, "total_bytes": lay["total"],
            "overhead_pct": round(100.0 * lay["need_bytes"] / lay["total"], 3)}


def kept_spread(data, net, TL, EB):
    """Per mark (min, max) over the tiles of the fraction of a tile's progressive elements its mark keeps."""
    import numpy as np
    lay = TL.layout(data)
    count = np.asarray([EB.layout(data[o:o + n])["marks"]["count"] for row in lay["head"] for o, n in row if n], dtype=np.float64)
    kept = count.sum(-1) / (lay["ns"] * net.dim_chunk * (lay["th"] // 16) * (lay["tw"] // 16))
    return [[round(float(kept[:, k].min()), 4), round(float(kept[:, k].max()), 4)] for k in range(kept.shape[1])]


def allocations(a, net, x, g, kw, TL, EB, ops):
    """The ``--allocation`` section: see the module docstring."""
    from vampic import bitstream as bs, progressive as P
    out, streams = {"marks": [float(q) for q in EB.Q_LIST]}, {}
    for name in a.allocation:
        ms, data = wall_ms(lambda: TL.encode(net, x, allocation=name, **kw), a.warmup, a.reps)
        streams[name] = data
        lay = TL.layout(data)
        out[name] = {"encode_ms": round(ms, 2), "total_bytes": lay["total"], "header_bytes": lay["header_end"],
                     "kept_min_max": kept_spread(data, net, TL, EB)}
    if "picture" not in streams:
        return out
    dev, qs, ns = x.device, [float(q) for q in EB.Q_LIST], net.ns0
    coords = TL.tiles_for(g)
    T, n, group = len(coords), net.dim_chunk * (g["th"] // 16) * (g["tw"] // 16), TL._default_group(g["th"], g["tw"])
    keys = torch.empty((T, ns, n), dtype=torch.int32, device=dev)
    coder, K, Kb = P._check_coder(net, a.coder), bs.check_lanes(a.lanes), bs.check_lanes(a.base_lanes)
    for i0 in range(0, T, group):                                  # the picture's own keys, as tiled.encode's first pass builds them
        part = coords[i0:i0 + group]
        t = torch.empty((len(part), 3, g["th"], g["tw"]), dtype=torch.float32, device=dev)
        ops.tile_extract(x, torch.tensor(part, dtype=torch.int32).to(dev), t, g["V"])
        st = EB._encode_front(net, t, qs, coder, K, Kb)
        ops.pool_keys(st["std_p"], st["perm"], keys, t0=i0, n_slice=ns)
    rows, like = keys[i0:i0 + len(part)], torch.empty_like(keys[i0:i0 + len(part)])
    thr = torch.empty((len(qs), ns), dtype=torch.float32, device=dev)
    count = torch.empty((len(qs), T, ns), dtype=torch.int32, device=dev)
    out["kernels"] = {
        "pool": [T, ns, n], "pool_keys_tiles": len(part),
        "pool_keys_us": round(event_us(lambda: ops.pool_keys(st["std_p"], st["perm"], keys, t0=i0, n_slice=ns)), 2),
        "pool_keys_copy_us": round(event_us(lambda: like.copy_(rows)), 2), "pool_keys_out_bytes": rows.numel() * 4,
        "pooled_select_us": round(event_us(lambda: ops.pooled_select(keys, qs, thr)), 2),
        "threshold_counts_us": round(event_us(lambda: ops.threshold_counts(keys, thr, count)), 2)}
    out["v2_header_extra_bytes"] = TL.layout(streams["picture"])["header_end"] - (
        TL.layout(streams["tile"])["header_end"] if "tile" in streams else
        TL.layout(streams["picture"])["header_end"] - 8 - 4 * len(qs) * ns)
    k = len(qs) // 2
    dp = TL.PictureDecoder(net, streams["picture"], coder=a.coder)
    out["decode_mark"] = {"mark": k, "q": qs[k], "picture_mark_ms": round(wall_ms(lambda: dp.decode(mark=k), a.warmup, a.reps)[0], 2)}
    if "tile" in streams:
        dt = TL.PictureDecoder(net, streams["tile"], coder=a.coder)
        out["decode_mark"]["tile_q_ms"] = round(wall_ms(lambda: dt.decode(q=qs[k]), a.warmup, a.reps)[0], 2)
        out["decode_mark"]["tile_mark_ms"] = round(wall_ms(lambda: dt.decode(mark=k), a.warmup, a.reps)[0], 2)
    return out


def budget(a, net, x, g, kw, TL, EB, ops):
    """The ``--budget`` section: see the module docstring."""
    import ctypes as C
    from vampic import _lib as L, bitstream as bs, control
    dev, ns = x.device, net.ns0
    budgets = [int(v) for v in a.budget]

    def runs(fn):
        times, out = [], None
        for i in range(a.warmup + a.reps):
            ms, out = timed(fn)
            if i >= a.warmup:
                times.append(ms)
        return spread(times), out                                  # [median, min, max]
    enc = lambda: TL.encode(net, x, allocation="picture", max_bytes=budgets, q_tol=a.q_tol, **kw)
    t_budget, data = runs(enc)
    solved = TL.budget_marks(data)
    qs = [q for q, _ in solved]
    t_marks, again = runs(lambda: TL.encode(net, x, allocation="picture", marks=qs, **kw))      # the path this section did not touch
    out = {"budgets": budgets, "q_tol": a.q_tol, "solved": [[q, e] for q, e in solved], "encode_budget_ms": t_budget,
           "encode_marks_ms": t_marks, "identical": again == data}
    # the search alone, and what it launches
    calls, took = {"round_ends": 0, "reads": 0}, []
    inner, solve = TL._round_ends, TL.solve_budgets

    def counted(*args):
        calls["round_ends"] += 1
        return inner(*args)

    def solve_timed(sizes, *args, **kwargs):
        def sizes_counted(rows):
            calls["reads"] += 1
            return sizes(rows)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = solve(sizes_counted, *args, **kwargs)
        torch.cuda.synchronize()
        took.append(1e3 * (time.perf_counter() - t0))
        return r
    TL._round_ends, TL.solve_budgets = counted, solve_timed
    try:
        for _ in range(a.reps):
            enc()
    finally:
        TL._round_ends, TL.solve_budgets = inner, solve
    out["search"] = {"ms": spread(took), "passes": control.rate_search_passes(a.q_tol), "read_backs": calls["reads"] // a.reps,
                     "pooled_select_launches": calls["round_ends"] // a.reps, "threshold_counts_launches": calls["round_ends"] // a.reps,
                     "launches_per_budget": 2 * calls["round_ends"] // a.reps // len(budgets)}
    # the cut-table launch alone beside the encode launch, on the last group of tiles
    coords = TL.tiles_for(g)
    T, n, group = len(coords), net.dim_chunk * (g["th"] // 16) * (g["tw"] // 16), TL._default_group(g["th"], g["tw"])
    out["cut_buffer"] = {"shape": [T, ns, n + 1], "bytes": 4 * T * ns * (n + 1)}
    part = coords[-group:]
    t = torch.empty((len(part), 3, g["th"], g["tw"]), dtype=torch.float32, device=dev)
    ops.tile_extract(x, torch.tensor(part, dtype=torch.int32).to(dev), t, g["V"])
    st = EB._encode_front(net, t, qs, "device", 1, 1)
    r_sym, r_idx = st["r_sym"], st["r_idx"]
    S = len(part) * ns
    tg = bs.DeviceCoderTables.of(net.gaussian_conditional, dev)
    cut, status = torch.empty((S, n + 1), dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    count = st["count"].contiguous()
    lib, stream = L.load(), ops.stream_ptr()
    out["kernels"] = {"streams": S, "n": n}
    for K in (1, 64):
        cap = 2 * n + 2 * K + 16
        regions = torch.empty(S * cap, dtype=torch.int32, device=dev)
        meta = torch.empty((2 + len(qs), S), dtype=torch.int32, device=dev)
        encode = lambda: L.check(lib.vam_rans_interleaved_encode_device(
            r_sym.data_ptr(), r_idx.data_ptr(), S, n, K, C.byref(tg.struct), regions.data_ptr(), cap, meta[0].data_ptr(), meta[1].data_ptr(),
            count.data_ptr(), len(qs), meta[2].data_ptr(), stream), "vam_rans_interleaved_encode_device")
        table = lambda: bs.cut_table_launch(r_sym, r_idx, tg, K, cut, status)
        out["kernels"][f"lanes_{K}"] = {"cut_table_us": [round(event_us(table), 2) for _ in range(3)],
                                        "encode_us": [round(event_us(encode), 2) for _ in range(3)]}
        assert not int(status.abs().sum()) and not int(meta[1].abs().sum())
    return out


ROI_QUALITIES, BACKGROUND_QUALITIES = (0.5, 2.5, 5.0), (0.05, 0.5, 2.5)


def scheduled(a, net, x, g, kw, plain, window, TL, EV, ops):
    """The ``--schedule roi`` section: see the module docstring.  ``plain``: the unscheduled stream of the same run."""
    H, W = g["H"], g["W"]
    y0, x0, h, w = window
    S = EV.picture_roi_schedule(H, W, [(y0, x0, y0 + h, x0 + w)], ROI_QUALITIES, BACKGROUND_QUALITIES, x.device)
    n_st = int(S.shape[0])
    ms, data = wall_ms(lambda: TL.encode(net, x, schedule=S, **kw), a.warmup, a.reps)
    lay = TL.layout(data)
    box_tiles = TL.tiles_for(g, window)
    out = {"box": [y0, x0, y0 + h, x0 + w], "roi_qualities": list(ROI_QUALITIES), "background_qualities": list(BACKGROUND_QUALITIES),
           "stages": n_st, "encode_ms": round(ms, 2), "total_bytes": lay["total"], "header_bytes": lay["header_end"],
           "head_bytes": lay["need_bytes"] - lay["header_end"], "box_tiles": len(box_tiles), "round_end": lay["round_end"][:n_st]}
    share = []
    for k in range(n_st):
        size = lay["piece"][k]
        total = sum(n for row in size for _, n in row)
        share.append({"round_bytes": total, "box_tiles_pct": round(100.0 * sum(size[r][c][1] for r, c in box_tiles) / max(total, 1), 2)})
    out["rounds"] = share
    dec = TL.PictureDecoder(net, data, coder=a.coder)
    out["decode_stage_ms"] = [round(wall_ms(lambda: dec.decode(stage=k), a.warmup, a.reps)[0], 2) for k in range(n_st)]
    dp = TL.PictureDecoder(net, plain, coder=a.coder)
    marks = TL.layout(plain)["marks"]
    out["decode_plain_mark_ms"] = {str(k): round(wall_ms(lambda: dp.decode(mark=k), a.warmup, a.reps)[0], 2)
                                   for k in sorted({min(2, len(marks) - 1), len(marks) // 2})}
    out["plain_marks"] = marks
    coords = TL.tiles_for(g)
    cd = torch.tensor(coords, dtype=torch.int32).to(x.device)
    st = torch.empty((len(coords), n_st, g["th"] // 16, g["tw"] // 16), dtype=torch.float32, device=x.device)
    src = torch.empty((len(coords) * n_st * g["th"] * g["tw"],), dtype=torch.float32, device=x.device)
    dst = torch.empty_like(src)
    out["tile_schedule_us"] = round(event_us(lambda: ops.tile_schedule(S, cd, st, g["th"], g["tw"], g["V"])), 2)
    out["tile_schedule_copy_us"] = round(event_us(lambda: dst.copy_(src)), 2)
    out["tile_schedule_in_bytes"], out["tile_schedule_out_bytes"] = src.numel() * 4, st.numel() * 4
    out["schedule_bytes"] = S.numel() * 4
    return out


def spread(times):
    return [round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def receiver(a, net, g, data, window, TL):
    """One stream of the ``--stream`` section: [median, min, max] ms over ``reps`` runs per feed, each run on new receivers."""
    lay = TL.layout(data)
    cuts = sorted({lay["need_bytes"], *lay["round_end"]})
    n_tiles = g["R"] * g["C"]
    keys = ("refresh_full_ms", "fresh_full_ms", "refresh_window_ms", "fresh_window_ms")
    times = [{k: [] for k in keys} for _ in cuts]
    decoded = [None] * len(cuts)
    for run in range(a.warmup + a.reps):
        full, part = (TL.PictureStream(net, coder=a.coder, cache_tiles=n_tiles) for _ in range(2))
        at, canvases = 0, None
        for i, n in enumerate(cuts):
            for st in (full, part):
                st.feed(data[at:n])
            at = n
            if canvases is None:
                canvases = (full.canvas(), part.canvas(window))
            fresh = TL.PictureDecoder(net, data[:n], coder=a.coder)
            row = {"refresh_full_ms": timed(canvases[0].refresh)[0], "fresh_full_ms": timed(fresh.decode)[0],
                   "refresh_window_ms": timed(canvases[1].refresh)[0], "fresh_window_ms": timed(lambda: fresh.decode(window))[0]}
            decoded[i] = [len(full.last_decoded), len(part.last_decoded)]
            if run == a.warmup + a.reps - 1:                       # what was timed is what a fresh decode gives
                assert torch.equal(canvases[0].out, fresh.decode()) and torch.equal(canvases[1].out, fresh.decode(window))
            if run >= a.warmup:
                for k in keys:
                    times[i][k].append(row[k])
    return {"tiles": [n_tiles, len(TL.tiles_for(g, window))], "runs": a.reps,
            "feeds": [dict({"bytes": n, "decoded_full": decoded[i][0], "decoded_window": decoded[i][1]},
                           **{k: spread(times[i][k]) for k in keys}) for i, n in enumerate(cuts)]}


def refresh_kernel(g, dev, TL, ops):
    """vam_tile_refresh alone beside vam_tile_blend of the same box: one dirty tile, nine, all; fp32 and uint8."""
    H, W, R, C = g["H"], g["W"], g["R"], g["C"]
    n = R * C
    tiles = torch.rand((n, 3, g["th"], g["tw"]), dtype=torch.float32, device=dev)
    slot = torch.arange(n, dtype=torch.int32, device=dev).view(R, C)
    w_lo, w_hi = (torch.from_numpy(t).to(dev) if g["V"] else None for t in TL.ramps(g["V"]))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    r0, c0 = R // 2, C // 2
    cases = {"one_tile": (r0, r0 + 1, c0, c0 + 1), "nine_tiles": (max(r0 - 1, 0), min(r0 + 2, R), max(c0 - 1, 0), min(c0 + 2, C)),
             "all_tiles": (0, R, 0, C)}
    out = {}
    for name, (ra, rb, ca, cb) in cases.items():
        dirty = torch.zeros((R, C), dtype=torch.int32)
        dirty[ra:rb, ca:cb] = 1
        dirty = dirty.to(dev)
        y0, y1 = ra * g["Sy"], min(H, (rb - 1) * g["Sy"] + g["th"])
        x0, x1 = ca * g["Sx"], min(W, (cb - 1) * g["Sx"] + g["tw"])
        box = (y0, x0, y1 - y0, x1 - x0)
        row = {"box": list(box), "dirty_tiles": (rb - ra) * (cb - ca)}
        for kind, canvas, crop in (("f32", torch.zeros((3, H, W), dtype=torch.float32, device=dev), torch.empty((3, box[2], box[3]), dtype=torch.float32, device=dev)),
                                   ("u8", torch.zeros((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((box[2], box[3], 3), dtype=torch.uint8, device=dev))):
            row[f"refresh_{kind}_us"] = spread([event_us(lambda: ops.tile_refresh(tiles, slot, dirty, w_lo, w_hi, H, W, g["V"], (0, 0, H, W), box,
                                                                                   canvas, status)) for _ in range(5)])
            row[f"blend_{kind}_us"] = spread([event_us(lambda: ops.tile_blend(tiles, slot, w_lo, w_hi, H, W, g["V"], box, crop, status))
                                              for _ in range(5)])
        out[name] = row
    assert int(status.item()) == 0
    return out


def pan(a, net, g, data, TL):
    """The ``--pan`` section: see the module docstring."""
    H, W = g["H"], g["W"]
    h, w = min(512, H), min(512, W)
    ym, xm = (H - h) // 2, (W - w) // 2
    path = [(ym, x0, h, w) for x0 in range(0, W - w + 1, g["Sx"])] + [(y0, xm, h, w) for y0 in range(0, H - h + 1, g["Sy"])]
    fresh = TL.PictureDecoder(net, data, coder=a.coder)
    times = [{"view_ms": [], "fresh_ms": []} for _ in path]
    decoded = [0] * len(path)
    for run in range(a.warmup + a.reps):
        st = TL.PictureStream(net, coder=a.coder)
        st.feed(data)
        for i, win in enumerate(path):
            tv, got = timed(lambda: st.view(win))
            decoded[i] = len(st.last_decoded)
            tf, want = timed(lambda: fresh.decode(win))
            assert torch.equal(got, want)
            if run >= a.warmup:
                times[i]["view_ms"].append(tv)
                times[i]["fresh_ms"].append(tf)
    steps = [{"window": list(win), "tiles": len(TL.tiles_for(g, win)), "decoded": decoded[i], "view_ms": spread(times[i]["view_ms"]),
              "fresh_ms": spread(times[i]["fresh_ms"])} for i, win in enumerate(path)]
    return {"runs": a.reps, "cache_tiles": st.cache_tiles, "steps": steps,
            "sum_view_ms": round(sum(s_["view_ms"][0] for s_ in steps), 2), "sum_fresh_ms": round(sum(s_["fresh_ms"][0] for s_ in steps), 2)}


PARENT_TILED_ENCODE_MS = 266.5             # DESIGN section 9y's recorded tiled.encode of this picture, the commit before 9z


def pyramid(a, net, x, g, kw, TL, PY, ops):
    """The ``--pyramid`` section: see the module docstring."""
    H, W = g["H"], g["W"]
    ms, data = wall_ms(lambda: PY.encode(net, x, **kw), a.warmup, a.reps)
    lay = PY.layout(data)
    n = lay["n_levels"]
    out = {"levels": n, "encode_ms": round(ms, 2), "parent_recorded_tiled_encode_ms": PARENT_TILED_ENCODE_MS, "runs": a.reps,
           "header_bytes": lay["header_end"], "need_bytes": lay["need_bytes"], "total_bytes": lay["total"],
           "level0_bytes": lay["levels"][0]["length"], "total_over_level0": round(lay["total"] / lay["levels"][0]["length"], 4),
           "viewport_512x768_level": PY.best_level(None, (512, 768), H, W, n)}
    dec = PY.PyramidDecoder(net, data, coder=a.coder)
    rows = []
    for lv in lay["levels"]:
        k = lv["level"]
        times, got = [], None
        for i in range(a.warmup + a.reps):
            t, got = timed(lambda: dec.decode(level=k))
            if i >= a.warmup:
                times.append(t)
        assert tuple(got.shape[1:]) == tuple(lv["shape"])
        if k:                                                      # what was timed is the level's own picture decode
            assert torch.equal(got, TL.PictureDecoder(net, PY.level_stream(data, k), coder=a.coder).decode())
        rows.append({"level": k, "shape": list(lv["shape"]), "tiles": lv["layout"]["R"] * lv["layout"]["C"], "bytes": lv["length"],
                     "need_bytes": lv["layout"]["need_bytes"], "decode_whole_ms": spread(times)})
    out["per_level"] = rows
    first, plain = [], []
    level0 = PY.level_stream(data, 0)
    need0 = TL.need_bytes(level0)
    for i in range(a.warmup + a.reps):
        def thumbnail():
            st = PY.PyramidStream(net, coder=a.coder)
            st.feed(data[:lay["need_bytes"]])
            return st.view(level=n - 1)

        def heads():
            st = TL.PictureStream(net, coder=a.coder, cache_tiles=g["R"] * g["C"])
            st.feed(level0[:need0])
            return st.view()
        t, _ = timed(thumbnail)
        u, _ = timed(heads)
        if i >= a.warmup:
            first.append(t)
            plain.append(u)
    out["first_view"] = {"pyramid_bytes": lay["need_bytes"], "pyramid_ms": spread(first), "level0_need_bytes": need0, "level0_ms": spread(plain)}
    dst, like = torch.empty((3, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=x.device), torch.empty_like(x)
    out["halve_kernel"] = {"in_bytes": x.numel() * 4, "out_bytes": dst.numel() * 4,
                           "mean_us": spread([event_us(lambda: ops.picture_halve(x, "mean", out=dst)) for _ in range(5)]),
                           "max_us": spread([event_us(lambda: ops.picture_halve(x, "max", out=dst)) for _ in range(5)]),
                           "copy_in_bytes_us": spread([event_us(lambda: like.copy_(x)) for _ in range(5)])}
    if a.fill:
        out["fill"] = fill(a, net, data, lay, g, TL, PY, ops)
    if a.zoom:
        out["zoom"] = zoom(a, net, data, lay, g, TL, PY, ops)
    if a.session:
        from vampic import session as SS
        out["session"] = session(a, net, data, lay, g, PY, SS)
    return out


def fill(a, net, data, lay, g, TL, PY, ops):
    """The ``--fill`` section: see the module docstring."""
    H, W, R, C, dev = g["H"], g["W"], g["R"], g["C"], next(net.parameters()).device
    h, w = min(512, H), min(768, W)
    win = ((H - h) // 2, (W - w) // 2, h, w)
    tiles = torch.rand((R * C, 3, g["th"], g["tw"]), dtype=torch.float32, device=dev)
    every = torch.arange(R * C, dtype=torch.int32).view(R, C)
    half = torch.where((torch.arange(R)[:, None] + torch.arange(C)[None, :]) % 2 == 0, every, torch.full_like(every, -1)).to(dev)
    every = every.to(dev)
    w_lo, w_hi = (torch.from_numpy(t).to(dev) if g["V"] else None for t in TL.ramps(g["V"]))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    kernel = {"window": list(win), "window_tiles": len(TL.tiles_for(g, win)), "timing": "200 launches in one graph, 5 replays, 5 times"}
    for kind, dst in (("f32", torch.empty((3, h, w), dtype=torch.float32, device=dev)), ("u8", torch.empty((h, w, 3), dtype=torch.uint8, device=dev))):
        src = torch.empty_like(dst)
        kernel[f"out_{kind}_bytes"] = dst.numel() * dst.element_size()
        kernel[f"copy_{kind}_us"] = spread([graph_us(lambda: dst.copy_(src)) for _ in range(5)])
        kernel[f"blend_{kind}_us"] = spread([graph_us(lambda: ops.tile_blend(tiles, every, w_lo, w_hi, H, W, g["V"], win, dst, status))
                                             for _ in range(5)])
        for d in (1, 3):
            Hj, Wj = -(-H // (1 << d)), -(-W // (1 << d))
            bwin = PY.source_window(win, d, Hj, Wj)
            below = torch.rand((3,) + bwin[2:], dtype=torch.float32, device=dev)
            for name, slot in (("all", every), ("half", half), ("none", None)):
                kernel[f"compose_{kind}_d{d}_{name}_us"] = spread([graph_us(lambda: ops.tile_compose(
                    None if slot is None else tiles, slot, w_lo, w_hi, H, W, g["V"], win, below, bwin, d, dst, status)) for _ in range(5)])
    assert int(status.item()) == 0
    heads0 = lay["levels"][0]["offset"] + lay["levels"][0]["layout"]["need_bytes"]
    filled, plain, chain = [], [], None
    for i in range(a.warmup + a.reps):
        def first_filled():
            st = PY.PyramidStream(net, coder=a.coder)
            st.feed(data[:lay["need_bytes"]])
            return st, st.view(level=0, fill=True)

        def first_plain():
            st = PY.PyramidStream(net, coder=a.coder, cache_tiles=R * C)
            st.feed(data[:heads0])
            return st.view(level=0)
        t, (st, got) = timed(first_filled)
        chain = [(k, len(s_), len(n_)) for k, s_, n_ in st.last_chain]
        assert tuple(got.shape) == (3, H, W)
        u, _ = timed(first_plain)
        if i >= a.warmup:
            filled.append(t)
            plain.append(u)
    return {"kernel": kernel, "first_level0_picture": {"fill_bytes": lay["need_bytes"], "fill_ms": spread(filled), "fill_chain": chain,
                                                        "plain_bytes": heads0, "plain_ms": spread(plain)}}


def zoom(a, net, data, lay, g, TL, PY, ops):
    """The ``--zoom`` section: see the module docstring."""
    H, W, R, C, dev = g["H"], g["W"], g["R"], g["C"], next(net.parameters()).device
    oh, ow = min(512, H), min(768, W)
    picture = torch.rand((3, H, W), dtype=torch.float32, device=dev)
    kernel = {"out_hw": [oh, ow], "timing": "200 launches in one graph, 5 replays, 5 times"}
    views = {}
    for name, num, den in (("1", 1, 1), ("1.5", 3, 2), ("2", 2, 1), ("1/3", 1, 3)):
        unit = den                                                              # the rect in 1 / den pixels: h = oh num exactly
        h, w = oh * num, ow * num
        rect = ((H * unit - h) // 2 | 1, (W * unit - w) // 2 | 1, h, w)
        win = PY.viewport_window(rect, (oh, ow), 0, H, W, unit)
        views[name] = (rect, unit, win, picture[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]].contiguous())
        kernel[f"scale_{name}"] = {"rect": list(rect), "unit": unit, "support_window": list(win),
                                   "taps": [max(len(u) for _, u in PY.viewport_taps(rect, (oh, ow), 0, H, W, unit, ax)) for ax in (0, 1)]}
    tiles = torch.rand((R * C, 3, g["th"], g["tw"]), dtype=torch.float32, device=dev)
    every = torch.arange(R * C, dtype=torch.int32, device=dev).view(R, C)
    w_lo, w_hi = (torch.from_numpy(t).to(dev) if g["V"] else None for t in TL.ramps(g["V"]))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    cwin = ((H - oh) // 2, (W - ow) // 2, oh, ow)
    bwin = PY.source_window(cwin, 1, -(-H // 2), -(-W // 2))
    below = torch.rand((3,) + bwin[2:], dtype=torch.float32, device=dev)
    for kind, dst in (("f32", torch.empty((3, oh, ow), dtype=torch.float32, device=dev)), ("u8", torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev))):
        like = torch.empty_like(dst)
        kernel[f"out_{kind}_bytes"] = dst.numel() * dst.element_size()
        kernel[f"copy_{kind}_us"] = spread([graph_us(lambda: dst.copy_(like)) for _ in range(5)])
        kernel[f"compose_{kind}_us"] = spread([graph_us(lambda: ops.tile_compose(tiles, every, w_lo, w_hi, H, W, g["V"], cwin, below, bwin, 1, dst, status))
                                               for _ in range(5)])
        for name, (rect, unit, win, src) in views.items():
            kernel[f"scale_{name}"][f"resample_{kind}_us"] = spread([graph_us(lambda: ops.picture_resample(src, win, (H, W), 0, rect, unit, (oh, ow), out=dst))
                                                                      for _ in range(5)])
    assert int(status.item()) == 0
    dec = PY.PyramidDecoder(net, data, coder=a.coder)

    def beside(rect, level):
        """Wall times of ``dec.viewport`` and of ``dec.decode`` of its support window alone, in turn."""
        k = PY.viewport_level(rect, (oh, ow), H, W, lay["n_levels"]) if level is None else level
        win = PY.viewport_window(rect, (oh, ow), k, H, W)
        tv, td = [], []
        for i in range(a.warmup + a.reps):
            t, got = timed(lambda: dec.viewport(rect, (oh, ow), level=level))
            u, _ = timed(lambda: dec.decode(win, level=k))
            assert tuple(got.shape) == (3, oh, ow)
            if i >= a.warmup:
                tv.append(t)
                td.append(u)
        return {"rect": None if rect is None else list(rect), "level": k, "support_window": list(win), "tiles": len(dec.last_tiles),
                "viewport_ms": spread(tv), "decode_ms": spread(td)}

    rect = ((H - oh * 3 // 2) // 2 | 1, (W - ow * 3 // 2) // 2 | 1, oh * 3 // 2, ow * 3 // 2)
    end = {"whole_picture": beside(None, None), "level0_scale_1.5": beside(rect, None)}
    st = PY.PyramidStream(net, coder=a.coder, cache_tiles=R * C)
    st.feed(data)
    st.viewport(rect, (oh, ow))                                                 # warm: the rect's tiles are cached
    steps, ran = [], 0
    for i in range(a.warmup + 8):
        pan = (rect[0] + 4 * (i + 1), rect[1] - 6 * (i + 1)) + rect[2:]
        t, got = timed(lambda: st.viewport(pan, (oh, ow)))
        ran += len(st.last_decoded)
        if i >= a.warmup:
            steps.append(t)
    assert torch.equal(got, dec.viewport(pan, (oh, ow)))
    end["pan_step_warm_stream"] = {"steps": len(steps), "tiles_composed": len(st.last_tiles), "tiles_that_ran_the_network": ran, "ms": spread(steps)}
    return {"kernel": kernel, "end_to_end": end}


def session(a, net, data, lay, g, PY, SS):
    """The ``--session`` section: see the module docstring."""
    H, W = g["H"], g["W"]
    oh, ow = min(512, H), min(768, W)
    n_marks = len(lay["levels"][0]["layout"]["marks"])
    low = min(2, n_marks)
    y0, x0 = (H - oh) // 2, (W - ow) // 2
    pans = [(min(y0 + 64 * (i + 1), H - oh), max(x0 - 96 * (i + 1), 0), oh, ow) for i in range(8)]
    tour = [("whole picture", None, low), ("zoom to level 0", (y0, x0, oh, ow), low)] + [(f"pan {i + 1}", rect, low) for i, rect in enumerate(pans)] \
        + [("all rounds", pans[-1], None), ("zoom out", None, None)]
    times = [{"session_ms": [], "stateless_ms": []} for _ in tour]
    rows = [None] * len(tour)
    for run in range(a.warmup + a.reps):
        server, client = SS.Server(data), SS.Client(net, coder=a.coder, cache_tiles=g["R"] * g["C"])
        opening = server.open()                                    # the headers, once, before the first request
        client.merge(opening)
        for i, (name, rect, rounds) in enumerate(tour):
            m = n_marks - 1 if rounds is None else rounds - 1
            message = server.viewport(rect, (oh, ow), 1, rounds)

            def step():
                client.merge(message)
                return client.viewport(rect, (oh, ow), mark=m, fill=True)
            ts, got = timed(step)
            rows[i] = {"step": name, "rect": None if rect is None else list(rect), "rounds": rounds, "level": client.last_chain[0][0],
                       "tiles": len(client.last_tiles), "decoded": sum(len(e[2]) for e in client.last_chain)}
            stateless = PY.extract_viewport(data, rect, (oh, ow), 1, rounds)
            tf, want = timed(lambda: PY.PyramidDecoder(net, stateless, coder=a.coder).viewport(rect, (oh, ow), mark=m, fill=True))
            rows[i].update({"bytes": len(message), "bytes_stateless": len(stateless)})
            if run == a.warmup + a.reps - 1:                       # what was timed is what the stateless extract shows
                assert torch.equal(got, want), name
            if run >= a.warmup:
                times[i]["session_ms"].append(ts)
                times[i]["stateless_ms"].append(tf)
    for row, t in zip(rows, times):
        row.update({k: spread(v) for k, v in t.items()})
    return {"runs": a.reps, "out_hw": [oh, ow], "open_bytes": len(opening), "steps": rows, "sum_bytes": sum(r["bytes"] for r in rows),
            "sum_bytes_stateless": sum(r["bytes_stateless"] for r in rows), "sum_decoded": sum(r["decoded"] for r in rows),
            "sum_session_ms": round(sum(r["session_ms"][0] for r in rows), 2), "sum_stateless_ms": round(sum(r["stateless_ms"][0] for r in rows), 2)}


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
    ap.add_argument("--allocation", nargs="+", default=None, choices=["tile", "picture"])
    ap.add_argument("--schedule", default=None, choices=["roi"])
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--pan", action="store_true")
    ap.add_argument("--pyramid", action="store_true")
    ap.add_argument("--fill", action="store_true")
    ap.add_argument("--zoom", action="store_true")
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--budget", type=int, nargs="+", default=None, metavar="BYTES")
    ap.add_argument("--q-tol", type=float, default=1e-3)
    a = ap.parse_args()
    if (a.fill or a.zoom or a.session) and not a.pyramid:
        ap.error("--fill, --zoom and --session are parts of --pyramid")
    from bench import build_model
    import vampic
    from vampic import embedded as EB, evaluate as EV, ops, pyramid as PY, tiled as TL
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
        if a.allocation:
            res["allocations"] = allocations(a, net, x, g, kw, TL, EB, ops)
        if a.budget:
            res["budget"] = budget(a, net, x, g, kw, TL, EB, ops)
        if a.schedule:
            res["scheduled"] = scheduled(a, net, x, g, kw, data, window, TL, EV, ops)
        if a.stream:
            res["receiver"] = {"plain": receiver(a, net, g, data, window, TL), "refresh_kernel": refresh_kernel(g, dev, TL, ops)}
            if a.schedule:
                y0, x0, h, w = window
                S = EV.picture_roi_schedule(H, W, [(y0, x0, y0 + h, x0 + w)], ROI_QUALITIES, BACKGROUND_QUALITIES, dev)
                res["receiver"]["roi"] = receiver(a, net, g, TL.encode(net, x, schedule=S, **kw), window, TL)
        if a.pan:
            res["pan"] = pan(a, net, g, data, TL)
        if a.pyramid:
            res["pyramid"] = pyramid(a, net, x, g, kw, TL, PY, ops)
    for k in ("encode_ms", "decode_full_ms", "decode_window_ms"):
        res[k] = round(res[k], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
