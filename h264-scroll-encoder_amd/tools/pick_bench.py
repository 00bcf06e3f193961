#!/usr/bin/env python3
"""What picking the rect's per-frame QP on the device buys (scroll_batch_dyn_pick).

BASELINE config 3 (bench.py's p720dyn batch: 256 streams x 16 frames of
1280x720, rect 28,10,25,25, synthetic source), 8 candidate QPs, wall-clock ms
per step from the first call to the end of scroll_batch_sync, interleaved
rounds in one process; one JSON line, also written to
profiles/pick_bench_p720dyn.json:

  device_ms   scroll_batch_dyn_probe -> scroll_batch_dyn_pick (FRAME mode) ->
              scroll_batch_compose: a QP per frame, nothing crosses to the host;
  host_ms     scroll_batch_dyn_probe -> S x F x 8 scroll_batch_dyn_probe_result
              -> h264scroll.pick_qp -> scroll_batch_set_dyn_qp_stream per stream
              (frame 0's choice for all its frames) -> scroll_batch_compose:
              the closest a caller gets without the per-frame table;
  compose_ms  the compose alone, for scale; pick_only_ms the pick's launch to
              its completion on an idle stream.
(median / min / max over the rounds)

Usage: python h264-scroll-encoder_amd/tools/pick_bench.py [--rounds 5]
       [--streams 256] [--frames 16] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
sys.path.insert(0, HERE)

QPS = [14, 18, 22, 26, 30, 34, 38, 42]


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pick_bench_p720dyn.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    import h264scroll as hs

    wl = dict(bench.WORKLOADS["p720dyn"])
    if args.streams:
        wl["streams"] = args.streams
    if args.frames:
        wl["frames"] = args.frames
    S, F = wl["streams"], wl["frames"]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    hq = stream.cuda_stream
    b = bench.build_compose_batch(hs, wl, 0, 0)

    def finish():
        if b.sync() != 0:
            raise RuntimeError(hs.last_error())

    def probe_async():
        rc = hs.lib.scroll_batch_dyn_probe(b.h, F, hs.u8buf(bytes(QPS)), len(QPS), hq)
        if rc != 0:
            raise RuntimeError(hs.last_error())

    # the budget: the median candidate's cost of the first frame
    res = b.dyn_probe(F, QPS, stream=hq)
    budget = int(np.median(res["bits"][0, 0]))
    rate = hs.ScrollDynRate(hs.SCROLL_DYN_RATE_FRAME, budget, 0, 0)

    def device_step():
        t = time.perf_counter()
        probe_async()
        rc = hs.lib.scroll_batch_dyn_pick(b.h, F, rate, None, hq)
        if rc != 0:
            raise RuntimeError(hs.last_error())
        b.compose(F, stream=hq, rewind=True)
        finish()
        return (time.perf_counter() - t) * 1e3

    def host_step():
        b.clear_dyn_qp_frames()
        t = time.perf_counter()
        r = b.dyn_probe(F, QPS, stream=hq)
        qp = hs.pick_qp(r, QPS, budget)
        for s in range(S):
            b.set_dyn_qp(int(qp[s, 0]) if qp[s, 0] >= 0 else QPS[-1], stream=s)
        b.compose(F, stream=hq, rewind=True)
        finish()
        return (time.perf_counter() - t) * 1e3

    def compose_step():
        t = time.perf_counter()
        b.compose(F, stream=hq, rewind=True)
        finish()
        return (time.perf_counter() - t) * 1e3

    def pick_only():
        probe_async()
        stream.synchronize()
        t = time.perf_counter()
        hs.lib.scroll_batch_dyn_pick(b.h, F, rate, None, hq)
        stream.synchronize()
        return (time.perf_counter() - t) * 1e3

    device_step()                               # warm-up: the record pool is sized here, once
    host_step()
    dev, host, comp, pick = [], [], [], []
    for _ in range(args.rounds):
        dev.append(device_step())
        comp.append(compose_step())
        pick.append(pick_only())
        host.append(host_step())
    k, qp, st = b.dyn_pick(F, budget, stream=hq)
    out = {
        "tool": "pick_bench",
        "config": {"workload": "BASELINE config 3", "resolution": f"{wl['w']}x{wl['h']}", "streams": S,
                   "frames_per_step": F, "rect": list(wl["rect"]), "candidates": QPS, "frame_bits": budget},
        "timing": f"{args.rounds} interleaved rounds, wall clock from the first call to the end of scroll_batch_sync",
        "device_ms": spread(dev),
        "host_ms": spread(host),
        "compose_ms": spread(comp),
        "pick_only_ms": spread(pick),
        "host_over_device": round(statistics.median(host) / statistics.median(dev), 2),
        "chosen_qp_histogram": {str(q): int((qp == q).sum()) for q in QPS},
        "over_budget_frames": int((st == 1).sum()),
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
