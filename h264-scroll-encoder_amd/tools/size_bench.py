#!/usr/bin/env python3
"""What sizing the plain rect per stream and per frame saves
(scroll_batch_set_dyn_rect_size_at).

BASELINE config 3's shape (bench.py's p720dyn batch: 256 streams x 16 frames
of 1280x720, the synthetic source generated on the device for each frame's
own rect), five batches in one process, HIP events on one stream around each
compose, 3 warm-up steps per arm, then interleaved rounds; one JSON line, also
written to profiles/size_bench_p720dyn.json:

  a  the 25x25-MB batch rect, scroll_batch_set_dyn_rect_moving on, a random
     legal origin per (stream, frame), no size set: the parent's moving rect;
  b  the same with every frame sized 5x5 inside the 25x25 batch rect;
  c  a 5x5 BATCH rect at the same origins: what (b) would cost if the launch
     were sized for it;
  d  the batch rect 80x45 (the whole picture, origin (0, 0)) with every frame
     sized 5x5;
  e  the batch rect 80x45, no size set.
(median / min / max of the per-step times over all rounds)

(b) and (c) are checked to have written the same bytes.  --arms picks a
subset; --pkg imports h264scroll from another tree, so arm (a) can be timed
on a build that lacks the call (the parent commit) with this very tool.

Usage: python h264-scroll-encoder_amd/tools/size_bench.py [--rounds 5]
       [--steps 4] [--arms abcde] [--streams 256] [--frames 16] [--pkg DIR] [--out PATH]
"""
import argparse
import json
import os
import random
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--arms", default="abcde")
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--pkg", default=PKG, help="the tree h264scroll is imported from")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "size_bench_p720dyn.json"))
    args = ap.parse_args()

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    import bench
    import h264scroll as hs

    wl = dict(bench.WORKLOADS["p720dyn"])
    if args.streams:
        wl["streams"] = args.streams
    if args.frames:
        wl["frames"] = args.frames
    S, F, W, H = wl["streams"], wl["frames"], wl["w"], wl["h"]
    mbw, mbh = W // 16, H // 16
    rw, rh = wl["rect"][2], wl["rect"][3]
    SW, SH = 5, 5
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    hq = stream.cuda_stream

    rng = random.Random(1)
    pos = [[(rng.randint(0, mbw - rw), rng.randint(0, mbh - rh)) for _ in range(F)] for _ in range(S)]

    def build(rect, placed, size):
        w = dict(wl)
        w["rect"] = rect
        b = bench.build_compose_batch(hs, w, 0, 0)
        b.set_dyn_rect_moving()
        for s in range(S):
            for f in range(F):
                if placed:
                    b.set_dyn_rect_at(s, f, *pos[s][f])
                if size:
                    b.set_dyn_rect_size_at(s, f, *size)
        b.dyn_source_synth(F, 0, 0)             # every frame's pattern for its own rect
        return b

    makers = {"a": lambda: build(wl["rect"], True, None),
              "b": lambda: build(wl["rect"], True, (SW, SH)),
              "c": lambda: build((wl["rect"][0], wl["rect"][1], SW, SH), True, None),
              "d": lambda: build((0, 0, mbw, mbh), False, (SW, SH)),
              "e": lambda: build((0, 0, mbw, mbh), False, None)}
    arms = [(k, makers[k]()) for k in "abcde" if k in args.arms]

    def step(b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        b.compose(F, stream=hq, rewind=True)
        e1.record(stream)
        if b.sync() != 0:
            raise RuntimeError(hs.last_error())
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _, b in arms:                           # warm-up: code objects, pools, the table's upload
        for _ in range(3):
            step(b)
    times = {k: [] for k, _ in arms}
    for _ in range(args.rounds):
        for k, b in arms:
            times[k] += [step(b) for _ in range(args.steps)]
    by = dict(arms)
    same = None
    if "b" in by and "c" in by:
        same = all(by["b"].output(s) == by["c"].output(s) for s in range(0, S, max(1, S // 8)))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "tool": "size_bench",
        "config": {"workload": "BASELINE config 3's shape", "resolution": f"{W}x{H}", "streams": S,
                   "frames_per_step": F, "batch_rect_mbs": [rw, rh], "sized_mbs": [SW, SH],
                   "positions": "random.Random(1), uniform over the 25x25 rect's legal origins, per (stream, "
                                "frame); arms d, e: (0, 0)"},
        "timing": f"HIP events on one stream around each compose; 3 warm-up steps per arm, then {args.rounds} "
                  f"interleaved rounds of {args.steps} steps",
        "arms_ms": {k: spread(v) for k, v in times.items()},
        "ratios": {n: round(med[x] / med[y], 3) for n, (x, y) in
                   {"b_over_a": ("b", "a"), "b_over_c": ("b", "c"), "d_over_c": ("d", "c"), "d_over_e": ("d", "e")}.items()
                   if x in med and y in med},
        "b_bytes_equal_c": same,
        "bytes_per_step": {k: b.last_bytes() for k, b in arms},
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    for _, b in arms:
        b.close()
    if same is False:
        sys.exit("size_bench: the sized frames and the small batch rect wrote different bytes")


if __name__ == "__main__":
    main()
