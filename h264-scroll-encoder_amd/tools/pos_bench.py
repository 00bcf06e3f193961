#!/usr/bin/env python3
"""What placing the plain rect per stream and per frame costs
(scroll_batch_set_dyn_rect_moving).

BASELINE config 3's shape (bench.py's p720dyn batch: 256 streams x 16 frames
of 1280x720, a 25x25-MB rect, the synthetic source generated on the device at
each frame's position), three batches in one process, HIP events on one
stream around each compose, interleaved rounds after a warm-up; one JSON
line, also written to profiles/pos_bench_p720dyn.json:

  uniform_ms  (a) every frame at the batch position, the flag off: bench.py's
              own step;
  moving_ms   (b) the flag on, a random legal position per (stream, frame):
              the same kernels, each frame's origin from the position table;
  hinted_ms   (c) the same positions through the hinted path with empty hint
              lists in EXACT mode (k_hdyn_code + k_splice_stage): the only
              way to compose them without the flag.
(median / min / max of the per-step times over all rounds; kernels_ms: one
step's split by scroll_batch_kernel_ms, taken after the rounds)

(b) and (c) are checked to have written the same bytes.

Usage: python h264-scroll-encoder_amd/tools/pos_bench.py [--rounds 5]
       [--steps 10] [--hinted-steps 2] [--streams 256] [--frames 16] [--out PATH]
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
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
sys.path.insert(0, HERE)

KERNELS = ["plan", "emit", "dyn_stage", "dyn_emit", "dyn_code", "dyn_pack"]


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--hinted-steps", type=int, default=2)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pos_bench_p720dyn.json"))
    args = ap.parse_args()

    import torch
    import bench
    import h264scroll as hs

    wl = dict(bench.WORKLOADS["p720dyn"])
    if args.streams:
        wl["streams"] = args.streams
    if args.frames:
        wl["frames"] = args.frames
    S, F, W, H = wl["streams"], wl["frames"], wl["w"], wl["h"]
    rw, rh = wl["rect"][2], wl["rect"][3]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    hq = stream.cuda_stream

    rng = random.Random(1)
    pos = [[(rng.randint(0, W // 16 - rw), rng.randint(0, H // 16 - rh)) for _ in range(F)] for _ in range(S)]

    def placed(b):
        for s in range(S):
            for f in range(F):
                b.set_dyn_rect_at(s, f, *pos[s][f])

    uniform = bench.build_compose_batch(hs, wl, 0, 0)
    moving = bench.build_compose_batch(hs, wl, 0, 0)
    moving.set_dyn_rect_moving()
    placed(moving)
    moving.dyn_source_synth(F, 0, 0)            # every frame's pattern at its own position
    hinted = bench.build_compose_batch(hs, wl, 0, 0)
    hinted.set_dyn_rect_moving()                # the same pixels: the generator follows the table with the flag
    placed(hinted)
    hinted.dyn_source_synth(F, 0, 0)
    hinted.set_dyn_rect_moving(False)
    for s in range(S):
        for f in range(F):
            hinted.set_hints(s, f, [], hs.SCROLL_HINT_EXACT)

    def step(b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        b.compose(F, stream=hq, rewind=True)
        e1.record(stream)
        if b.sync() != 0:
            raise RuntimeError(hs.last_error())
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = [("uniform_ms", uniform, args.steps), ("moving_ms", moving, args.steps),
            ("hinted_ms", hinted, args.hinted_steps)]
    for _, b, _ in arms:                         # warm-up: code objects, pools, the table's upload
        for _ in range(3):
            step(b)
    times = {name: [] for name, _, _ in arms}
    for _ in range(args.rounds):
        for name, b, n in arms:
            times[name] += [step(b) for _ in range(n)]
    same = all(moving.output(s) == hinted.output(s) for s in range(0, S, max(1, S // 8)))
    kernels = {}
    for name, b, _ in arms[:2]:
        b.enable_timing(True)
        step(b)
        kernels[name] = {k: round(b.kernel_ms(i), 4) for i, k in enumerate(KERNELS)}
        b.enable_timing(False)
    out = {
        "tool": "pos_bench",
        "config": {"workload": "BASELINE config 3's shape", "resolution": f"{W}x{H}", "streams": S,
                   "frames_per_step": F, "rect_mbs": [rw, rh], "uniform_at": list(wl["rect"][:2]),
                   "positions": "random.Random(1), uniform over the legal origins, per (stream, frame)"},
        "timing": f"HIP events on one stream around each compose; 3 warm-up steps per arm, then {args.rounds} "
                  f"interleaved rounds of {args.steps} / {args.steps} / {args.hinted_steps} steps",
        "uniform_ms": spread(times["uniform_ms"]),
        "moving_ms": spread(times["moving_ms"]),
        "hinted_ms": spread(times["hinted_ms"]),
        "moving_over_uniform": round(statistics.median(times["moving_ms"]) / statistics.median(times["uniform_ms"]), 3),
        "hinted_over_moving": round(statistics.median(times["hinted_ms"]) / statistics.median(times["moving_ms"]), 1),
        "kernels_ms": kernels,
        "moving_bytes_equal_hinted": bool(same),
        "bytes_per_step": {"uniform": uniform.last_bytes(), "moving": moving.last_bytes()},
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    for _, b, _ in arms:
        b.close()
    if not same:
        sys.exit("pos_bench: the moving and the hinted compose wrote different bytes")


if __name__ == "__main__":
    main()
