#!/usr/bin/env python3
"""What cutting the rect's source out of renderer surfaces costs
(scroll_batch_dyn_source_from_surfaces, k_csc).

BASELINE config 3's shape: 256 streams x 16 frames, the 25x25-MB rect at MB
(28, 10) of 1280x720 BGRA surfaces at their real strides (one surface per
stream and frame, 15.1 GB), BT.709 limited range.  In one process, interleaved
rounds, HIP events on one stream:

  csc_ms    the conversion (scroll_batch_surface_ms): reads the rect's
            400x400 pixels x 4 bytes of every surface in 1,600-byte row runs,
            writes 1.5 bytes per pixel of I420;
  copy_ms   the yardstick: one device-to-device copy (torch's copy_ of a
            contiguous byte tensor: hipMemcpyAsync) of (bytes read + bytes
            written) / 2 bytes -- the same traffic as the conversion, as one
            stream.
(median / min / max over the rounds; TB/s over the algorithmic bytes)
One JSON line, also written to profiles/surface_bench_p720dyn.json.

Usage: python h264-scroll-encoder_amd/tools/surface_bench.py [--rounds 5]
       [--streams 256] [--frames 16] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)
sys.path.insert(0, PKG)

W, H, RECT = 1280, 720, (28, 10, 25, 25)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_bench_p720dyn.json"))
    args = ap.parse_args()

    import torch
    import h264scroll as hs

    S, F = args.streams, args.frames
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    hq = stream.cuda_stream
    pitch, fstride = 4 * W, 4 * W * H
    sstride = fstride * F
    surf = torch.empty(S * sstride, dtype=torch.uint8, device="cuda")
    step = 1 << 30                                  # random pixels, a piece at a time
    for at in range(0, surf.numel(), step):
        surf[at:at + step].random_(0, 256)
    px = 256 * RECT[2] * RECT[3]
    rd, wr = S * F * px * 4, S * F * px * 3 // 2
    n_copy = (rd + wr) // 2
    a, c = torch.empty(n_copy, dtype=torch.uint8, device="cuda"), torch.empty(n_copy, dtype=torch.uint8, device="cuda")
    a.random_(0, 256)

    b = hs.Batch(S, F, 1 << 20, device=0)
    for _ in range(S):
        b.add_stream(hs.make_config(W, H))
    b.set_dyn_rect(*RECT)
    b.enable_timing()

    def csc():
        b.dyn_source_from_surfaces(surf.data_ptr(), F, pitch, fstride, sstride, fmt=hs.SCROLL_SURF_BGRA,
                                   matrix=hs.SCROLL_SURF_BT709, stream=hq)
        ms = b.surface_ms()
        if ms <= 0:
            raise RuntimeError("no timing: " + hs.last_error())
        return ms

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy():
        with torch.cuda.stream(stream):
            e0.record()
            c.copy_(a, non_blocking=True)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):                              # warm-up
        csc()
        copy()
    t_csc, t_copy = [], []
    for _ in range(args.rounds):
        t_csc.append(csc())
        t_copy.append(copy())
    m_csc, m_copy = statistics.median(t_csc), statistics.median(t_copy)
    out = {
        "tool": "surface_bench",
        "config": {"workload": "BASELINE config 3's shape", "surfaces": f"{W}x{H} BGRA, BT.709 limited", "streams": S,
                   "frames_per_step": F, "rect": list(RECT), "pitch": pitch, "frame_stride": fstride,
                   "stream_stride": sstride},
        "timing": f"{args.rounds} interleaved rounds after 2 warm-up rounds, HIP events on one stream",
        "bytes_read": rd,
        "bytes_written": wr,
        "copy_bytes": n_copy,
        "csc_ms": spread(t_csc),
        "copy_ms": spread(t_copy),
        "csc_tb_per_s": round((rd + wr) / m_csc / 1e9, 3),
        "copy_tb_per_s": round(2 * n_copy / m_copy / 1e9, 3),
        "csc_over_copy": round(m_csc / m_copy, 3),
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
