#!/usr/bin/env python3
"""What locating the rect from renderer surfaces costs
(scroll_batch_dyn_locate: a dry state pass, k_dmg_rows, k_dyn_damage,
k_dyn_place).

BASELINE config 3's shape: 256 streams x 16 frames of 1280x720 BGRA surfaces
at their real strides (one surface per stream and frame, 15.1 GB), BT.709
limited range, the 25x25-MB rect; every surface is the stream's reference
picture A in grey with a 25x25-MB region of noise at MB (28, 10); mb_sse =
2^20 lies between the limited-range mapping's error on the grey MBs and the
noise MBs', so the frames, all at offset 0, locate there (reported as
"located").  In one process, interleaved rounds, HIP events on one stream:

  locate_ms   the whole call (scroll_batch_dyn_locate_ms);
  damage_ms   k_dyn_damage alone (scroll_batch_dyn_locate_kernel_ms): reads
              every surface byte once and one luma picture per frame, writes
              4 bytes per MB;
  copy_ms     the yardstick: one device-to-device copy (torch's copy_ of a
              contiguous byte tensor: hipMemcpyAsync) of (bytes read + bytes
              written) / 2 bytes -- surfaces, one luma picture per frame and
              the map.
(median / min / max over the rounds; TB/s over the algorithmic bytes)
One JSON line, also written to profiles/locate_bench_p720dyn.json.

Usage: python h264-scroll-encoder_amd/tools/locate_bench.py [--rounds 5]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "locate_bench_p720dyn.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import h264scroll as hs

    S, F = args.streams, args.frames
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    hq = stream.cuda_stream
    pitch, fstride = 4 * W, 4 * W * H
    sstride = fstride * F

    # reference pictures: random luma; the surface that matches A exactly at
    # offset 0 would be grey in full range -- in limited range it differs by
    # the range mapping everywhere, which costs the kernel nothing more or
    # less: it reads and squares every pixel either way
    rng = np.random.default_rng(1)
    ya = rng.integers(0, 256, (H, W), dtype=np.uint8)
    refs = [np.concatenate([y.reshape(-1), np.full(W * H // 2, 128, np.uint8)]).tobytes()
            for y in (ya, rng.integers(0, 256, (H, W), dtype=np.uint8))]
    one = torch.from_numpy(np.repeat(ya[..., None], 4, axis=2).copy()).cuda()          # [H][W][4] grey
    x0, y0, rw, rh = (16 * v for v in RECT)
    surf = torch.empty(S * sstride, dtype=torch.uint8, device="cuda")
    view = surf.view(S * F, H, W, 4)
    for i in range(S * F):
        view[i].copy_(one)
        view[i, y0:y0 + rh, x0:x0 + rw].random_(0, 256)

    nmb = (W // 16) * (H // 16)
    rd, wr = S * F * (W * H * 4 + W * H), S * F * nmb * 4
    n_copy = (rd + wr) // 2
    a, c = torch.empty(n_copy, dtype=torch.uint8, device="cuda"), torch.empty(n_copy, dtype=torch.uint8, device="cuda")
    a.random_(0, 256)

    b = hs.Batch(S, F, 1 << 20, device=0)
    for _ in range(S):
        b.add_stream(hs.make_config(W, H))
    b.set_dyn_rect(*RECT)
    b.set_dyn_refs(refs[0], refs[1])
    b.set_dyn_rect_moving()
    b.set_offsets(np.zeros((S, F), np.int32))
    b.enable_timing()

    def locate():
        b.dyn_locate(surf.data_ptr(), F, pitch, fstride, sstride, fmt=hs.SCROLL_SURF_BGRA, matrix=hs.SCROLL_SURF_BT709,
                     mb_sse=1 << 20, stream=hq)
        ms, k = b.dyn_locate_ms(), b.dyn_locate_ms(kernel=True)
        if ms <= 0 or k <= 0:
            raise RuntimeError("no timing: " + hs.last_error())
        return ms, k

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy():
        with torch.cuda.stream(stream):
            e0.record()
            c.copy_(a, non_blocking=True)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):                              # warm-up
        locate()
        copy()
    t_loc, t_dmg, t_copy = [], [], []
    for _ in range(args.rounds):
        ms, k = locate()
        t_loc.append(ms)
        t_dmg.append(k)
        t_copy.append(copy())
    res = b.dyn_locate_result(1)[:4, 0]
    m_loc, m_dmg, m_copy = (statistics.median(t) for t in (t_loc, t_dmg, t_copy))
    out = {
        "tool": "locate_bench",
        "config": {"workload": "BASELINE config 3's shape", "surfaces": f"{W}x{H} BGRA, BT.709 limited", "streams": S,
                   "frames_per_step": F, "rect": list(RECT), "pitch": pitch, "frame_stride": fstride,
                   "stream_stride": sstride, "mb_sse": 1 << 20},
        "timing": f"{args.rounds} interleaved rounds after 2 warm-up rounds, HIP events on one stream",
        "located": [[int(r["x0"]), int(r["y0"]), int(r["status"]), int(r["n_mb"])] for r in res],
        "bytes_read": rd,
        "bytes_written": wr,
        "copy_bytes": n_copy,
        "locate_ms": spread(t_loc),
        "damage_ms": spread(t_dmg),
        "copy_ms": spread(t_copy),
        "damage_tb_per_s": round((rd + wr) / m_dmg / 1e9, 3),
        "copy_tb_per_s": round(2 * n_copy / m_copy / 1e9, 3),
        "locate_over_copy": round(m_loc / m_copy, 3),
        "damage_over_copy": round(m_dmg / m_copy, 3),
        "allowance": 1.5,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
