#!/usr/bin/env python3
"""What detecting the scroll offsets from renderer surfaces costs
(scroll_batch_detect_offsets: k_det_refs, k_det_surf, k_det_score,
k_det_pick).

BASELINE config 3's shape: 256 streams x 16 frames of 1280x720 BGRA surfaces
at their real strides (one surface per stream and frame, 15.1 GB), BT.709
limited range; every surface shows the shared references' stacked rows at the
frame's offset, grey, with a 25x25-MB region of noise at MB (28, 10).  The
references' luma is made limited-range so that the grey surface's luma under
BT.709 limited is exactly the reference's: the frames are FOUND at their
offsets (reported as "found"), from estimates off by 5.  In one process,
interleaved rounds, HIP events on one stream, per configuration (seg_step 1
and 4, radius 32 and the full 720):

  detect_ms   the whole call (scroll_batch_detect_ms);
  surf_ms     k_det_surf alone (scroll_batch_detect_kernel_ms): reads the used
              segments' surface bytes once, writes 2 bytes per row and used
              segment;
  score_ms    k_det_score + k_det_pick (scroll_batch_detect_score_ms);
  copy_ms     the yardstick of k_det_surf: one device-to-device copy (torch's
              copy_ of a contiguous byte tensor: hipMemcpyAsync) of (bytes
              read + bytes written) / 2 bytes, sized to what that seg_step
              actually reads.
(median / min / max over the rounds; TB/s over the algorithmic bytes)
One JSON line, also written to profiles/detect_bench_p720dyn.json.

Usage: python h264-scroll-encoder_amd/tools/detect_bench.py [--rounds 5]
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
CONFIGS = [(1, 32), (4, 32), (1, H), (4, H)]        # (seg_step, radius)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detect_bench_p720dyn.json"))
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

    # a grey pixel v has luma y(v) = (56284 v + 1081344) >> 16 under BT.709
    # limited (the luma row sums to 56284): the surfaces hold v, the references y(v)
    rng = np.random.default_rng(1)
    grey = rng.integers(0, 256, (2 * H, W), dtype=np.uint8)
    luma = ((56284 * grey.astype(np.int64) + 1081344) >> 16).astype(np.uint8)
    refs = [np.concatenate([y.reshape(-1), np.full(W * H // 2, 128, np.uint8)]).tobytes()
            for y in (luma[:H], luma[H:])]
    stack = torch.from_numpy(np.repeat(grey[..., None], 4, axis=2).copy()).cuda()       # [2H][W][4] grey
    truth = (np.arange(S * F, dtype=np.int64) * 37 % (H + 1)).astype(np.int32).reshape(S, F)
    x0, y0, rw, rh = (16 * v for v in RECT)
    surf = torch.empty(S * sstride, dtype=torch.uint8, device="cuda")
    view = surf.view(S * F, H, W, 4)
    for i in range(S * F):
        o = int(truth.reshape(-1)[i])
        view[i].copy_(stack[o:o + H])
        view[i, y0:y0 + rh, x0:x0 + rw].random_(0, 256)
    est = np.clip(truth + 5, 0, H).astype(np.int32)

    nseg = (W + 63) // 64
    b = hs.Batch(S, F, 1 << 20, device=0)
    for _ in range(S):
        b.add_stream(hs.make_config(W, H))
    b.set_dyn_rect(*RECT)
    b.set_dyn_refs(refs[0], refs[1])
    b.set_offsets(est)
    b.enable_timing()

    def detect(seg_step, radius):
        b.detect_offsets(surf.data_ptr(), F, pitch, fstride, sstride, fmt=hs.SCROLL_SURF_BGRA,
                         matrix=hs.SCROLL_SURF_BT709, radius=radius, seg_step=seg_step, min_match=H, apply=False,
                         stream=hq)
        ms = b.detect_ms(), b.detect_ms(kernel=True), b.detect_ms(score=True)
        if min(ms) <= 0:
            raise RuntimeError("no timing: " + hs.last_error())
        return ms

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nbytes = {}
    for step in sorted({c[0] for c in CONFIGS}):
        nuse = (nseg + step - 1) // step
        rd, wr = S * F * H * nuse * 256, S * F * H * nuse * 2
        nbytes[step] = (rd, wr, (rd + wr) // 2)
    n_max = max(v[2] for v in nbytes.values())
    a, c = torch.empty(n_max, dtype=torch.uint8, device="cuda"), torch.empty(n_max, dtype=torch.uint8, device="cuda")
    a.random_(0, 256)

    def copy(n):
        with torch.cuda.stream(stream):
            e0.record()
            c[:n].copy_(a[:n], non_blocking=True)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {cfg: ([], [], [], []) for cfg in CONFIGS}
    for r in range(2 + args.rounds):                    # 2 warm-up rounds, then interleaved
        for cfg in CONFIGS:
            ms = detect(*cfg) + (copy(nbytes[cfg[0]][2]),)
            if r >= 2:
                for t, v in zip(times[cfg], ms):
                    t.append(v)
    results = []
    for cfg in CONFIGS:
        detect(*cfg)
        res = b.detect_result(F)
        ok = int(((res["status"] == hs.SCROLL_DET_FOUND) & (res["off"] == truth)).sum())
        rd, wr, n_copy = nbytes[cfg[0]]
        t_all, t_surf, t_score, t_copy = times[cfg]
        m_surf, m_copy = statistics.median(t_surf), statistics.median(t_copy)
        results.append({
            "seg_step": cfg[0], "radius": cfg[1], "found": ok, "frames": S * F,
            "bytes_read": rd, "bytes_written": wr, "copy_bytes": n_copy,
            "detect_ms": spread(t_all), "surf_ms": spread(t_surf), "score_ms": spread(t_score),
            "copy_ms": spread(t_copy),
            "surf_tb_per_s": round((rd + wr) / m_surf / 1e9, 3),
            "copy_tb_per_s": round(2 * n_copy / m_copy / 1e9, 3),
            "surf_over_copy": round(m_surf / m_copy, 3),
            "score_over_surf": round(statistics.median(t_score) / m_surf, 3),
        })
    out = {
        "tool": "detect_bench",
        "config": {"workload": "BASELINE config 3's shape", "surfaces": f"{W}x{H} BGRA, BT.709 limited", "streams": S,
                   "frames_per_step": F, "pitch": pitch, "frame_stride": fstride, "stream_stride": sstride,
                   "painted": list(RECT), "estimate_error": 5},
        "timing": f"{args.rounds} interleaved rounds after 2 warm-up rounds, HIP events on one stream",
        "results": results,
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
