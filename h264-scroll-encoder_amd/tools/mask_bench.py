#!/usr/bin/env python3
"""What the per-MB source mask costs and saves (scroll_batch_dyn_mask: a dry
state pass, k_dyn_rows, k_dyn_mask_diff, k_dyn_mask_fill, k_dyn_mask_rec).

BASELINE config 3's batch (bench.py's p720dyn: 256 streams x 16 frames, the
25x25-MB rect at MB (28, 10), per-stream references, the synthetic offsets).
The source is the prediction +- amp (default 1) on every sample with a
5x5-MB block of noise in the middle: the prediction comes from the device
itself (a mask with maximal thresholds and apply = 1 leaves it in the source
buffer), noise and block are added on the device, every round anew: a
compose moves the streams on, and with them the prediction.  A second batch
in lockstep composes the same source unmasked.  The rule: mb_sse_y = 256
amp^2, mb_sse_c = 128 amp^2 (what the noise can reach), grow = 1: 25 MBs
changed, 49 kept.  In one process, interleaved rounds, HIP events on one
stream:

  mask_ms     the whole call (scroll_batch_dyn_mask_ms);
  diff_ms     k_dyn_mask_diff alone (scroll_batch_dyn_mask_kernel_ms): reads
              every source byte of the rect and as many reference bytes,
              writes 8 bytes per MB;
  copy_ms     the yardstick: one device-to-device copy (torch's copy_ of a
              contiguous byte tensor: hipMemcpyAsync) of (bytes read + bytes
              written) / 2 bytes of the whole call -- the difference kernel's
              traffic, and for every MB not kept its chroma source and its
              prediction read and 384 bytes written, the map read twice and
              its second word rewritten;
  totals      scroll_batch_dyn_totals' RBSP bytes of a compose of the pristine
              source and of the masked one, and k_dyn_row's time on each
              (lite timing: that kernel alone).
(median / min / max over the rounds; TB/s over the algorithmic bytes)
One JSON line, also written to profiles/mask_bench_p720dyn.json.

Usage: python h264-scroll-encoder_amd/tools/mask_bench.py [--rounds 5]
       [--streams 256] [--frames 16] [--amp 1] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)
sys.path.insert(0, PKG)
sys.path.insert(0, REPO)

MAXT = 0xFFFFFFFF
D2D = 3


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--amp", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mask_bench_p720dyn.json"))
    args = ap.parse_args()

    import torch
    import bench
    import h264scroll as hs

    wl = dict(bench.WORKLOADS["p720dyn"])
    if args.streams:
        wl["streams"] = args.streams
    if args.frames:
        wl["frames"] = args.frames
    S, F, rect = wl["streams"], wl["frames"], wl["rect"]
    rw, rh = rect[2:]
    nmb, fb = rw * rh, 384 * rw * rh
    amp = args.amp
    ty, tc, grow = 256 * amp * amp, 128 * amp * amp, 1
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()          # not the null stream: the events must bracket the work
    hq = stream.cuda_stream
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def build():
        x = bench.build_compose_batch(hs, wl, 0, 0)
        x.enable_timing(True, lite=True)
        return x

    # two batches in lockstep: b is masked, b2 composes the same source as it is
    b, b2 = build(), build()
    dsrc, ls, lf = b.dyn_source_device()
    dsrc2 = b2.dyn_source_device()[0]
    assert lf >= fb and ls >= F * lf and b2.dyn_source_device()[1:] == (ls, lf)
    pris = torch.empty(S * ls, dtype=torch.uint8, device="cuda")
    frames = torch.as_strided(pris, (S, F, fb), (ls, lf, 1))
    bx, by = (rw - 5) // 2, (rh - 5) // 2

    def results(n=4):
        return b.dyn_mask_result(1)[:n, 0]

    def prepare():
        """the source of the next compose in both batches: its prediction, from
        the device (every MB dropped), + noise + the block"""
        b.dyn_mask(F, MAXT, MAXT, 0, apply=True, stream=hq)
        assert all(int(r["status"]) == 0 and int(r["n_kept"]) == 0 for r in results())
        assert hip.hipMemcpy(pris.data_ptr(), dsrc, S * ls, D2D) == 0
        assert hip.hipDeviceSynchronize() == 0
        for s in range(S):
            x = frames[s].to(torch.int16) + torch.randint(-amp, amp + 1, (F, fb), dtype=torch.int16, device="cuda")
            x = x.clamp_(0, 255).to(torch.uint8)
            x[:, :256 * nmb].view(F, 16 * rh, 16 * rw)[:, 16 * by:16 * by + 80, 16 * bx:16 * bx + 80].random_(0, 256)
            for p in range(2):
                c = x[:, 256 * nmb + 64 * nmb * p:256 * nmb + 64 * nmb * (p + 1)].view(F, 8 * rh, 8 * rw)
                c[:, 8 * by:8 * by + 40, 8 * bx:8 * bx + 40].random_(0, 256)
            frames[s].copy_(x)
        torch.cuda.synchronize()
        for d in (dsrc, dsrc2):
            assert hip.hipMemcpy(d, pris.data_ptr(), S * ls, D2D) == 0
        assert hip.hipDeviceSynchronize() == 0

    def mask():
        b.dyn_mask(F, ty, tc, grow, apply=True, stream=hq)
        ms, k = b.dyn_mask_ms(), b.dyn_mask_ms(kernel=True)
        if ms <= 0 or k <= 0:
            raise RuntimeError("no timing: " + hs.last_error())
        return ms, k

    def compose(x):
        """(RBSP bytes, k_dyn_row ms) of one compose of what the source holds"""
        x.kernel_stats_ex()                         # reset the accumulators
        x.compose(F, stream=hq, rewind=True)
        if x.sync() != 0:
            raise RuntimeError(hs.last_error())
        ms, n = x.kernel_stats_ex()
        return x.dyn_totals()[0], ms[4] / max(n, 1)

    prepare()
    mask()
    rec = results()
    n_kept = int(rec[0]["n_kept"])
    ndrop = nmb - n_kept
    NF = S * F
    rd_diff, wr_diff = NF * 2 * fb, NF * nmb * 8
    rd = rd_diff + NF * (2 * nmb * 8 + ndrop * (128 + 384) + rh * 16)
    wr = wr_diff + NF * (ndrop * 384 + rh * 16 + nmb * 4 + 40)
    n_copy = (rd + wr) // 2
    a, c = torch.empty(n_copy, dtype=torch.uint8, device="cuda"), torch.empty(n_copy, dtype=torch.uint8, device="cuda")
    a.random_(0, 256)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy():
        with torch.cuda.stream(stream):
            e0.record()
            c.copy_(a, non_blocking=True)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    compose(b)
    compose(b2)
    copy()
    t_mask, t_diff, t_copy, row_plain, row_masked = [], [], [], [], []
    for i in range(1 + args.rounds):                # (the round above and this loop's first: the 2 warm-up rounds)
        prepare()
        ms, k = mask()
        assert [int(r["n_kept"]) for r in results()] == [n_kept] * len(rec)
        bytes_masked, km = compose(b)
        bytes_plain, kp = compose(b2)
        t = copy()
        if i == 0:
            continue
        t_mask.append(ms)
        t_diff.append(k)
        row_masked.append(km)
        row_plain.append(kp)
        t_copy.append(t)
    m_mask, m_diff, m_copy = (statistics.median(t) for t in (t_mask, t_diff, t_copy))
    out = {
        "tool": "mask_bench",
        "config": {"workload": "BASELINE config 3 (bench.py p720dyn)", "streams": S, "frames_per_step": F,
                   "rect": list(rect), "source": f"prediction +- {amp}, a 5x5-MB block of noise",
                   "rule": {"mb_sse_y": ty, "mb_sse_c": tc, "grow": grow, "apply": 1}},
        "timing": f"{args.rounds} interleaved rounds after 2 warm-up rounds, HIP events on one stream",
        "records": [[int(r["n_changed"]), int(r["n_kept"])] + [int(v) for v in r["sse_drop"]] for r in rec],
        "bytes_read": rd,
        "bytes_written": wr,
        "copy_bytes": n_copy,
        "mask_ms": spread(t_mask),
        "diff_ms": spread(t_diff),
        "copy_ms": spread(t_copy),
        "diff_tb_per_s": round((rd_diff + wr_diff) / m_diff / 1e9, 3),
        "copy_tb_per_s": round(2 * n_copy / m_copy / 1e9, 3),
        "mask_over_copy": round(m_mask / m_copy, 3),
        "diff_over_copy": round(m_diff / (m_copy * (rd_diff + wr_diff) / (rd + wr)), 3),
        "allowance": 1.5,
        "dyn_totals_rbsp_bytes": {"plain": int(bytes_plain), "masked": int(bytes_masked)},
        "k_dyn_row_ms": {"plain": spread(row_plain), "masked": spread(row_masked)},
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    b.close()
    b2.close()


if __name__ == "__main__":
    main()
