#!/usr/bin/env python3
"""What probing the dynamic rect at candidate QPs costs (scroll_batch_dyn_probe).

BASELINE config 3 (bench.py's p720dyn batch: 256 streams x 16 frames of
1280x720, rect 28,10,25,25, synthetic source, striped references per
stream), one JSON line, also written to profiles/probe_bench_p720dyn.json:

  probe_ms         the probe's launches (state pass, k_dyn_rows, k_dyn_probe)
                   at nq = 1, 4, 8 candidates, by the batch's HIP events
                   around them, --steps probes per round;
  step_on_ms       the compose step with the reconstruction on, a block of
                   --steps composes between two HIP events, in the same
                   interleaved rounds of the same process;
  vs_trial_composes   probe_ms / (nq x step_on_ms): the caller's only other
                   way to the same numbers is nq trial composes with the
                   reconstruction on, on cloned batches (a compose cannot be
                   taken back);
  recon_kernel_ms  k_dyn_recon alone in the same run, and probe_ms at nq = 1
                   against it: the same blocks are read, the counting is added.
(median / min / max over the rounds)

Usage: python h264-scroll-encoder_amd/tools/probe_bench.py [--rounds 7]
       [--steps 5] [--streams 256] [--frames 16] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)

CANDIDATES = {1: [26], 4: [20, 26, 32, 38], 8: [14, 18, 22, 26, 30, 34, 38, 42]}


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="composes per timed block, probes per round and nq")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "probe_bench_p720dyn.json"))
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
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()          # not the null stream: the events must bracket the work
    b = bench.build_compose_batch(hs, wl, 0, 0)
    b.set_dyn_recon(True)
    b.enable_timing(True, lite=True)

    def block(n):
        """ms per compose of n composes between two HIP events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            b.compose(F, stream=stream.cuda_stream, rewind=True)
        e1.record(stream)
        e1.synchronize()
        if b.sync() != 0:
            raise RuntimeError(hs.last_error())
        return e0.elapsed_time(e1) / n, b.dyn_recon_ms()

    def probe(qps, n):
        """mean ms of n probes, each by the batch's events around its launches"""
        q = hs.u8buf(bytes(qps))
        ms = []
        for _ in range(n):
            rc = hs.lib.scroll_batch_dyn_probe(b.h, F, q, len(qps), stream.cuda_stream)
            if rc != 0:
                raise RuntimeError(hs.last_error())
            ms.append(b.dyn_probe_ms())
        return sum(ms) / n

    block(args.warmup)
    for qps in CANDIDATES.values():
        probe(qps, args.warmup)
    step, kern = [], []
    pms = {nq: [] for nq in CANDIDATES}
    for _ in range(args.rounds):
        s, k = block(args.steps)
        step.append(s)
        kern.append(k)
        for nq, qps in CANDIDATES.items():
            pms[nq].append(probe(qps, args.steps))
    bytes_after = b.last_bytes()

    # what the last probe says, summed: a sanity figure for the record
    r = hs.ScrollDynProbe()
    import ctypes
    tot = {"bits": 0, "nonzero": 0, "sse": 0}
    for s in range(min(S, 4)):
        for f in range(F):
            if hs.lib.scroll_batch_dyn_probe_result(b.h, s, f, 3, ctypes.byref(r)) == 0:
                tot["bits"] += r.bits
                tot["nonzero"] += r.nonzero
                tot["sse"] += sum(r.sse)

    smed, kmed = statistics.median(step), statistics.median(kern)
    out = {
        "tool": "probe_bench",
        "config": {"workload": "BASELINE config 3", "resolution": f"{wl['w']}x{wl['h']}", "streams": S,
                   "frames_per_step": F, "rect": list(rect), "source": "synthetic (k_dyn_synth)"},
        "timing": f"{args.rounds} interleaved rounds: {args.steps} composes (reconstruction on) between two HIP "
                  f"events, then {args.steps} probes per nq by the batch's events around their launches",
        "candidates": {str(k): v for k, v in CANDIDATES.items()},
        "probe_ms": {str(nq): spread(v) for nq, v in pms.items()},
        "step_on_ms": spread(step),
        "recon_kernel_ms": spread(kern),
        "vs_trial_composes": {str(nq): round(statistics.median(v) / (nq * smed), 4) for nq, v in pms.items()},
        "nq1_vs_recon_kernel": round(statistics.median(pms[1]) / kmed, 4),
        "step_bytes": bytes_after,
        "probe_nq8_cand3_first4_streams": tot,
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
