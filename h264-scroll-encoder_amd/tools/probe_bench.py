#!/usr/bin/env python3
"""What probing the dynamic rect at candidate QPs costs (scroll_batch_dyn_probe,
--hinted: scroll_batch_dyn_probe_hinted).

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
                   against it: the same blocks are read, the counting is added;
  parent_probe_ms  with --parent-lib: the same probes through another build
                   of the library (the parent revision's), in the same rounds.
(median / min / max over the rounds)

--hinted: tools/recon_bench.py --hinted's batch (config 3 plus one PSKIP hint
band over the rect in every frame), the hinted reconstruction on; the probe
is scroll_batch_dyn_probe_hinted (state pass, k_hprobe_class, k_hdyn_probe) at
nq = 1, 2, 4, 8, the step is the hinted compose (k_hdyn_code, k_hdyn_recon,
k_splice_stage), recon_kernel_ms is k_hdyn_recon; with --parent-lib the
parent's hinted compose step (parent_step_on_ms) runs in the same rounds --
eight of those are what the 8-candidate probe replaces.  Written to
profiles/hprobe_bench_p720dyn.json.

Usage: python h264-scroll-encoder_amd/tools/probe_bench.py [--rounds 7]
       [--steps 5] [--streams 256] [--frames 16] [--hinted]
       [--parent-lib PATH] [--out PATH]
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
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
sys.path.insert(0, HERE)

CANDIDATES = {1: [26], 4: [20, 26, 32, 38], 8: [14, 18, 22, 26, 30, 34, 38, 42]}
CANDIDATES_HINTED = {1: [26], 2: [22, 30], 4: [20, 26, 32, 38], 8: [14, 18, 22, 26, 30, 34, 38, 42]}


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
    ap.add_argument("--hinted", action="store_true", help="UI hints on: one band crossing the rect per frame, "
                                                          "PSKIP; the hinted probe against the hinted compose")
    ap.add_argument("--parent-lib", default=None, help="libh264scroll.so of the revision to compare with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles",
                                "hprobe_bench_p720dyn.json" if args.hinted else "probe_bench_p720dyn.json")

    import torch
    import bench
    from recon_bench import load_binding

    wl = dict(bench.WORKLOADS["p720dyn"])
    if args.streams:
        wl["streams"] = args.streams
    if args.frames:
        wl["frames"] = args.frames
    S, F, rect = wl["streams"], wl["frames"], wl["rect"]
    cands = CANDIDATES_HINTED if args.hinted else CANDIDATES
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()          # not the null stream: the events must bracket the work

    def make(mod):
        bb = bench.build_compose_batch(mod, wl, 0, 0)
        if args.hinted:
            mbw = wl["w"] // 16
            for s in range(S):
                for f in range(F):
                    y = rect[1] + (3 * s + f) % rect[3]
                    bb.set_hints(s, f, [(0, y, mbw, y + 2, 0, 8 * (f % 5) - 13, 0)], mod.SCROLL_HINT_PSKIP)
        bb.set_dyn_recon(True, hinted=args.hinted)
        bb.enable_timing(True, lite=True)
        return bb

    hs = load_binding("h264scroll_tree")
    b = make(hs)
    hp = pb = None
    if args.parent_lib:
        hp = load_binding("h264scroll_parent", args.parent_lib)
        pb = make(hp)

    def block(mod, bb, n):
        """ms per compose of n composes between two HIP events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            bb.compose(F, stream=stream.cuda_stream, rewind=True)
        e1.record(stream)
        e1.synchronize()
        if bb.sync() != 0:
            raise RuntimeError(mod.last_error())
        return e0.elapsed_time(e1) / n, bb.dyn_recon_ms()

    def probe(mod, bb, qps, n, hinted):
        """mean ms of n probes, each by the batch's events around its launches"""
        q = mod.u8buf(bytes(qps))
        fn = mod.lib.scroll_batch_dyn_probe_hinted if hinted else mod.lib.scroll_batch_dyn_probe
        ms = []
        for _ in range(n):
            rc = fn(bb.h, F, q, len(qps), stream.cuda_stream)
            if rc != 0:
                raise RuntimeError(mod.last_error())
            ms.append(bb.dyn_probe_ms())
        return sum(ms) / n

    parent_probes = pb is not None and not args.hinted     # the parent has no hinted probe
    block(hs, b, args.warmup)
    if pb:
        block(hp, pb, args.warmup)
    for qps in cands.values():
        probe(hs, b, qps, args.warmup, args.hinted)
        if parent_probes:
            probe(hp, pb, qps, args.warmup, False)
    step, kern, pstep = [], [], []
    pms = {nq: [] for nq in cands}
    ppms = {nq: [] for nq in cands}
    for _ in range(args.rounds):
        s, k = block(hs, b, args.steps)
        step.append(s)
        kern.append(k)
        if pb:
            pstep.append(block(hp, pb, args.steps)[0])
        for nq, qps in cands.items():
            pms[nq].append(probe(hs, b, qps, args.steps, args.hinted))
            if parent_probes:
                ppms[nq].append(probe(hp, pb, qps, args.steps, False))
    bytes_after = b.last_bytes()

    # what the last probe says, summed: a sanity figure for the record
    r = hs.ScrollDynProbe()
    tot = {"bits": 0, "nonzero": 0, "sse": 0}
    for s in range(min(S, 4)):
        for f in range(F):
            if hs.lib.scroll_batch_dyn_probe_result(b.h, s, f, 3, ctypes.byref(r)) == 0:
                tot["bits"] += r.bits
                tot["nonzero"] += r.nonzero
                tot["sse"] += sum(r.sse)

    smed, kmed = statistics.median(step), statistics.median(kern)
    out = {
        "tool": "probe_bench" + (" --hinted" if args.hinted else ""),
        "config": {"workload": "BASELINE config 3" + (" + UI hints (one band over the rect, PSKIP)" if args.hinted
                                                      else ""), "resolution": f"{wl['w']}x{wl['h']}", "streams": S,
                   "frames_per_step": F, "rect": list(rect), "source": "synthetic (k_dyn_synth)"},
        "timing": f"{args.rounds} interleaved rounds: {args.steps} composes (reconstruction on) between two HIP "
                  f"events, then {args.steps} probes per nq by the batch's events around their launches",
        "candidates": {str(k): v for k, v in cands.items()},
        "probe_ms": {str(nq): spread(v) for nq, v in pms.items()},
        "step_on_ms": spread(step),
        "recon_kernel_ms": spread(kern),
        "vs_trial_composes": {str(nq): round(statistics.median(v) / (nq * smed), 4) for nq, v in pms.items()},
        "nq1_vs_recon_kernel": round(statistics.median(pms[1]) / kmed, 4),
        "step_bytes": bytes_after,
        "probe_nq8_cand3_first4_streams": tot,
    }
    if pb:
        out["parent_step_on_ms"] = spread(pstep)
        out["vs_parent_trial_composes"] = {str(nq): round(statistics.median(v) / (nq * statistics.median(pstep)), 4)
                                           for nq, v in pms.items()}
    if parent_probes:
        out["parent_probe_ms"] = {str(nq): spread(v) for nq, v in ppms.items()}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    b.close()
    if pb:
        pb.close()


if __name__ == "__main__":
    main()
