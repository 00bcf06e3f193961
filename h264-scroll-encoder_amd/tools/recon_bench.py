#!/usr/bin/env python3
"""What the dynamic rect's reconstruction costs (scroll_batch_set_dyn_recon).

BASELINE config 3 (bench.py's p720dyn batch: 256 streams x 16 frames of
1280x720, rect 28,10,25,25, synthetic source, striped references per
stream), one JSON line:

  step_ms          the compose step with the reconstruction off and on,
                   interleaved rounds in one process, each round a block of
                   --steps composes between two HIP events on the compose
                   stream (median / min / max over the rounds);
  parent_off       with --parent-lib: the same step through another build
                   of the library (the parent revision's), in the same
                   rounds -- the reconstruction off must cost nothing, so the
                   pair is judged by its run-to-run spread;
  recon_kernel_ms  k_dyn_recon (--hinted: k_hdyn_recon) alone, by the batch's
                   HIP events around it;
  alg_bytes        its algorithmic bytes: dynamic NALs x rect MBs x 1152
                   (384 B of source and of prediction read, 384 B written);
  hbm_frac         alg_bytes / time against bench.py's HBM peak.

--hinted: the same batch with UI hints on -- one hint band (ref 0, a
horizontal motion) crossing the rect in every frame, SCROLL_HINT_PSKIP -- so
the rect is coded by k_hdyn_code / k_splice_stage and reconstructed by
k_hdyn_recon (scroll_batch_set_dyn_recon_hinted).

Usage: python h264-scroll-encoder_amd/tools/recon_bench.py [--rounds 7]
       [--steps 10] [--streams 256] [--frames 16] [--parent-lib PATH]
       [--hinted]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(PKG))
sys.path.insert(0, PKG)


def load_binding(name, lib_path=None):
    """the ctypes binding over the tree's library, or over another build of
    it (the binding's H264SCROLL_LIB variant mode), as its own module"""
    old = os.environ.pop("H264SCROLL_LIB", None)
    if lib_path:
        os.environ["H264SCROLL_LIB"] = os.path.abspath(lib_path)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "h264scroll.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.environ.pop("H264SCROLL_LIB", None)
        if old is not None:
            os.environ["H264SCROLL_LIB"] = old
    return mod


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="composes per timed block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--parent-lib", default=None, help="libh264scroll.so of the revision to compare the "
                                                       "reconstruction-off step with")
    ap.add_argument("--hinted", action="store_true", help="UI hints on: one band crossing the rect per frame, "
                                                          "PSKIP (k_hdyn_code + k_hdyn_recon)")
    args = ap.parse_args()

    import torch
    import bench

    wl = dict(bench.WORKLOADS["p720dyn"])
    if args.streams:
        wl["streams"] = args.streams
    if args.frames:
        wl["frames"] = args.frames
    S, F, rect = wl["streams"], wl["frames"], wl["rect"]
    torch.cuda.set_device(0)
    # a stream of its own: on torch's default (null) stream the composes would
    # run on the batch's own stream, beside the events instead of between them
    stream = torch.cuda.Stream()

    hs = load_binding("h264scroll_tree")
    arms = {"off": (hs, bench.build_compose_batch(hs, wl, 0, 0))}
    if args.parent_lib:
        hp = load_binding("h264scroll_parent", args.parent_lib)
        arms["parent_off"] = (hp, bench.build_compose_batch(hp, wl, 0, 0))

    def block(mod, b, n):
        """ms per compose of n composes between two HIP events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            b.compose(F, stream=stream.cuda_stream, rewind=True)
        e1.record(stream)
        e1.synchronize()
        if b.sync() != 0:
            raise RuntimeError(mod.last_error())
        return e0.elapsed_time(e1) / n

    if args.hinted:
        mbw = wl["w"] // 16
        for mod, bb in arms.values():
            for s in range(S):
                for f in range(F):
                    y = rect[1] + (3 * s + f) % rect[3]
                    bb.set_hints(s, f, [(0, y, mbw, y + 2, 0, 8 * (f % 5) - 13, 0)], mod.SCROLL_HINT_PSKIP)
    b = arms["off"][1]
    times = {k: [] for k in list(arms) + ["on"]}
    out_bytes = {}
    for mod, bb in arms.values():
        block(mod, bb, args.warmup)
    for _ in range(args.rounds):
        for k, (mod, bb) in arms.items():
            times[k].append(block(mod, bb, args.steps))
            out_bytes[k] = bb.last_bytes()
        b.set_dyn_recon(True, hinted=args.hinted)
        block(hs, b, 1)
        times["on"].append(block(hs, b, args.steps))
        out_bytes["on"] = b.last_bytes()
        b.set_dyn_recon(False)

    # the kernel alone: the batch's own event pair around it
    b.set_dyn_recon(True, hinted=args.hinted)
    b.enable_timing(True, lite=True)
    kern = []
    for _ in range(max(args.rounds, 5)):
        b.compose(F, stream=stream.cuda_stream, rewind=True)
        if b.sync() != 0:
            raise RuntimeError(hs.last_error())
        kern.append(b.dyn_recon_ms())
    b.enable_timing(False)
    _, _, dyn_nals = b.dyn_totals()
    sse = [0, 0, 0]
    for s in range(S):
        for f in range(F):
            v = b.dyn_sse(s, f)
            if v:
                sse = [a + c for a, c in zip(sse, v)]
    ps = b.dyn_psnr(0, 0)

    alg = dyn_nals * rect[2] * rect[3] * 1152
    kms = statistics.median(kern)
    achieved = alg / (kms * 1e-3) / 1e9
    out = {
        "tool": "recon_bench",
        "config": {"workload": "BASELINE config 3" + (" + UI hints (one band over the rect, PSKIP)" if args.hinted
                                                      else ""), "resolution": f"{wl['w']}x{wl['h']}", "streams": S,
                   "frames_per_step": F, "rect": list(rect), "source": "synthetic (k_dyn_synth)"},
        "timing": f"{args.rounds} interleaved rounds, {args.steps} composes per block between two HIP events",
        "step_ms": {k: spread(v) for k, v in times.items()},
        "step_bytes": out_bytes,
        "recon_on_minus_off_ms": round(statistics.median(times["on"]) - statistics.median(times["off"]), 4),
        "recon_kernel_ms": spread(kern),
        "dyn_nals": dyn_nals,
        "alg_bytes": alg,
        "achieved_gbs": round(achieved, 1),
        "hbm_peak_gbs": bench.HBM_PEAK_GBS,
        "hbm_frac": round(achieved / bench.HBM_PEAK_GBS, 4),
        "sse_total": sse,
        "psnr_stream0_frame0": [round(x, 2) for x in ps],
    }
    print(json.dumps(out))
    for _, bb in arms.values():
        bb.close()


if __name__ == "__main__":
    main()
