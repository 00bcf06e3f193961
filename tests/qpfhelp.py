"""The plain dynamic rect at a QP of its own per frame, from the oracle: the
oracle is called one frame at a time anyway, with the QP in its or_dyn_rect,
so a per-frame-QP stream is or_compose_dyn called per frame with that frame's
QP.  Also the numpy restatement of the device pick's rule
(h264-scroll-encoder_amd/csrc/pick_device.h).  For
tests/test_qp_frames_oracle.py, tests/test_pick_hostsim.py and
tests/test_gpu_qp_frames.py."""
import ctypes

import numpy as np

from dynhelp import OrCfg, Rect, qp_field, split_nals
from probehelp import TRACE, se_len
from reconhelp import decode_rect, sse3


def oracle_qp_frames(lib, w, h, offs, rect, srcs, R, qps, waypoints=(), mode=0, decode=False, deblock=1):
    """one stream through or_compose_dyn, frame f at QP qps[f].  Returns (its
    bytes, per frame a dict: data (the frame's bytes), nal (its dynamic NAL),
    qp, and with decode: rec, sse of the test decoder's picture; None for a
    frame without a dynamic NAL (mode 1: a waypoint NAL replaces it))"""
    lib.or_compose_dyn.restype = ctypes.c_size_t
    cfg = OrCfg()
    lib.or_cfg_init(ctypes.byref(cfg), w, h)
    cfg.frame_num = 2
    cfg.deblock = deblock
    for i, (o, lt, v) in enumerate(waypoints):
        cfg.wp_off[i], cfg.wp_lt[i], cfg.wp_valid[i] = o, lt, v
    cfg.nwp = len(waypoints)
    buf = (ctypes.c_uint8 * (4 << 20))()
    out, frames = bytearray(), []
    for off, src, qp in zip(offs, srcs, qps):
        qp = int(qp)
        rc = Rect(*rect, qp_field(qp))
        sp = np.ascontiguousarray(src, dtype=np.uint8)
        state = OrCfg.from_buffer_copy(cfg)
        seen = []
        fn = TRACE(lambda *a: seen.append(1))
        lib.or_dyn_set_trace(fn)
        try:
            n = lib.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(off), mode, ctypes.byref(rc),
                                   sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), None)
        finally:
            lib.or_dyn_set_trace(None)
        assert n > 0
        data = bytes(buf[:n])
        out += data
        if not seen:
            frames.append(None)
            continue
        nals = split_nals(data)
        fr = dict(data=data, nal=nals[-1], qp=qp)
        if decode:
            if len(nals) == 2:                # the frame's waypoint NAL comes first
                scratch = (ctypes.c_uint8 * (1 << 20))()
                lib.or_waypoint_nal(scratch, len(scratch), ctypes.byref(state), int(off))
            rec = decode_rect(lib, state, R, rc, nals[-1], w, h, int(off), qp)[0]
            fr.update(rec=rec, sse=sse3(sp, rec, rect))
        frames.append(fr)
    return bytes(out), frames


def cost_of(res, qps):
    """bits + len(se(qp - 26)) per candidate of a dyn_probe result [..., nq]"""
    return res["bits"].astype(np.int64) + np.array([se_len(int(q) - 26) for q in qps], np.int64)


def pick_np(res, qps, allow):
    """(k, over) of one frame: the rule of pick_device.h restated.  res: the
    frame's nq candidates; allow: what it may cost"""
    cost = cost_of(res, qps)
    err = [int(e[0]) + int(e[1]) + int(e[2]) for e in res["sse"]]
    fit = [k for k in range(len(qps)) if cost[k] <= allow]
    if fit:
        return min(fit, key=lambda k: (err[k], cost[k], k)), 0
    return min(range(len(qps)), key=lambda k: (cost[k], err[k], k)), 1


def bucket_np(res, qps, has, frame_bits, bucket_bits, level):
    """one stream's frames through the leaky bucket: res [F][nq], has [F].
    Returns (k[F], status[F], level after): status 0 / 1 / 2 as
    scroll_batch_dyn_pick_result"""
    ks, sts = [], []
    cost = cost_of(res, qps)
    for f in range(res.shape[0]):
        allow = min(bucket_bits, level + frame_bits)
        k, st, c = -1, 2, 0
        if has[f]:
            k, st = pick_np(res[f], qps, max(allow, 0))
            c = int(cost[f, k])
        level = max(allow - c, -bucket_bits)
        ks.append(k)
        sts.append(st)
    return ks, sts, level
