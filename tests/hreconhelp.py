"""The expected reconstruction of the dynamic rect under UI hints, for
tests/test_hrecon_hostsim.py and tests/test_gpu_recon_hint.py: what the test
decoder (tests/h264_pslice.py decode_p_slice + reconstruct_mb) makes of the
emitted NAL, every rect MB predicted at ITS decoded motion through the
oracle's or_ref_sample -- full-pel luma, 2-D 1/8-pel chroma (pred2d restates
tests/test_hintdyn_oracle.py::_pred)."""
import ctypes

import numpy as np

import h264_pslice as hp
from dynhelp import OrCfg, Rect, hint_array, qp_field, split_nals
from reconhelp import _put, count_clips, qpc_of

EXACT, PSKIP, SPEC = 0, 1, 2


def pred2d(lib, cfg, R, ref, mvx, mvy, mbx, mby):
    """(py, pu, pv) rows of MB (mbx, mby) predicted from reference ref at
    (mvx, mvy) pixels; or_ref_sample clamps to the picture"""
    s = lambda p, x, y: lib.or_ref_sample(ctypes.byref(cfg), ctypes.byref(R.refs), ref, p, x, y)  # noqa: E731
    py = [[s(0, 16 * mbx + j + mvx, 16 * mby + i + mvy) for j in range(16)] for i in range(16)]
    qx, qy = 4 * mvx, 4 * mvy
    fx, fy = qx & 7, qy & 7
    pc = []
    for p in (1, 2):
        rows = []
        for i in range(8):
            row = []
            for j in range(8):
                xi, yi = 8 * mbx + j + (qx >> 3), 8 * mby + i + (qy >> 3)
                A, B = s(p, xi, yi), s(p, xi + 1, yi)
                C, D = s(p, xi, yi + 1), s(p, xi + 1, yi + 1)
                row.append(((8 - fx) * (8 - fy) * A + fx * (8 - fy) * B + (8 - fx) * fy * C
                            + fx * fy * D + 32) >> 6)
            rows.append(row)
        pc.append(rows)
    return py, pc[0], pc[1]


def make_cfg(lib, w, h, waypoints=()):
    c = OrCfg()
    lib.or_cfg_init(ctypes.byref(c), w, h)
    c.frame_num = 2
    for i, (o, lt, v) in enumerate(waypoints):
        c.wp_off[i], c.wp_lt[i], c.wp_valid[i] = o, lt, v
    c.nwp = len(waypoints)
    return c


def decode_rect_hinted(lib, state, R, rc, nal, w, h, mode, clips=None):
    """rect rc of scroll NAL `nal` (written with config `state` in hint mode
    `mode`) -> dict(rec, pred: rect-layout bytes; motion: [(ref, mvx, mvy)]
    of the rect's MBs in raster order; skips: its P_Skip MBs; qps: the QPs of
    its MBs with a residual)"""
    _, mbs = hp.decode_p_slice(nal, w, h, "ref" if mode == EXACT else "spec")
    rec = bytearray(384 * rc.w * rc.h)
    pred = bytearray(384 * rc.w * rc.h)
    motion, skips, qps = [], 0, set()
    for y in range(rc.y0, rc.y0 + rc.h):
        for x in range(rc.x0, rc.x0 + rc.w):
            g = mbs[y][x]
            assert g["mx"] % 4 == 0 and g["my"] % 4 == 0
            ref, mvx, mvy = g["ref"], g["mx"] // 4, g["my"] // 4
            motion.append((ref, mvx, mvy))
            skips += bool(g["skip"])
            py, pu, pv = pred2d(lib, state, R, ref, mvx, mvy, x, y)
            qp = g["qp"]
            if g["cbp"]:
                qps.add(qp)
            ry, ru, rv = hp.reconstruct_mb(g["luma"], g["cdc"], g["cac"], py, pu, pv, qp=qp, qpc=qpc_of(qp))
            _put(rec, rc, x, y, ry, ru, rv)
            _put(pred, rc, x, y, py, pu, pv)
            if clips is not None:
                lo, hi = count_clips(g["luma"], g["cdc"], g["cac"], py, pu, pv, qp, qpc_of(qp))
                clips[0] += lo
                clips[1] += hi
    return dict(rec=bytes(rec), pred=bytes(pred), motion=motion, skips=skips, qps=qps)


def oracle_hinted(lib, w, h, offs, plan, rw, rh, srcs, R, qp_of=None, waypoints=(), fallback=False,
                  clips=None):
    """one stream through or_compose_hint_dyn.  plan[f] = (hint rects, hint
    mode, rect origin or None); srcs[f]: the frame's source (uint8, 384 rw rh);
    qp_of(f): its rect QP.  fallback: a frame the oracle refuses (a hint on a
    missing reference) is the whole-picture frame without hint rects instead.
    -> (its bytes, per frame None (no rect coded) or decode_rect_hinted's dict
    + fell, the cfg after the last frame)"""
    lib.or_compose_hint_dyn.restype = ctypes.c_size_t
    cfg = make_cfg(lib, w, h, waypoints)
    buf = (ctypes.c_uint8 * (4 << 20))()
    err = ctypes.c_int()
    out, frames = bytearray(), []
    for f, off in enumerate(offs):
        rects, mode, pos = plan[f]
        qp = qp_of(f) if qp_of else 26
        rc = Rect(pos[0], pos[1], rw, rh, qp_field(qp) if qp != 26 else 0) if pos else None
        arr, n = hint_array(rects)
        sp = np.ascontiguousarray(srcs[f], dtype=np.uint8)
        state = OrCfg.from_buffer_copy(cfg)
        c2 = OrCfg.from_buffer_copy(cfg)
        k = lib.or_compose_hint_dyn(buf, len(buf), ctypes.byref(c2), int(off), 0, arr, n, mode,
                                    ctypes.byref(rc) if rc else None, sp.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(R.refs), ctypes.byref(err))
        fell = False
        if err.value != 0 and fallback:
            fell = True
            rc = Rect(0, 0, rw, rh, qp_field(qp) if qp != 26 else 0)
            c2 = OrCfg.from_buffer_copy(cfg)
            k = lib.or_compose_hint_dyn(buf, len(buf), ctypes.byref(c2), int(off), 0, None, 0, mode,
                                        ctypes.byref(rc), sp.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(R.refs), ctypes.byref(err))
        assert err.value == 0 and k > 0, (f, err.value)
        cfg = c2
        data = bytes(buf[:k])
        out += data
        nals = split_nals(data)
        if len(nals) == 2:                    # the frame's waypoint NAL comes first
            scratch = (ctypes.c_uint8 * (1 << 20))()
            lib.or_waypoint_nal(scratch, len(scratch), ctypes.byref(state), int(off))
        if rc is None:
            frames.append(None)
        else:
            d = decode_rect_hinted(lib, state, R, rc, nals[-1], w, h, mode, clips)
            d["fell"] = fell
            frames.append(d)
    return bytes(out), frames, cfg
