"""The plain dynamic rect placed per stream and per frame
(scroll_batch_set_dyn_rect_moving), from the oracle.  Prediction is from the
static pictures only, so nothing of a frame's NAL depends on where the rect
sat in the frames before it; the expected stream of a moving-rect compose is
therefore DEFINED frame by frame:

  frame f with its rect at (x, y):  the bytes frame f has in the run of
      or_compose_dyn over the same stream (offsets, sources, QPs) with the
      uniform rect at (x, y);
  frame f without a rect:           the bytes frame f has in the scroll
      oracle's run (or_compose, the rect off);

a frame's bytes being its waypoint NAL, where it has one (the same in every
run), and its scroll NAL.  oracle_moving assembles that, literally: one
whole-stream run per distinct position.  per_position does the same
selection on what the other oracle helpers return per frame (qpfhelp's
decoded rects, probehelp's bit counts).  For tests/test_dyn_pos_oracle.py and
tests/test_gpu_dyn_pos.py."""
import ctypes

import numpy as np

from dynhelp import OrCfg, Rect, qp_field


def _cfg(lib, w, h, waypoints, deblock):
    cfg = OrCfg()
    lib.or_cfg_init(ctypes.byref(cfg), w, h)
    cfg.frame_num = 2
    cfg.deblock = deblock
    for i, (o, lt, v) in enumerate(waypoints):
        cfg.wp_off[i], cfg.wp_lt[i], cfg.wp_valid[i] = o, lt, v
    cfg.nwp = len(waypoints)
    return cfg


def uniform_run(lib, w, h, offs, rect, srcs, R, qps=None, waypoints=(), mode=0, deblock=1):
    """one stream with the rect (x0, y0, w, h) in every frame, frame f at QP
    qps[f] (None: 26); rect None: the scroll oracle, the rect off.  Returns
    the frames' bytes, one entry per frame"""
    lib.or_compose_dyn.restype = ctypes.c_size_t
    lib.or_compose.restype = ctypes.c_size_t
    cfg = _cfg(lib, w, h, waypoints, deblock)
    buf = (ctypes.c_uint8 * (4 << 20))()
    out = []
    for f, off in enumerate(offs):
        if rect is None:
            n = lib.or_compose(buf, len(buf), ctypes.byref(cfg), int(off), mode, None)
        else:
            rc = Rect(*rect, qp_field(int(qps[f])) if qps is not None else 0)
            sp = np.ascontiguousarray(srcs[f], dtype=np.uint8)
            n = lib.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(off), mode, ctypes.byref(rc),
                                   sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), None)
        assert n > 0
        out.append(bytes(buf[:n]))
    return out


def oracle_moving(lib, w, h, offs, rw, rh, pos, srcs, R, qps=None, waypoints=(), mode=0, deblock=1):
    """one stream, frame f with its rw x rh rect at pos[f] = (x0, y0), or
    without one (pos[f] None).  Returns (its bytes, the frames' bytes)"""
    assert len(pos) == len(offs)
    runs = {}
    for p in pos:
        if p not in runs:
            runs[p] = uniform_run(lib, w, h, offs, None if p is None else (p[0], p[1], rw, rh), srcs, R, qps,
                                  waypoints, mode, deblock)
    frames = [runs[p][f] for f, p in enumerate(pos)]
    return b"".join(frames), frames


def per_position(fn, pos, rw, rh):
    """fn((x0, y0, rw, rh)) -> a list with one entry per frame (an oracle
    helper's frames at that uniform rect).  Returns entry f of the run at
    pos[f]; None for a frame without a rect"""
    runs = {}
    out = []
    for f, p in enumerate(pos):
        if p is None:
            out.append(None)
            continue
        if p not in runs:
            runs[p] = fn((p[0], p[1], rw, rh))
        out.append(runs[p][f])
    return out
