"""The plain dynamic rect sized per stream and per frame
(scroll_batch_set_dyn_rect_size_at), from the oracle.  Prediction is from the
static pictures only, so a frame's NAL depends on nothing but its own rect
{x0, y0, w_f, h_f, qp}, its own source and the stream's state; the expected
stream of a sized compose is therefore DEFINED as

  per stream, one or_compose_dyn call per frame on one or_cfg, with that
  frame's rect and its source in the sized layout (or_dyn_source's for a
  w_f x h_f rect: luma 16 h_f rows of 16 w_f bytes, then Cb, Cr at 8 w_f x
  8 h_f -- the head of the frame's slot);
  a frame without a rect: the scroll oracle's call (or_compose).

Also the numpy restatement of the locate's size rule.  For
tests/test_dyn_size_oracle.py, tests/test_dyn_size_hostsim.py and
tests/test_gpu_dyn_size.py."""
import ctypes

import numpy as np

from dynhelp import OrCfg, Rect, qp_field


def sized_stream(lib, w, h, offs, rects, srcs, R, qps=None, waypoints=(), mode=0, deblock=1):
    """one stream; rects[f] = (x0, y0, w_f, h_f) or None, srcs[f] = the
    frame's slot (its first 384 w_f h_f bytes are read), qps[f] its QP (None:
    26).  Returns (the stream's bytes, the frames' bytes)"""
    lib.or_compose_dyn.restype = ctypes.c_size_t
    lib.or_compose.restype = ctypes.c_size_t
    cfg = OrCfg()
    lib.or_cfg_init(ctypes.byref(cfg), w, h)
    cfg.frame_num = 2
    cfg.deblock = deblock
    for i, (o, lt, v) in enumerate(waypoints):
        cfg.wp_off[i], cfg.wp_lt[i], cfg.wp_valid[i] = o, lt, v
    cfg.nwp = len(waypoints)
    buf = (ctypes.c_uint8 * (4 << 20))()
    frames = []
    for f, off in enumerate(offs):
        rc = rects[f]
        if rc is None:
            n = lib.or_compose(buf, len(buf), ctypes.byref(cfg), int(off), mode, None)
        else:
            r = Rect(*rc, qp_field(int(qps[f])) if qps is not None else 0)
            sp = np.ascontiguousarray(np.asarray(srcs[f], dtype=np.uint8)[:384 * rc[2] * rc[3]])
            n = lib.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(off), mode, ctypes.byref(r),
                                   sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), None)
        assert n > 0
        frames.append(bytes(buf[:n]))
    return b"".join(frames), frames


def sized_streams(lib, w, h, offs, rects, srcs, R, qps=None, mode=0):
    """rects[s][f], srcs[s][f], qps[s][f] -> the streams' bytes"""
    return [sized_stream(lib, w, h, offs[s], rects[s], srcs[s], R, None if qps is None else qps[s], mode=mode)[0]
            for s in range(len(rects))]


def per_rect(fn, rects):
    """fn((x0, y0, w_f, h_f)) -> a list with one entry per frame (an oracle
    helper's frames with that rect in every frame).  Returns entry f of the
    run with rects[f]; None for a frame without a rect"""
    runs, out = {}, []
    for f, rc in enumerate(rects):
        if rc is None:
            out.append(None)
            continue
        if rc not in runs:
            runs[rc] = fn(tuple(rc))
        out.append(runs[rc][f])
    return out


# ---- the locate's size rule (damage_device.h: place with size = 1) ----

def sized_place(box, w, h, mbw, mbh):
    """box = (bx0, by0, bx1, by1), the damaged MBs' box after the margin.
    Returns (x0, y0, w_f, h_f): the placed origin rule, then from that origin
    to the box's end or to the batch size"""
    bx0, by0, bx1, by1 = box
    x0, y0 = min(bx0, mbw - w), min(by0, mbh - h)
    return x0, y0, min(bx1, x0 + w) - x0, min(by1, y0 + h) - y0


def size_word(wf, hf):
    """the record's reserved word under size = 1"""
    return (wf - 1) | (hf - 1) << 8


def table_word(x0, y0, w, h, wf, hf):
    """the position table's entry (DynGeom.dpos) of a sized frame"""
    return x0 | (w - wf) << 8 | y0 << 16 | (h - hf) << 24


def locate_sized_np(dmap, w, h, mb_sse, margin):
    """damagehelp.locate_np with size = 1: the same record, its reserved word
    the size, sse_out summed outside the sized rect.  Returns (record dict,
    (x0, y0, w_f, h_f) or None)"""
    from damagehelp import FIT, OVER, locate_np
    mbh, mbw = dmap.shape
    r = dict(locate_np(dmap, w, h, mb_sse, margin))
    if r["status"] not in (FIT, OVER):
        return r, None
    x0, y0, wf, hf = sized_place((r["bx0"], r["by0"], r["bx1"], r["by1"]), w, h, mbw, mbh)
    assert (x0, y0) == (r["x0"], r["y0"])
    r["reserved"] = size_word(wf, hf)
    r["sse_out"] = int(dmap.astype(np.uint64).sum()) - int(dmap[y0:y0 + hf, x0:x0 + wf].astype(np.uint64).sum())
    return r, (x0, y0, wf, hf)
