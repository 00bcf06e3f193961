"""The per-MB source mask of scroll_batch_dyn_mask, restated in numpy from its
definition (include/composer_batch.h) -- not from
csrc/mask_device.h, which the tests check against this.

  pred   the rect's prediction in the source layout, sampled pixel by pixel
         through the oracle's or_ref_sample (reconhelp._pred over
         reconhelp._regions): independent of k_dyn_rows / RowPred;
  map    per rect MB Dy (256 luma samples) and Dc (64 Cb + 64 Cr) of
         (src - pred)^2, Dcb apart for the record;
  rule   changed iff Dy > mb_sse_y or Dc > mb_sse_c; kept iff a changed MB
         lies within grow MBs in both directions;
  fill   the source of every MB not kept replaced by its prediction;
  record n_changed, n_kept, sse_drop[Y, Cb, Cr] over the MBs not kept.

For tests/test_mask_hostsim.py and tests/test_gpu_mask.py."""
import ctypes

import numpy as np

from dynhelp import OrCfg, Rect, qp_field, split_nals
from reconhelp import _pred, _put, _regions

OK, NOFRAME = 0, 1
KEPT = 0x80000000
MASK_DTYPE = np.dtype([("status", np.int32), ("n_changed", np.uint32), ("n_kept", np.uint32),
                       ("reserved", np.uint32), ("sse_drop", np.uint64, 3)])
assert MASK_DTYPE.itemsize == 40


# ----------------------------------------------------------- the prediction
def pred_rect(lib, state, R, rect, off):
    """uint8 [384 w h]: what a decoder predicts for the MBs of rect = (x0, y0,
    w, h) of the scroll frame at offset off written with config `state`"""
    rc = Rect(*rect, 0)
    a_end, ra, mva, rb, mvb = _regions(state, int(off))
    buf = bytearray(384 * rc.w * rc.h)
    for y in range(rc.y0, rc.y0 + rc.h):
        ref, mv = (ra, mva) if y < a_end else (rb, mvb)
        for x in range(rc.x0, rc.x0 + rc.w):
            _put(buf, rc, x, y, *_pred(lib, state, R, ref, mv, x, y))
    return np.frombuffer(bytes(buf), np.uint8).copy()


def scroll_nals(lib, w, h, offs, rect, srcs, R, qp=26, waypoints=()):
    """one stream through or_compose_dyn, as reconhelp.oracle_frames composes
    it: every frame's scroll NAL (the last NAL of the frame: a waypoint NAL
    comes before it)"""
    lib.or_compose_dyn.restype = ctypes.c_size_t
    rc = Rect(*rect, qp_field(qp))
    cfg = OrCfg()
    lib.or_cfg_init(ctypes.byref(cfg), w, h)
    cfg.frame_num = 2
    for i, (o, lt, v) in enumerate(waypoints):
        cfg.wp_off[i], cfg.wp_lt[i], cfg.wp_valid[i] = o, lt, v
    cfg.nwp = len(waypoints)
    buf = (ctypes.c_uint8 * (4 << 20))()
    out = []
    for off, src in zip(offs, srcs):
        sp = np.ascontiguousarray(src, dtype=np.uint8)
        n = lib.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(off), 0, ctypes.byref(rc),
                               sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), None)
        assert n > 0
        out.append(split_nals(bytes(buf[:n]))[-1])
    return out


# ------------------------------------------------------------ layout access
def planes(buf, w, h):
    """the three planes of a rect-layout buffer as [16 h][16 w], [8 h][8 w] x 2 views"""
    b = np.asarray(buf)
    n = w * h
    return (b[:256 * n].reshape(16 * h, 16 * w), b[256 * n:320 * n].reshape(8 * h, 8 * w),
            b[320 * n:384 * n].reshape(8 * h, 8 * w))


def _mb_sums(d, h, w, k):
    return d.reshape(h, k, w, k).sum(axis=(1, 3))


# ----------------------------------------------------------------- the map
def mask_map_np(src, pred, w, h):
    """(map uint32 [h][w][2] = { Dy, Dc }, Dcb [h][w]) of a source against its prediction"""
    d = [(s.astype(np.int64) - p.astype(np.int64)) ** 2 for s, p in zip(planes(src, w, h), planes(pred, w, h))]
    dy, dcb, dcr = _mb_sums(d[0], h, w, 16), _mb_sums(d[1], h, w, 8), _mb_sums(d[2], h, w, 8)
    return np.stack([dy, dcb + dcr], axis=-1).astype(np.uint32), dcb.astype(np.uint32)


# ---------------------------------------------------------------- the rule
def rule_np(m, mb_sse_y=0, mb_sse_c=0, grow=0):
    """(changed, kept) boolean [h][w] of a map (KEPT bits ignored)"""
    m = np.asarray(m).astype(np.int64)
    changed = (m[..., 0] > mb_sse_y) | ((m[..., 1] & 0x7FFFFFFF) > mb_sse_c)
    h, w = changed.shape
    kept = np.zeros_like(changed)
    for y in range(h):
        for x in range(w):
            kept[y, x] = changed[max(y - grow, 0):y + grow + 1, max(x - grow, 0):x + grow + 1].any()
    return changed, kept


def record_np(m, dcb, mb_sse_y=0, mb_sse_c=0, grow=0):
    """(record dict, map with the KEPT bits set) of one frame; m None: no dynamic NAL"""
    if m is None:
        return dict(status=NOFRAME, n_changed=0, n_kept=0, reserved=0, sse_drop=(0, 0, 0)), None
    changed, kept = rule_np(m, mb_sse_y, mb_sse_c, grow)
    mm = np.asarray(m).astype(np.int64)
    dc = mm[..., 1] & 0x7FFFFFFF
    cb = np.asarray(dcb).astype(np.int64)
    drop = ~kept
    out = np.stack([mm[..., 0], dc | np.where(kept, KEPT, 0)], axis=-1).astype(np.uint32)
    return dict(status=OK, n_changed=int(changed.sum()), n_kept=int(kept.sum()), reserved=0,
                sse_drop=(int(mm[..., 0][drop].sum()), int(cb[drop].sum()), int((dc - cb)[drop].sum()))), out


def record_tuple(r):
    """a dict of record_np or a numpy record -> a plain tuple in MASK_DTYPE's order"""
    return (int(r["status"]), int(r["n_changed"]), int(r["n_kept"]), int(r["reserved"]),
            tuple(int(v) for v in r["sse_drop"]))


# ---------------------------------------------------------------- the fill
def doctor(src, pred, kept, w, h):
    """the source with every MB not kept replaced by its prediction"""
    out = np.array(src, dtype=np.uint8, copy=True)
    for o, p, k in zip(planes(out, w, h), planes(pred, w, h), (16, 8, 8)):
        sel = np.repeat(np.repeat(~np.asarray(kept), k, axis=0), k, axis=1)
        o[sel] = p[sel]
    return out


def mask_np(src, pred, w, h, mb_sse_y=0, mb_sse_c=0, grow=0):
    """(map with KEPT bits, record, kept, doctored source) of one frame"""
    m, dcb = mask_map_np(src, pred, w, h)
    rec, mk = record_np(m, dcb, mb_sse_y, mb_sse_c, grow)
    kept = (mk[..., 1] & KEPT) != 0
    return mk, rec, kept, doctor(src, pred, kept, w, h)


# ------------------------------------------------------------ test sources
def noisy(pred, rng, amp=1):
    """the prediction plus noise of -amp .. amp on every sample, clipped"""
    n = rng.integers(-amp, amp + 1, pred.shape)
    return np.clip(pred.astype(np.int64) + n, 0, 255).astype(np.uint8)


def paint_mbs(src, mbs, w, h, rng):
    """random samples over the listed rect MBs [(mx, my), ...] (all three planes), each differing from what was there"""
    for pl, k in zip(planes(src, w, h), (16, 8, 8)):
        for mx, my in mbs:
            blk = pl[k * my:k * my + k, k * mx:k * mx + k]
            blk[:] = (blk.astype(np.int64) + rng.integers(64, 192, blk.shape)) % 256
    return src
