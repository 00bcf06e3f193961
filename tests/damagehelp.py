"""The damage map and the placement rule of scroll_batch_dyn_locate, restated
in numpy from their definition (include/composer_batch.h) --
not from csrc/damage_device.h, which the tests check against this.

  Ysrc   cschelp.luma_np on the surface pixel;
  Ypred  the luma of the frame's scroll NAL, sampled pixel by pixel through
         the oracle's or_ref_sample with reconhelp._regions, the way
         reconhelp._pred samples luma: independent of luma_row();
  D      per MB the sum of (Ysrc - Ypred)^2;
  rule   damaged iff D > mb_sse; the bounding box grown by margin and clipped;
         NONE / FIT / OVER / NOFRAME; sse_all, sse_out, max_sse.

Device memory through ctypes HIP, as tests/test_gpu_surface.py (its small Hip
/ Surfaces helpers restated here).  For tests/test_damage_hostsim.py and
tests/test_gpu_damage.py."""
import ctypes

import numpy as np

from cschelp import luma_np, rgb_of
from dynhelp import OrCfg, split_nals
from reconhelp import _regions

NONE, FIT, OVER, NOFRAME = 0, 1, 2, 3
DAMAGE_DTYPE = np.dtype([("x0", np.int16), ("y0", np.int16), ("bx0", np.uint16), ("by0", np.uint16),
                         ("bx1", np.uint16), ("by1", np.uint16), ("status", np.uint16), ("reserved", np.uint16),
                         ("n_mb", np.uint32), ("max_sse", np.uint32), ("sse_all", np.uint64), ("sse_out", np.uint64)])
assert DAMAGE_DTYPE.itemsize == 40
PAD = 0xFF


# ---------------------------------------------------------------- the rule
def locate_np(dmap, w, h, mb_sse=0, margin=0):
    """one frame's record (a dict of DAMAGE_DTYPE's fields) from its [mbh][mbw]
    map, for a w x h rect; dmap None: a frame without a scroll NAL"""
    r = dict(x0=-1, y0=-1, bx0=0, by0=0, bx1=0, by1=0, status=NOFRAME, reserved=0, n_mb=0, max_sse=0, sse_all=0,
             sse_out=0)
    if dmap is None:
        return r
    m = np.asarray(dmap).astype(np.int64)
    mbh, mbw = m.shape
    r["sse_all"] = r["sse_out"] = int(m.sum())
    r["max_sse"] = int(m.max())
    ys, xs = np.nonzero(m > mb_sse)
    r["n_mb"] = len(xs)
    r["status"] = NONE
    if len(xs) == 0:
        return r
    bx0, by0 = max(int(xs.min()) - margin, 0), max(int(ys.min()) - margin, 0)
    bx1, by1 = min(int(xs.max()) + 1 + margin, mbw), min(int(ys.max()) + 1 + margin, mbh)
    r.update(bx0=bx0, by0=by0, bx1=bx1, by1=by1)
    r["status"] = FIT if bx1 - bx0 <= w and by1 - by0 <= h else OVER
    x0, y0 = min(bx0, mbw - w), min(by0, mbh - h)
    r.update(x0=x0, y0=y0)
    r["sse_out"] = r["sse_all"] - int(m[y0:y0 + h, x0:x0 + w].sum())
    return r


def record_tuple(r):
    """a dict of locate_np or a numpy record -> a plain tuple in DAMAGE_DTYPE's order"""
    return tuple(int(r[n]) for n in DAMAGE_DTYPE.names)


def position(r):
    """(x0, y0) or None"""
    return None if int(r["x0"]) < 0 else (int(r["x0"]), int(r["y0"]))


# ----------------------------------------------------------------- the map
def frame_states(lib, w, h, offs, mode=0, waypoints=(), deblock=1):
    """one stream composed by the scroll oracle (or_compose, the rect off):
    per frame the config its scroll NAL was written with (the waypoint its
    own waypoint NAL added included), or None for a frame without a scroll
    NAL (experiment mode: the waypoint NAL replaced it)"""
    lib.or_compose.restype = ctypes.c_size_t
    cfg = OrCfg()
    lib.or_cfg_init(ctypes.byref(cfg), w, h)
    cfg.frame_num = 2
    cfg.deblock = deblock
    for i, (o, lt, v) in enumerate(waypoints):
        cfg.wp_off[i], cfg.wp_lt[i], cfg.wp_valid[i] = o, lt, v
    cfg.nwp = len(waypoints)
    buf = (ctypes.c_uint8 * (4 << 20))()
    out = []
    for off in offs:
        state = OrCfg.from_buffer_copy(cfg)
        n = lib.or_compose(buf, len(buf), ctypes.byref(cfg), int(off), mode, None)
        assert n > 0
        nals = split_nals(bytes(buf[:n]))
        wp = cfg.nwp > state.nwp                   # the frame wrote a waypoint NAL
        assert len(nals) == (2 if wp and mode == 0 else 1)
        if wp and mode == 1:
            out.append(None)
            continue
        if wp:
            scratch = (ctypes.c_uint8 * (1 << 20))()
            lib.or_waypoint_nal(scratch, len(scratch), ctypes.byref(state), int(off))
        out.append(state)
    return out


def ypred(lib, state, R, off):
    """[h][w] uint8: the luma a decoder shows for the residual-free scroll
    frame at offset off written with config `state`"""
    a_end, ra, mva, rb, mvb = _regions(state, int(off))
    w, h = state.w, state.h
    cp, rp = ctypes.byref(state), ctypes.byref(R.refs)
    out = np.empty((h, w), np.uint8)
    f = lib.or_ref_sample
    for y in range(h):
        ref, mv = (ra, mva) if y // 16 < a_end else (rb, mvb)
        out[y] = [f(cp, rp, ref, 0, x, y + mv) for x in range(w)]
    return out


def ypred_frames(lib, w, h, offs, R, mode=0):
    """per frame of one stream: its ypred, or None (no scroll NAL)"""
    return [None if st is None else ypred(lib, st, R, off)
            for st, off in zip(frame_states(lib, w, h, offs, mode), offs)]


def damage_map_np(img, yp, fmt, matrix, full):
    """[h][w][4] u8 surface against [h][w] prediction -> [mbh][mbw] uint32;
    yp None: zeroes"""
    h, w = img.shape[:2]
    if yp is None:
        return np.zeros((h // 16, w // 16), np.uint32)
    d = luma_np(*rgb_of(img, fmt), matrix, full) - yp.astype(np.int64)
    return (d * d).reshape(h // 16, 16, w // 16, 16).sum(axis=(1, 3)).astype(np.uint32)


def grey_surface(yp, fmt, rng):
    """the surface whose full-range luma is exactly yp: R = G = B = v (the
    table's luma row sums to 65536), alpha random"""
    img = np.empty(yp.shape + (4,), np.uint8)
    img[..., :3] = yp[..., None]
    img[..., 3] = rng.integers(0, 256, yp.shape)
    return img


def paint(img, mbs, rng):
    """random pixels over the listed MBs [(mx, my), ...], each guaranteed to differ from what was there"""
    for mx, my in mbs:
        blk = img[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
        blk[..., :3] = (blk[..., :3].astype(np.int64) + rng.integers(64, 192, blk[..., :3].shape)) % 256
    return img


# ------------------------------------------------------------ device memory
class Hip:
    """Device buffers through the HIP runtime libh264scroll itself links"""

    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so.7")
        L = self.lib
        L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        L.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        L.hipFree.argtypes = [ctypes.c_void_p]
        for f in (L.hipMalloc, L.hipMemcpy, L.hipMemset, L.hipFree, L.hipDeviceSynchronize):
            f.restype = ctypes.c_int

    def alloc(self, n):
        p = ctypes.c_void_p()
        assert self.lib.hipMalloc(ctypes.byref(p), n) == 0
        return p.value

    def free(self, p):
        self.lib.hipFree(p)

    def fill(self, p, value, n):
        assert self.lib.hipMemset(p, value, n) == 0
        assert self.lib.hipDeviceSynchronize() == 0

    def write(self, p, data):
        a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0         # host -> device

    def read(self, p, n):
        host = np.empty(n, np.uint8)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(host.ctypes.data, p, n, 2) == 0             # device -> host
        return host


class Surfaces:
    """img [S][F][ph][pw][4] (or [1][F]... with shared=True: every stream
    reads the same) laid out at the given pitch and strides in one host image
    (every other byte PAD), uploaded to the device"""

    def __init__(self, hip, img, pitch=None, fstride=None, sstride=None, shared=False):
        self.hip, self.img = hip, img
        ns, F, ph, pw = img.shape[:4]
        self.pitch = pitch or 4 * pw
        self.fstride = fstride if fstride is not None else self.pitch * ph
        self.sstride = 0 if shared else (sstride if sstride is not None else self.fstride * F)
        assert not shared or ns == 1
        self.bytes = (ns - 1) * self.sstride + (F - 1) * self.fstride + (ph - 1) * self.pitch + 4 * pw
        mem = np.full(self.bytes, PAD, np.uint8)
        for s in range(ns):
            for f in range(F):
                at = s * self.sstride + f * self.fstride
                rows = np.lib.stride_tricks.as_strided(mem[at:], (ph, 4 * pw), (self.pitch, 1))
                rows[:] = img[s, f].reshape(ph, 4 * pw)
        self.p = hip.alloc(self.bytes)
        hip.write(self.p, mem)

    def args(self):
        """(ptr, pitch, frame_stride, stream_stride) as Batch.dyn_locate takes them after nframes"""
        return self.pitch, self.fstride, self.sstride

    def free(self):
        self.hip.free(self.p)
