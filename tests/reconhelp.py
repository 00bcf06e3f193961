"""The expected reconstruction of the dynamic rect, for tests/test_recon_hostsim.py
and tests/test_gpu_recon.py: what the test decoder (tests/h264_pslice.py
parse_p_slice + reconstruct_mb) decodes from the emitted NAL, with the
prediction sampled through the oracle's or_ref_sample -- the way
tests/test_dyn_oracle.py::test_dyn_rect_qp_decodes does it (_pred, _regions
and _QPC are its helpers)."""
import ctypes

import numpy as np

import h264_pslice as hp
from dynhelp import OrCfg, Pic, Rect, Refs, StripedRefs, qp_field, split_nals

# Table 8-15 (chroma_qp_index_offset 0): QPc for QP 30..51
_QPC = [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]


def qpc_of(qp):
    return qp if qp < 30 else _QPC[qp - 30]


def _pred(lib, cfg, R, ref, mv, mbx, mby):
    py = [[lib.or_ref_sample(ctypes.byref(cfg), ctypes.byref(R.refs), ref, 0, 16 * mbx + j, 16 * mby + i + mv)
           for j in range(16)] for i in range(16)]
    pc = []
    for p in (1, 2):
        q = 4 * mv
        o, f = q >> 3, q & 7
        rows = []
        for i in range(8):
            row = []
            for j in range(8):
                X, Y = 8 * mbx + j, 8 * mby + i
                a = lib.or_ref_sample(ctypes.byref(cfg), ctypes.byref(R.refs), ref, p, X, Y + o)
                b = lib.or_ref_sample(ctypes.byref(cfg), ctypes.byref(R.refs), ref, p, X, Y + o + 1)
                row.append(((8 - f) * a + f * b + 4) >> 3)
            rows.append(row)
        pc.append(rows)
    return py, pc[0], pc[1]


def _regions(cfg, off):
    """(a_end, ra, mva, rb, mvb) of a scroll frame, src/h264_writer.c:555-588"""
    h = cfg.h
    wa, woa, wb, wob = -1, 0, -1, 0
    if off > 496 and cfg.nwp > 0:
        for i in range(cfg.nwp):
            wo = cfg.wp_off[i]
            if cfg.wp_valid[i] and wo <= off and wo > woa and off - wo <= 496:
                wa, woa = i, wo
    if off - h < -496 and cfg.nwp > 0:
        for i in range(cfg.nwp):
            wo = cfg.wp_off[i]
            if cfg.wp_valid[i] and wo > off and off - wo >= -496:
                wb, wob = i, wo
                break
    ra, mva = (2 + wa, off - woa) if wa >= 0 else (0, off)
    rb, mvb = (2 + wb, off - wob) if wb >= 0 else (1, off - h)
    return (h - off) // 16, ra, mva, rb, mvb


class ArrayRefs:
    """Reference pictures A, B from numpy planes (I420 bytes for the GPU,
    or_refs for the oracle)."""

    def __init__(self, planes):               # planes: [(y, u, v), (y, u, v)] uint8 arrays
        self.planes = [tuple(np.ascontiguousarray(p, dtype=np.uint8) for p in pic) for pic in planes]
        h, w = self.planes[0][0].shape
        self.pics = [Pic(w, h, p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data)
                     for p in self.planes]
        self.refs = Refs()
        self.refs.ab[0] = ctypes.pointer(self.pics[0])
        self.refs.ab[1] = ctypes.pointer(self.pics[1])

    def i420(self, k):
        return b"".join(p.tobytes() for p in self.planes[k])


def random_refs(w, h, seed):
    rng = np.random.default_rng(seed)
    return ArrayRefs([(rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h // 2, w // 2)),
                       rng.integers(0, 256, (h // 2, w // 2))) for _ in range(2)])


def striped_refs(oracle, w, h):
    sr = StripedRefs(oracle, w, h)
    return ArrayRefs([(np.frombuffer(bytes(y), np.uint8).reshape(h, w),
                       np.frombuffer(bytes(u), np.uint8).reshape(h // 2, w // 2),
                       np.frombuffer(bytes(v), np.uint8).reshape(h // 2, w // 2)) for y, u, v in sr.planes])


def _put(buf, rc, x, y, ry, ru, rv):
    """one MB's 16x16 / 8x8 / 8x8 rows into a rect-layout buffer (384 w h)"""
    lw, cw = 16 * rc.w, 8 * rc.w
    lx, ly = 16 * (x - rc.x0), 16 * (y - rc.y0)
    for i in range(16):
        buf[(ly + i) * lw + lx:(ly + i) * lw + lx + 16] = bytes(ry[i])
    cbase = lw * 16 * rc.h
    for p, rr in enumerate((ru, rv)):
        base = cbase + p * cw * 8 * rc.h
        for i in range(8):
            at = base + (8 * (y - rc.y0) + i) * cw + 8 * (x - rc.x0)
            buf[at:at + 8] = bytes(rr[i])


def count_clips(luma, cdc, cac, py, pu, pv, qp, qpc):
    """(below 0, above 255): samples of one MB whose prediction + residual
    the decoder clips, from the decoder's own dequant4x4 / idct4x4"""
    lo = hi = 0

    def tally(res, pred, bx, by):
        nonlocal lo, hi
        for i in range(4):
            for j in range(4):
                v = pred[by + i][bx + j] + res[4 * i + j]
                lo += v < 0
                hi += v > 255

    for r in range(16):
        tally(hp.idct4x4(hp.dequant4x4(luma[r], qp)), py, 4 * (r % 4), 4 * (r // 4))
    for p, pred in enumerate((pu, pv)):
        c = cdc[p]
        f = [c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3],
             c[0] + c[1] - c[2] - c[3], c[0] - c[1] - c[2] + c[3]]
        dcs = [((v * 16 * hp.V[qpc % 6][0]) << (qpc // 6)) >> 5 for v in f]
        for k in range(4):
            tally(hp.idct4x4(hp.dequant4x4([0] + cac[p][k], qpc, dc=dcs[k])), pred, 4 * (k % 2), 4 * (k // 2))
    return lo, hi


def decode_rect(lib, state, R, rc, nal, w, h, off, qp, clips=None):
    """(decoded rect, its prediction), both in the source layout, of scroll
    NAL `nal` at offset off; state: the config the NAL was written with;
    clips: a [below 0, above 255] tally of clipped samples to add to"""
    a_end, ra, mva, rb, mvb = _regions(state, off)
    got = {}

    def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
        if rc.x0 <= x < rc.x0 + rc.w and rc.y0 <= y < rc.y0 + rc.h:
            got[(x, y)] = (luma, cdc, cac)

    H, nmb = hp.parse_p_slice(nal, w, h, on_mb=on_mb)
    assert H["qp_delta"] == qp - 26 and nmb == (w // 16) * (h // 16)
    assert len(got) == rc.w * rc.h
    rec = bytearray(384 * rc.w * rc.h)
    pred = bytearray(384 * rc.w * rc.h)
    for (x, y), (luma, cdc, cac) in got.items():
        mv = mva if y < a_end else mvb
        ref = ra if y < a_end else rb
        py, pu, pv = _pred(lib, state, R, ref, mv, x, y)
        ry, ru, rv = hp.reconstruct_mb(luma, cdc, cac, py, pu, pv, qp=qp, qpc=qpc_of(qp))
        _put(rec, rc, x, y, ry, ru, rv)
        _put(pred, rc, x, y, py, pu, pv)
        if clips is not None:
            lo, hi = count_clips(luma, cdc, cac, py, pu, pv, qp, qpc_of(qp))
            clips[0] += lo
            clips[1] += hi
    return bytes(rec), bytes(pred)


def oracle_frames(lib, w, h, offs, rect, srcs, R, qp=26, waypoints=(), clips=None):
    """one stream through or_compose_dyn: (its bytes, per frame the (decoded
    rect, prediction) of decode_rect).  offs: the frames' offsets, srcs: their
    source rects (uint8 arrays of 384 w h), rect = (x0, y0, w, h)"""
    lib.or_compose_dyn.restype = ctypes.c_size_t
    rc = Rect(*rect, qp_field(qp))
    cfg = OrCfg()
    lib.or_cfg_init(ctypes.byref(cfg), w, h)
    cfg.frame_num = 2
    for i, (o, lt, v) in enumerate(waypoints):
        cfg.wp_off[i], cfg.wp_lt[i], cfg.wp_valid[i] = o, lt, v
    cfg.nwp = len(waypoints)
    buf = (ctypes.c_uint8 * (4 << 20))()
    out, frames = bytearray(), []
    for off, src in zip(offs, srcs):
        sp = np.ascontiguousarray(src, dtype=np.uint8)
        state = OrCfg.from_buffer_copy(cfg)
        n = lib.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(off), 0, ctypes.byref(rc),
                               sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), None)
        assert n > 0
        data = bytes(buf[:n])
        out += data
        nals = split_nals(data)
        if len(nals) == 2:                    # the frame's waypoint NAL comes first
            scratch = (ctypes.c_uint8 * (1 << 20))()
            lib.or_waypoint_nal(scratch, len(scratch), ctypes.byref(state), int(off))
        frames.append(decode_rect(lib, state, R, rc, nals[-1], w, h, int(off), qp, clips))
    return bytes(out), frames


def sse3(src, rec, rect):
    """(Y, Cb, Cr) sums of squared errors of two rect-layout buffers"""
    a = np.frombuffer(bytes(src), np.uint8).astype(np.int64)
    b = np.frombuffer(bytes(rec), np.uint8).astype(np.int64)
    n = rect[2] * rect[3]
    d = (a - b) ** 2
    return int(d[:256 * n].sum()), int(d[256 * n:320 * n].sum()), int(d[320 * n:].sum())
