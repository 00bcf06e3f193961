"""What the QP probe (scroll_batch_dyn_probe) must report, from the oracle:
per frame and QP the rect MBs' bits and non-zero levels out of
or_compose_dyn's own levels (the or_dyn_set_trace hook), each MB fed back
through or_dyn_mb_levels_bits with its traced neighbours, and the squared
error of what the test decoder decodes from the NAL (reconhelp).  For
tests/test_probe_hostsim.py and tests/test_gpu_probe.py."""
import ctypes

import numpy as np

from dynhelp import OrCfg, Rect, qp_field, split_nals
from reconhelp import decode_rect, sse3

TRACE = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int),
                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int))

PROBE_DTYPE = np.dtype([("sse", np.uint64, 3), ("bits", np.uint32), ("nonzero", np.uint32)])


def se_len(v):
    """bits of se(v)"""
    k = 2 * v - 1 if v > 0 else -2 * v
    return 2 * (k + 1).bit_length() - 1


def rbsp_bits(nal):
    """RBSP bits of an Annex-B NAL before rbsp_stop_one_bit (the NAL header
    byte not counted, emulation prevention removed)"""
    assert nal[:4] == b"\x00\x00\x00\x01"
    body, out, zeros = nal[5:], bytearray(), 0
    for b in body:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    while out and out[-1] == 0:
        out.pop()
    last = out[-1]
    return 8 * (len(out) - 1) + 7 - ((last & -last).bit_length() - 1)


def mb_levels_bits(lib, lv, tcl, tct, al, at):
    """(bits, nonzero) of one MB through or_dyn_mb_levels_bits; lv = (luma
    [16][16], cdc [2][4], cac [2][4][15]) in scan order"""
    luma, cdc, cac = lv
    L = ((ctypes.c_int * 16) * 16)(*[(ctypes.c_int * 16)(*r) for r in luma])
    D = ((ctypes.c_int * 4) * 2)(*[(ctypes.c_int * 4)(*r) for r in cdc])
    A = (((ctypes.c_int * 15) * 4) * 2)(*[((ctypes.c_int * 15) * 4)(*[(ctypes.c_int * 15)(*b) for b in p])
                                           for p in cac])
    buf = (ctypes.c_uint8 * (1 << 14))()
    cbp, tco, nbits = ctypes.c_int(), (ctypes.c_int * 24)(), ctypes.c_size_t()
    lib.or_dyn_mb_levels_bits.restype = ctypes.c_size_t
    lib.or_dyn_mb_levels_bits(buf, len(buf), L, D, A, (ctypes.c_int * 24)(*tcl), (ctypes.c_int * 24)(*tct),
                              int(al), int(at), ctypes.byref(cbp), tco, ctypes.byref(nbits))
    nz = sum(1 for r in luma for v in r if v) + sum(1 for p in cdc for v in p if v) + \
        sum(1 for p in cac for b in p for v in b if v)
    return int(nbits.value), nz, list(tco)


def _read_levels(lp, dp, ap):
    luma = [[lp[16 * r + k] for k in range(16)] for r in range(16)]
    cdc = [[dp[4 * p + k] for k in range(4)] for p in range(2)]
    cac = [[[ap[60 * p + 15 * k + i] for i in range(15)] for k in range(4)] for p in range(2)]
    return luma, cdc, cac


def oracle_probe(lib, w, h, offs, rect, srcs, R, qp, waypoints=(), decode=True, clips=None, mode=0):
    """one stream through or_compose_dyn at QP qp.  Returns (its bytes, per
    frame a dict: bits / nonzero (the traced MBs through
    or_dyn_mb_levels_bits), nal (the dynamic NAL), mbs (the trace), and with
    decode: sse (Y, Cb, Cr of the test decoder's picture), rec, pred); None
    for a frame without a dynamic NAL (mode 1, the experiment's: a waypoint
    NAL replaces the scroll NAL)"""
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
        got = []

        def cb(x, y, bit, lp, dp, ap, tl, tt):
            got.append((x, y, int(bit), _read_levels(lp, dp, ap),
                        [tl[i] for i in range(24)] if tl else [0] * 24,
                        [tt[i] for i in range(24)] if tt else [0] * 24, bool(tl), bool(tt)))

        fn = TRACE(cb)
        lib.or_dyn_set_trace(fn)
        try:
            n = lib.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(off), mode, ctypes.byref(rc),
                                   sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), None)
        finally:
            lib.or_dyn_set_trace(None)
        assert n > 0
        data = bytes(buf[:n])
        out += data
        if mode == 1 and not got:
            frames.append(None)
            continue
        assert len(got) == rect[2] * rect[3]
        nals = split_nals(data)
        if len(nals) == 2:                    # the frame's waypoint NAL comes first
            scratch = (ctypes.c_uint8 * (1 << 20))()
            lib.or_waypoint_nal(scratch, len(scratch), ctypes.byref(state), int(off))
        bits = nz = 0
        for x, y, _, lv, tcl, tct, al, at in got:
            b, z, _ = mb_levels_bits(lib, lv, tcl, tct, al, at)
            bits += b
            nz += z
        fr = dict(bits=bits, nonzero=nz, nal=nals[-1], mbs=got)
        if decode:
            rec, pred = decode_rect(lib, state, R, rc, nals[-1], w, h, int(off), qp, clips)
            fr.update(rec=rec, pred=pred, sse=sse3(sp, rec, rect))
        frames.append(fr)
    return bytes(out), frames


def constant_of(fr, qp):
    """C(frame) of the header's identity: RBSP bits before the stop bit -
    bits(q) - len(se(q - 26))"""
    return rbsp_bits(fr["nal"]) - fr["bits"] - se_len(qp - 26)



def synth(lib, S, F, rect, t0=0):
    """[S][F][384 w h] of the documented synthetic source"""
    from dynhelp import rect_source
    rc = Rect(*rect, 0)
    return np.stack([np.stack([np.frombuffer(bytes(rect_source(lib, s, t0 + t, rc)), np.uint8)
                               for t in range(F)]) for s in range(S)])


def make_batch(gpu, w, h, rect, S, F, R, qps=None, waypoints=(), recon=False, mode=None):
    b = gpu.Batch(S, F, 8 << 20) if mode is None else gpu.Batch(S, F, 8 << 20, mode=mode)
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h, waypoints=waypoints))
    b.set_dyn_rect(*rect)
    for s, q in enumerate(qps or []):
        b.set_dyn_qp(q, stream=s)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon()
    return b


def load(b, offs, src):
    """offsets and source of the frames to probe or compose"""
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])
    return offs.shape[1]
