"""What the hinted QP probe (scroll_batch_dyn_probe_hinted) must report, from
existing yardsticks only: per candidate q the stream is composed by
hreconhelp.oracle_hinted at q (or_compose_hint_dyn), every frame's scroll NAL
is decoded by the test decoder (h264_pslice.decode_p_slice), and each rect
MB's decoded levels go through probehelp.mb_levels_bits
(or_dyn_mb_levels_bits) with the left / top rect MBs' tc_out -- zeros outside
the rect, a neighbour available unless it is off the picture.  sse is sse3
of decode_rect_hinted's picture, skips its P_Skip count.  For
tests/test_hprobe_expect.py and tests/test_gpu_hprobe.py."""
import contextlib

import numpy as np

import h264_pslice as hp
import hreconhelp
from hreconhelp import oracle_hinted
from probehelp import mb_levels_bits, rbsp_bits, se_len
from reconhelp import sse3

_PRED = {}


@contextlib.contextmanager
def _tap(R):
    """while open: decode_p_slice's (nal, mbs) of every call are recorded in
    the list this yields (oracle_hinted decodes each rect frame's scroll NAL
    once, in frame order), and pred2d, which does not depend on the QP, is
    remembered per (config, references, MB, motion) across candidates"""
    calls = []
    dec, pred = hp.decode_p_slice, hreconhelp.pred2d

    def decode(nal, *a, **kw):
        r = dec(nal, *a, **kw)
        calls.append((nal, r[1]))
        return r

    def pred2d(lib, cfg, Rr, ref, mvx, mvy, mbx, mby):
        key = (id(R), bytes(cfg), ref, mvx, mvy, mbx, mby)
        if key not in _PRED:                   # R is kept with the entry: its id stays its own
            _PRED[key] = (R, pred(lib, cfg, Rr, ref, mvx, mvy, mbx, mby))
        return _PRED[key][1]

    hp.decode_p_slice, hreconhelp.pred2d = decode, pred2d
    try:
        yield calls
    finally:
        hp.decode_p_slice, hreconhelp.pred2d = dec, pred


def rect_bits(lib, mbs, pos, rw, rh):
    """(bits, nonzero) of the rw x rh rect at MB pos of a decoded picture"""
    x0, y0 = pos
    zero = [0] * 24
    tcs, bits, nz = {}, 0, 0
    for y in range(y0, y0 + rh):
        for x in range(x0, x0 + rw):
            g = mbs[y][x]
            b, z, tco = mb_levels_bits(lib, (g["luma"], g["cdc"], g["cac"]), tcs.get((x - 1, y), zero),
                                       tcs.get((x, y - 1), zero), x > 0, y > 0)
            tcs[(x, y)] = tco
            bits += b
            nz += z
    return bits, nz


def expect_stream(lib, w, h, offs, plan, rw, rh, srcs, R, qps, waypoints=(), fallback=False, clips=None,
                  bits_for=None):
    """one stream at every candidate.  -> (exp, datas): exp[f][k] = None (no
    rect coded) or dict(bits, nonzero, sse, skips, fell, nal, D, C) at
    qps[k], C = rbsp_bits(nal) - bits - D; datas[k]: the stream's bytes at
    qps[k].  bits_for: the candidate indices whose bits / nonzero are wanted
    (None: all; the others carry sse only)"""
    F = len(offs)
    exp, datas = [[None] * len(qps) for _ in range(F)], []
    for k, q in enumerate(qps):
        with _tap(R) as calls:
            data, frames, _ = oracle_hinted(lib, w, h, offs, plan, rw, rh, srcs, R, qp_of=lambda f, q=q: q,
                                            waypoints=waypoints, fallback=fallback, clips=clips)
        datas.append(data)
        it = iter(calls)
        for f, d in enumerate(frames):
            if d is None:
                continue
            nal, mbs = next(it)
            e = dict(sse=sse3(srcs[f], d["rec"], (0, 0, rw, rh)), skips=d["skips"], fell=d["fell"], nal=nal)
            if bits_for is None or k in bits_for:
                pos = (0, 0) if d["fell"] else plan[f][2]
                e["bits"], e["nonzero"] = rect_bits(lib, mbs, pos, rw, rh)
                e["D"] = se_len(q - 26) - 1 if e["nonzero"] > 0 else 0
                e["C"] = rbsp_bits(nal) - e["bits"] - e["D"]
            exp[f][k] = e
    return exp, datas


def check(res, s, exp, bits_for=None):
    """a Batch.dyn_probe(..., hinted=True) result of stream s against
    expect_stream's exp, integer-exact"""
    for f, per in enumerate(exp):
        for k, e in enumerate(per):
            got = res[s, f, k]
            if e is None:
                assert got["valid"] == 0, (s, f, k)
                continue
            assert got["valid"] == 1, (s, f, k)
            assert tuple(int(v) for v in got["sse"]) == tuple(e["sse"]), (s, f, k, got["sse"], e["sse"])
            if bits_for is None or k in bits_for:
                assert (int(got["bits"]), int(got["nonzero"])) == (e["bits"], e["nonzero"]), \
                    (s, f, k, int(got["bits"]), int(got["nonzero"]), e["bits"], e["nonzero"])


# ---- the two designed cases of tests/test_hprobe_expect.py ----
QPS6 = [0, 12, 22, 26, 39, 51]


def case_a(lib, mode):
    """picture 96x96, rect 2x2 at (0,0), (2,2), (4,4) (frames 0..2), offset
    40, one hint rect"""
    from reconhelp import random_refs
    w, h, rw, rh = 96, 96, 2, 2
    src = np.random.default_rng(3).integers(0, 256, 1536, dtype=np.uint8)
    R = random_refs(w, h, 31)
    plan = [([(0, 2, 6, 4, 1, -16, 8)], mode, pos) for pos in ((0, 0), (2, 2), (4, 4))]
    return dict(w=w, h=h, rw=rw, rh=rh, offs=[40, 40, 40], plan=plan, srcs=[src] * 3, R=R)


def case_b(lib, mode):
    """test_gpu_recon_hint.skip_case's prediction at offset 16 (rect 3x2 at
    (2,2), no hint rects) plus noise of -3..3"""
    from dynhelp import Rect
    from hreconhelp import _put, make_cfg, pred2d
    from reconhelp import _regions, random_refs
    w, h, rw, rh, pos = 96, 96, 3, 2, (2, 2)
    R = random_refs(w, h, 71)
    cfg = make_cfg(lib, w, h)
    a_end, ra, mva, rb, mvb = _regions(cfg, 16)
    pred = bytearray(384 * rw * rh)
    rc = Rect(pos[0], pos[1], rw, rh, 0)
    for y in range(pos[1], pos[1] + rh):
        for x in range(pos[0], pos[0] + rw):
            ref, mv = (ra, mva) if y < a_end else (rb, mvb)
            _put(pred, rc, x, y, *pred2d(lib, cfg, R, ref, 0, mv, x, y))
    noise = np.random.default_rng(9).integers(-3, 4, len(pred))
    src = np.clip(np.frombuffer(bytes(pred), np.uint8).astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return dict(w=w, h=h, rw=rw, rh=rh, offs=[16], plan=[([], mode, pos)], srcs=[src], R=R)


def case_expect(lib, c, qps=QPS6):
    return expect_stream(lib, c["w"], c["h"], c["offs"], c["plan"], c["rw"], c["rh"], c["srcs"], c["R"], qps)
