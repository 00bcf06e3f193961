"""What the QP probe, the device pick and the moved rect must give on the
designed corpus (tests/designed.py), from the oracle only: per case, stream,
frame and candidate QP the numbers of probehelp.oracle_probe (bits, nonzero,
the squared error and the picture of the test decoder, the NAL) plus the
header's constant C, cached per (case, stream, QP) so that the modules that
ask for overlapping candidate lists share the work.  Also the tallies that
prove from those traced levels what the probe's length functions are asked
(reach), and the geometry of the corpus under a moved rect.  For
tests/test_probe_designed.py, tests/test_gpu_probe_designed.py,
tests/test_gpu_hprobe_designed.py and tests/test_gpu_pos_designed.py."""
import re

import numpy as np

import designed as dz
from probehelp import PROBE_DTYPE, constant_of, oracle_probe
from reconhelp import ArrayRefs

BASE_QPS = [0, 12, 21, 22, 26, 39, 51]
MAX_QPS = 8                               # SCROLL_DYN_PROBE_MAX_QPS
_ORDER = [n for n, _ in dz.CASE_GROUPS]


def own_qp(name):
    """the case's QP, from its name (a_walk and a_tzrb: 28); expect() checks it"""
    m = re.search(r"_qp(\d+)$", name)
    return int(m.group(1)) if m else 28


def candidates(name):
    """the case's own QP plus BASE_QPS, de-duplicated, rotated so that the own
    QP is candidate (position of the case in CASE_GROUPS) mod nq: the
    per-candidate registers and LDS slices are indexed by k"""
    own = own_qp(name)
    qps = [own] + [q for q in BASE_QPS if q != own]
    assert len(qps) <= MAX_QPS
    k = _ORDER.index(name) % len(qps)
    return qps[len(qps) - k:] + qps[:len(qps) - k]


def three_of(name):
    """three of candidates(name), the own QP among them at index (position of
    the case) mod 3: what the hinted probe's tests can afford per case"""
    qps = candidates(name)
    k, at = qps.index(own_qp(name)), _ORDER.index(name) % 3
    return [qps[(k - at + i) % len(qps)] for i in range(3)]


_frames = {}


def frames_at(oracle, c, s, qp):
    """oracle_probe's frames of stream s of case c at QP qp, each with C; the
    trace (mbs) is kept at the case's own QP only.  c: a designed.Case (the
    cache is by its name: a local variant of a case carries a name of its own)"""
    key = (c.name, s, qp)
    if key not in _frames:
        fr = oracle_probe(oracle, c.w, c.h, c.offs[s], c.rc, c.src[s], c.R, qp)[1]
        for d in fr:
            d["C"] = constant_of(d, qp)
            if qp != c.qp:
                del d["mbs"]
        _frames[key] = fr
    return _frames[key]


def expect_case(oracle, c, s, qps):
    """[frame][candidate] of frames_at"""
    per = [frames_at(oracle, c, s, q) for q in qps]
    return [[per[k][f] for k in range(len(qps))] for f in range(c.F)]


def expect(oracle, name, s, qps=None):
    """per frame and candidate (candidates(name), or qps) of stream s the dict
    of oracle_probe -- bits, nonzero, sse, nal, rec -- plus C =
    constant_of(frame, qp).  Stream 1 goes through the oracle like stream 0"""
    c = dz.cases(oracle)[name]
    assert c.qp == own_qp(name)
    return expect_case(oracle, c, s, candidates(name) if qps is None else qps)


def as_result(exp):
    """expect()'s [F][nq] of one stream as the structured array a dyn_probe
    result holds (sse, bits, nonzero), for qpfhelp.pick_np / bucket_np"""
    out = np.zeros((len(exp), len(exp[0])), PROBE_DTYPE)
    for f, per in enumerate(exp):
        for k, e in enumerate(per):
            out[f, k] = (e["sse"], e["bits"], e["nonzero"])
    return out


def check_probe(res, s, exp):
    """a Batch.dyn_probe result of stream s against expect()'s, integer-exact,
    every (frame, candidate); every mismatch is listed before the assertion"""
    bad = []
    for f, per in enumerate(exp):
        for k, e in enumerate(per):
            got = res[s, f, k]
            g = (int(got["valid"]), int(got["bits"]), int(got["nonzero"]), tuple(int(v) for v in got["sse"]))
            w = (1, e["bits"], e["nonzero"], tuple(e["sse"]))
            if g != w:
                bad.append((s, f, k, g, w))
    assert not bad, bad


# ------------------------------------------------------------------- reach ----
def blocks_of(mbs):
    """(maxc, coefficients in scan order) of every block of a frame's traced MBs"""
    for _, _, _, (luma, cdc, cac), *_ in mbs:
        for b in luma:
            yield 16, b
        for b in cdc:
            yield 4, b
        for p in cac:
            for b in p:
                yield 15, b


def level_calls(coef):
    """the (levelCode, suffixLength) arguments level_len gets for a block, by
    the standard's rule (9.2.2.1) as probe_device.h's block_len walks it"""
    lv = [v for v in reversed(coef) if v]
    tc, t1 = len(lv), 0
    while t1 < min(3, tc) and abs(lv[t1]) == 1:
        t1 += 1
    sl = 1 if (tc > 10 and t1 < 3) else 0
    out = []
    for i, v in enumerate(lv[t1:]):
        code = 2 * abs(v) - 2 + (v < 0) - (2 if (i == 0 and t1 < 3) else 0)
        out.append((code, sl))
        if sl == 0:
            sl = 1
        if abs(v) > (3 << (sl - 1)) and sl < 6:
            sl += 1
    return out


def escape_class(code, sl):
    """0: level_prefix below 14, 1: prefix 14, 2: prefix 15 (the escape)"""
    if sl == 0:
        return 0 if code < 14 else 1 if code < 30 else 2
    return 2 if code >= (15 << sl) else 1 if (code >> sl) == 14 else 0


def zeros_calls(coef):
    """(TotalCoeff, the zerosLeft values of the block's run_before look-ups),
    as zeros_len walks them; None for an empty block"""
    nz = [k for k, v in enumerate(coef) if v]
    if not nz:
        return None
    tc = len(nz)
    zl, zls = nz[-1] + 1 - tc, []
    hi = list(reversed(nz))
    for a, b in zip(hi, hi[1:]):
        if zl <= 0:
            break
        zls.append(zl)
        zl -= a - b - 1
    return tc, zls


# ------------------------------------------------------------ the moved rect --
class Moved:
    """a corpus case under scroll_batch_set_dyn_rect_moving.  The picture is
    32 pixels wider and 16 taller than the case's; slot d of the references
    (rows 16 (Y0 + rh d) ...) holds the prediction band of designed frame
    d mod F at that slot's own x0: 0 (the left neighbour unavailable), flush
    with the right edge, the corpus origin, in turn.  A case of fewer than
    three frames repeats its frames to three slots (and is that much taller),
    or its single band could sit at one x0 only.  Stream 0 takes the slots in
    order and sits one MB row lower in its odd frames, the offset 16 less (the
    same prediction rows); stream 1 takes them in reverse, is lower in its
    even frames whose offset allows it, and has no rect in frame 1.
      w, h, rw, rh, F, qp, R, offs [2][F], src [2][F], pos [2][F] ((x0, y0) or
      None), slot [2][F] (the designed frame of each stream frame)"""

    def __init__(self, c):
        rw, rh = c.rw, c.rh
        n = max(c.F, 3)
        self.name, self.qp, self.rw, self.rh, self.F = c.name, c.qp, rw, rh, n
        self.w, self.h = c.w + 32, max(64, 16 * (dz.Y0 + rh * n)) + 16
        right = self.w // 16 - rw
        xs = [(0, right, dz.X0)[d % 3] for d in range(n)]
        assert len({0, right, dz.X0}) == 3
        planes = [np.full((self.h, self.w), 128, np.int64), np.full((self.h // 2, self.w // 2), 128, np.int64),
                  np.full((self.h // 2, self.w // 2), 128, np.int64)]
        for d in range(n):
            fr = c.frames[d % c.F]
            y, x = 16 * (dz.Y0 + rh * d), 16 * xs[d]
            planes[0][y:y + 16 * rh, x:x + 16 * rw] = fr.p[0]
            for k in (1, 2):
                planes[k][y // 2:y // 2 + 8 * rh, x // 2:x // 2 + 8 * rw] = fr.p[k]
        self.R = ArrayRefs([tuple(planes), tuple(planes)])
        one = np.stack([c.frames[d % c.F].source() for d in range(n)])
        self.src = np.stack([one, one[::-1]])
        order = [list(range(n)), list(range(n))[::-1]]
        self.slot = [[d % c.F for d in row] for row in order]
        self.offs = np.zeros((2, n), np.int32)
        self.pos = [[None] * n for _ in range(2)]
        for s in range(2):
            for f, d in enumerate(order[s]):
                off = 16 * rh * d
                dy = 1 if (off >= 16 and f % 2 == (1 - s)) else 0
                self.offs[s, f] = off - 16 * dy
                if not (s == 1 and f == 1):
                    self.pos[s][f] = (xs[d], dz.Y0 + dy)
        assert 16 * rh * (n - 1) < 496
        seen = [p for row in self.pos for p in row]
        assert None in seen and (dz.X0, dz.Y0) in seen and any(p and p[0] == 0 for p in seen)
        assert any(p and p[0] == right for p in seen) and any(p and p[1] == dz.Y0 + 1 for p in seen)


_moved = {}


def moved(oracle, name):
    if name not in _moved:
        _moved[name] = Moved(dz.cases(oracle)[name])
    return _moved[name]


MOVED_INT8 = ["a_walk", "a_tzrb", "b_levels_qp22", "c_lengths_qp24", "d_extremes_qp22", "d_epdense_qp22"]
MOVED_GENERAL = ["a_walk_qp20", "e_levels_qp0", "e_extremes_qp0", "e_clamp_qp0"]
HINTED = ["a_walk", "a_tzrb", "a_walk_qp20", "b_levels_qp22", "b_searched_qp22", "c_lengths_qp24", "d_extremes_qp22",
          "d_epdense_qp22", "e_levels_qp0", "e_extremes_qp0", "e_clamp_qp0"]
