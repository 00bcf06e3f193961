"""The designed corpus of the dynamic-rect coders: source rects built from
TARGET LEVELS, for tests/test_designed_oracle.py (which proves from the
oracle's own NALs what the corpus reaches) and tests/test_gpu_designed.py
(which demands the kernels' bytes equal the oracle's).

Construction.  For a 4x4 block choose the levels in scan order and a QP; the
decoder's residual of those levels, hp.idct4x4(hp.dequant4x4(levels, qp)),
is added to the block's prediction.  The prediction of a pixel is 128 where
the residual fits (-128 .. 127), else 0 (residual above) or 255 (below), so a
residual may span -255 .. 255; what does not fit even then is clipped, and the
quantiser then finds other levels than the target -- every condition of the
tests is on what the parser finds in the oracle's NAL, never on the target.

Geometry.  Every frame of a case has a prediction of its own: frame f is
composed at offset 16 rh f (rh = the rect's height in MBs), so its rect rows
predict from reference rows 16 (y0 + rh f) ..., full-pel in luma and chroma,
all in region A.  Reference B is a copy of A.  Stream 1 holds stream 0's
frames in reverse order.  Offsets stay below 496: no waypoints.

Groups: a table walk (QP 28; a20: designed again at QP 20 for
the general path), b level walk, c block-length and accumulator edges,
d extremes, e = b, c, d below QP 22."""
import ctypes
import random

import numpy as np

import h264_pslice as hp
from dynhelp import Rect, qp_field
from reconhelp import ArrayRefs, qpc_of

X0, Y0 = 1, 1                             # the rect's origin in every case (MBs)

# forward core transform and quantiser (8.5 inverse; the JM forward scale),
# used only to PREDICT the levels of candidate pixels while searching
_CF = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], np.int64)
_MF = [(13107, 5243, 8066), (11916, 4660, 7490), (10082, 4194, 6554),
       (9362, 3647, 5825), (8192, 3355, 5243), (7282, 2893, 4559)]
_CLS = np.array([[0 if (i % 2 == 0 and j % 2 == 0) else (1 if (i % 2 and j % 2) else 2)
                  for j in range(4)] for i in range(4)])
LEVEL_MAX = 2063


def predict_levels(res, qp):
    """4x4 residual (array) -> levels in scan order as the forward transform
    and quantiser of the standard's inverse give them"""
    W = _CF @ np.asarray(res, np.int64).reshape(4, 4) @ _CF.T
    qb = 15 + qp // 6
    mf = np.array(_MF[qp % 6])[_CLS]
    z = np.minimum((np.abs(W) * mf + (1 << qb) // 6) >> qb, LEVEL_MAX) * np.sign(W)
    z = z.reshape(16)
    return [int(z[hp.ZZ[k]]) for k in range(16)]


def block_residual(scan, qp, dc=None):
    return np.array(hp.idct4x4(hp.dequant4x4(list(scan), qp, dc=dc)), np.int64).reshape(4, 4)


def chroma_residual(cdc, cac, qpc):
    """8x8 residual of one chroma plane from its DC levels [4] and AC levels [4][15]"""
    c = cdc
    f = [c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3],
         c[0] + c[1] - c[2] - c[3], c[0] - c[1] - c[2] + c[3]]
    dcs = [((v * 16 * hp.V[qpc % 6][0]) << (qpc // 6)) >> 5 for v in f]
    out = np.zeros((8, 8), np.int64)
    for k in range(4):
        bx, by = 4 * (k % 2), 4 * (k // 2)
        out[by:by + 4, bx:bx + 4] = block_residual([0] + list(cac[k]), qpc, dc=dcs[k])
    return out


def split_pred(res):
    """residual -> (prediction, source) with the free prediction rule"""
    res = np.clip(res, -255, 255)
    pred = np.where(res > 127, 0, np.where(res < -128, 255, 128))
    return pred, np.clip(pred + res, 0, 255)


class Frame:
    """the source and prediction planes of one rect frame"""

    def __init__(self, rw, rh):
        self.rw, self.rh = rw, rh
        self.s = [np.full((16 * rh, 16 * rw), 128, np.int64), np.full((8 * rh, 8 * rw), 128, np.int64),
                  np.full((8 * rh, 8 * rw), 128, np.int64)]
        self.p = [a.copy() for a in self.s]
        self.design = {}                  # (mx, my) -> [luma[16][16], cdc[2][4], cac[2][4][15]]

    def _d(self, mx, my):
        return self.design.setdefault((mx, my), [[[0] * 16 for _ in range(16)], [[0] * 4 for _ in range(2)],
                                                 [[[0] * 15 for _ in range(4)] for _ in range(2)]])

    def luma_block(self, mx, my, r, scan, qp):
        """raster block r of MB (mx, my) from levels in scan order"""
        pred, src = split_pred(block_residual(scan, qp))
        y, x = 16 * my + 4 * (r // 4), 16 * mx + 4 * (r % 4)
        self.p[0][y:y + 4, x:x + 4] = pred
        self.s[0][y:y + 4, x:x + 4] = src
        self._d(mx, my)[0][r] = list(scan)

    def chroma(self, mx, my, plane, cdc, cac, qpc):
        pred, src = split_pred(chroma_residual(cdc, cac, qpc))
        y, x = 8 * my, 8 * mx
        self.p[1 + plane][y:y + 8, x:x + 8] = pred
        self.s[1 + plane][y:y + 8, x:x + 8] = src
        d = self._d(mx, my)
        d[1][plane] = list(cdc)
        d[2][plane] = [list(a) for a in cac]

    def luma_residual(self, mx, my, r, res):
        """raster block r of MB (mx, my) from a 4x4 residual within +-255"""
        pred, src = split_pred(np.asarray(res, np.int64).reshape(4, 4))
        y, x = 16 * my + 4 * (r // 4), 16 * mx + 4 * (r % 4)
        self.p[0][y:y + 4, x:x + 4] = pred
        self.s[0][y:y + 4, x:x + 4] = src

    def pixels(self, mx, my, plane, src, pred):
        """an MB's plane given as pixels (16x16 luma, 8x8 chroma arrays)"""
        n = 16 if plane == 0 else 8
        self.s[plane][n * my:n * my + n, n * mx:n * mx + n] = src
        self.p[plane][n * my:n * my + n, n * mx:n * mx + n] = pred

    def source(self):
        return np.concatenate([a.reshape(-1) for a in self.s]).astype(np.uint8)


class Case:
    """name, group, qp, rect, picture, references, sources [S][F][384 rw rh],
    offsets [S][F]; the oracle's streams are made once by want_of"""

    def __init__(self, name, group, qp, frames, exact=False):
        self.name, self.group, self.qp, self.frames, self.exact = name, group, qp, frames, exact
        rw, rh, F = frames[0].rw, frames[0].rh, len(frames)
        assert 16 * rh * (F - 1) < 496
        self.rw, self.rh, self.F = rw, rh, F
        self.w, self.h = max(64, 16 * (X0 + rw)), max(64, 16 * (Y0 + rh * F))
        self.rc = (X0, Y0, rw, rh)
        planes = [np.full((self.h, self.w), 128, np.int64), np.full((self.h // 2, self.w // 2), 128, np.int64),
                  np.full((self.h // 2, self.w // 2), 128, np.int64)]
        for f, fr in enumerate(frames):
            y = 16 * (Y0 + rh * f)
            planes[0][y:y + 16 * rh, 16 * X0:16 * (X0 + rw)] = fr.p[0]
            for k in (1, 2):
                planes[k][y // 2:y // 2 + 8 * rh, 8 * X0:8 * (X0 + rw)] = fr.p[k]
        self.R = ArrayRefs([tuple(planes), tuple(planes)])
        one = np.stack([fr.source() for fr in frames])
        self.src = np.stack([one, one[::-1]])
        o = np.arange(F, dtype=np.int32) * 16 * rh
        self.offs = np.stack([o, o[::-1]])

    def rect(self, qp=None):
        return Rect(*self.rc, qp_field(self.qp if qp is None else qp))


# ------------------------------------------------------------- level helpers --
def place(levels_coding_order, positions, maxc=16):
    """levels in coding order (highest scan position first) at the given
    scan positions -> the block in scan order"""
    pos = sorted(positions, reverse=True)
    assert len(pos) == len(levels_coding_order)
    out = [0] * maxc
    for p, v in zip(pos, levels_coding_order):
        out[p] = v
    return out


def token_block(rng, tc, t1, maxc=16, big=2):
    """TotalCoeff tc with t1 trailing ones at random positions, the other
    levels +-1 / +-big (the first of them +-big where t1 < 3)"""
    lv = [rng.choice((-1, 1)) for _ in range(t1)]
    for i in range(tc - t1):
        m = big if (i == 0 and t1 < 3) else rng.choice((1, big))
        lv.append(rng.choice((-m, m)))
    return place(lv, rng.sample(range(maxc), tc), maxc)


def token_entries(maxc):
    return [(tc, t1) for tc in range(maxc + 1) for t1 in range(min(tc, 3) + 1)]


ESCALATE = [4, 7, 13, 25, 49]           # |level| > 3 << (sl - 1): suffixLength 2, 3, 4, 5, 6


def context_levels(ctx, v, rng):
    """levels in coding order that code v with the context ctx live:
    ("first", t1) suffixLength 0 after t1 trailing ones (t1 < 3: the first-level
    adjustment); ("first11", t1): TotalCoeff 11, suffixLength 1, adjusted;
    ("sl", k): suffixLength k, a later level"""
    sg = lambda m: rng.choice((-m, m))  # noqa: E731
    if ctx[0] == "first":
        return [sg(1) for _ in range(ctx[1])] + [v]
    if ctx[0] == "first11":
        return [sg(1) for _ in range(ctx[1])] + [v] + [sg(1) for _ in range(10 - ctx[1])]
    k = ctx[1]
    if k == 1:
        return [sg(2), v]
    return [sg(m) for m in ESCALATE[:k - 1]] + [v]


CONTEXTS = [("first", 0), ("first", 1), ("first", 2), ("first", 3), ("first11", 0), ("first11", 2)] + \
           [("sl", k) for k in range(1, 7)]


def low_positions(n, maxc=16):
    """the n lowest scan positions: the large levels at the low frequencies"""
    return list(range(n))


# ------------------------------------------------------------------ group a ---
def walk_frame(N, seed, qp=28, rw=16, rh=4):
    """checkerboard of target blocks (every coeff_token entry in turn, random
    positions) among neighbour blocks of TotalCoeff N, luma and chroma AC;
    chroma DC blocks walk TotalCoeff x TrailingOnes x positions"""
    rng = random.Random(seed)
    fr = Frame(rw, rh)
    qpc = qpc_of(qp)
    le, ce = token_entries(16), token_entries(15)
    dcd = [(tc, t1, pos) for tc in range(5) for t1 in range(min(tc, 3) + 1)
           for pos in _subsets(4, tc)]
    il = ic = idc = seed * 7
    for my in range(rh):
        for mx in range(rw):
            for r in range(16):
                if (r % 4 + r // 4) % 2 == 0:
                    tc, t1 = le[il % len(le)]
                    il += 1
                else:
                    tc, t1 = N, min(N, rng.randint(0, 3))
                fr.luma_block(mx, my, r, token_block(rng, tc, t1), qp)
            for p in range(2):
                tc, t1, pos = dcd[idc % len(dcd)]
                idc += 1
                lv = [rng.choice((-1, 1)) for _ in range(t1)]
                lv += [rng.choice((-2, 2)) if (i == 0 and t1 < 3) else rng.choice((-2, -1, 1, 2))
                       for i in range(tc - t1)]
                cdc = place(lv, pos, 4)
                cac = []
                for k in range(4):
                    if (k % 2 + k // 2) % 2 == 0:
                        tc, t1 = ce[ic % len(ce)]
                        ic += 1
                    else:
                        tc, t1 = N, min(N, rng.randint(0, 3))
                    cac.append(token_block(rng, tc, t1, 15))
                fr.chroma(mx, my, p, cdc, cac, qpc)
    return fr


def _subsets(n, k):
    import itertools
    return [list(c) for c in itertools.combinations(range(n), k)]


def tzrb_frame(seed, qp=28, rw=16, rh=2):
    """every total_zeros entry (TotalCoeff tc, the last coefficient behind tz
    zeros -- tc = 1, tz = 15 is the lone coefficient at scan position 15) and
    every run_before entry (zerosLeft zl, run), for 16- and 15-coefficient
    blocks"""
    rng = random.Random(seed)
    fr = Frame(rw, rh)
    qpc = qpc_of(qp)

    def blocks(maxc):
        out = []
        for tc in range(1, maxc):
            for tz in range(maxc - tc + 1):
                pos = list(range(tc - 1)) + [tc + tz - 1]
                out.append(place([rng.choice((-1, 1)) for _ in range(min(tc, 3))] +
                                 [rng.choice((-2, 2)) for _ in range(tc - min(tc, 3))], pos, maxc))
        for zl in range(1, maxc - 1):
            for run in range(zl + 1):
                out.append(place([rng.choice((-1, 1)), rng.choice((-1, 1))], [zl + 1, zl - run], maxc))
        # runs in the middle of longer blocks: zerosLeft falls as the runs are coded
        for _ in range(24):
            tc = rng.randint(3, 8)
            out.append(token_block(rng, tc, rng.randint(0, 3), maxc))
        return out

    lb, cb = blocks(16), blocks(15)
    assert len(lb) <= 16 * rw * rh and len(cb) <= 8 * rw * rh
    for i, b in enumerate(lb):
        m, r = divmod(i, 16)
        fr.luma_block(m % rw, m // rw, r, b, qp)
    cb += [[0] * 15] * (-len(cb) % 4)
    for i in range(0, len(cb), 4):
        m, p = divmod(i // 4, 2)
        fr.chroma(m % rw, m // rw, p, [0, 0, 0, 0], cb[i:i + 4], qpc)
    return fr


# ------------------------------------------------------------------ group b ---
def level_walk_frames(qp, vmax, seed, rw=16, rh=2, step=1, chroma_dc_max=0):
    """per context, blocks that code v = +-1 .. +-vmax (every step-th value and
    every value around the boundaries) with that context live; luma blocks on
    a checkerboard among empty ones (nC 0), the same blocks without their
    lowest position as chroma AC; chroma DC blocks walk to chroma_dc_max"""
    rng = random.Random(seed)
    qpc = qpc_of(qp)
    edges = set()
    for e in (1, 2, 3, 4, 6, 7, 8, 12, 13, 15, 16, 17, 24, 25, 30, 31, 32, 46, 47, 48, 49, 60, 61, 62, 96, 97,
              120, 121, 122, 126, 127, 128, 240, 241, 242, 255, 256, 480, 481, 482, 960, 961, 1632, 2047, 2048):
        edges.add(e)
    vals = sorted(v for v in set(range(1, vmax + 1, step)) | edges | {vmax} if v <= vmax)
    blocks = []
    for ctx in CONTEXTS:
        for m in vals:
            for v in (m, -m):
                if ctx[0] != "sl" and ctx[1] < 3 and m < 2:
                    continue              # a first level of +-1 would be a trailing one
                lv = context_levels(ctx, v, rng)
                blocks.append(place(lv, low_positions(len(lv))))
    per_frame = 8 * rw * rh
    frames = []
    dcv = sorted(set(range(1, chroma_dc_max + 1, max(1, chroma_dc_max // 24))) | {chroma_dc_max}) \
        if chroma_dc_max else []
    idc = 0
    for i in range(0, len(blocks), per_frame):
        fr = Frame(rw, rh)
        chunk = blocks[i:i + per_frame]
        for j, b in enumerate(chunk):
            m, t = divmod(j, 8)
            r = [0, 2, 5, 7, 8, 10, 13, 15][t]
            fr.luma_block(m % rw, m // rw, r, b, qp)
        # chroma AC: the same level strings one position up (no DC position)
        for j in range(0, len(chunk), 4):
            m, p = divmod(j // 4, 2)
            cac = [b[:15] for b in chunk[j:j + 4]]
            cac += [[0] * 15] * (4 - len(cac))
            cdc = [0, 0, 0, 0]
            if dcv:
                n = 1 + idc % 4
                cdc = place([rng.choice((-1, 1)) * dcv[(idc + q) % len(dcv)] for q in range(n)], range(n), 4)
                idc += 1
            fr.chroma(m % rw, m // rw, p, cdc, cac, qpc)
        frames.append(fr)
    return frames


# residual blocks (raster) found by a linear-programming search over sign and
# position choices: at QP 22 they code a level of 113 or more at suffixLength 5
# and of 97 or more at suffixLength 6 (level_prefix 7 and 3, the largest an
# int8 level has there), which no idct of a target within +-255 reaches
SEARCHED_QP22 = [
    [-231, -255, 67, 255, -255, -255, 255, 255, -255, -230, 214, 255, -255, -117, 255, 255],
    [-255, -227, 255, 255, -255, -255, 239, 87, 161, -228, 255, 255, -255, -255, 255, 255],
    [-150, -255, -209, -26, 191, -119, 207, 178, 255, -158, 181, 255, -53, -255, -222, 83],
    [255, -255, -221, 255, 255, -92, -225, 32, 69, 98, 1, -197, -255, 255, 255, -255],
    # +-48, the first level past k_dyn_row's level table, at suffixLength 6
    [255, 107, -255, 255, 78, 255, 255, 255, 255, 168, -239, -255, 255, 255, 185, 255],
]


def searched_frame(rw=3, rh=1):
    fr = Frame(rw, rh)
    for i, res in enumerate(SEARCHED_QP22):
        for k, sign in enumerate((1, -1)):
            fr.luma_residual(k, 0, [0, 2, 5, 7, 8, 10, 13, 15][i], [sign * v for v in res])
            if i < 4:                                 # side by side: nC from the left
                fr.luma_residual(2, 0, 4 * i + 2 * k, [sign * v for v in res])
    return fr


# ------------------------------------------------------------------ group c ---
class OrBits(ctypes.Structure):
    _fields_ = [("buf", ctypes.c_void_p), ("cap", ctypes.c_size_t), ("nbits", ctypes.c_size_t)]


def coded_bits(oracle, coef, maxc, nC=0):
    buf = (ctypes.c_uint8 * 1024)()
    b = OrBits()
    oracle.or_bits_init(ctypes.byref(b), buf, len(buf))
    oracle.or_cavlc_block(ctypes.byref(b), (ctypes.c_int * 16)(*coef), maxc, nC)
    return int(b.nbits)


_TZLEN = {tc: {z: len(code) for code, z in row.items()} for tc, row in hp.TZ.items()}
_RBLEN = {zl: {r: len(code) for code, r in row.items()} for zl, row in hp.RB.items()}


def body_pushes(coef, maxc):
    """the codewords after coeff_token as k_dyn_row's accumulator takes them:
    the trailing-one signs at once, each level, then total_zeros with the
    run_befores as one field -> (the first bit, the bit count after each);
    lengths by the standard's rule (9.2.2.1) and tables (h264_pslice.py)"""
    nz = [k for k, v in enumerate(coef) if v]
    tc = len(nz)
    if tc == 0:
        return 0, []
    lv = [coef[k] for k in reversed(nz)]
    t1 = 0
    while t1 < min(3, tc) and abs(lv[t1]) == 1:
        t1 += 1
    sums, n, first = [t1], t1, (1 if lv[0] < 0 else 0) if t1 else None
    sl = 1 if (tc > 10 and t1 < 3) else 0
    for i, v in enumerate(lv[t1:]):
        code = 2 * abs(v) - 2 + (v < 0) - (2 if (i == 0 and t1 < 3) else 0)
        if code >= (15 << sl if sl else 30):
            ln = 28
        elif sl == 0 and code >= 14:
            ln = 19
        else:
            ln = (code >> sl) + 1 + sl
        if first is None:
            first = 1 if (code >> sl) == 0 else 0     # level_prefix 0: the codeword starts with its one
        n += ln
        sums.append(n)
        if sl == 0:
            sl = 1
        if abs(v) > (3 << (sl - 1)) and sl < 6:
            sl += 1
    tz = nz[-1] + 1 - tc
    ln = _TZLEN[tc][tz] if tc < maxc else 0
    zl = tz
    for hi, lo in zip(reversed(nz), list(reversed(nz))[1:]):
        if zl <= 0:
            break
        ln += _RBLEN[min(zl, 7)][hi - lo - 1]
        zl -= hi - lo - 1
    sums.append(n + ln)
    return first, sums


def accumulator_edge(coef, maxc):
    """64, 65 or 66 when the block's first bit after coeff_token is a one and a
    codeword brings k_dyn_row's 64-bit accumulator, not yet spilled, to
    exactly that many bits; else None"""
    first, sums = body_pushes(coef, maxc)
    if first != 1:
        return None
    for a, b in zip(sums, sums[1:]):
        if b > 63:
            return b if (a <= 64 and b in (64, 65, 66) and b > a) else None
    return None


LENGTH_TARGETS = [60, 62, 63, 64, 65, 66, 67, 70, 120, 124, 126, 127, 128, 129, 130, 131, 134, 140]


def length_frames(oracle, qp, seed, rw=8, rh=2):
    """blocks whose coded length (nC 0: the neighbours are empty) is each of
    LENGTH_TARGETS after the pixel round trip, 16 coefficients (luma) and 15
    (chroma AC); found by a seeded random search with or_cavlc_block's count"""
    rng = random.Random(seed)
    qpc = qpc_of(qp)
    found = {16: {}, 15: {}}
    scale = max(1, int(round(2 ** ((28 - qp) / 6.0))))
    for maxc, q in ((16, qp), (15, qpc)):
        want = {(t, k) for t in LENGTH_TARGETS for k in range(3 if t in (64, 65, 128, 129) else 1)}
        if qp >= 22:
            want |= {(-e, k) for e in (64, 65, 66) for k in range(3)}    # accumulator edges, as -64 ...
        for it in range(5000):
            if not want:
                break
            tc = rng.randint(6, maxc)
            top = rng.choice((3, 6, 12, 20)) * scale
            lv = sorted((rng.randint(1, top) for _ in range(tc)))
            lv = [rng.choice((-1, 1)) * m for m in lv]
            if it % 2:
                lv[0] = -1                            # a trailing one whose sign bit is a one
            blk = place(lv, rng.sample(range(maxc), tc), maxc)
            scan = blk if maxc == 16 else [0] + blk
            pred, src = split_pred(block_residual(scan, q))
            got = predict_levels(src - pred, q)
            got = got if maxc == 16 else got[1:]
            n = coded_bits(oracle, got, maxc)
            e = accumulator_edge(got, maxc)
            for k in range(3):
                if e and (-e, k) in want:
                    want.discard((-e, k))
                    found[maxc][(-e, k)] = blk
                    break
            for k in range(3):
                if (n, k) in want:
                    want.discard((n, k))
                    found[maxc][(n, k)] = blk
                    break
    lb = [found[16][k] for k in sorted(found[16])]
    cb = [found[15][k] for k in sorted(found[15])]
    fr = Frame(rw, rh)
    for j, b in enumerate(lb):
        m, t = divmod(j, 8)
        fr.luma_block(m % rw, m // rw, [0, 2, 5, 7, 8, 10, 13, 15][t], b, qp)
    for j in range(0, len(cb), 2):
        m, p = divmod(j // 2, 2)
        cac = [[0] * 15 for _ in range(4)]
        cac[0] = cb[j]
        if j + 1 < len(cb):
            cac[3] = cb[j + 1]
        fr.chroma(m % rw, m // rw, p, [0, 0, 0, 0], cac, qpc)
    return [fr]


# ------------------------------------------------------------------ group d ---
def checker(n, pitch, phase=0):
    i, j = np.indices((n, n))
    return (((i // pitch + j // pitch + phase) % 2) * 255).astype(np.int64)


def extreme_frames(seed, rw=4, rh=2):
    """[saturated and checkerboard MBs, an all-zero rect, the same with the
    colours swapped, the MB of the most bits this construction gives]"""
    rng = np.random.default_rng(seed)
    frames = []
    for sign in (0, 1):
        fr = Frame(rw, rh)
        hi, lo = (255, 0) if sign == 0 else (0, 255)
        flat = lambda n, v: np.full((n, n), v, np.int64)  # noqa: E731
        # MB 0: everything saturated; 1: luma only; 2: chroma only; 3: Cr only with Cb inverted
        for mx, planes in ((0, (0, 1, 2)), (1, (0,)), (2, (1, 2)), (3, (2,))):
            for p in planes:
                n = 16 if p == 0 else 8
                fr.pixels(mx, 0, p, flat(n, hi), flat(n, lo))
        fr.pixels(3, 0, 1, flat(8, lo), flat(8, hi))
        # second row: +-255 checkerboards at pixel, 2-pixel and 4-pixel pitch, luma and chroma;
        # the last MB: chroma whose 4x4 blocks alternate in sign (chroma DC positions 1, 2, 3)
        for mx, pitch in ((0, 1), (1, 2), (2, 4)):
            for p in range(3):
                n = 16 if p == 0 else 8
                c = checker(n, pitch, sign)
                fr.pixels(mx, 1, p, c, 255 - c)
        for p, pat in ((1, [[0, 1], [0, 1]]), (2, [[0, 0], [1, 1]])):
            c = np.kron(np.array(pat) ^ sign, np.ones((4, 4), np.int64)) * 255
            fr.pixels(3, 1, p, c, 255 - c)
        c = np.kron(np.array([[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0], [1, 0, 0, 1]]) ^ sign,
                    np.ones((4, 4), np.int64)) * 255
        fr.pixels(3, 1, 0, c, 255 - c)
        frames.append(fr)
        if sign == 0:
            frames.append(Frame(rw, rh))              # source = prediction: every MB cbp 0
    # candidates for the largest MB: random 0 / 255 pixels over their inverse
    fr = Frame(rw, rh)
    for my in range(rh):
        for mx in range(rw):
            for p in range(3):
                n = 16 if p == 0 else 8
                c = rng.integers(0, 2, (n, n)) * 255
                if (mx + my) % 2:                     # over black and white halves: large and mixed
                    fr.pixels(mx, my, p, c, 255 - c)
                else:
                    fr.pixels(mx, my, p, rng.integers(0, 256, (n, n)), 255 - c)
    frames.append(fr)
    return frames


def epdense_frames(qp, rw=4, rh=2):
    """emulation-prevention bytes by design: levels that sit exactly on the
    level_prefix 15 escape of their suffixLength (17, 31, 61, 121 in coding
    order) have an all-zero 12-bit suffix, so each is 15 zero bits, a one and
    12 zero bits, and two in a row give 27 zero bits.  Every chroma DC block
    holds four of them, every other luma block three"""
    frames = []
    qpc = qpc_of(qp)
    for sign in (1, -1, 0):
        fr = Frame(rw, rh)
        for my in range(rh):
            for mx in range(rw):
                sg = sign or (1 if (mx + my) % 2 else -1)
                for p in range(2):
                    fr.chroma(mx, my, p, [121 * sg, 61 * sg, 31 * sg, 17 * sg], [[0] * 15] * 4, qpc)
                for r in (0, 2, 5, 7, 8, 10, 13, 15):
                    fr.luma_block(mx, my, r, [61 * sg, 31 * sg, 17 * sg] + [0] * 13, qp)
        frames.append(fr)
    return frames


def clamp_frames(rw=4, rh=1):
    """white and black chroma over black and white references with the 4x4
    blocks' signs in each 2x2 Hadamard pattern: at QPc 0-5 the chroma DC level
    meets the clamp in each of the four positions, both signs, and mixed"""
    frames = []
    pats = [[[0, 0], [0, 0]], [[0, 1], [0, 1]], [[0, 0], [1, 1]], [[0, 1], [1, 0]]]
    for sign in (0, 1):
        fr = Frame(rw, rh)
        for mx in range(rw):
            for p in (1, 2):
                pat = np.array(pats[(mx + (p - 1)) % 4]) ^ sign ^ (p - 1)
                c = np.kron(pat, np.ones((4, 4), np.int64)) * 255
                fr.pixels(mx, 0, p, c, 255 - c)
            c = checker(16, 4, sign) if mx % 2 else np.full((16, 16), 255 * (1 - sign), np.int64)
            fr.pixels(mx, 0, 0, c, 255 - c)
        frames.append(fr)
    # three positions at once: blocks (+, +, +, -) give |F| = 8160 in every position
    fr = Frame(rw, rh)
    for mx in range(rw):
        for p in (1, 2):
            pat = np.zeros((2, 2), np.int64)
            pat[divmod((mx + p) % 4, 2)] = 1
            c = np.kron(pat ^ (mx & 1), np.ones((4, 4), np.int64)) * 255
            fr.pixels(mx, 0, p, c, 255 - c)
    frames.append(fr)
    return frames


# ------------------------------------------------------------------ corpus ----
_cases = None


def cases(oracle):
    """name -> Case; built once"""
    global _cases
    if _cases is None:
        cs = []
        walk = [walk_frame(N, 1 + i) for i, N in enumerate((0, 3, 6, 12))]
        cs.append(Case("a_walk", "a", 28, walk, exact=True))
        cs.append(Case("a_tzrb", "a", 28, [tzrb_frame(5)], exact=True))
        cs.append(Case("a_walk_qp20", "a20", 20, [walk_frame(N, 1 + i, qp=20) for i, N in enumerate((0, 3, 6, 12))],
                       exact=True))
        cs.append(Case("a_tzrb_qp20", "a20", 20, [tzrb_frame(5, qp=20)], exact=True))
        cs.append(Case("b_levels_qp22", "b", 22, level_walk_frames(22, 127, 11, chroma_dc_max=255)))
        cs.append(Case("b_levels_qp24", "b", 24, level_walk_frames(24, 100, 12, step=3, chroma_dc_max=200)))
        cs.append(Case("b_searched_qp22", "b", 22, [searched_frame()]))
        cs.append(Case("c_lengths_qp24", "c", 24, length_frames(oracle, 24, 21)))
        cs.append(Case("c_lengths_qp34", "c", 34, length_frames(oracle, 34, 22)))
        ext = extreme_frames(31)
        for qp in (22, 23, 24, 25, 26, 27):
            cs.append(Case(f"d_extremes_qp{qp}", "d", qp, ext))
        cs.append(Case("d_epdense_qp22", "d", 22, epdense_frames(22)))
        cs.append(Case("e_epdense_qp12", "e", 12, epdense_frames(12)))
        cs.append(Case("e_levels_qp0", "e", 0, level_walk_frames(0, 1632, 41, step=29, chroma_dc_max=2063)))
        cs.append(Case("e_levels_qp10", "e", 10, level_walk_frames(10, 500, 42, step=11, chroma_dc_max=1000)))
        cs.append(Case("e_levels_qp21", "e", 21, level_walk_frames(21, 145, 43, step=2, chroma_dc_max=290)))
        cs.append(Case("e_lengths_qp0", "e", 0, length_frames(oracle, 0, 51)))
        cs.append(Case("e_lengths_qp12", "e", 12, length_frames(oracle, 12, 52)))
        for qp in (0, 5, 12, 21):
            cs.append(Case(f"e_extremes_qp{qp}", "e", qp, ext))
        clamp = clamp_frames()
        for qp in (0, 1, 2, 3, 4, 5):
            cs.append(Case(f"e_clamp_qp{qp}", "e", qp, clamp))
        assert [(c.name, c.group) for c in cs] == CASE_GROUPS
        _cases = {c.name: c for c in cs}
    return _cases


def names(*groups):
    """case names of the groups, without building anything (for parametrize)"""
    return [n for n, g in CASE_GROUPS if g in groups]


CASE_GROUPS = [("a_walk", "a"), ("a_tzrb", "a"), ("a_walk_qp20", "a20"), ("a_tzrb_qp20", "a20"),
               ("b_levels_qp22", "b"), ("b_levels_qp24", "b"), ("b_searched_qp22", "b"), ("c_lengths_qp24", "c"),
               ("c_lengths_qp34", "c")] + [(f"d_extremes_qp{q}", "d") for q in range(22, 28)] + \
              [("d_epdense_qp22", "d"), ("e_epdense_qp12", "e")] + \
              [("e_levels_qp0", "e"), ("e_levels_qp10", "e"), ("e_levels_qp21", "e"), ("e_lengths_qp0", "e"),
               ("e_lengths_qp12", "e")] + [(f"e_extremes_qp{q}", "e") for q in (0, 5, 12, 21)] + \
              [(f"e_clamp_qp{q}", "e") for q in range(6)]

_want = {}


def want_of(oracle, name, qp=None):
    """the oracle's streams of a case (at another QP than its own: qp), made once"""
    from test_gpu_dyn import oracle_streams
    key = (name, qp)
    if key not in _want:
        c = cases(oracle)[name]
        _want[key] = oracle_streams(oracle, c.w, c.h, c.offs, c.rect(qp), c.src, c.R)
    return _want[key]
