"""The designed corpus of the pre-encoded MB splice: external pictures written
MB by MB from an explicit description (or_ext_slice_script, oracle/
splice_oracle.h), for tests/test_splice_designed_oracle.py (which proves from
the parsed slices and composed NALs what the corpus reaches) and
tests/test_gpu_splice_designed.py (which demands the kernels' bytes equal the
oracle's).

Blocks are given as coefficients in scan order, so no quantiser sits between
the design and the bits: every designed block comes back exactly.

Every picture is rendered in up to three slice shapes, one per parse route:
  "one"   one slice                        -> k_splice_parse
  "rows"  one slice per MB row (>= 4 rows) -> k_splice_lanes
  "two"   one slice per two MB rows (>= 4) -> the lanes hand back, k_splice_parse
so pictures are 8 MB rows high.  A case is a 256x256 or 320x256 stream; frame
t of stream s splices picture t in shape s.

Groups: w table walk, r re-coded tokens, z total_zeros and
run_before, l levels, n lengths and phases, i intra pieces, m motion, q QP
chain, e emulation prevention."""
import ctypes
import random

import designed as dz
from dynhelp import OrCfg, ExtParams, EXT_DEFAULT

SKIP, P16, P16X8, P8X16, P8X8, P8X8REF0, I4, I16, PCM = range(9)
SHAPES = ("one", "rows", "two")
MAX_MV = 16383
ERR_SYNTAX = 4


class ExtMb(ctypes.Structure):
    """or_ext_mb (oracle/splice_oracle.h)"""
    _fields_ = [("kind", ctypes.c_int), ("sub", ctypes.c_int * 4), ("ref", ctypes.c_int * 4),
                ("mvx", ctypes.c_int * 16), ("mvy", ctypes.c_int * 16), ("cbp", ctypes.c_int),
                ("qp", ctypes.c_int), ("imode", ctypes.c_int * 16), ("cmode", ctypes.c_int),
                ("coef", (ctypes.c_int * 16) * 27), ("pcm", ctypes.c_uint8 * 384)]


def cfg_of(oracle, w, h, frame_num=2):
    c = OrCfg()
    oracle.or_cfg_init(ctypes.byref(c), w, h)
    c.frame_num = frame_num
    return c


# ----------------------------------------------------------- MB descriptions --
def cbp_of(coef, i16=False):
    """coded_block_pattern of the pieces {piece: coefficients}"""
    cbp = 0
    for r in range(16):
        if any(coef.get(r, ())):
            cbp |= 15 if i16 else 1 << (2 * (r // 8) + (r % 4) // 2)
    if any(any(coef.get(i, ())) for i in range(18, 26)):
        cbp |= 32
    elif any(coef.get(16, ())) or any(coef.get(17, ())):
        cbp |= 16
    return cbp


def skip():
    return dict(kind=SKIP)


def inter(kind=P16, ref=(0, 0, 0, 0), mv=((0, 0),), sub=(0, 0, 0, 0), coef=None, cbp=None, qp=26):
    coef = coef or {}
    return dict(kind=kind, ref=tuple(ref), mv=list(mv), sub=tuple(sub), coef=coef,
                cbp=cbp_of(coef) if cbp is None else cbp, qp=qp)


def i16(coef=None, cbp=None, qp=26, mode=1, cmode=1):
    """I_16x16 predicting from the left MB only (mode 1, chroma mode 1), which
    every slice shape leaves in place away from the picture's left column"""
    coef = coef or {}
    return dict(kind=I16, imode=[mode] * 16, cmode=cmode, coef=coef,
                cbp=cbp_of(coef, True) if cbp is None else cbp, qp=qp)


def i4(coef=None, cbp=None, qp=26, modes=None, cmode=0):
    coef = coef or {}
    return dict(kind=I4, imode=list(modes or [2] * 16), cmode=cmode, coef=coef,
                cbp=cbp_of(coef) if cbp is None else cbp, qp=qp)


def pcm(samples):
    return dict(kind=PCM, pcm=bytes(samples))


class Pic:
    """an external picture of W x H MBs (mbs: raster), spliced at MB `at`;
    hdr: or_ext_params header fields; status: the oracle's refusal, or 0"""

    def __init__(self, W, H, mbs, at=(2, 2), status=0, **hdr):
        assert len(mbs) == W * H
        self.W, self.H, self.mbs, self.at, self.status, self.hdr = W, H, mbs, at, status, hdr
        self._nal = {}

    def firsts(self, shape):
        if shape == "one":
            return []
        return [y * self.W for y in range(1 if shape == "rows" else 2, self.H, 1 if shape == "rows" else 2)]

    def mb(self, x, y):
        return self.mbs[y * self.W + x]

    def nal(self, oracle, shape):
        if shape not in self._nal:
            arr = (ExtMb * len(self.mbs))()
            for e, d in zip(arr, self.mbs):
                e.kind = d["kind"]
                if d["kind"] == PCM:
                    e.pcm[:] = d["pcm"]
                    continue
                if d["kind"] == SKIP:
                    continue
                e.cbp, e.qp = d["cbp"], d["qp"]
                if d["kind"] >= I4:
                    e.imode[:] = d["imode"]
                    e.cmode = d["cmode"]
                else:
                    e.sub[:] = d["sub"]
                    e.ref[:] = d["ref"]
                    for k, (vx, vy) in enumerate(d["mv"]):
                        e.mvx[k], e.mvy[k] = vx, vy
                for i, c in d["coef"].items():
                    e.coef[i][:len(c)] = list(c)
            p = ExtParams(**{**EXT_DEFAULT, "nrefs": 2, **self.hdr})
            fs = self.firsts(shape)
            cap = 4096 + len(self.mbs) * 8192
            buf = (ctypes.c_uint8 * cap)()
            c = cfg_of(oracle, 256, 256)
            n = oracle.or_ext_slice_script(buf, cap, ctypes.byref(c), self.W, self.H, ctypes.byref(p), arr,
                                           (ctypes.c_int * max(1, len(fs)))(*fs), len(fs))
            assert 0 < n < cap
            self._nal[shape] = bytes(buf[:n])
        return self._nal[shape]


class Case:
    def __init__(self, name, group, pics, w=256, h=256, shapes=SHAPES, offs=None, modes=(0, 1, 2)):
        self.name, self.group, self.pics, self.w, self.h = name, group, pics, w, h
        self.shapes, self.modes = shapes, modes
        self.offs = offs or [40 + 3 * t for t in range(len(pics))]
        for p in pics:
            assert p.W <= 12 and p.H <= 8 and p.at[0] + p.W <= w // 16 and p.at[1] + p.H <= h // 16

    def n_mbs(self):
        return sum(p.W * p.H for p in self.pics) * len(self.shapes)


# ------------------------------------------------------------------ builders --
W12, H8 = 12, 8


def _tb(rng, tc, maxc=16):
    return dz.token_block(rng, tc, min(tc, rng.randint(0, 3)), maxc)


def _mv_of(m):
    return ((m * 7) % 33 - 16, (m * 5) % 17 - 8)


def walk_pic(N, seed, at, W=12, H=8):
    """group w: checkerboard of target blocks (every coeff_token entry in turn)
    among neighbour blocks of TotalCoeff N, luma and chroma AC, chroma DC blocks
    walking TotalCoeff x TrailingOnes x positions (designed.walk_frame as
    coefficients); every MB P_L0_16x16 with cbp 47"""
    rng = random.Random(seed)
    le, ce = dz.token_entries(16), dz.token_entries(15)
    dcd = [(tc, t1, pos) for tc in range(5) for t1 in range(min(tc, 3) + 1) for pos in dz._subsets(4, tc)]
    il = ic = idc = seed * 7
    mbs = []
    for m in range(W * H):
        coef = {}
        for r in range(16):
            if (r % 4 + r // 4) % 2 == 0:
                tc, t1 = le[il % len(le)]
                il += 1
            else:
                tc, t1 = N, min(N, rng.randint(0, 3))
            coef[r] = dz.token_block(rng, tc, t1)
        for p in range(2):
            tc, t1, pos = dcd[idc % len(dcd)]
            idc += 1
            lv = [rng.choice((-1, 1)) for _ in range(t1)]
            lv += [rng.choice((-2, 2)) if (i == 0 and t1 < 3) else rng.choice((-2, -1, 1, 2)) for i in range(tc - t1)]
            coef[16 + p] = dz.place(lv, pos, 4)
            for k in range(4):
                if (k % 2 + k // 2) % 2 == 0:
                    tc, t1 = ce[ic % len(ce)]
                    ic += 1
                else:
                    tc, t1 = min(N, 15), min(N, rng.randint(0, 3))
                coef[18 + 4 * p + k] = dz.token_block(rng, tc, t1, 15)
        mbs.append(inter(mv=[_mv_of(m)], coef=coef, cbp=47, qp=20 + m % 12))
    return Pic(W, H, mbs, at=at)


# (nA inside the MB, nB from the MB above) per (external class, composed class):
# on the first MB row of a slice the external nC is nA alone, the composed one
# (nA + nB + 1) >> 1
RECODE_AB = {(0, 0): (0, 0), (0, 2): (0, 4), (0, 4): (0, 8), (0, 8): (0, 16), (2, 0): (2, 0), (2, 2): (2, 2),
             (2, 4): (2, 8), (2, 8): (2, 16), (4, 2): (4, 0), (4, 4): (4, 4), (4, 8): (4, 12), (8, 4): (8, 0),
             (8, 8): (8, 8)}


def recode_pics(seed):
    """group r ("rows" only): MB rows in pairs, the upper one giving nB, the
    lower one -- the first row of its slice -- holding target blocks right of a
    block of TotalCoeff nA: luma blocks 1 and 3 and chroma AC block 1 of each
    plane walk every coeff_token entry for every (external, composed) class"""
    rng = random.Random(seed)
    le, ce = dz.token_entries(16), dz.token_entries(15)
    per = (len(le) + 1) // 2
    jobs = [(ab, j) for ab in RECODE_AB.values() for j in range(per)]
    pics = []
    per_pic = W12 * H8 // 2
    for i in range(0, len(jobs), per_pic):
        chunk = jobs[i:i + per_pic]
        mbs = [skip() for _ in range(W12 * H8)]
        for n, ((a, b), j) in enumerate(chunk):
            x, y = n % W12, 2 * (n // W12)
            up = {13: dz.token_block(rng, b, min(b, 3)), 15: dz.token_block(rng, b, min(b, 2))}
            lo = {}
            for q, r in enumerate((1, 3)):
                tc, t1 = le[(2 * j + q) % len(le)]
                lo[r - 1] = dz.token_block(rng, a, min(a, rng.randint(0, 3)))
                lo[r] = dz.token_block(rng, tc, t1)
            for p in range(2):
                tc, t1 = ce[(2 * j + p) % len(ce)]
                up[18 + 4 * p + 3] = dz.token_block(rng, min(b, 15), min(b, 3), 15)
                lo[18 + 4 * p] = dz.token_block(rng, a, min(a, rng.randint(0, 3)), 15)
                lo[18 + 4 * p + 1] = dz.token_block(rng, tc, t1, 15)
            mbs[y * W12 + x] = inter(mv=[_mv_of(n)], coef=up, cbp=44)
            mbs[(y + 1) * W12 + x] = inter(mv=[_mv_of(n + 1)], coef=lo, cbp=35)
        pics.append(Pic(W12, H8, mbs, at=(3 + len(pics) % 3, 2 + len(pics) % 5)))
    return pics


def _fill_pics(luma, chroma, at=(2, 2), W=W12, H=H8, qp=26):
    """16-coefficient blocks and 15-coefficient blocks into P_L0_16x16 MBs, 16
    luma and 8 chroma AC per MB"""
    pics = []
    nl, ncb = (len(luma) + 15) // 16, (len(chroma) + 7) // 8
    n = max(nl, ncb)
    for i in range(0, n, W * H):
        mbs = []
        for m in range(i, min(n, i + W * H)):
            coef = {r: b for r, b in enumerate(luma[16 * m:16 * m + 16])}
            coef.update({18 + k: b for k, b in enumerate(chroma[8 * m:8 * m + 8])})
            mbs.append(inter(mv=[_mv_of(m)], coef=coef, qp=qp))
        mbs += [skip()] * (W * H - len(mbs))
        pics.append(Pic(W, H, mbs, at=at))
    return pics


def tzrb_pics(seed):
    """group z: every total_zeros entry (TotalCoeff tc, the last coefficient
    behind tz zeros) and every run_before entry (zerosLeft, run), runs up to
    14 at zerosLeft > 6 included, for 16- and 15-coefficient blocks"""
    rng = random.Random(seed)

    def blocks(maxc):
        out = []
        for tc in range(1, maxc):
            for tz in range(maxc - tc + 1):
                pos = list(range(tc - 1)) + [tc + tz - 1]
                out.append(dz.place([rng.choice((-1, 1)) for _ in range(min(tc, 3))] +
                                    [rng.choice((-2, 2)) for _ in range(tc - min(tc, 3))], pos, maxc))
        for zl in range(1, maxc - 1):
            for run in range(zl + 1):
                out.append(dz.place([rng.choice((-1, 1)), rng.choice((-1, 1))], [zl + 1, zl - run], maxc))
        for _ in range(24):
            out.append(dz.token_block(rng, rng.randint(3, 8), rng.randint(0, 3), maxc))
        return out

    return _fill_pics(blocks(16), blocks(15))


LEVEL_EDGES = (1, 2, 3, 4, 6, 7, 8, 12, 13, 15, 16, 17, 24, 25, 30, 31, 32, 46, 47, 48, 49, 60, 61, 62, 96, 97, 120,
               121, 122, 126, 127, 128, 240, 241, 242, 255, 256, 480, 481, 482, 960, 961, 1632, 2047, 2048, 2063)
THRESHOLDS = (3, 6, 12, 24, 48)            # |level| > 3 << (suffixLength - 1): the next suffixLength


def level_blocks(seed):
    """group l: per context (designed.CONTEXTS), blocks that code +-v with that
    context live, v = 1 .. 66 and the edges up to 2063; the suffixLength chain
    with each threshold met and passed by one, followed by a level that shows
    the suffixLength it left; TotalCoeff 11 with 2 and 3 trailing ones"""
    rng = random.Random(seed)
    # and the first level of every level_prefix at every suffixLength
    vals = sorted(set(range(1, 67)) | set(LEVEL_EDGES) | {((p << sl) >> 1) + 1 for sl in range(7) for p in range(16)})
    out = []
    for ctx in dz.CONTEXTS:
        for m in vals:
            for v in (m, -m):
                if ctx[0] != "sl" and ctx[1] < 3 and m < 2:
                    continue                  # a first level of +-1 would be a trailing one
                lv = dz.context_levels(ctx, v, rng)
                out.append(dz.place(lv, range(len(lv))))
    for k, thr in enumerate(THRESHOLDS, 1):
        for v in (thr, thr + 1, -thr, -thr - 1):
            lv = [rng.choice((-m, m)) for m in ((2,) if k == 1 else dz.ESCALATE[:k - 1])] + [v, 2 * thr, -1 - 2 * thr]
            out.append(dz.place(lv, range(len(lv))))
    for t1 in (2, 3):
        lv = [rng.choice((-1, 1)) for _ in range(t1)] + [rng.choice((-9, 9))] + [2] * (10 - t1)
        out.append(dz.place(lv, range(11)))
    return out


def level_pics(seed):
    b = level_blocks(seed)
    return _fill_pics(b, [x[:15] for x in b])


BIG = dz.LEVEL_MAX                           # 2063: level_prefix 15 at every suffixLength


def longest_block(maxc):
    """every level a 28-bit level_prefix-15 escape: TotalCoeff = maxc, no
    trailing ones, no total_zeros"""
    return [BIG if k % 2 else -BIG for k in range(maxc)]


def longest_pics(W=4, H=8, at=(3, 4)):
    """group n: a whole MB of the longest blocks with cbp 47, and the same as
    an I_16x16 MB, each alone in a 4 x 8 picture"""
    coef = {r: longest_block(16) for r in range(16)}
    coef.update({16: longest_block(4), 17: longest_block(4)})
    coef.update({i: longest_block(15) for i in range(18, 26)})
    pics = []
    for kind in (P16, I16):
        mbs = [skip() for _ in range(W * H)]
        for y in (1, 3, 6):
            if kind == P16:
                mbs[W * y + 1] = inter(mv=[(4, -4)], coef=coef, cbp=47, qp=12)
            else:
                c16 = {k: (v[:15] if k < 16 else v) for k, v in coef.items()}
                c16[26] = longest_block(16)
                mbs[W * y + 1] = i16(coef=c16, cbp=47, qp=12)
        pics.append(Pic(W, H, mbs, at=at))
    return pics


def phase_pics(seed, n=3):
    """group n: per MB a filler block of a random length, then a block with a
    16-bit coeff_token and sixteen 28-bit escapes, a lone coefficient at scan
    position 15 (9-bit total_zeros) and coefficients at 15 and 0 (11-bit
    run_before), so each starts at every bit position modulo 32"""
    rng = random.Random(seed)
    pics = []
    for _ in range(n):
        mbs = []
        for m in range(W12 * H8):
            coef = {0: dz.token_block(rng, rng.randint(1, 9), rng.randint(0, 1), big=rng.choice((2, 3, 5))),
                    1: [rng.choice((-BIG, BIG)) for _ in range(16)],
                    2: [0] * 15 + [rng.choice((-1, 1))],
                    3: [rng.choice((-1, 1))] + [0] * 14 + [rng.choice((-1, 1))],
                    8: [0] * 15 + [rng.choice((-3, 3))],
                    10: [rng.choice((-2, 2))] + [0] * 14 + [rng.choice((-1, 1))]}
            mbs.append(inter(mv=[(rng.randint(-40, 40), rng.randint(-9, 9))], coef=coef, qp=30))
        pics.append(Pic(W12, H8, mbs, at=(1, 3)))
    return pics


def intra_pics(seed):
    """group i: the Intra16x16DCLevel piece with TotalCoeff 0, 1, 15 and 16,
    I_16x16 AC blocks and I_4x4 blocks at TotalCoeff = maxc, in the rect's
    interior.  I_4x4 needs the MB above as available as in the composed
    picture, so the "rows" variant has I_16x16 in those places and its I_4x4
    MBs in row 0 of a rect on the picture's top edge"""
    rng = random.Random(seed)
    out = {}
    for with_i4 in (True, False):
        mbs = [inter(mv=[_mv_of(m)], coef={5: [1, -1] + [0] * 14}) for m in range(W12 * H8)]
        for y in (1, 3, 5, 7):
            for x in range(1, W12 - 1):
                tc = (0, 1, 15, 16)[(x + y // 2) % 4]
                dc = dz.token_block(rng, tc, min(tc, rng.randint(0, 3)))
                if x % 2 and with_i4:
                    coef = {r: _tb(rng, 16 if r % 3 == 0 else rng.randint(0, 16))
                            for r in range(16)}
                    coef[16] = [3, 0, -1, 1]
                    mbs[y * W12 + x] = i4(coef=coef, cbp=31, qp=24 + x,
                                          modes=[rng.choice((0, 1, 2, 8)) for _ in range(16)], cmode=x % 4)
                else:
                    coef = {26: dc}
                    if x % 4 != 2:
                        coef.update({r: _tb(rng, 15 if r % 3 == 0 else rng.randint(0, 15), 15) for r in range(16)})
                        coef[18] = dz.token_block(rng, 15, 1, 15)
                    mbs[y * W12 + x] = i16(coef=coef, qp=30 - x)
        mbs[2 * W12] = pcm(bytes((7 * k + 3) % 256 for k in range(384)))       # I_PCM: anywhere
        mbs[6 * W12 - 1] = pcm(bytes(384))
        if not with_i4:
            # the rect on the picture's top edge: in its row 0 the MB above is missing in both
            # pictures, so I_4x4 with modes that read nothing from above (1, 2, 8) splices there
            for x in range(1, W12 - 1, 2):
                coef = {r: _tb(rng, 16 if r % 3 == 0 else rng.randint(0, 16)) for r in range(16)}
                coef[17] = [-2, 1, 0, 0]
                mbs[x] = i4(coef=coef, cbp=31, qp=20 + x, modes=[rng.choice((1, 2, 8)) for _ in range(16)],
                            cmode=1)
        out[with_i4] = Pic(W12, H8, mbs, at=(4, 6) if with_i4 else (4, 0))
    return out


def islice_pics(seed, with_i4):
    """group i: the same writer's I slices (no mb_skip_run, mb_type k = the P
    slice's 5 + k) and IDR pictures (nal_unit_type 5): an I_PCM left column,
    I_16x16 predicting from the left elsewhere, I_4x4 (not in the "rows"
    shape) where the MB above is in its slice"""
    rng = random.Random(seed)
    W, H = 6, 8
    pics = []
    for islice in (1, 2):
        mbs = []
        for m in range(W * H):
            x, y = m % W, m // W
            if x == 0:
                mbs.append(pcm(bytes((m + 5 * k) % 256 for k in range(384))))
            elif with_i4 and y % 2 and x % 2:
                coef = {r: _tb(rng, rng.randint(0, 16)) for r in range(16)}
                mbs.append(i4(coef=coef, cbp=15, qp=22 + x, modes=[rng.choice((0, 1, 2, 8)) for _ in range(16)]))
            else:
                coef = {26: _tb(rng, rng.randint(0, 16))}
                if m % 3:
                    coef.update({r: _tb(rng, rng.randint(0, 15), 15) for r in range(16)})
                    coef[16] = [1, -1, 0, 2]
                mbs.append(i16(coef=coef, qp=28 + y))
        pics.append(Pic(W, H, mbs, at=(7 + islice, 3), islice=islice, slice_qp_delta=islice - 3))
    return pics


E = MAX_MV


def motion_pics():
    """group m: motion at +-16383 next to a neighbour at the opposite extreme
    (mvd +-32766: a 31-bit Exp-Golomb code) in P_L0_16x16 and each partition
    shape, a P_Skip whose predicted motion is at the bound, slices that are one
    mb_skip_run and slices that end in one"""
    W, H = 6, 8
    mbs = []
    for y in range(H):
        for x in range(W):
            s = 1 if (x + y) % 2 == 0 else -1
            k = (x + 2 * y) % 6
            res = {0: [1] + [0] * 15} if (x + y) % 3 == 0 else {}
            if y in (2, 3):                  # rows of one motion, then P_Skips predicting it
                mbs.append(skip() if y == 3 and x in (1, 2, 4) else inter(mv=[(E, -E)], coef=res))
            elif k == 0 or k == 5:
                mbs.append(inter(mv=[(s * E, -s * E)], coef=res))
            elif k == 1:
                mbs.append(inter(P16X8, mv=[(s * E, s * E), (-s * E, -s * E)], coef=res))
            elif k == 2:
                mbs.append(inter(P8X16, mv=[(-s * E, s * E), (s * E, -s * E)], coef=res))
            elif k == 3:
                sub = (0, 1, 2, 3)
                nmv = 1 + 2 + 2 + 4
                mbs.append(inter(P8X8, sub=sub, mv=[((s if j % 2 else -s) * E, (-s if j % 3 else s) * E)
                                                    for j in range(nmv)], coef=res))
            else:
                mbs.append(inter(P8X8REF0, sub=(3, 0, 0, 1), mv=[((s if j % 2 else -s) * E, s * E)
                                                                 for j in range(4 + 1 + 1 + 2)], coef=res))
    ext = Pic(W, H, mbs, at=(5, 3))
    # mb_skip_run: rows 0-1 and 4-5 all skipped, rows 2-3 and 6-7 ending in a run
    mbs = []
    for y in range(H):
        for x in range(W):
            coded = y % 4 >= 2 and x < 2
            mbs.append(inter(mv=[(8 * x, -4 * y)], coef={3: [2, 1] + [0] * 14}) if coded else skip())
    runs = Pic(W, H, mbs, at=(9, 7))
    return [ext, runs]


def refs_pic(nrefs, at):
    """ref_idx as ue for a list of nrefs references, every partition with a
    reference of its own; the first MB of each partition shape uses the largest
    index nrefs - 1"""
    W, H = 6, 8
    mbs = []
    for m in range(W * H):
        r = [(nrefs - 1 - m // 4 - j) % nrefs for j in range(4)]
        k = m % 4
        if k == 0:
            mbs.append(inter(ref=r, mv=[_mv_of(m)]))
        elif k == 1:
            mbs.append(inter(P16X8, ref=r, mv=[_mv_of(m), _mv_of(m + 1)]))
        elif k == 2:
            mbs.append(inter(P8X16, ref=r, mv=[_mv_of(m), _mv_of(m + 2)], coef={0: [-1] + [0] * 15}))
        else:
            mbs.append(inter(P8X8, ref=r, mv=[_mv_of(m + j) for j in range(4)]))
    return Pic(W, H, mbs, at=at, nrefs=nrefs)


def refs_pics():
    """group m: 3 references (a frame at and one past the first waypoint)"""
    return [refs_pic(3, (0, 0)), refs_pic(3, (10, 8))]


WAYPOINTS = 8                                 # MAX_WAYPOINTS (include/h264_writer.h)
ALL_WP_OFFS = [496 * (k + 1) for k in range(WAYPOINTS)] + [496 * WAYPOINTS + 6]


def refs_all_pics():
    """group m: a scroll over every waypoint (offsets 496, 992, ... 3968: a
    waypoint each); frame t splices a picture of the 3 + t references its frame
    has, the last one -- past all eight -- of 10, each using up to the largest
    index in P_L0_16x16, 16x8, 8x16 and P_8x8"""
    return [refs_pic(min(3 + t, 2 + WAYPOINTS), (1 + t, t % 5)) for t in range(len(ALL_WP_OFFS))]


def refused_pic():
    """|mv| = 16384: refused"""
    mbs = [inter(mv=[(4, 4)]) for _ in range(4 * 8)]
    mbs[9] = inter(mv=[(E + 1, 0)])
    return Pic(4, 8, mbs, at=(2, 2), status=ERR_SYNTAX)


ESCAPE_2063 = "0" * 15 + "1" + format(4092, "012b")   # +2063 as an adjusted first level at suffixLength 0


class Prefix16Pic(Pic):
    """a picture whose one escape is rewritten as a level_prefix 16 code (16
    zeros, a one, a 13-bit suffix: High profiles only), in the bits of its
    slice: the oracle's writer cannot make one, and its parser refuses it"""

    def __init__(self):
        mbs = [inter(mv=[(4, 4)]) for _ in range(4 * 8)]
        mbs[4 * 2 + 1] = inter(mv=[(4, 4)], coef={0: [BIG] + [0] * 15})
        super().__init__(4, 8, mbs, at=(5, 5), status=ERR_SYNTAX)
        self.patched = {}                     # shape -> (slice index, bit position of the code in its RBSP)

    def nal(self, oracle, shape):
        import h264_pslice as hp
        if shape not in self._nal:
            units = hp.nal_units(super().nal(oracle, shape))
            out, hits = b"", 0
            for k, u in enumerate(units):
                rb = hp.ebsp_to_rbsp(u[1:])
                bits = "".join(format(x, "08b") for x in rb).rstrip("0")[:-1]     # without the trailing bits
                at = bits.find(ESCAPE_2063)
                if at >= 0:
                    assert bits.count(ESCAPE_2063) == 1
                    bits = bits[:at] + "0" * 16 + "1" + "0" * 13 + bits[at + 28:]
                    self.patched[shape] = (k, at)
                    hits += 1
                bits += "1"
                bits += "0" * (-len(bits) % 8)
                rb = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
                esc, zeros = bytearray(), 0
                for x in rb:                  # emulation prevention (7.4.1)
                    if zeros >= 2 and x <= 3:
                        esc.append(3)
                        zeros = 0
                    esc.append(x)
                    zeros = zeros + 1 if x == 0 else 0
                out += b"\x00\x00\x00\x01" + u[:1] + bytes(esc)
            assert hits == 1
            self._nal[shape] = out
        return self._nal[shape]


QP_CHAIN = (0, 51, 0, 26, 51)


def qp_pics(W=6, H=8, at=None):
    """group q: MB QPs 0 -> 51 -> 0 -> 26 -> 51 inside a slice (mb_qp_delta
    wraps: +51 is written as -1), slice_qp_delta -26 and +25, rows that end at
    QP 51 before one that starts at 0 and the reverse, the first spliced MB at
    QP 0 and at QP 51 against the composed slice QP 26"""
    res = {0: [2, -1] + [0] * 14, 17: [1, 0, 0, 0]}
    pics = []
    for first, sqd in ((0, 0), (51, 0), (0, -26), (51, 25), (26, -26), (26, 25)):
        mbs = []
        for y in range(H):
            for x in range(W):
                if y % 4 == 0:
                    qp = ((first,) + QP_CHAIN)[x % 6] if y == 0 else (QP_CHAIN + (51,))[x % 6]
                else:                        # rows that start and end at 0 or 51, each way round
                    qp = ((0, 26, 51, 26, 51, 0), (51, 0, 26, 51, 0, 0), (51, 26, 0, 51, 26, 51))[y % 4 - 1][x % 6]
                mbs.append(skip() if (x, y) == (3, 5) else
                           (i16(coef={26: [1] + [0] * 15}, qp=qp) if (x, y) == (2, 3) else inter(mv=[_mv_of(x)], coef=res, qp=qp)))
        pics.append(Pic(W, H, mbs, at=at or (1 + len(pics), 2), slice_qp_delta=sqd))
    return pics


def ep_pics():
    """group e: bodies that are level_prefix-15 escapes with all-zero suffixes
    (17, 31, 61, 121 in coding order): 15 zero bits, a one and 12
    zero bits each, so the external NAL is dense in emulation prevention
    bytes; a filler of 0 .. 15 trailing ones per MB moves them over every byte
    position"""
    pics = []
    for sign in (1, -1):
        mbs = []
        for m in range(W12 * H8):
            sg = sign if m % 3 else -sign
            coef = {16: [121 * sg, 61 * sg, 31 * sg, 17 * sg], 17: [121 * sg, 61 * sg, 31 * sg, 17 * sg]}
            for r in (0, 2, 5, 7, 8, 10, 13, 15):
                coef[r] = [61 * sg, 31 * sg, 17 * sg] + [0] * 13
            coef[1] = [1] * (m % 16) + [0] * (16 - m % 16)
            mbs.append(inter(mv=[_mv_of(m)], coef=coef, qp=26))
        pics.append(Pic(W12, H8, mbs, at=(6, 5)))
    return pics


# ------------------------------------------------------------------- corpus ---
_cases = None

CASE_GROUPS = [("w_walk", "w"), ("r_recode", "r"), ("z_tzrb", "z"), ("l_levels", "l"), ("n_longest", "n"),
               ("n_phases", "n"), ("w_corner", "w"), ("i_intra", "i"), ("i_intra_rows", "i"), ("m_motion", "m"),
               ("m_refs", "m"), ("m_refs_all", "m"),
               ("m_refused", "m"), ("q_chain", "q"), ("e_epdense", "e"), ("l_prefix16", "l")]
REFUSED = ("m_refused", "l_prefix16")


def cases():
    """name -> Case; built once"""
    global _cases
    if _cases is None:
        intra = intra_pics(9)
        cs = [
            # the rect in the picture's top-left and bottom-right corner, and inside it
            Case("w_walk", "w", [walk_pic(N, 1 + i, at) for i, (N, at) in
                                 enumerate(((0, (0, 0)), (3, (3, 3)), (6, (6, 5)), (12, (8, 8))))], w=320),
            Case("r_recode", "r", recode_pics(3), w=320, shapes=("rows",)),
            Case("z_tzrb", "z", tzrb_pics(5)),
            Case("l_levels", "l", level_pics(7)),
            Case("n_longest", "n", longest_pics()),
            Case("n_phases", "n", phase_pics(13)),
            # the rect in the picture's corner for every neighbour TotalCoeff; two seeds each, so
            # that the top row's 48 chroma AC targets reach all 58 entries
            Case("w_corner", "w", [walk_pic(N, 11 + i + 4 * k, (0, 0)) for i, N in enumerate((0, 3, 6, 12))
                                   for k in range(2)], w=320),
            Case("i_intra", "i", [intra[True]] + islice_pics(15, True), w=320, shapes=("one", "two")),
            Case("i_intra_rows", "i", [intra[False]] + islice_pics(16, False), w=320, shapes=("rows",)),
            Case("m_motion", "m", motion_pics(), w=320),
            # offset 496 makes a waypoint, so the composed list has 3 references from there on
            Case("m_refs", "m", refs_pics(), w=320, offs=[496, 500]),
            Case("m_refs_all", "m", refs_all_pics(), w=320, offs=ALL_WP_OFFS),
            Case("m_refused", "m", [refused_pic()]),
            Case("q_chain", "q", qp_pics()),
            Case("e_epdense", "e", ep_pics(), w=320),
            Case("l_prefix16", "l", [Prefix16Pic()]),
        ]
        assert [(c.name, c.group) for c in cs] == CASE_GROUPS
        _cases = {c.name: c for c in cs}
    return _cases


def reference_pics():
    """(name, Pic) for tests/golden/splice_ref.json: pictures of the reference
    parser's fixed 20 x 20 MBs -- the table walk, the longest MBs, the QP chain --
    as external slices in one-slice form; their 12 x 8 forms are spliced into
    its 320 x 320 picture"""
    ext = [(f"walk{N}", walk_pic(N, 1 + i, (0, 0), 20, 20)) for i, N in enumerate((0, 3, 6, 12))]
    ext += [(f"longest{i}", p) for i, p in enumerate(longest_pics(20, 20, (0, 0)))]
    ext += [(f"qp{i}", p) for i, p in enumerate(qp_pics(20, 20, (0, 0))[:4])]
    cs = cases()
    comp = [(f"walk{i}", p) for i, p in enumerate(cs["w_walk"].pics)]
    comp += [(f"longest{i}", p) for i, p in enumerate(cs["n_longest"].pics)]
    comp += [(f"qp{i}", p) for i, p in enumerate(cs["q_chain"].pics[:4])]
    return ext, comp


def names(refused=False):
    return [n for n, _ in CASE_GROUPS if (n in REFUSED) == refused]


def frames_of(oracle, case, mode, shapes=None):
    """the frames dict of tests/test_gpu_splice.py (gpu_streams / plan_from):
    stream s splices the case's pictures in slice shape s"""
    return {(s, t): ([], mode, (p.at[0], p.at[1], p.W, p.H, p.nal(oracle, shape)))
            for s, shape in enumerate(shapes or case.shapes) for t, p in enumerate(case.pics)}


def offsets_of(case, S=None):
    import numpy as np
    return np.array([case.offs] * (S or len(case.shapes)), np.int32)


def route_mbs():
    """designed MBs per parse route, by k_splice_units' rule: a picture of
    SPLICE_LANE_MIN = 4 or more slices goes to k_splice_lanes, which hands a
    picture back (SPLICE_REDO) when a slice is longer than one MB row"""
    out = {"k_splice_parse": 0, "k_splice_lanes": 0, "k_splice_lanes -> k_splice_parse": 0}
    for c in cases().values():
        for p in c.pics:
            for shape in c.shapes:
                nsl = 1 + len(p.firsts(shape))
                key = "k_splice_parse" if nsl < 4 else ("k_splice_lanes" if shape == "rows"
                                                        else "k_splice_lanes -> k_splice_parse")
                out[key] += p.W * p.H
    return out
