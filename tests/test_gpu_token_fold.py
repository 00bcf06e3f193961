"""k_dyn_row's coeff_token where TotalCoeff is first known: a piece whose top
neighbour is in its own rect row (interior) takes its nC in the sort's
scatter and is coded token first (or, without levels, written there as its
token); the token phase is left with the 8 top-row pieces per MB, which wait
for the row above's TotalCoeffs.  Byte for byte
against oracle/dyn_oracle.c, S = 2, F = 3, small pictures:

  widths   1 (every left neighbour outside the rect), 2, 8 and 9 (a wave's 8
           MBs filled exactly, then the first second wave), 25 (config 3), 33
           (256 threads, an MB pass with one MB in it), 41, 47, 65
  rect     x0 = 0 (left unavailable) and x0 > 0 (left a static MB: zero);
           y0 = 0 and y0 > 0; heights 1 and 3
  inputs   QP 22 and 26, the synthetic source over random references; QP 34;
           QP 42-46 with test_gpu_row_prologue's sparse_source over flat
           references (empty interior blocks beside coded ones, rows with
           none); the same at QP 22 / 26 (empty blocks between heavy ones: the
           token of TotalCoeff 0 at nC >= 8); QP 51; one QP-18 case on the
           general path; one with a waypoint in the chain
  designed frames of their own (tests/designed.py's helpers): blocks whose
           token + body straddle 128 bits in interior and in top-row
           positions, bodies over 128 bits in interior positions, chroma DC
           pieces in the same MBs

The oracle's own NALs must show all of that (test_oracle_token_coverage, no
GPU): a case that falls short gets another seed, QP or rect, never a weaker
condition.
Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import designed as dz
import h264_pslice as hp
from dynhelp import Rect, qp_field, split_nals
from reconhelp import qpc_of
from test_gpu_dyn import (check_equal, gpu, gpu_streams, oracle_streams, random_refs,  # noqa: F401
                          striped_refs, synth_source)
from test_gpu_dyn_mbphase import F, OFFS, S, flat_refs
from test_gpu_row_prologue import sparse_source

# name: picture, rect (x0, y0, w, h), rect QP, input, seed.  Input "synth": the
# synthetic source over random references; ("flat", y, c): the synthetic
# source over flat references; ("sparse", y, c): sparse_source over flat ones
CASES = {
    "w1_inside_qp22": ((64, 64), (1, 1, 1, 3), 22, "synth", 71),
    "w1_edge_qp44": ((64, 64), (0, 0, 1, 3), 44, ("sparse", 120, 124), 72),
    "w2_qp26": ((64, 64), (0, 1, 2, 3), 26, "synth", 73),
    "w2_sparse_qp22": ((64, 64), (1, 0, 2, 1), 22, ("sparse", 120, 124), 74),
    "w8_qp34": ((176, 64), (2, 0, 8, 3), 34, "synth", 75),
    "w8_sparse_qp26": ((128, 64), (0, 1, 8, 3), 26, ("sparse", 120, 124), 76),
    "w9_qp42": ((176, 64), (1, 0, 9, 3), 42, ("sparse", 120, 124), 77),
    "w9_sparse_qp22": ((176, 64), (0, 1, 9, 3), 22, ("sparse", 120, 124), 78),
    "w25_qp26": ((464, 64), (3, 1, 25, 3), 26, "synth", 79),
    "w25_qp46": ((432, 64), (0, 3, 25, 1), 46, ("sparse", 120, 124), 80),
    "w25_sparse_qp26": ((432, 64), (1, 0, 25, 3), 26, ("sparse", 120, 124), 81),
    "w33_qp22": ((560, 64), (1, 1, 33, 1), 22, "synth", 82),
    "w33_qp44": ((528, 64), (0, 0, 33, 3), 44, ("sparse", 120, 124), 83),
    "w41_qp26": ((672, 64), (1, 1, 41, 3), 26, "synth", 84),
    "w41_flat_qp34": ((656, 64), (0, 0, 41, 3), 34, ("flat", 110, 116), 85),
    "w47_qp22": ((768, 64), (1, 0, 47, 3), 22, "synth", 86),
    "w47_qp43": ((752, 64), (0, 1, 47, 3), 43, ("sparse", 120, 124), 87),
    "w65_qp51": ((1056, 64), (1, 1, 65, 3), 51, ("flat", 128, 120), 88),
    "w65_qp45": ((1040, 64), (0, 0, 65, 1), 45, ("sparse", 120, 124), 89),
    "w25_general_qp18": ((432, 64), (1, 1, 25, 3), 18, "synth", 90),
}

_want = {}
_designed = {}


def want_of(oracle, name):
    """the case's inputs and the oracle's streams, made once"""
    if name not in _want:
        (w, h), rc, qp, inp, seed = CASES[name]
        rect = Rect(*rc, qp_field(qp))
        if inp == "synth":
            R, src = random_refs(w, h, seed), synth_source(oracle, S, F, rect)
        elif inp[0] == "flat":
            R, src = flat_refs(w, h, *inp[1:]), synth_source(oracle, S, F, rect)
        else:
            R, src = flat_refs(w, h, *inp[1:]), sparse_source(rect, inp[1], inp[2], seed)
        _want[name] = (w, h, rect, R, src, oracle_streams(oracle, w, h, OFFS, rect, src, R))
    return _want[name]


# ------------------------------------------------------------ designed frames --
RW, RH = 4, 3


def long_blocks(qp, seed):
    """per maxc (16 luma, 15 chroma AC) two blocks whose body alone is over 128
    bits after the pixel round trip, int8 levels: a seeded search, as
    designed.length_frames makes its own"""
    import random
    rng = random.Random(seed)
    out = {}
    for maxc, q in ((16, qp), (15, qpc_of(qp))):
        found = []
        for it in range(4000):
            if len(found) == 2:
                break
            tc = rng.randint(8, maxc)
            top = rng.choice((12, 20, 32, 48))
            lv = [rng.choice((-1, 1)) * rng.randint(top // 2, top) for _ in range(tc)]
            blk = dz.place(lv, rng.sample(range(maxc), tc), maxc)
            pred, src = dz.split_pred(dz.block_residual(blk if maxc == 16 else [0] + blk, q))
            got = dz.predict_levels(src - pred, q)[16 - maxc:]
            if all(abs(g) <= 127 for g in got) and any(got) and dz.body_pushes(got, maxc)[1][-1] > 128:
                found.append(blk)
        assert len(found) == 2, (qp, maxc)
        out[maxc] = found
    return out


def straddle_case(oracle, qp, seed):
    """designed.length_frames' blocks (coded lengths 120 ... 140 at nC 0 on a
    checkerboard of raster positions 0, 2 (top row) and 5, 7, 8, 10, 13, 15
    (interior), luma and chroma AC) over a 4 x 3-MB rect, so that rect rows 1
    and 2 hold them too; and in the last MB blocks of large levels in interior
    positions (a body over 128 bits by itself) with chroma DC levels beside
    them.  Three frames: the frame, its blocks again at another seed, the
    frame again"""
    key = (qp, seed)
    if key not in _designed:
        frames = []
        for sd in (seed, seed + 1, seed):
            fr = dz.length_frames(oracle, qp, sd, rw=RW, rh=RH)[0]
            lb = long_blocks(qp, sd)
            for r, lv in ((5, lb[16][0]), (15, lb[16][1]), (10, lb[16][0])):
                fr.luma_block(RW - 1, RH - 1, r, lv, qp)
            fr.chroma(RW - 1, RH - 1, 0, [5, -3, 2, 1], [[0] * 15, [0] * 15, lb[15][0], [0] * 15], qpc_of(qp))
            fr.chroma(RW - 1, RH - 1, 1, [-1, 0, 1, 0], [[0] * 15, [0] * 15, [0] * 15, lb[15][1]], qpc_of(qp))
            frames.append(fr)
        c = dz.Case(f"tok_straddle_qp{qp}", "tok", qp, frames)
        _designed[key] = (c, oracle_streams(oracle, c.w, c.h, c.offs, c.rect(), c.src, c.R))
    return _designed[key]


DESIGNED = [(22, 301), (24, 302)]


# ----------------------------------------------------- the oracle's own pieces --
def pieces_of(oracle, streams, w, h, rect, nframes, lengths=False):
    """every coded residual piece of the rect in the oracle's NALs: (kind,
    interior, nC, TotalCoeff, piece bits, body bits) with kind "luma" / "cac" /
    "cdc"; nC as 9.2.1 gives it from the parsed TotalCoeffs (an MB outside the
    rect is coded without residual: available, zero); the bit counts only
    with lengths (the oracle's count of the block, the body's by the standard's
    tables: designed.body_pushes)"""
    out = []

    def bits(coef, maxc, nC):
        if not lengths:
            return 0, 0
        return dz.coded_bits(oracle, list(coef) + [0] * (16 - len(coef)), maxc, nC), (dz.body_pushes(coef, maxc)[1] or [0])[-1]

    for stream in streams:
        nals = split_nals(stream)
        assert len(nals) == nframes
        for nal in nals:
            tcs = {}

            def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
                t = [sum(1 for c in b if c) for b in luma] + [sum(1 for c in b if c) for p in cac for b in p]
                tcs[(x, y)] = t
                if not (rect.x0 <= x < rect.x0 + rect.w and rect.y0 <= y < rect.y0 + rect.h):
                    assert cbp == 0
                    return
                left, top = tcs.get((x - 1, y)), tcs.get((x, y - 1))

                def ctx(i, bx, by, dl, dt, ul, ut):
                    nA = t[i - dl] if bx > 0 else (left[i + ul] if left else -1)
                    nB = t[i - dt] if by > 0 else (top[i + ut] if top else -1)
                    return (nA + nB + 1) >> 1 if nA >= 0 and nB >= 0 else max(nA, nB, 0)

                for r in range(16):
                    bx, by = r % 4, r // 4
                    if cbp & (1 << (2 * (by // 2) + bx // 2)):
                        nC = ctx(r, bx, by, 1, 4, 3, 12)
                        out.append(("luma", by > 0, nC, t[r], *bits(luma[r], 16, nC)))
                if cbp >> 4:
                    for p in range(2):
                        out.append(("cdc", True, -1, sum(1 for c in cdc[p] if c), 0, 0))
                if (cbp >> 4) == 2:
                    for p in range(2):
                        for k in range(4):
                            i, bx, by = 16 + 4 * p + k, k % 2, k // 2
                            nC = ctx(i, bx, by, 1, 2, 1, 2)
                            out.append(("cac", by > 0, nC, t[i], *bits(cac[p][k], 15, nC)))

            hp.parse_p_slice(nal, w, h, on_mb=on_mb)
    return out


def ncls(nC):
    return 0 if nC < 2 else (1 if nC < 4 else (2 if nC < 8 else 3))


def test_oracle_token_coverage(oracle):
    """in the oracle's own bytes: interior pieces without levels and with
    them at every coeff_token table, luma and chroma AC; top-row pieces at
    every table; and in the designed frames pieces over 128 bits only with
    their token in interior and top-row positions, pieces of exactly 128 and
    129 bits, bodies over 128 bits in interior positions, chroma DC pieces"""
    empty, coded, toprow = set(), set(), set()
    for name in CASES:
        if "general" in name:
            continue
        w, h, rect, _, _, want = want_of(oracle, name)
        for kind, inner, nC, tc, n, nb in pieces_of(oracle, want, w, h, rect, F):
            if kind == "cdc":
                continue
            (toprow if not inner else (coded if tc else empty)).add((kind, ncls(nC)))
    print("interior, no levels:", sorted(empty), " interior, coded:", sorted(coded), " top row:", sorted(toprow))
    every = {(k, c) for k in ("luma", "cac") for c in range(4)}
    assert empty == every and coded == every and toprow == every
    for qp, seed in DESIGNED:
        c, want = straddle_case(oracle, qp, seed)
        ps = pieces_of(oracle, want, c.w, c.h, Rect(*c.rc, 0), c.F, lengths=True)
        tok_only = {(k, inner) for k, inner, nC, tc, n, nb in ps if k != "cdc" and nb <= 128 < n}
        body_over = {k for k, inner, nC, tc, n, nb in ps if k != "cdc" and inner and nb > 128}
        lens = {n for k, inner, nC, tc, n, nb in ps if k != "cdc"}
        print(f"qp {qp}: over 128 with the token only {sorted(tok_only)}, bodies over 128 (interior) "
              f"{sorted(body_over)}, chroma DC pieces {sum(1 for p in ps if p[0] == 'cdc' and p[3])}")
        assert {("luma", True), ("luma", False), ("cac", True), ("cac", False)} <= tok_only
        assert {"luma", "cac"} <= body_over
        assert {127, 128, 129} <= lens
        assert any(k == "cdc" and tc for k, inner, nC, tc, n, nb in ps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_token_fold_widths(gpu, oracle, name):
    w, h, rect, R, src, want = want_of(oracle, name)
    b, rc = gpu_streams(gpu, w, h, OFFS, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("qp,seed", DESIGNED)
def test_token_fold_designed(gpu, oracle, qp, seed):
    c, want = straddle_case(oracle, qp, seed)
    b, rc = gpu_streams(gpu, c.w, c.h, c.offs, c.rect(), c.R, c.src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.gpu
def test_token_fold_with_waypoints(gpu, oracle):
    """a waypoint in the chain (two waves: w = 9; rows that poll)"""
    w, h = 176, 512
    rect = Rect(1, 3, 9, 3, qp_field(26))
    offs = np.stack([np.arange(490, 502), np.arange(998, 986, -1)]).astype(np.int32)   # cross 496 and 992
    R = striped_refs(oracle, w, h)
    src = synth_source(oracle, 2, 12, rect)
    want = oracle_streams(oracle, w, h, offs, rect, src, R)
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    for s in (0, 1):
        assert any(k == 1 and sl == 0 for k, _, _, sl in b.nals(s))
    b.close()
