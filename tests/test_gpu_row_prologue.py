"""k_dyn_row's tables (coeff_token / chroma DC fields, piece-class
descriptors, level codewords, the waypoint table, the MB-head classes) reach
LDS from its last wave, after that wave's own level passes and before the
barrier that closes the levels; the prologue loads only the row table and
the quantiser.  Byte for byte against oracle/dyn_oracle.c at the rect widths
where the copying wave's place changes:

  w = 1     one wave: the copying wave is the only wave
  w = 9     the first width with two waves
  w = 16    two waves (128 threads), both with three level passes: no spare
            pass, the copy follows the last pass of a full wave
  w = 25    config 3: four waves, the last with one pass fewer
  w = 41    five waves, four block tasks per thread
  w = 47    config 5's width

with rect heights 1 (no hand-off), 2 and 3 (rows that poll the row above),
each width with the synthetic source at QP 22 (every block coded: the chroma
DC and coeff_token tables are read at once) and with flat references at QP
42-46 under a source that differs from them in a few blocks only (rows
nearly or wholly empty: the CAVLC phase starts the moment the levels end, a
table that arrives late shows), one case on the general path
(k_dyn_row<true>, which copies in its prologue) and one with a waypoint in
the chain (the head classes differ per NAL).  The oracle's own bytes must show
the sparse rows (test_oracle_sparse_rows); a case that falls short gets
another rect or QP, never a weaker condition.
Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import test_gpu_cavlc_balance as cb
from dynhelp import Rect, qp_field
from test_gpu_cavlc_balance import (F, OFFS, S, block_counts, check_equal, flat_refs, gpu,  # noqa: F401
                                    gpu_streams, oracle_streams, synth_source)
from test_gpu_dyn import random_refs, striped_refs

# name: picture, rect (x0, y0, w, h), rect QP, input ("synth": the synthetic
# source over random references; (y, c): sparse_source over flat ones), seed
CASES = {
    "prologue_w1_heavy": ((64, 64), (1, 1, 1, 3), 22, "synth", 51),
    "prologue_w1_sparse": ((64, 64), (0, 0, 1, 2), 44, (120, 124), 52),
    "prologue_w9_heavy": ((176, 64), (1, 1, 9, 2), 22, "synth", 53),
    "prologue_w9_sparse": ((176, 64), (2, 0, 9, 3), 46, (120, 124), 54),
    "prologue_w16_heavy": ((288, 64), (1, 2, 16, 1), 22, "synth", 55),
    "prologue_w16_sparse": ((272, 64), (0, 1, 16, 3), 42, (120, 124), 56),
    "prologue_w25_heavy": ((464, 64), (3, 0, 25, 3), 22, "synth", 57),
    "prologue_w25_sparse": ((432, 64), (1, 3, 25, 1), 46, (120, 124), 58),
    "prologue_w41_heavy": ((672, 64), (1, 3, 41, 1), 22, "synth", 59),
    "prologue_w41_sparse": ((656, 64), (0, 1, 41, 2), 44, (120, 124), 60),
    "prologue_w47_heavy": ((768, 64), (1, 0, 47, 3), 22, "synth", 61),
    "prologue_w47_sparse": ((752, 64), (0, 2, 47, 2), 46, (120, 124), 62),
    "prologue_w25_general": ((432, 64), (1, 1, 25, 3), 18, "synth", 63),
}


def sparse_source(rect, y, c, seed):
    """[S][F][384 w h]: the flat references' own values, so nothing is coded,
    except in a few 4x4 blocks (an offset of 40-100 and noise: a DC level of
    one to five at QP 42-46, some AC).  Rect row r of frame f of stream s has
    no such block when (s F + f + r) % 3 == 0, fewer than a wave's 64 when it
    is 1, and about a quarter of its blocks otherwise"""
    rng = np.random.default_rng(seed)
    w, h = rect.w, rect.h
    out = np.zeros((S, F, 384 * w * h), np.uint8)

    def stir(plane, by, bx):
        blk = int(y if plane.shape[1] == 16 * w else c) + int(rng.choice((-1, 1))) * int(rng.integers(40, 101)) \
            + rng.integers(-40, 41, (4, 4))
        plane[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = np.clip(blk, 0, 255)

    for s in range(S):
        for f in range(F):
            luma = np.full((16 * h, 16 * w), y, np.uint8)
            chroma = [np.full((8 * h, 8 * w), c, np.uint8) for _ in range(2)]
            for r in range(h):
                mode = (s * F + f + r) % 3
                if mode == 0:
                    continue
                nl = int(rng.integers(1, min(48, 16 * w) + 1)) if mode == 1 else 4 * w
                ncb = int(rng.integers(0, min(8, 8 * w) + 1)) if mode == 1 else 2 * w
                for k in rng.choice(16 * w, nl, replace=False):
                    stir(luma, 4 * r + int(k) // (4 * w), int(k) % (4 * w))
                for k in rng.choice(8 * w, ncb, replace=False):
                    stir(chroma[int(k) // (4 * w)], 2 * r + (int(k) % (4 * w)) // (2 * w), int(k) % (2 * w))
            out[s, f] = np.concatenate([luma.ravel(), chroma[0].ravel(), chroma[1].ravel()])
    return out


def want_of(oracle, name):
    """the case's inputs and the oracle's streams, made once -- kept in
    test_gpu_cavlc_balance's cache, where its block_counts looks them up"""
    if name not in cb._want:
        (w, h), rc, qp, rnd, seed = CASES[name]
        rect = Rect(*rc, qp_field(qp))
        R = flat_refs(w, h, *rnd) if isinstance(rnd, tuple) else random_refs(w, h, seed)
        src = sparse_source(rect, *rnd, seed) if isinstance(rnd, tuple) else synth_source(oracle, S, F, rect)
        cb._want[name] = (w, h, rect, R, src, oracle_streams(oracle, w, h, OFFS, rect, src, R))
    return cb._want[name]


def test_cases_cover_the_layouts():
    """every width with both sources, and the heights 1, 2, 3 among them"""
    for w in (1, 9, 16, 25, 41, 47):
        kinds = {n.rsplit("_", 1)[1] for n, c in CASES.items() if c[1][2] == w}
        assert {"heavy", "sparse"} <= kinds, w
    assert {c[1][3] for c in CASES.values()} == {1, 2, 3}
    for kind in ("heavy", "sparse"):
        assert {c[1][3] for n, c in CASES.items() if n.endswith(kind)} == {1, 2, 3}, kind
    assert all(c[2] == 22 for n, c in CASES.items() if n.endswith("heavy"))
    assert all(42 <= c[2] <= 46 for n, c in CASES.items() if n.endswith("sparse"))
    assert all(c[2] < 22 for n, c in CASES.items() if n.endswith("general"))


def test_oracle_sparse_rows(oracle):
    """in the oracle's own bytes: every heavy case codes nearly all its
    blocks; every sparse case has a row with coded blocks but fewer than one
    wave holds (64), and a row with none"""
    for name in CASES:
        want_of(oracle, name)
        coded = [sum(1 for t in r if t) for r in block_counts(oracle, name)]
        w = CASES[name][1][2]
        print(f"{name}: coded blocks per row {min(coded)}..{max(coded)} of {24 * w}, "
              f"{sum(1 for c in coded if c == 0)} of {len(coded)} rows empty")
        if name.endswith("_heavy"):
            assert min(coded) > 0.9 * 24 * w, (name, min(coded))
        if name.endswith("_sparse"):
            assert any(0 < c < 64 for c in coded), (name, sorted(set(coded))[:8])
            assert min(coded) == 0, (name, min(coded))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_row_prologue_widths(gpu, oracle, name):
    w, h, rect, R, src, want = want_of(oracle, name)
    b, rc = gpu_streams(gpu, w, h, OFFS, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.gpu
def test_row_prologue_with_waypoints(gpu, oracle):
    """a waypoint in the chain: the 12 head classes and the waypoint table
    the last wave copies differ per NAL (two waves: w = 9)"""
    w, h = 176, 512
    rect = Rect(1, 3, 9, 2, qp_field(30))
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
