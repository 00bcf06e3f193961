"""k_dyn_row's MB phase (cbp, coded_block_pattern code, piece offsets, the
row's MB offsets) in its run-parallel form: eight lanes per MB, T / 8 MBs a
pass, a one-pass row scan up to 64 MBs.  Byte for byte against
oracle/dyn_oracle.c at the rect widths around every boundary of that layout:

  w = 1, 2, 3   one 64-thread workgroup, part of its one wave
  w = 7, 8, 9   8 fills the 64-thread workgroup's pass exactly; 9 is the
                first width with two waves
  w = 24, 25    192 threads filled exactly; config 3's 256 threads, the
                fourth wave with one MB
  w = 40, 41    320 threads filled exactly; the first width with four block
                tasks per thread, and with a second pass (one MB in it)
  w = 64, 65    the last row scan in one pass, the first in two (both in two
                passes of the MB phase)

with rect QPs from fully coded to fully empty (and 12 / 18 for the general
path's instantiation), the rect at the picture's left edge and away from it,
a top rect row and rows that take the row above's TotalCoeffs.  The oracle's
own bytes must show the cbp values these cases are meant to produce
(test_oracle_cbp_coverage); a case that falls short gets another seed or QP,
never a weaker condition.
Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import h264_pslice as hp
from dynhelp import Rect, qp_field, split_nals
from test_gpu_dyn import (ArrayRefs, check_equal, gpu, gpu_streams, oracle_streams, random_refs,  # noqa: F401
                          striped_refs, synth_source)

S, F = 2, 3
OFFS = np.array([[3, 7, 12], [40, 33, 20]], np.int32)      # no waypoint on the way

# name: picture, rect (x0, y0, w, h), rect QP, source, seed.  Source "synth":
# the synthetic source over random references (every block coded, whatever
# the QP); "random": random source pixels over them; (y, c): the synthetic
# source over references of one luma and one chroma value everywhere (small
# residuals: the higher QPs empty some 8x8 blocks, the chroma AC or whole
# MBs; a chroma value off 128 keeps the chroma DC alive)
CASES = {
    "w1": ((64, 64), (0, 0, 1, 3), 30, "synth", 11),
    "w2": ((64, 64), (1, 1, 2, 2), 22, "synth", 12),
    "w3": ((64, 64), (0, 1, 3, 3), 38, (120, 124), 13),
    "w7": ((128, 64), (0, 1, 7, 2), 42, (120, 124), 22),
    "w8": ((176, 64), (2, 0, 8, 2), 46, (120, 124), 14),
    "w9": ((176, 64), (1, 0, 9, 3), 34, (120, 124), 23),
    "w24_random_source": ((384, 64), (0, 0, 24, 2), 30, "random", 15),
    "w25": ((464, 64), (3, 1, 25, 3), 42, (120, 124), 16),
    "w25_general": ((432, 64), (1, 0, 25, 2), 12, "synth", 17),
    "w3_general": ((64, 64), (1, 1, 3, 2), 18, (128, 128), 18),
    "w40": ((672, 64), (1, 1, 40, 2), 38, (110, 116), 24),
    "w41": ((656, 64), (0, 1, 41, 2), 22, "synth", 19),
    "w64": ((1056, 64), (1, 0, 64, 2), 51, (128, 128), 20),
    "w65": ((1040, 64), (0, 1, 65, 3), 46, (128, 120), 21),
}

_want = {}


def flat_refs(w, h, y, c):
    return ArrayRefs([(np.full((h, w), y), np.full((h // 2, w // 2), c), np.full((h // 2, w // 2), c))
                      for _ in range(2)])


def want_of(oracle, name):
    """the case's inputs and the oracle's streams, made once"""
    if name not in _want:
        (w, h), rc, qp, rnd, seed = CASES[name]
        rect = Rect(*rc, qp_field(qp))
        R = flat_refs(w, h, *rnd) if isinstance(rnd, tuple) else random_refs(w, h, seed)
        if rnd == "random":
            src = np.random.default_rng(seed).integers(0, 256, (S, F, 384 * rc[2] * rc[3])).astype(np.uint8)
        else:
            src = synth_source(oracle, S, F, rect)
        _want[name] = (w, h, rect, R, src, oracle_streams(oracle, w, h, OFFS, rect, src, R))
    return _want[name]


def test_oracle_cbp_coverage(oracle):
    """the inputs reach what the MB phase has to get right: every chroma cbp,
    partly coded luma, empty MBs beside coded ones, many distinct patterns"""
    seen, chroma, partial, mixed_row = set(), set(), 0, 0
    for name in CASES:
        w, h, rect, _, _, want = want_of(oracle, name)
        for stream in want:
            nals = split_nals(stream)
            assert len(nals) == F
            for nal in nals:
                rows = {}

                def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
                    if rect.x0 <= x < rect.x0 + rect.w and rect.y0 <= y < rect.y0 + rect.h:
                        rows.setdefault(y, []).append(cbp)

                hp.parse_p_slice(nal, w, h, on_mb=on_mb)
                assert sum(len(v) for v in rows.values()) == rect.w * rect.h
                for v in rows.values():
                    seen.update(v)
                    chroma.update(c >> 4 for c in v)
                    partial += sum(1 for c in v if 0 < (c & 15) < 15)
                    mixed_row += any((a == 0) != (b == 0) for a, b in zip(v, v[1:]))
    print(f"distinct cbp {len(seen)}, chroma {sorted(chroma)}, partly coded luma {partial}, "
          f"rows with an empty MB beside a coded one {mixed_row}")
    assert chroma == {0, 1, 2}
    assert partial > 0
    assert mixed_row > 0
    assert len(seen) >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_mbphase_widths(gpu, oracle, name):
    w, h, rect, R, src, want = want_of(oracle, name)
    b, rc = gpu_streams(gpu, w, h, OFFS, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.gpu
def test_mbphase_with_waypoints(gpu, oracle):
    """waypoints on the way: the MB heads take more than one class"""
    w, h = 64, 512
    rect = Rect(1, 3, 2, 3, qp_field(30))
    offs = np.stack([np.arange(484, 508), np.arange(1004, 980, -1)]).astype(np.int32)   # cross 496 and 992
    R = striped_refs(oracle, w, h)
    src = synth_source(oracle, 2, 24, rect)
    want = oracle_streams(oracle, w, h, offs, rect, src, R)
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    for s in (0, 1):
        assert any(k == 1 and sl == 0 for k, _, _, sl in b.nals(s))
    b.close()
