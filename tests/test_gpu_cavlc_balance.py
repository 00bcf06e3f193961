"""k_dyn_row's CAVLC phase (the counting sort's order coded in passes of one
block per thread, cavlc_body_t with its lean level loop).  Byte for byte
against oracle/dyn_oracle.c at the rect widths where the number of 64-block
chunks of the sorted order and the number of waves change:

  w = 1     one wave, one chunk
  w = 3     one wave, two chunks: two passes
  w = 8     one wave filled exactly, three chunks
  w = 9     the first width with two waves (128 threads): four chunks, the
            polling wave is the chroma DC wave's neighbour
  w = 24    192 threads filled exactly: nine chunks on three waves
  w = 25    config 3's 256 threads and 10 chunks: three passes, the last short
  w = 41    320 threads, four block tasks per thread: 16 chunks on five waves
  w = 47    config 5's width: 18 chunks

each with the synthetic source at QP 22 (every block coded and heavy: every
chunk full) and with flat references at QP 42-46 (most blocks empty: few
chunks, whole waves without one), and a random source at QP 22 whose oracle
bytes show blocks with TotalCoeff 16 (the level loop's longest run).  A case
that falls short gets another seed, never a weaker condition.
Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import h264_pslice as hp
from dynhelp import Rect, qp_field, split_nals
from test_gpu_dyn import check_equal, gpu, gpu_streams, oracle_streams, random_refs, synth_source  # noqa: F401
from test_gpu_dyn_mbphase import F, OFFS, S, flat_refs

# name: picture, rect (x0, y0, w, h), rect QP, source ("synth" over random
# references, "random" pixels over them, (y, c): synthetic over flat ones), seed
CASES = {
    "w1_heavy": ((64, 64), (1, 0, 1, 3), 22, "synth", 31),
    "w1_sparse": ((64, 64), (0, 1, 1, 3), 42, (120, 124), 32),
    "w3_heavy": ((64, 64), (0, 1, 3, 3), 22, "synth", 33),
    "w3_sparse": ((64, 64), (1, 0, 3, 3), 44, (120, 124), 34),
    "w8_heavy": ((176, 64), (2, 0, 8, 2), 22, "synth", 35),
    "w8_sparse": ((176, 64), (1, 1, 8, 3), 46, (120, 124), 36),
    "w9_heavy": ((176, 64), (1, 0, 9, 3), 22, "synth", 44),
    "w9_sparse": ((176, 64), (2, 1, 9, 2), 42, (120, 124), 45),
    "w24_heavy": ((400, 64), (1, 1, 24, 2), 22, "synth", 46),
    "w25_heavy": ((464, 64), (3, 1, 25, 3), 22, "synth", 37),
    "w25_sparse": ((432, 64), (1, 0, 25, 3), 42, (120, 124), 38),
    "w41_heavy": ((656, 64), (0, 1, 41, 2), 22, "synth", 39),
    "w41_sparse": ((672, 64), (1, 0, 41, 3), 44, (120, 124), 40),
    "w47_heavy": ((768, 64), (1, 1, 47, 2), 22, "synth", 41),
    "w47_sparse": ((752, 64), (0, 0, 47, 3), 46, (120, 124), 42),
    "w25_random_source": ((464, 64), (2, 1, 25, 2), 22, "random", 43),
}

_want = {}


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


def block_counts(oracle, name):
    """per rect row of the oracle's bytes: the TotalCoeffs of its 24 w blocks"""
    w, h, rect, _, _, want = want_of(oracle, name)
    rows = []
    for stream in want:
        nals = split_nals(stream)
        assert len(nals) == F
        for nal in nals:
            per = {}

            def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
                if rect.x0 <= x < rect.x0 + rect.w and rect.y0 <= y < rect.y0 + rect.h:
                    tcs = per.setdefault(y, [])
                    tcs.extend(sum(1 for c in blk if c) for blk in luma)
                    tcs.extend(sum(1 for c in blk if c) for plane in cac for blk in plane)

            hp.parse_p_slice(nal, w, h, on_mb=on_mb)
            assert len(per) == rect.h and all(len(v) == 24 * rect.w for v in per.values())
            rows.extend(per.values())
    return rows


def test_oracle_block_coverage(oracle):
    """the inputs reach what the body passes have to get right, seen in the
    oracle's own bytes: rows whose coded blocks fill every chunk, rows with
    fewer chunks than waves, rows with none, and blocks with TotalCoeff 16"""
    for name in CASES:
        rows = block_counts(oracle, name)
        w = CASES[name][1][2]
        coded = [sum(1 for t in r if t) for r in rows]
        print(f"{name}: coded blocks per row {min(coded)}..{max(coded)} of {24 * w}, "
              f"max TotalCoeff {max(max(r) for r in rows)}")
        if name.endswith("_heavy"):
            assert min(coded) > 0.9 * 24 * w, (name, min(coded))
            assert max(max(r) for r in rows) >= 12, name
        if name.endswith("_sparse"):
            assert max(coded) > 0, name
            assert min(coded) < 0.5 * 24 * w, (name, min(coded))
    nwv = {25: 4, 41: 5, 47: 5}
    for name in ("w25_sparse", "w41_sparse", "w47_sparse"):
        rows = block_counts(oracle, name)
        chunks = [-(-sum(1 for t in r if t) // 64) for r in rows]
        assert min(chunks) < nwv[CASES[name][1][2]], (name, chunks)
    full = sum(1 for r in block_counts(oracle, "w25_random_source") for t in r if t == 16)
    print(f"w25_random_source: {full} blocks with TotalCoeff 16")
    assert full > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_cavlc_balance_widths(gpu, oracle, name):
    w, h, rect, R, src, want = want_of(oracle, name)
    b, rc = gpu_streams(gpu, w, h, OFFS, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()
