"""The sized POS instantiations of k_dyn_row, k_dyn_code_general, k_dyn_static
and k_dyn_recon (scroll_batch_set_dyn_rect_size_at) on the
designed corpus (tests/designed.py, untouched): the moved cases of
designedprobe.Moved -- every frame's rect at a position of its own, its
designed prediction band in the references at that x0 -- with every frame
also sized on its own.  A sized frame codes the top-left w_f x h_f MBs of the
case's rect: its source is the designed frame's planes cropped to that
window, laid out as a w_f x h_f rect's at the head of the frame's slot (the
rest of the slot holds noise).  The cropped MBs keep their designed source and
prediction, hence their designed levels: asserted here on the oracle's trace
(extremes, and 16-bit levels on the general path).  Two int8 cases and one
k_dyn_row<true, POS> case.  Bytes against dynsizehelp.sized_streams,
reconstruction and squared errors against the test decoder per rect.  Every
comparison is exact.  Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import designedprobe as dp
from dynsizehelp import per_rect, sized_streams
from maskhelp import planes
from probehelp import oracle_probe
from qpfhelp import oracle_qp_frames
from test_gpu_dyn import check_equal, gpu  # noqa: F401
from test_gpu_dyn_size import batch, compose_ok, load, place

pytestmark = pytest.mark.gpu


def sizes_of(rw, rh, s, f):
    """the frame's own size: full, one column short, one MB, one row short (or
    half the columns where the rect has one row), half the columns -- in turn"""
    opts = [(rw, rh), (rw - 1, rh), (1, 1), (rw, rh - 1) if rh > 1 else (rw // 2 + 1, rh), (max(1, rw // 2), rh)]
    return opts[(f + 2 * s) % len(opts)]


def crop(slot, rw, rh, wf, hf):
    """the top-left wf x hf MBs of a rw x rh rect-layout block, in the sized layout"""
    y, cb, cr = planes(slot, rw, rh)
    return np.concatenate([y[:16 * hf, :16 * wf].reshape(-1), cb[:8 * hf, :8 * wf].reshape(-1),
                           cr[:8 * hf, :8 * wf].reshape(-1)]).astype(np.uint8)


def sized_case(oracle, name):
    """(the moved case, rects [2][F], sources [2][F][384 rw rh] with each
    frame's cropped block at the head of its slot)"""
    m = dp.moved(oracle, name)
    rects = [[None if m.pos[s][f] is None else (*m.pos[s][f], *sizes_of(m.rw, m.rh, s, f)) for f in range(m.F)]
             for s in range(2)]
    src = np.random.default_rng(7).integers(0, 256, m.src.shape, dtype=np.uint8)
    for s in range(2):
        for f in range(m.F):
            if rects[s][f]:
                v = crop(m.src[s][f], m.rw, m.rh, *rects[s][f][2:])
                src[s, f, :len(v)] = v
    sizes = {rc[2:] for row in rects for rc in row if rc}
    assert (m.rw, m.rh) in sizes and len(sizes) >= 3 and (1, 1) in sizes
    return m, rects, src


def levels_of(oracle, m, rects, src, s):
    """per sized frame of stream s: every coded level of the oracle's trace"""
    out = []
    frames = per_rect(lambda rc: oracle_probe(oracle, m.w, m.h, m.offs[s], rc,
                                              np.ascontiguousarray(src[s][:, :384 * rc[2] * rc[3]]), m.R, m.qp)[1],
                      rects[s])
    for fr in frames:
        if fr is not None:
            out.append([v for _, b in dp.blocks_of(fr["mbs"]) for v in b if v])
    return out


def reach(oracle, m, rects, src):
    """the largest level the sized frames code; in each stream a frame SMALLER
    than the case's rect codes levels, three of them over both streams (one
    designed frame of the extremes is all prediction: it codes none at any size)"""
    top, total = 0, 0
    for s in range(2):
        small = 0
        for rc, lv in zip([rc for rc in rects[s] if rc], levels_of(oracle, m, rects, src, s)):
            if lv:
                top = max(top, max(abs(v) for v in lv))
                small += rc[2:] != (m.rw, m.rh)
        assert small >= 1, (s, small)
        total += small
    assert total >= 3, total
    return top


def run(gpu, oracle, name, recon=True):
    m, rects, src = sized_case(oracle, name)
    per = [[m.qp] * m.F] * 2
    b = batch(gpu, m.w, m.h, 2, m.F, (1, 1, m.rw, m.rh), m.R, recon=recon)
    b.set_dyn_qp(m.qp)
    place(b, rects)
    load(b, m.offs, src)
    compose_ok(gpu, b, m.F)
    check_equal(b, sized_streams(oracle, m.w, m.h, m.offs, rects, src, m.R, qps=per))
    for s in range(2):
        frames = per_rect(lambda rc: oracle_qp_frames(oracle, m.w, m.h, m.offs[s], rc,
                                                      np.ascontiguousarray(src[s][:, :384 * rc[2] * rc[3]]), m.R,
                                                      per[s], decode=True)[1], rects[s])
        for f, fr in enumerate(frames):
            if fr is None:
                assert b.dyn_recon(s, f) is None and b.dyn_sse(s, f) is None, (s, f)
                continue
            assert b.dyn_recon(s, f)[:len(fr["rec"])] == fr["rec"], (s, f)
            assert b.dyn_sse(s, f) == fr["sse"], (s, f)
    assert b.dyn_totals()[2] == sum(rc is not None for row in rects for rc in row)
    b.close()
    return m, rects, src


@pytest.mark.parametrize("name", ["a_walk", "d_extremes_qp22"])
def test_int8_rows_at_sizes_of_their_own(gpu, oracle, name):
    """k_dyn_row<false, POS>: a 16-MB row of the coeff_token / total_zeros walk
    and the 4-MB rows of the extremes, int8 levels"""
    assert name in dp.MOVED_INT8 and dp.moved(oracle, name).qp >= 22
    m, rects, src = run(gpu, oracle, name)
    top = reach(oracle, m, rects, src)
    print(name, "largest level", top)
    assert top >= (255 if name == "d_extremes_qp22" else 2)    # the extremes' chroma DC; the walk's +-1 / +-2


def test_general_rows_at_sizes_of_their_own(gpu, oracle):
    """k_dyn_code_general -> k_dyn_row<true, POS>: the extremes at QP 0, 16-bit levels"""
    name = "e_extremes_qp0"
    assert name in dp.MOVED_GENERAL and dp.moved(oracle, name).qp < 22
    m, rects, src = run(gpu, oracle, name)
    top = reach(oracle, m, rects, src)
    print(name, "largest level", top)
    assert top == 2063                                         # the clamp: past what an int8 record holds
