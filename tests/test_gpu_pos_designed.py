"""The POS instantiations of k_dyn_code / k_dyn_code_general, k_dyn_row,
k_dyn_static and k_dyn_recon (scroll_batch_set_dyn_rect_moving) on the
designed corpus (tests/designed.py): every frame's rect at a position of its
own -- x0 0 (no left neighbour), flush with the right edge, the corpus
origin, one MB row lower, and a frame without a rect -- with its designed
prediction band placed in the references at that x0 (designedprobe.Moved).
tests/test_probe_designed.py proves that the moved frames code the unmoved
levels, so what DESIGN 4b says the corpus reaches holds for these bytes.
Bytes against dynposhelp.oracle_moving, reconstruction and squared errors
against the test decoder per position.  Every comparison is exact.  Run on
an MI355X: -m gpu."""
import pytest

import designedprobe as dp
from dynposhelp import oracle_moving, per_position
from qpfhelp import oracle_qp_frames
from test_gpu_dyn import check_equal, gpu  # noqa: F401
from test_gpu_dyn_pos import batch, compose_ok, load, place

pytestmark = pytest.mark.gpu


def run(gpu, oracle, name, qps=None, recon=False):
    """compose the moved case (qps [2][F]: a per-frame QP table, else the
    case's QP in every stream) and compare the bytes; returns the batch"""
    m = dp.moved(oracle, name)
    per = qps if qps is not None else [[m.qp] * m.F] * 2
    want = [oracle_moving(oracle, m.w, m.h, m.offs[s], m.rw, m.rh, m.pos[s], m.src[s], m.R, per[s])[0]
            for s in range(2)]
    b = batch(gpu, m.w, m.h, 2, m.F, (1, 1, m.rw, m.rh), m.R, recon=recon)
    b.set_dyn_qp(m.qp)
    if qps is not None:
        b.set_dyn_qp_frames(qps)
    place(b, m.pos)
    load(b, m.offs, m.src)
    compose_ok(gpu, b, m.F)
    check_equal(b, want)
    return b, m, per


def check_recon(oracle, b, m, per):
    for s in range(2):
        frames = per_position(lambda rect: oracle_qp_frames(oracle, m.w, m.h, m.offs[s], rect, m.src[s], m.R, per[s],
                                                            decode=True)[1], m.pos[s], m.rw, m.rh)
        for f, fr in enumerate(frames):
            if fr is None:
                assert b.dyn_recon(s, f) is None and b.dyn_sse(s, f) is None, (s, f)
                continue
            assert b.dyn_recon(s, f) == fr["rec"], (s, f)
            assert b.dyn_sse(s, f) == fr["sse"], (s, f)


@pytest.mark.parametrize("name", dp.MOVED_INT8)
def test_int8_rows(gpu, oracle, name):
    assert dp.moved(oracle, name).qp >= 22
    b, m, _ = run(gpu, oracle, name)
    assert b.dyn_totals()[2] == sum(p is not None for row in m.pos for p in row)
    b.close()


@pytest.mark.parametrize("name", dp.MOVED_GENERAL)
def test_general_rows(gpu, oracle, name):
    """k_dyn_code_general -> k_dyn_row<true, POS>: 16-bit levels"""
    assert dp.moved(oracle, name).qp < 22
    b, _, _ = run(gpu, oracle, name)
    b.close()


@pytest.mark.parametrize("name", ["d_extremes_qp22", "e_clamp_qp0"])
def test_reconstruction(gpu, oracle, name):
    b, m, per = run(gpu, oracle, name, recon=True)
    check_recon(oracle, b, m, per)
    b.close()


def test_per_frame_qps_while_the_rect_moves(gpu, oracle):
    """d_extremes' pixels at QPs on both sides of 22 per frame: int8 and
    16-bit rows of one compose at different origins"""
    m = dp.moved(oracle, "d_extremes_qp22")
    qps = [[(22, 0, 30, 21, 12, 27)[(f + 2 * s) % 6] for f in range(m.F)] for s in range(2)]
    assert all(min(q) < 22 <= max(q) for q in qps)
    b, m, per = run(gpu, oracle, "d_extremes_qp22", qps=qps, recon=True)
    check_recon(oracle, b, m, per)
    b.close()
