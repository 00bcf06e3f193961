"""The dynamic-rect kernels against the designed corpus (tests/designed.py),
byte for byte with the oracle's cached streams.  What the corpus reaches --
every CAVLC table entry, every level triple, the level table's edge 47 / 48
in every class, levels +-127 at QP 22 and +-2063 below, blocks of 64 / 65 /
128 / 129 bits -- is proven from those same streams, without a GPU, by
tests/test_designed_oracle.py.

  plain path     k_dyn_code -> k_dyn_row, int8 records: groups a-d (QP >= 22)
  general path   k_dyn_code_general -> k_dyn_row<true>, 16-bit levels: group e,
                 group a designed again at QP 20 and its QP-28 pixels at QP 16
  mixed batch    streams of one launch at QPs on both sides of 22
  large NALs     SCROLL_DEBUG_DYN_EPCAP4 / _EPWIN on the EP-dense and extreme cases
  hinted coder   k_hdyn_code: the rect under hints (no hint rects, EXACT), moved
                 per frame, QPs per frame on both sides of 22; the fallback's
                 whole-frame rect
  reconstruction k_dyn_recon / k_hdyn_recon: recon bytes and SSE, clipping at
                 both ends
Every picture is tiny.  Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import designed as dz
import test_gpu_recon as tr
import test_gpu_recon_hint as th
from dynhelp import Rect
from hreconhelp import EXACT
from reconhelp import ArrayRefs
from test_gpu_dyn import check_equal, gpu, gpu_streams, oracle_streams  # noqa: F401
from test_gpu_hintdyn import apply_plan, gpu_batch, oracle_hintdyn

pytestmark = pytest.mark.gpu


def run_plain(gpu, oracle, name, qp=None, debug=0):
    c = dz.cases(oracle)[name]
    want = dz.want_of(oracle, name, qp)
    b, rc = gpu_streams(gpu, c.w, c.h, c.offs, c.rect(qp), c.R, c.src, debug=debug)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    return b, c


@pytest.mark.parametrize("name", dz.names("a", "b", "c", "d"))
def test_plain_path(gpu, oracle, name):
    assert dz.cases(oracle)[name].qp >= 22
    b, _ = run_plain(gpu, oracle, name)
    b.close()


@pytest.mark.parametrize("name,qp", [(n, None) for n in dz.names("a20", "e")] + [("a_walk", 16), ("a_tzrb", 16)])
def test_general_path(gpu, oracle, name, qp):
    assert (qp if qp is not None else dz.cases(oracle)[name].qp) < 22
    b, _ = run_plain(gpu, oracle, name, qp)
    b.close()


MIXED_QPS = [22, 21, 30, 0, 27]          # two general-path streams: within the batch's record pool


@pytest.mark.parametrize("name", ["b_levels_qp22", "b_searched_qp22", "d_extremes_qp22", "d_epdense_qp22",
                                  "e_levels_qp21", "e_extremes_qp0", "e_clamp_qp0"])
def test_mixed_batch(gpu, oracle, name):
    """five streams of one batch at QPs on both sides of 22: int8 and 16-bit
    rows share every launch"""
    c = dz.cases(oracle)[name]
    pick = [k % 2 for k in range(len(MIXED_QPS))]
    offs, src = c.offs[pick], c.src[pick]
    want = []
    for s, q in enumerate(MIXED_QPS):
        want += oracle_streams(oracle, c.w, c.h, offs[s:s + 1], c.rect(q), src[s:s + 1], c.R)
    b, rc = gpu_streams(gpu, c.w, c.h, offs, Rect(*c.rc), c.R, src, stream_qp=dict(enumerate(MIXED_QPS)))
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.parametrize("flag,cap", [("SCROLL_DEBUG_DYN_EPCAP4", 4), ("SCROLL_DEBUG_DYN_EPWIN", 7)])
@pytest.mark.parametrize("name", ["d_epdense_qp22", "e_epdense_qp12", "d_extremes_qp22", "e_extremes_qp0",
                                  "e_extremes_qp12"])
def test_large_nal_and_window_paths(gpu, oracle, name, flag, cap):
    """k_dyn_emit (EP list capped at 4) and the EP windows of k_dyn_gather (7
    positions a window): the EP-dense cases hold far more EP bytes than
    either cap in two of their three frames"""
    b, c = run_plain(gpu, oracle, name, debug=getattr(gpu, flag))
    eps = [b.dyn_frame_info(s, t)[1] for s in range(2) for t in range(c.F)]
    if "epdense" in name:
        assert sum(e > cap for e in eps) >= 4, eps
        assert max(eps) > 50, eps
    b.close()


# ------------------------------------------------------------- hinted coder --
SLOT = 2048                               # slot bytes per MB: an MB's region under hints at its bound,
                                          # MB_BITS_MAX / 8 (the default 512 holds no extreme MB below QP 16)


def hinted_plan(c):
    """no hint rects, EXACT; the rect one MB row lower in the frames whose
    offset allows it, the offset 16 less there (the same prediction rows);
    QPs per frame: the case's, and every third frame on the other side of 22"""
    offs = c.offs.copy()
    plan_ = {}
    for s in range(2):
        for f in range(c.F):
            dy = 1 if (offs[s, f] >= 16 and f % 2) else 0
            offs[s, f] -= 16 * dy
            plan_[(s, f)] = ([], EXACT, (dz.X0, dz.Y0 + dy))
    other = 16 if c.qp >= 22 else 28
    return offs, plan_, (lambda s, f: other if f % 3 == 2 else c.qp)


@pytest.mark.parametrize("name", dz.names("a", "b", "d"))
def test_hinted_coder(gpu, oracle, name):
    c = dz.cases(oracle)[name]
    offs, plan_, qp_of = hinted_plan(c)
    if c.F > 1:
        assert any(p[2][1] != dz.Y0 for p in plan_.values())
    h = c.h + 16                                      # room for the rect one row lower
    R = ArrayRefs([tuple(np.pad(p, ((0, 16 if k == 0 else 8), (0, 0)), constant_values=128)
                         for k, p in enumerate(c.R.planes[0]))] * 2)
    want = oracle_hintdyn(oracle, c.w, h, offs, c.rw, c.rh, plan_, c.src, R, qp_of=qp_of)
    b = gpu_batch(gpu, c.w, h, 2, c.F, c.rc, R)
    apply_plan(b, plan_, c.F)
    for (s, f) in plan_:
        b.set_dyn_qp_at(s, f, qp_of(s, f))
    b.set_offsets(np.ascontiguousarray(offs))
    b.set_dyn_source(c.src.tobytes(), c.F)
    b.compose(c.F)
    assert b.sync() == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


def whole_frame_extremes(oracle):
    """the extreme frames 0, 2 and 3 (both colours, the largest MBs) stacked
    into one 4 x 6-MB picture that is all rect: the references are its
    prediction, offset 0"""
    fr = dz.cases(oracle)["d_extremes_qp22"].frames
    s = [np.concatenate([fr[0].s[k], fr[2].s[k], fr[3].s[k]]) for k in range(3)]
    p = [np.concatenate([fr[0].p[k], fr[2].p[k], fr[3].p[k]]) for k in range(3)]
    src = np.concatenate([a.reshape(-1) for a in s]).astype(np.uint8)
    return 64, 96, 4, 6, src, ArrayRefs([tuple(p), tuple(p)])


@pytest.mark.parametrize("qp", [22, 0])
def test_fallback_whole_frame_extremes(gpu, oracle, qp):
    """a hint on a reference the frame lacks, scroll_batch_set_fallback: the
    picture is coded as one whole-frame rect of the extreme MBs; bytes,
    reconstruction and SSE; at QP 22 the decoder clips at both ends (at QP 0
    the decoded picture is the source to within a sample: nothing overshoots)"""
    w, h, rw, rh, src1, R = whole_frame_extremes(oracle)
    offs = np.array([[0]], np.int32)
    src = src1[None, None]
    plans = [[([(0, 0, 2, 2, 2 + 6, 16, -32)], EXACT, (0, 0))]]      # waypoint 6: never valid here
    clips = [0, 0]
    want = th.expect(oracle, w, h, offs, plans, rw, rh, src, R, fallback=True, qp_of=lambda s, f: qp, clips=clips)
    assert want[0][1][0]["fell"]
    assert qp < 21 or (clips[0] > 0 and clips[1] > 0), clips
    b = th.make_batch(gpu, w, h, (0, 0, rw, rh), 1, 1, R, slot=SLOT * rw * rh, fallback=True)
    th.apply_plans(b, plans, qp_of=lambda s, f: qp)
    th.compose(b, offs, src)
    assert b.sync() == 0, gpu.last_error()
    assert b.output(0) == want[0][0]
    assert b.fallback_frame(0, 0) == 1
    th.check_frames(b, want, src, rw, rh)
    b.close()


# ----------------------------------------------------------- reconstruction --
# the cases whose decoded picture overshoots 0 and 255 before the clip: large
# residuals at a coarse quantiser.  At QP 0-5 the quantiser is close to
# lossless and the clamped chroma DC (2063 of up to 3264) undershoots, so the
# saturated cases there never reach the clip; their dequantiser range is
# checked through the recon bytes
CLIPPING = {"b_levels_qp22", "b_levels_qp24", "b_searched_qp22", "e_levels_qp10", "e_levels_qp21",
            "e_extremes_qp12", "e_extremes_qp21"} | {f"d_extremes_qp{q}" for q in range(22, 28)}
RECON = dz.names("b", "d", "e")


@pytest.mark.parametrize("name", RECON)
def test_reconstruction(gpu, oracle, name):
    """k_dyn_recon on stream 0 of the case: recon bytes and the three SSE
    integers equal the test decoder's, the emitted bytes stay the oracle's;
    the CLIPPING cases clip at both ends (asserted on the expectation first)"""
    c = dz.cases(oracle)[name]
    offs, src = c.offs[:1], c.src[:1]
    clips = [0, 0]
    want = tr.expect(oracle, c.w, c.h, c.rc, offs, src, c.R, qps=[c.qp], clips=clips)
    assert want[0][0] == dz.want_of(oracle, name)[0]
    if name in CLIPPING:
        assert clips[0] > 0 and clips[1] > 0, clips
    b = tr.make_batch(gpu, c.w, c.h, c.rc, 1, c.F, c.R, qps=[c.qp])
    tr.compose(gpu, b, offs, src)
    assert b.output(0) == want[0][0]
    tr.check_frames(b, want, src, c.rc)
    b.close()


@pytest.mark.parametrize("name", ["b_searched_qp22", "d_extremes_qp22", "e_extremes_qp0", "e_clamp_qp0",
                                  "e_clamp_qp3"])
def test_reconstruction_hinted(gpu, oracle, name):
    """k_hdyn_recon: the same under hints (no hint rects, EXACT, the rect in
    place), the QP per frame"""
    c = dz.cases(oracle)[name]
    offs, src = c.offs[:1], c.src[:1]
    plans = [[([], EXACT, (dz.X0, dz.Y0)) for _ in range(c.F)]]
    clips = [0, 0]
    want = th.expect(oracle, c.w, c.h, offs, plans, c.rw, c.rh, src, c.R, qp_of=lambda s, f: c.qp, clips=clips)
    if name in CLIPPING:
        assert clips[0] > 0 and clips[1] > 0, clips
    b = th.make_batch(gpu, c.w, c.h, (0, 0, c.rw, c.rh), 1, c.F, c.R, slot=SLOT * c.rw * c.rh)
    th.apply_plans(b, plans, qp_of=lambda s, f: c.qp)
    th.compose(b, offs, src)
    assert b.sync() == 0, gpu.last_error()
    assert b.output(0) == want[0][0]
    th.check_frames(b, want, src, c.rw, c.rh)
    b.close()
