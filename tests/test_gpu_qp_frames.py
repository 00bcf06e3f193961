"""GPU check of the plain dynamic rect at a QP of its own per frame
(scroll_batch_set_dyn_qp_frames: k_dyn_rows resolves it, k_dyn_code_general /
k_dyn_row / k_dyn_static / k_dyn_recon code at it) and of the pick that
chooses those QPs on the device from the probe (scroll_batch_dyn_pick,
k_dyn_pick).  Bytes against the oracle called per frame with the frame's QP
(tests/qpfhelp.py; tests/test_qp_frames_oracle.py pins that premise), the
reconstruction against the test decoder at that QP, the pick against the
numpy restatement of its rule on the probe's own array.  Every comparison is
exact.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from probehelp import constant_of, load, make_batch, oracle_probe, rbsp_bits, synth
from qpfhelp import bucket_np, cost_of, oracle_qp_frames, pick_np
from reconhelp import random_refs, striped_refs

pytestmark = pytest.mark.gpu

QPS6 = [0, 12, 22, 26, 39, 51]


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def compose_ok(gpu, b, F):
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()


def test_mixed_qps_across_the_int8_line(gpu, oracle):
    """one stream with QP-12 / 0 / 21 NALs (general path, 16-bit levels)
    beside QP-22 / 26 / 30 / 51 NALs (int8) in one compose; a stream whose
    entries are all -1 at its own QP 18; a stream without entries"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    S, F = 3, 8
    offs = np.array([[0, 5, 40, 96, 41, 6, 13, 77], [96, 41, 6, 0, 5, 40, 33, 9], [3, 30, 50, 64, 17, 95, 1, 48]],
                    np.int32)
    R = random_refs(w, h, 11)
    src = synth(oracle, S, F, rect)
    table = [12, 30, 0, 26, 51, 21, 22, -1]
    want_qp = [[12, 30, 0, 26, 51, 21, 22, 26], [18] * F, [26] * F]
    b = make_batch(gpu, w, h, rect, S, F, R, qps=[26, 18, 26], recon=True)
    b.set_dyn_qp_frames(table, stream=0)
    b.set_dyn_qp_frames([-1] * F, stream=1)
    assert b.dyn_qp_frames(F).tolist() == [table, [-1] * F, [-1] * F]
    load(b, offs, src)
    compose_ok(gpu, b, F)
    for s in range(S):
        want, frames = oracle_qp_frames(oracle, w, h, offs[s], rect, src[s], R, want_qp[s], decode=True)
        assert b.output(s) == want, s
        for f, fr in enumerate(frames):
            assert b.dyn_recon(s, f) == fr["rec"], (s, f)
            assert b.dyn_sse(s, f) == fr["sse"], (s, f)
    b.close()


def test_frame_index_not_nal_index(gpu, oracle):
    """waypoint NALs between the scroll NALs: the table is indexed by frame.
    Then the experiment mode, where frame 2 has no dynamic NAL and its entry
    is ignored"""
    w, h, rect = 64, 512, (1, 20, 2, 6)
    R = striped_refs(oracle, w, h)
    offs = np.array([[0, 17, 496, 500, 505, 400, 300]], np.int32)
    F = offs.shape[1]
    qps = [20, 33, 21, 32, 22, 31, 23]
    src = synth(oracle, 1, F, rect)
    b = make_batch(gpu, w, h, rect, 1, F, R)
    b.set_dyn_qp_frames(qps, stream=0)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    want, frames = oracle_qp_frames(oracle, w, h, offs[0], rect, src[0], R, qps)
    assert len(b.nals(0)) > F                  # waypoint NALs sit between the scroll NALs
    assert b.output(0) == want
    b.close()
    offs = np.array([[0, 17, 496, 300]], np.int32)
    qps = [20, 33, 5, 31]
    b = make_batch(gpu, w, h, rect, 1, 4, R, mode=gpu.SCROLL_MODE_EXPERIMENT)
    b.set_dyn_qp_frames(qps, stream=0)
    load(b, offs, src[:, :4])
    compose_ok(gpu, b, 4)
    want, frames = oracle_qp_frames(oracle, w, h, offs[0], rect, src[0, :4], R, qps, mode=1)
    assert [fr is None for fr in frames] == [False, False, True, False]
    assert b.output(0) == want
    b.close()


@pytest.mark.parametrize("rect", [(11, 0, 1, 4), (0, 1, 12, 2), (0, 1, 17, 2)])
def test_row_widths(gpu, oracle, rect):
    """rows of 1, 12 and 17 MBs, a QP-10 frame (general path) beside a QP-40 one"""
    w, h = max(192, 16 * (rect[0] + rect[2])), 64
    offs = np.array([[3, 30]], np.int32)
    R = random_refs(w, h, 41)
    src = synth(oracle, 1, 2, rect)
    b = make_batch(gpu, w, h, rect, 1, 2, R)
    b.set_dyn_qp_frames([[10, 40]])
    load(b, offs, src)
    compose_ok(gpu, b, 2)
    assert b.output(0) == oracle_qp_frames(oracle, w, h, offs[0], rect, src[0], R, [10, 40])[0]
    b.close()


def test_chunked_composes(gpu, oracle):
    """the table set once applies to frame f of every compose; clearing it
    gives the streams' QPs again; set_dyn_rect drops it"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    S, F = 2, 4
    R = random_refs(w, h, 23)
    offs = np.array([[0, 5, 40, 96, 41, 6, 13, 77, 3, 30, 50, 64, 17, 95, 1, 48],
                     [96, 41, 6, 0, 5, 40, 33, 9, 12, 13, 50, 77, 8, 21, 60, 90]], np.int32)
    src = synth(oracle, S, 16, rect)
    table = [12, 30, 22, -1]
    b = make_batch(gpu, w, h, rect, S, F, R, qps=[26, 35])
    b.set_dyn_qp_frames(table)                 # every stream
    for c in range(2):
        load(b, offs[:, 4 * c:4 * c + 4], src[:, 4 * c:4 * c + 4])
        compose_ok(gpu, b, F)
    b.clear_dyn_qp_frames()
    assert (b.dyn_qp_frames(F) == -1).all()
    load(b, offs[:, 8:12], src[:, 8:12])
    compose_ok(gpu, b, F)
    b.set_dyn_qp_frames(table)
    b.set_dyn_rect(*rect)                      # a new rect: no table, the streams' QPs
    b.set_dyn_refs(R.i420(0), R.i420(1))
    assert (b.dyn_qp_frames(F) == -1).all()
    assert gpu.lib.scroll_batch_dyn_pick_result(b.h, 0, 0, None, None) == gpu.SCROLL_ERR_CONFIG
    load(b, offs[:, 12:16], src[:, 12:16])
    compose_ok(gpu, b, F)
    for s, own in enumerate([26, 35]):
        per = [own if q < 0 else q for q in table]
        assert b.output(s) == oracle_qp_frames(oracle, w, h, offs[s], rect, src[s], R, per + per + [own] * 8)[0], s
    b.close()


def test_contract(gpu, oracle):
    w, h, rect = 96, 96, (1, 1, 4, 4)
    lib, R = gpu.lib, random_refs(w, h, 61)
    F = 2
    i8 = lambda v: (ctypes.c_int8 * len(v))(*v)
    # no dynamic rect
    b0 = gpu.Batch(1, F, 1 << 20)
    b0.add_stream(gpu.make_config(w, h))
    assert lib.scroll_batch_set_dyn_qp_frames(b0.h, 0, 0, 2, i8([30, 30])) == gpu.SCROLL_ERR_CONFIG
    assert b0.dyn_qp_frames_device()[0] is None
    b0.close()
    # a stream with the deblocking filter on keeps QP 26
    b = gpu.Batch(2, F, 8 << 20)
    b.add_stream(gpu.make_config(w, h))
    b.add_stream(gpu.make_config(w, h, deblock=0))
    b.set_dyn_rect(*rect)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    assert (b.dyn_qp_frames(F) == -1).all()    # before the table exists
    assert lib.scroll_batch_set_dyn_qp_frames(b.h, 1, 0, 2, i8([26, 30])) == gpu.SCROLL_ERR_CONFIG
    assert "deblocking filter on" in gpu.last_error()
    assert lib.scroll_batch_set_dyn_qp_frames(b.h, -1, 0, 1, i8([30])) == gpu.SCROLL_ERR_CONFIG
    assert lib.scroll_batch_set_dyn_qp_frames(b.h, 1, 0, 2, i8([26, -1])) == 0
    assert (b.dyn_qp_frames(F) == [[-1, -1], [26, -1]]).all()
    # argument errors
    for s, f0, n, v in ((2, 0, 1, [30]), (-2, 0, 1, [30]), (0, -1, 1, [30]), (0, 2, 1, [30]), (0, 1, 2, [30, 30]),
                        (0, 0, -1, [30]), (0, 0, 1, [52]), (0, 0, 1, [-2])):
        assert lib.scroll_batch_set_dyn_qp_frames(b.h, s, f0, n, i8(v)) == gpu.SCROLL_ERR_ARG, (s, f0, n, v)
    assert lib.scroll_batch_set_dyn_qp_frames(b.h, 0, 0, 1, None) == gpu.SCROLL_ERR_ARG
    out = i8([0, 0])
    for s, f0, n in ((2, 0, 1), (-1, 0, 1), (0, 2, 1), (0, 1, 2)):
        assert lib.scroll_batch_dyn_qp_frames(b.h, s, f0, n, out) == gpu.SCROLL_ERR_ARG
    ptr, ls = b.dyn_qp_frames_device()
    assert ptr and ls == F
    # the pick's refusals: no probe yet, an unknown mode, no rate
    rate = gpu.ScrollDynRate(gpu.SCROLL_DYN_RATE_FRAME, 1000, 0, 0)
    assert lib.scroll_batch_dyn_pick(b.h, F, ctypes.byref(rate), None, None) == gpu.SCROLL_ERR_CONFIG
    assert lib.scroll_batch_dyn_pick_result(b.h, 0, 0, None, None) == gpu.SCROLL_ERR_CONFIG
    assert lib.scroll_batch_dyn_pick(b.h, F, None, None, None) == gpu.SCROLL_ERR_ARG
    bad = gpu.ScrollDynRate(7, 1000, 0, 0)
    assert lib.scroll_batch_dyn_pick(b.h, F, ctypes.byref(bad), None, None) == gpu.SCROLL_ERR_ARG
    # a probe returns the same arrays with a table set as without
    offs = np.array([[5, 40], [96, 41]], np.int32)
    src = synth(oracle, 2, F, rect)
    load(b, offs, src)
    b.clear_dyn_qp_frames()
    before = b.dyn_probe(F, [12, 26, 39])
    b.set_dyn_qp_frames([12, 40], stream=0)
    after = b.dyn_probe(F, [12, 26, 39])
    assert before["valid"].all() and (before == after).all()
    # nframes beyond the last probe's
    b.dyn_probe(1, [26, 30])
    assert lib.scroll_batch_dyn_pick(b.h, 2, ctypes.byref(rate), None, None) == gpu.SCROLL_ERR_CONFIG
    # a compose under hints with the table set is refused and commits nothing
    compose_ok(gpu, b, F)
    size, cfg = [b.output_size(s) for s in range(2)], [bytes(b.config(s)) for s in range(2)]
    b.set_hints(0, 0, [(0, 0, 6, 1, 0, 0, 0)])
    assert lib.scroll_batch_compose(b.h, F, None) == gpu.SCROLL_ERR_CONFIG
    assert "scroll_batch_clear_dyn_qp_frames" in gpu.last_error()
    assert b.sync() == 0
    assert [b.output_size(s) for s in range(2)] == size and [bytes(b.config(s)) for s in range(2)] == cfg
    # ... and so are the setter, the pick and a pick after the hinted probe's turn
    assert lib.scroll_batch_set_dyn_qp_frames(b.h, 0, 0, 1, i8([30])) == gpu.SCROLL_ERR_CONFIG
    assert lib.scroll_batch_dyn_pick(b.h, 1, ctypes.byref(rate), None, None) == gpu.SCROLL_ERR_CONFIG
    b.clear_hints()
    compose_ok(gpu, b, F)
    want = oracle_qp_frames(oracle, w, h, list(offs[0]) * 2, rect, np.concatenate([src[0], src[0]]), R,
                            [12, 40, 12, 40])[0]
    assert b.output(0) == want
    # set_dyn_qp_at names the call that does this without hints
    assert lib.scroll_batch_set_dyn_qp_at(b.h, 0, 0, 30) == gpu.SCROLL_ERR_ARG
    assert "scroll_batch_set_dyn_qp_frames" in gpu.last_error()
    b.close()


def pick_batch(gpu, w, h, rect, S, F, R, deblock0=()):
    b = gpu.Batch(S, F, 8 << 20)
    for s in range(S):
        b.add_stream(gpu.make_config(w, h, deblock=0 if s in deblock0 else 1))
    b.set_dyn_rect(*rect)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    b.set_dyn_recon()
    return b


def test_pick_end_to_end(gpu, oracle):
    """probe -> dyn_pick (FRAME mode) -> compose: the device's choices are
    the rule's on the probe's array, and the compose delivers them"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    S, F = 4, 6
    R = random_refs(w, h, 91)
    offs = np.array([[0, 5, 40, 96, 41, 6], [96, 41, 6, 0, 5, 40], [3, 30, 50, 64, 17, 95], [13, 77, 33, 9, 1, 48]],
                    np.int32)
    src = synth(oracle, S, F, rect)
    b = pick_batch(gpu, w, h, rect, S, F, R, deblock0=(3,))
    load(b, offs, src)
    res = b.dyn_probe(F, QPS6)
    assert res["valid"].all()
    cost = cost_of(res, QPS6)
    budget = int(cost[0, 0].min() + cost[0, 0].max()) // 2
    wk = np.full((S, F), -1, np.int32)
    wst = np.full((S, F), 2, np.int32)
    for s in range(3):                         # stream 3 keeps QP 26: its filter is on
        for f in range(F):
            wk[s, f], wst[s, f] = pick_np(res[s, f], QPS6, budget)
    wqp = np.where(wk >= 0, np.array(QPS6)[np.maximum(wk, 0)], -1)
    print("budget", budget, "\nk", wk, "\nstatus", wst)
    assert (wst == 0).any() and (wk[wst == 0] > 0).any()
    k, qp, st = b.dyn_pick(F, budget)
    assert (k == wk).all() and (qp == wqp).all() and (st == wst).all()
    assert (b.dyn_qp_frames(F) == wqp).all()
    compose_ok(gpu, b, F)
    for s in range(S):
        per = [26 if q < 0 else int(q) for q in wqp[s]]
        want, frames = oracle_qp_frames(oracle, w, h, offs[s], rect, src[s], R, per, deblock=0 if s == 3 else 1)
        assert b.output(s) == want, s
        if s == 3:
            continue
        at26 = oracle_probe(oracle, w, h, offs[s], rect, src[s], R, 26, decode=False)[1]
        for f in range(F):
            assert b.dyn_sse(s, f) == tuple(int(v) for v in res[s, f, wk[s, f]]["sse"]), (s, f)
            assert rbsp_bits(frames[f]["nal"]) - constant_of(at26[f], 26) == cost[s, f, wk[s, f]], (s, f)
    b.close()


def test_bucket_mode(gpu, oracle):
    """two picks of three frames on one batch carry the level; reading,
    setting and resetting it; a budget below every candidate"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    S, F = 2, 3
    R = random_refs(w, h, 93)
    offs = np.array([[0, 5, 40, 96, 41, 6], [96, 41, 6, 0, 5, 40]], np.int32)
    src = synth(oracle, S, 6, rect)
    b = pick_batch(gpu, w, h, rect, S, F, R)
    level = [0, 0]
    assert [b.dyn_rate_level(s) for s in range(S)] == level
    frame_bits = bucket_bits = None
    for c in range(2):
        load(b, offs[:, 3 * c:3 * c + 3], src[:, 3 * c:3 * c + 3])
        res = b.dyn_probe(F, QPS6)
        if frame_bits is None:                 # from the probe's own numbers: between the third and the fourth
            c0 = np.sort(cost_of(res, QPS6)[0, 0])             # cheapest candidate of stream 0, frame 0
            frame_bits = int(c0[2] + c0[3]) // 2
            bucket_bits = 2 * frame_bits
        k, qp, st = b.dyn_pick(F, frame_bits, bucket_bits=bucket_bits)
        for s in range(S):
            wk, wst, level[s] = bucket_np(res[s], QPS6, [True] * F, frame_bits, bucket_bits, level[s])
            assert (list(k[s]), list(st[s])) == (wk, wst), (c, s)
            assert b.dyn_rate_level(s) == level[s], (c, s)
        print("call", c, "k", k.tolist(), "levels", level)
        compose_ok(gpu, b, F)
    assert level != [0, 0]
    # per-stream frame_bits; set and read
    assert b.dyn_rate_level(1, set=-123456789012) == -123456789012
    assert b.dyn_rate_level(1) == -123456789012 and b.dyn_rate_level(0) == level[0]
    b.dyn_rate_level(1, set=7)
    level[1] = 7
    res = b.dyn_probe(F, QPS6)
    k, qp, st = b.dyn_pick(F, 0, bucket_bits=bucket_bits, per_stream=[frame_bits, 3 * frame_bits])
    for s, fb in enumerate([frame_bits, 3 * frame_bits]):
        wk, wst, level[s] = bucket_np(res[s], QPS6, [True] * F, fb, bucket_bits, level[s])
        assert (list(k[s]), list(st[s]), b.dyn_rate_level(s)) == (wk, wst, level[s]), s
    # a bucket below every candidate: the cheapest each time, the debt at its clamp
    k, qp, st = b.dyn_pick(F, 5, bucket_bits=5)
    assert (st == 1).all() and (k == cost_of(res, QPS6).argmin(-1)).all()
    assert [b.dyn_rate_level(s) for s in range(S)] == [-5, -5]
    b.set_dyn_rect(*rect)                      # resets the levels
    assert [b.dyn_rate_level(s) for s in range(S)] == [0, 0]
    b.close()


def test_record_pool_sized_at_the_pick(gpu, oracle):
    """a batch that has only composed at QP 26 (general-path record slots for
    32 of its 48 NALs) picks QP 0 for every frame: the compose after the pick
    succeeds on the first try"""
    w, h, rect = 96, 96, (1, 1, 2, 2)
    S, F = 6, 8
    R = random_refs(w, h, 95)
    rng = np.random.default_rng(2)
    offs = rng.integers(0, 97, (S, F)).astype(np.int32)
    src = synth(oracle, S, F, rect)
    b = pick_batch(gpu, w, h, rect, S, F, R)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    res = b.dyn_probe(F, [0, 26])
    k, qp, st = b.dyn_pick(F, 1 << 30)
    err = res["sse"].astype(np.int64).sum(-1)
    assert (err[..., 0] < err[..., 1]).all()   # the expectation: QP 0 everywhere
    assert (k == 0).all() and (qp == 0).all() and (st == 0).all()
    compose_ok(gpu, b, F)
    for s in range(S):
        want = oracle_qp_frames(oracle, w, h, list(offs[s]) * 2, rect, np.concatenate([src[s], src[s]]), R,
                                [26] * F + [0] * F)[0]
        assert b.output(s) == want, s
    b.close()
