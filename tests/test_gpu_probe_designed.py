"""k_dyn_probe, k_dyn_pick and the per-frame QP table on the designed corpus
(tests/designed.py): every number is compared with the oracle's
(tests/designedprobe.py; tests/test_probe_designed.py proves without a GPU
what that expectation reaches), none with another GPU result.

  probe     all 32 cases, both streams, every frame, up to 8 candidates with
            the case's own QP at a different index per case: valid, bits,
            nonzero and the three squared errors
  identity  a compose after the probe gives the oracle's bytes, and each
            dynamic NAL holds bits[own] + len(se(qp - 26)) + C RBSP bits,
            bits and C the oracle's
  pick      budget and expected choices from the oracle's numbers through
            qpfhelp.pick_np / bucket_np; the compose at the picked QPs, its
            reconstruction and squared errors against the oracle per frame
Every picture is tiny.  Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import designed as dz
import designedprobe as dp
from dynhelp import split_nals
from probehelp import load, make_batch, rbsp_bits, se_len
from qpfhelp import bucket_np, cost_of, oracle_qp_frames, pick_np
from test_gpu_dyn import check_equal, gpu  # noqa: F401
from test_gpu_qp_frames import pick_batch

pytestmark = pytest.mark.gpu


def probed(gpu, c, qps, recon=False):
    """a batch of both streams of case c, loaded and probed at qps"""
    b = make_batch(gpu, c.w, c.h, c.rc, 2, c.F, c.R, qps=[c.qp, c.qp], recon=recon)
    load(b, c.offs, c.src)
    res = b.dyn_probe(c.F, qps)
    assert res.shape == (2, c.F, len(qps))
    return b, res


@pytest.mark.parametrize("name", dz.names("a", "a20", "b", "c", "d", "e"))
def test_probe(gpu, oracle, name):
    c = dz.cases(oracle)[name]
    qps = dp.candidates(name)
    b, res = probed(gpu, c, qps)
    b.close()
    for s in range(2):
        dp.check_probe(res, s, dp.expect(oracle, name, s))


@pytest.mark.parametrize("name", ["b_levels_qp22", "d_extremes_qp22", "e_extremes_qp0", "e_clamp_qp0"])
def test_compose_after_the_probe(gpu, oracle, name):
    c = dz.cases(oracle)[name]
    qps = dp.candidates(name)
    k_own = qps.index(c.qp)
    b, res = probed(gpu, c, qps)
    b.compose(c.F)
    assert b.sync() == 0, gpu.last_error()
    check_equal(b, dz.want_of(oracle, name))
    for s in range(2):
        nals = split_nals(b.output(s))
        assert len(nals) == c.F
        for f, per in enumerate(dp.expect(oracle, name, s)):
            e = per[k_own]
            assert rbsp_bits(nals[f]) == e["bits"] + se_len(c.qp - 26) + e["C"], (s, f)
            assert int(res[s, f, k_own]["bits"]) == e["bits"], (s, f)
    b.close()


# ------------------------------------------------------------------- the pick --
# 27 before 25 (they cost the same where nothing is coded: the order decides), no 26, both sides of 22,
# and three candidates at or above 22: the budget, between the fourth and the fifth cheapest of stream 0,
# frame 0, then admits QP 16 there
PICK_QPS = [27, 25, 0, 16, 22, 4, 8, 12]


def flat_variant(oracle, name):
    """a local copy of the case with an all-128 frame appended (source =
    prediction: no error and the same bits at every candidate); the cached
    corpus is left alone"""
    c = dz.cases(oracle)[name]
    return dz.Case(name + "+flat", c.group, c.qp, list(c.frames) + [dz.Frame(c.rw, c.rh)])


_pick = {}


def pick_case(oracle, name):
    """(case, expectation [2][F][8], the same as result arrays, budget), made
    once per case.  A case without a frame whose error is the same at every
    candidate gets an all-128 frame appended"""
    if name not in _pick:
        c = dz.cases(oracle)[name]
        if not any(all((a == 128).all() for a in fr.s + fr.p) for fr in c.frames):
            c = flat_variant(oracle, name)
        exp = [dp.expect_case(oracle, c, s, PICK_QPS) for s in range(2)]
        res = np.stack([dp.as_result(e) for e in exp])
        c0 = np.sort(cost_of(res, PICK_QPS)[0, 0])
        budget = int(c0[3] + c0[4]) // 2       # between the median candidate cost and the next
        _pick[name] = (c, exp, res, budget)
    return _pick[name]


def expected_picks(c, res, budget):
    wk = np.zeros((2, c.F), np.int32)
    wst = np.zeros((2, c.F), np.int32)
    for s in range(2):
        for f in range(c.F):
            wk[s, f], wst[s, f] = pick_np(res[s, f], PICK_QPS, budget)
    return wk, wst, np.array(PICK_QPS)[wk]


def check_compose(b, exp, res, wk, f0, n):
    """frames f0 .. f0 + n - 1, just composed at the picked QPs: the
    reconstruction, the squared errors and the RBSP bits of the oracle at the
    chosen candidate (the bytes are checked by the caller, whole streams)"""
    cost = cost_of(res, PICK_QPS)
    for s in range(2):
        nals = split_nals(b.output(s))
        for f in range(f0, f0 + n):
            e = exp[s][f][wk[s, f]]
            assert b.dyn_sse(s, f - f0) == tuple(e["sse"]), (s, f)
            assert b.dyn_recon(s, f - f0) == e["rec"], (s, f)
            assert rbsp_bits(nals[f]) == cost[s, f, wk[s, f]] + e["C"], (s, f)


def want_streams(oracle, c, wqp):
    return [oracle_qp_frames(oracle, c.w, c.h, c.offs[s], c.rc, c.src[s], c.R, [int(q) for q in wqp[s]])[0]
            for s in range(2)]


@pytest.mark.parametrize("name", ["d_extremes_qp22", "e_levels_qp21"])
def test_pick(gpu, oracle, name):
    """FRAME mode.  On the expectation first: one stream picks a QP below 22
    in one frame and one at or above 22 in another (general-path and int8 rows
    in one compose), a frame goes over budget, and a frame whose error is the
    same at every candidate is decided by cost and then by order"""
    c, exp, res, budget = pick_case(oracle, name)
    wk, wst, wqp = expected_picks(c, res, budget)
    print("budget", budget, "\nk", wk, "\nqp", wqp, "\nstatus", wst)
    assert any((wqp[s] < 22).any() and (wqp[s] >= 22).any() for s in range(2))
    assert (wst == 1).any() and (wst == 0).any()
    err = res["sse"].astype(np.int64).sum(-1)
    cost = cost_of(res, PICK_QPS)
    tied = [(s, f) for s in range(2) for f in range(c.F) if len(set(err[s, f])) == 1]
    assert tied
    for s, f in tied:                          # 27 and 25 cost the same and the least: 27 comes first
        assert wst[s, f] == 0 and cost[s, f, 0] == cost[s, f, 1] == cost[s, f].min()
        assert PICK_QPS[wk[s, f]] == 27
    b = pick_batch(gpu, c.w, c.h, c.rc, 2, c.F, c.R)
    load(b, c.offs, c.src)
    got = b.dyn_probe(c.F, PICK_QPS)
    for s in range(2):
        dp.check_probe(got, s, exp[s])
    k, qp, st = b.dyn_pick(c.F, budget)
    assert (k == wk).all() and (qp == wqp).all() and (st == wst).all(), (k, qp, st)
    assert (b.dyn_qp_frames(c.F) == wqp).all()
    b.compose(c.F)
    assert b.sync() == 0, gpu.last_error()
    check_equal(b, want_streams(oracle, c, wqp))
    check_compose(b, exp, res, wk, 0, c.F)
    b.close()


@pytest.mark.parametrize("name", ["d_extremes_qp22", "e_levels_qp21"])
def test_pick_bucket(gpu, oracle, name):
    """BUCKET mode: two picks of half the frames each on one batch, a compose
    after each, the level carried between them; choices, statuses and levels
    from bucket_np on the oracle's numbers"""
    c, exp, res, budget = pick_case(oracle, name)
    frame_bits, bucket_bits = budget, 2 * budget
    half = (c.F + 1) // 2
    b = pick_batch(gpu, c.w, c.h, c.rc, 2, half, c.R)
    level = [0, 0]
    wk = np.zeros((2, c.F), np.int32)
    sts = []
    for f0, n in ((0, half), (half, c.F - half)):
        load(b, c.offs[:, f0:f0 + n], c.src[:, f0:f0 + n])
        got = b.dyn_probe(n, PICK_QPS)
        for s in range(2):
            dp.check_probe(got, s, exp[s][f0:f0 + n])
        k, qp, st = b.dyn_pick(n, frame_bits, bucket_bits=bucket_bits)
        for s in range(2):
            ks, ss, level[s] = bucket_np(res[s, f0:f0 + n], PICK_QPS, [True] * n, frame_bits, bucket_bits, level[s])
            assert (list(k[s]), list(st[s])) == (ks, ss), (f0, s)
            assert list(qp[s]) == [PICK_QPS[i] for i in ks], (f0, s)
            assert b.dyn_rate_level(s) == level[s], (f0, s)
            wk[s, f0:f0 + n] = ks
            sts += ss
        assert (b.dyn_qp_frames(n) == np.array(PICK_QPS)[wk[:, f0:f0 + n]]).all()
        b.compose(n)
        assert b.sync() == 0, gpu.last_error()
        check_compose(b, exp, res, wk, f0, n)
    print("k", wk, "levels", level)
    assert level != [0, 0] and 0 in sts
    check_equal(b, want_streams(oracle, c, np.array(PICK_QPS)[wk]))
    b.close()
