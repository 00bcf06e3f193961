"""The rule of the rect's per-frame QP pick (h264-scroll-encoder_amd/csrc/
pick_device.h: k_dyn_pick runs it on the device), compiled for the CPU
(tests/hostsim/pick_sim.cpp), against a numpy restatement (tests/qpfhelp.py)
and, in FRAME mode, against h264scroll.pick_qp on a copy of the results whose
bits field holds the cost.  Every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from probehelp import PROBE_DTYPE, se_len
from qpfhelp import bucket_np, cost_of, pick_np

MAXQ = 8


@pytest.fixture(scope="module")
def picksim(tmp_path_factory):
    """TEST-ONLY CPU build of pick_device.h; the library lands in pytest's
    temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("picksim") / "libpicksim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(PKG, "csrc"), os.path.join(d, "pick_sim.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.pksim_pick.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64,
                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]
    lib.pksim_stream.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64),
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def sim_pick(lib, res, qps, allow):
    r = np.ascontiguousarray(res)
    q = np.array(qps, np.uint8)
    over, cost = ctypes.c_int(), ctypes.c_uint32()
    k = lib.pksim_pick(r.ctypes.data, q.ctypes.data, len(q), int(allow), ctypes.byref(over), ctypes.byref(cost))
    return k, over.value, cost.value


def sim_stream(lib, mode, res, qps, has, frame_bits, bucket_bits, level):
    F, nq = res.shape
    r = np.zeros((F, MAXQ), PROBE_DTYPE)
    r[:, :nq] = res
    q = np.array(qps, np.uint8)
    hs = np.array(has, np.uint8)
    k, st, en = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.uint8)
    lv = ctypes.c_int64(level)
    lib.pksim_stream(mode, r.ctypes.data, q.ctypes.data, nq, hs.ctypes.data, F, frame_bits, bucket_bits,
                     ctypes.byref(lv), k.ctypes.data, st.ctypes.data, en.ctypes.data)
    return list(k), list(st), list(en), lv.value


def table(rng, shape, bits_hi=3000, sse_hi=5000):
    r = np.zeros(shape, PROBE_DTYPE)
    r["sse"] = rng.integers(0, sse_hi, shape + (3,))
    r["bits"] = rng.integers(0, bits_hi, shape)
    return r


def cand(rows):
    """[(sse total, bits), ...] -> one frame's candidates"""
    r = np.zeros(len(rows), PROBE_DTYPE)
    for i, (e, b) in enumerate(rows):
        r[i]["sse"] = (e, 0, 0)
        r[i]["bits"] = b
    return r


def test_se_len(picksim):
    for v in range(-26, 26):
        assert picksim.pksim_se_len(v) == se_len(v), v


def test_frame_mode_is_pick_qp_on_cost(picksim, scroll):
    """FRAME mode where something fits: h264scroll.pick_qp on a copy of the
    results whose bits field holds the cost"""
    rng = np.random.default_rng(5)
    fits = 0
    for it in range(300):
        nq = 1 + it % MAXQ
        qps = list(rng.integers(0, 52, nq))
        res = table(rng, (1, 6, nq))
        allow = int(rng.integers(0, 3200))
        costed = res.copy()
        costed["bits"] = cost_of(res, qps)
        want = scroll.pick_qp(costed, qps, allow)
        for f in range(6):
            k, over, cost = sim_pick(picksim, res[0, f], qps, allow)
            assert cost == int(costed["bits"][0, f, k])
            if want[0, f] < 0:
                assert over == 1
            else:
                fits += 1
                assert over == 0 and cost <= allow and qps[k] == want[0, f], (it, f)
                # pick_qp names a QP; where two candidates share it, the rule's own order decides
                assert k == pick_np(res[0, f], qps, allow)[0]
    assert fits > 300


def test_none_fits_and_ties(picksim):
    qps = [20, 26, 30, 40]
    # none fits: the cheapest (cost = bits + se_len(qp - 26): 7, 1, 7, 9 on top)
    assert [se_len(q - 26) for q in qps] == [7, 1, 7, 9]
    r = cand([(10, 500), (20, 400), (30, 380), (40, 390)])
    assert sim_pick(picksim, r, qps, 100) == (2, 1, 387)
    # none fits, equal costs: the smaller error, then the earlier candidate
    r = cand([(50, 500 - 7), (40, 500 - 1), (40, 500 - 7), (60, 500 - 9)])
    assert sim_pick(picksim, r, qps, 0) == (1, 1, 500)
    # ties on the error among those that fit: the smaller cost
    r = cand([(7, 300), (7, 200), (7, 250), (9, 10)])
    assert sim_pick(picksim, r, qps, 1000) == (1, 0, 201)
    # ties on error and cost: the earlier candidate
    r = cand([(7, 200 - 7), (7, 200 - 1), (7, 200 - 7), (7, 200 - 9)])
    assert sim_pick(picksim, r, qps, 1000) == (0, 0, 200)
    # the smallest error does not fit: the next one that does; the boundary is inclusive
    r = cand([(1, 900), (5, 493), (3, 494), (9, 10)])
    assert sim_pick(picksim, r, qps, 500) == (1, 0, 494)
    assert sim_pick(picksim, r, qps, 501) == (2, 0, 501)
    for case in (cand([(10, 500), (20, 400)]), cand([(7, 200), (7, 200), (3, 900)])):
        for allow in (0, 199, 201, 207, 401, 513, 2000):
            k, over, _ = sim_pick(picksim, case, qps[:len(case)], allow)
            assert (k, over) == pick_np(case, qps[:len(case)], allow)


def test_frame_mode_random(picksim):
    rng = np.random.default_rng(9)
    for it in range(400):
        nq = 1 + it % MAXQ
        qps = list(rng.integers(0, 52, nq))
        res = table(rng, (nq,), bits_hi=40 if it % 3 == 0 else 3000, sse_hi=4 if it % 2 else 5000)
        allow = int(rng.integers(0, 60 if it % 3 == 0 else 3200))
        k, over, _ = sim_pick(picksim, res, qps, allow)
        assert (k, over) == pick_np(res, qps, allow), it


@pytest.mark.parametrize("frame_bits,bucket_bits", [(1500, 6000), (0, 4000), (700, 5), (3000, 100000)])
def test_bucket_mode(picksim, frame_bits, bucket_bits):
    """64 streams x 12 frames x 1..8 candidates with frames that have no
    dynamic NAL; a bucket smaller than every candidate (the debt clamp) and
    frame_bits 0 among the parameters"""
    rng = np.random.default_rng(frame_bits + bucket_bits)
    S, F = 64, 12
    seen = set()
    for s in range(S):
        nq = 1 + s % MAXQ
        qps = list(rng.integers(0, 52, nq))
        res = table(rng, (F, nq))
        res["bits"] += 20                     # every candidate costs more than the 5-bit bucket
        has = list(rng.integers(0, 4, F) != 0)
        level = int(rng.integers(-bucket_bits, bucket_bits + 1))
        k, st, en, after = sim_stream(picksim, 1, res, qps, has, frame_bits, bucket_bits, level)
        wk, wst, wafter = bucket_np(res, qps, has, frame_bits, bucket_bits, level)
        assert (k, st, after) == (wk, wst, wafter), s
        assert en == [0xFF if kk < 0 else qps[kk] for kk in wk]
        assert -bucket_bits <= after <= bucket_bits
        seen |= set(wst)
        # FRAME mode on the same table: stateless
        k0, st0, _, lv0 = sim_stream(picksim, 0, res, qps, has, frame_bits, bucket_bits, level)
        assert lv0 == level
        for f in range(F):
            assert (k0[f], st0[f]) == ((-1, 2) if not has[f] else pick_np(res[f], qps, frame_bits))
    assert 2 in seen and 1 in seen
    if bucket_bits == 5:
        assert 0 not in seen                  # nothing ever fits: always the cheapest, the debt at its clamp
    else:
        assert 0 in seen
