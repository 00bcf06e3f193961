"""GPU check of the dynamic rect's QP probe (scroll_batch_dyn_probe,
k_dyn_probe): per frame and candidate QP its bits and non-zero levels against
the oracle's traced MBs (tests/probehelp.py), its squared error against the
test decoder's picture of the oracle's NAL at that QP or against dyn_sse of a
real compose, and that a probe commits and disturbs nothing.  Every
comparison is integer-exact.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from probehelp import constant_of, load, make_batch, oracle_probe, rbsp_bits, se_len, synth
from dynhelp import split_nals
from reconhelp import random_refs, striped_refs

pytestmark = pytest.mark.gpu

QPS6 = [0, 12, 22, 26, 39, 51]


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def check(res, s, f, k, fr, sse=True):
    got = res[s, f, k]
    assert got["valid"] == 1, (s, f, k)
    print(f"stream {s} frame {f} cand {k}: bits {got['bits']} / {fr['bits']}, nonzero {got['nonzero']} / "
          f"{fr['nonzero']}, sse {tuple(int(v) for v in got['sse'])} / {fr.get('sse')}")
    assert (int(got["bits"]), int(got["nonzero"])) == (fr["bits"], fr["nonzero"]), (s, f, k)
    if sse:
        assert tuple(int(v) for v in got["sse"]) == fr["sse"], (s, f, k)


def probe_case(gpu, oracle, w, h, rect, offs, R, qps, src=None, waypoints=(), decode=True, clips=None):
    """probe offs at qps and compare every (stream, frame, candidate) with
    the oracle at that QP; returns (batch, result, src)"""
    offs = np.asarray(offs, np.int32)
    S, F = offs.shape
    if src is None:
        src = synth(oracle, S, F, rect)
    b = make_batch(gpu, w, h, rect, S, F, R, waypoints=waypoints)
    load(b, offs, src)
    res = b.dyn_probe(F, qps)
    assert res.shape == (S, F, len(qps))
    for s in range(S):
        for k, qp in enumerate(qps):
            frames = oracle_probe(oracle, w, h, offs[s], rect, src[s], R, qp, waypoints, decode, clips)[1]
            for f, fr in enumerate(frames):
                check(res, s, f, k, fr, sse=decode)
    return b, res, src


def test_seam_and_chroma_fractions(gpu, oracle):
    """rect touching the region seam at odd offsets (1/8-pel chroma
    fractions), two streams, six QPs from 0 to 51"""
    w, h = 96, 96
    b, _, _ = probe_case(gpu, oracle, w, h, (1, 1, 4, 4), [[0, 5, 40, 96], [96, 41, 6, 0]], random_refs(w, h, 11),
                         QPS6)
    b.close()


@pytest.mark.parametrize("rect", [(0, 0, 2, 2), (2, 2, 2, 2)])
def test_availability(gpu, oracle, rect):
    """the rect in the picture's corners: left and top unavailable in the
    first, MBs outside the rect available with TotalCoeff 0 in the second"""
    w, h = 64, 64
    b, _, _ = probe_case(gpu, oracle, w, h, rect, [[3, 30]], random_refs(w, h, 13), [12, 26, 39])
    b.close()


@pytest.mark.parametrize("rect", [(11, 0, 1, 4), (0, 1, 12, 2), (0, 1, 17, 2)])
def test_row_loop_and_chroma_waves(gpu, oracle, rect):
    """rows of 1, 12 (288 blocks: the row loops) and 17 MBs (a second, partly
    filled chroma wave per plane)"""
    w, h = max(192, 16 * (rect[0] + rect[2])), 64
    b, _, _ = probe_case(gpu, oracle, w, h, rect, [[3, 30]], random_refs(w, h, 41), [12, 26, 39])
    b.close()


def test_wide_row_eight_candidates(gpu, oracle):
    """an 80-MB row at 8 candidates: bits against the oracle, the squared
    error against dyn_sse of eight streams composed at those QPs"""
    w, h, rect = 1280, 64, (0, 1, 80, 2)
    qps = [0, 10, 20, 26, 30, 36, 44, 51]
    offs = np.array([[7]], np.int32)
    R = random_refs(w, h, 43)
    b, res, src = probe_case(gpu, oracle, w, h, rect, offs, R, qps, decode=False)
    b.close()
    S = len(qps)
    c = make_batch(gpu, w, h, rect, S, 1, R, qps=qps, recon=True)
    load(c, np.repeat(offs, S, 0), np.repeat(src, S, 0))
    c.compose(1)
    assert c.sync() == 0, gpu.last_error()
    for k in range(S):
        assert c.dyn_sse(k, 0) == tuple(int(v) for v in res[0, 0, k]["sse"]), k
    c.close()


def test_clipping(gpu, oracle):
    """a source of random 0 / 255 pixels at QP 0 and 51: the decoder clips at
    both ends (asserted on the expectation first)"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    rng = np.random.default_rng(3)
    src = (rng.integers(0, 2, (1, 2, 384 * 16)) * 255).astype(np.uint8)
    R = random_refs(w, h, 31)
    clips = [0, 0]
    for qp in (0, 51):
        oracle_probe(oracle, w, h, [7, 50], rect, src[0], R, qp, clips=clips)
    assert clips[0] > 0 and clips[1] > 0, clips
    b, _, _ = probe_case(gpu, oracle, w, h, rect, [[7, 50]], R, [0, 51], src=src)
    b.close()


def test_waypoint_references(gpu, oracle):
    w, h = 64, 512
    b, _, _ = probe_case(gpu, oracle, w, h, (1, 20, 2, 6), [[0, 17, 496, 500, 505, 400, 300]],
                         striped_refs(oracle, w, h), [12, 26, 39])
    b.close()


def test_half_pel_chain(gpu, oracle):
    """a resumed waypoint at an odd offset: rows predict chroma through a
    half-pel waypoint step (the general instantiation)"""
    w, h = 64, 1024
    b, _, _ = probe_case(gpu, oracle, w, h, (1, 20, 2, 12), [[600, 610, 777, 900, 505, 996]], random_refs(w, h, 5),
                         [12, 26, 39], waypoints=[(501, 2, 1)])
    b.close()


def _records(b, S, F):
    return [(b.output(s), b.nals(s), [b.dyn_frame_info(s, f) for f in range(F)],
             [b.dyn_recon(s, f) for f in range(F)], [b.dyn_sse(s, f) for f in range(F)]) for s in range(S)]


def test_nothing_is_committed(gpu, oracle):
    w, h, rect = 96, 96, (1, 1, 4, 4)
    S, F = 2, 4
    R = random_refs(w, h, 71)
    offs_a = np.array([[0, 9, 18, 33], [96, 41, 6, 0]], np.int32)
    offs_b = np.array([[5, 40, 64, 96], [12, 13, 50, 77]], np.int32)
    src_a, src_b = synth(oracle, S, F, rect), synth(oracle, S, F, rect, t0=9)
    b = make_batch(gpu, w, h, rect, S, F, R, recon=True)
    load(b, offs_a, src_a)
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()
    before = _records(b, S, F)
    cfg_before = [bytes(b.config(s)) for s in range(S)]
    load(b, offs_b, src_b)
    res = b.dyn_probe(F, [20, 26, 33])
    assert res["valid"].all()
    assert b.sync() == 0
    assert _records(b, S, F) == before
    assert [bytes(b.config(s)) for s in range(S)] == cfg_before
    # the compose after the probe: the oracle's bytes, and those of a batch that never probed
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()
    n = make_batch(gpu, w, h, rect, S, F, R, recon=True)
    load(n, offs_a, src_a)
    n.compose(F)
    assert n.sync() == 0, gpu.last_error()   # before its source is replaced
    load(n, offs_b, src_b)
    n.compose(F)
    assert n.sync() == 0, gpu.last_error()
    for s in range(S):
        want = oracle_probe(oracle, w, h, list(offs_a[s]) + list(offs_b[s]), rect,
                            np.concatenate([src_a[s], src_b[s]]), R, 26, decode=False)[0]
        assert b.output(s) == want, s
        assert n.output(s) == want, s
        for f in range(F):
            assert b.dyn_sse(s, f) == n.dyn_sse(s, f) == tuple(int(v) for v in res[s, f, 1]["sse"])
    n.close()
    # nframes < max_frames, twice with different sources: the second does not carry the first
    load(b, offs_a[:, :2], src_a[:, :2])
    r1 = b.dyn_probe(2, [26])
    load(b, offs_a[:, :2], src_b[:, :2])
    r2 = b.dyn_probe(2, [26])
    load(b, offs_a[:, :2], src_a[:, :2])
    r3 = b.dyn_probe(2, [26])
    assert (r1 == r3).all() and not (r1 == r2).all()
    r = gpu.ScrollDynProbe()                   # frame 2 is outside the last probe
    assert gpu.lib.scroll_batch_dyn_probe_result(b.h, 0, 2, 0, ctypes.byref(r)) == gpu.SCROLL_ERR_ARG
    b.close()


def test_probe_against_real_compose(gpu, oracle):
    """nq streams with identical references, offsets and source, stream k at
    candidate k: dyn_sse of the compose equals the probe's sse, and the
    emitted NAL's RBSP bits before the stop bit - len(se(q - 26)) - bits are
    one constant per frame across the candidates"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    qps = QPS6
    S, F = len(qps), 3
    R = random_refs(w, h, 81)
    offs = np.repeat(np.array([[5, 40, 96]], np.int32), S, 0)
    src = np.repeat(synth(oracle, 1, F, rect), S, 0)
    b = make_batch(gpu, w, h, rect, S, F, R, qps=qps, recon=True)
    load(b, offs, src)
    res = b.dyn_probe(F, qps)
    for s in range(1, S):                      # every stream is probed at every candidate alike
        assert (res[s] == res[0]).all()
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()
    nals = [split_nals(b.output(k)) for k in range(S)]
    for f in range(F):
        cs = set()
        for k, qp in enumerate(qps):
            assert b.dyn_sse(k, f) == tuple(int(v) for v in res[0, f, k]["sse"]), (f, k)
            assert len(nals[k]) == F
            cs.add(rbsp_bits(nals[k][f]) - se_len(qp - 26) - int(res[0, f, k]["bits"]))
        assert len(cs) == 1, (f, cs)
    b.close()


def test_experiment_mode(gpu, oracle):
    """a frame whose waypoint NAL replaces the scroll NAL has nothing to
    probe: _result returns 1 and writes nothing"""
    w, h, rect = 64, 512, (1, 20, 2, 6)
    offs = np.array([[0, 17, 496, 300]], np.int32)
    R = striped_refs(oracle, w, h)
    src = synth(oracle, 1, 4, rect)
    b = make_batch(gpu, w, h, rect, 1, 4, R, mode=gpu.SCROLL_MODE_EXPERIMENT)
    load(b, offs, src)
    res = b.dyn_probe(4, [26, 39])
    assert list(res["valid"][0, :, 0]) == [1, 1, 0, 1]
    r = gpu.ScrollDynProbe()
    r.bits = 12345
    assert gpu.lib.scroll_batch_dyn_probe_result(b.h, 0, 2, 0, ctypes.byref(r)) == 1 and r.bits == 12345
    for k, qp in enumerate([26, 39]):
        frames = oracle_probe(oracle, w, h, offs[0], rect, src[0], R, qp, decode=False, mode=1)[1]
        assert frames[2] is None
        for f in (0, 1, 3):
            check(res, 0, f, k, frames[f], sse=False)
    b.close()


def test_contract(gpu, oracle):
    w, h, rect = 96, 96, (1, 1, 4, 4)
    lib, R = gpu.lib, random_refs(w, h, 61)
    q = gpu.u8buf(bytes([26, 30]))
    r = gpu.ScrollDynProbe()
    # no dynamic rect; a rect without references
    b0 = gpu.Batch(1, 2, 1 << 20)
    b0.add_stream(gpu.make_config(w, h))
    assert lib.scroll_batch_dyn_probe(b0.h, 2, q, 2, None) == gpu.SCROLL_ERR_CONFIG
    assert lib.scroll_batch_dyn_probe_result(b0.h, 0, 0, 0, ctypes.byref(r)) == gpu.SCROLL_ERR_CONFIG
    b0.set_dyn_rect(*rect)
    assert lib.scroll_batch_dyn_probe(b0.h, 2, q, 2, None) == gpu.SCROLL_ERR_CONFIG
    b0.close()
    b = make_batch(gpu, w, h, rect, 1, 2, R)
    assert b.dyn_probe_device()[0] is None
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 0, ctypes.byref(r)) == gpu.SCROLL_ERR_CONFIG   # before any probe
    load(b, [[5, 40]], synth(oracle, 1, 2, rect))
    for nq in (0, 9, -1):
        assert lib.scroll_batch_dyn_probe(b.h, 2, gpu.u8buf(bytes(9)), nq, None) == gpu.SCROLL_ERR_ARG
    assert lib.scroll_batch_dyn_probe(b.h, 2, gpu.u8buf(bytes([26, 52])), 2, None) == gpu.SCROLL_ERR_ARG
    for nf in (-1, 3):
        assert lib.scroll_batch_dyn_probe(b.h, nf, q, 2, None) == gpu.SCROLL_ERR_ARG
    b.set_hints(0, 0, [(0, 0, 6, 1, 0, 0, 0)])
    assert lib.scroll_batch_dyn_probe(b.h, 2, q, 2, None) == gpu.SCROLL_ERR_CONFIG
    assert "hints" in gpu.last_error()
    b.clear_hints()
    assert lib.scroll_batch_dyn_probe(b.h, 0, q, 2, None) == 0            # no frames: nothing to read
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 0, ctypes.byref(r)) == gpu.SCROLL_ERR_ARG
    assert lib.scroll_batch_dyn_probe(b.h, 2, q, 2, None) == 0
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 1, 1, ctypes.byref(r)) == 0 and r.bits > 0
    for s, f, k in ((1, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)):
        assert lib.scroll_batch_dyn_probe_result(b.h, s, f, k, ctypes.byref(r)) == gpu.SCROLL_ERR_ARG
    ptr, ls, lf = b.dyn_probe_device()
    assert ptr and lf == gpu.SCROLL_DYN_PROBE_MAX_QPS * ctypes.sizeof(gpu.ScrollDynProbe) == 256 and ls == 2 * lf
    assert b.dyn_probe_ms() == -1.0                                        # timing is off
    b.set_dyn_rect(*rect)                                                  # drops the probe
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 0, ctypes.byref(r)) == gpu.SCROLL_ERR_CONFIG
    assert b.dyn_probe_device()[0] is None
    b.close()
