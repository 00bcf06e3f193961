"""GPU check of the QP probe of the dynamic rect under UI hints
(scroll_batch_dyn_probe_hinted, k_hprobe_class + k_hdyn_probe): bits, nonzero
and sse of every frame and candidate, integer-exact, against
tests/hprobehelp.py (or_compose_hint_dyn at that QP, the test decoder,
or_dyn_mb_levels_bits), and against real hinted composes.  The Python decoder
dominates: at most 2 streams x 3 frames x 3 candidates a test unless the case
needs more.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from dynhelp import split_nals
from hprobehelp import QPS6, case_a, case_b, case_expect, check, expect_stream
from hreconhelp import EXACT, PSKIP, SPEC, oracle_hinted
from probehelp import rbsp_bits, se_len
from dynhelp import Rect, rect_source
from reconhelp import random_refs, striped_refs

pytestmark = pytest.mark.gpu


def synth(oracle, S, F, rw, rh, t0=0):
    """[S][F][384 rw rh] of the documented synthetic source"""
    rc = Rect(0, 0, rw, rh, 0)
    return np.stack([np.stack([np.frombuffer(bytes(rect_source(oracle, s, t0 + t, rc)), np.uint8)
                               for t in range(F)]) for s in range(S)])


def apply_plans(b, plans, f0=0, n=None, qp_of=None):
    """plans[s][f] = (hint rects, mode, rect origin or None)"""
    for s, plan in enumerate(plans):
        for f, (rects, mode, pos) in enumerate(plan[f0:f0 + n if n else None]):
            b.set_hints(s, f, rects, mode)
            b.set_dyn_rect_at(s, f, *(pos if pos else (-1, -1)))
            if qp_of:
                b.set_dyn_qp_at(s, f, qp_of(s, f0 + f))


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def make_batch(gpu, w, h, rect, S, F, R, waypoints=(), slot=0, recon=False, fallback=False, mode=None):
    b = gpu.Batch(S, F, 8 << 20) if mode is None else gpu.Batch(S, F, 8 << 20, mode=mode)
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h, waypoints=waypoints))
    b.set_dyn_rect(*rect, slot)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon(True, hinted=True)
    if fallback:
        b.set_fallback(True)
    return b


def load(b, offs, src):
    """offsets and source of the frames to probe or compose"""
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])
    return offs.shape[1]


def d_of(q, nonzero):
    return se_len(q - 26) - 1 if nonzero > 0 else 0


def status(gpu, b, s, f, k=0):
    r = gpu.ScrollDynProbe()
    r.bits = 12345
    rc = gpu.lib.scroll_batch_dyn_probe_result(b.h, s, f, k, ctypes.byref(r))
    return rc, r.bits


def probe_case(gpu, c, qps):
    b = make_batch(gpu, c["w"], c["h"], (0, 0, c["rw"], c["rh"]), 1, len(c["offs"]), c["R"])
    apply_plans(b, [c["plan"]])
    F = load(b, [c["offs"]], [c["srcs"]])
    res = b.dyn_probe(F, qps, hinted=True)
    b.close()
    return res


# 1. the designed cases of tests/test_hprobe_expect.py
@pytest.mark.parametrize("mode", [EXACT, PSKIP, SPEC])
def test_case_a(gpu, oracle, mode):
    c = case_a(oracle, mode)
    exp, _ = case_expect(oracle, c)
    res = probe_case(gpu, c, QPS6)
    check(res, 0, exp)
    for f in range(3):                         # the identity, on the probe's own numbers
        cs = {rbsp_bits(e["nal"]) - int(res[0, f, k]["bits"]) - d_of(q, int(res[0, f, k]["nonzero"]))
              for k, (q, e) in enumerate(zip(QPS6, exp[f]))}
        assert len(cs) == 1, (f, cs)


@pytest.mark.parametrize("mode", [EXACT, PSKIP, SPEC])
def test_case_b(gpu, oracle, mode):
    c = case_b(oracle, mode)
    exp, _ = case_expect(oracle, c)
    res = probe_case(gpu, c, QPS6)
    check(res, 0, exp)
    cs = [rbsp_bits(e["nal"]) - int(res[0, 0, k]["bits"]) - d_of(q, int(res[0, 0, k]["nonzero"]))
          for k, (q, e) in enumerate(zip(QPS6, exp[0]))]
    if mode == PSKIP:
        assert exp[0][0]["skips"] == 0 and exp[0][2]["skips"] > 0 and exp[0][5]["skips"] > 0
        assert cs[1] == cs[0]
        assert cs[2] < cs[0] and cs[5] < cs[0]            # QP 22, 51: bits + D + C strictly above the NAL
    else:
        assert len(set(cs)) == 1, cs


# 2. slot layout and availability
@pytest.mark.parametrize("rw,rh,pos", [(17, 2, (2, 5)), (12, 1, (8, 14)), (1, 1, (19, 14)), (3, 2, (0, 0)),
                                       (3, 2, (2, 2))])
def test_slot_layout_edges(gpu, oracle, rw, rh, pos):
    """17 MBs wide: a second, partly filled chroma wave and 272 luma slots;
    12 x 1; one MB in the bottom-right corner whose hint motion points off
    both edges; a rect at (0, 0) (left and top unavailable) and one at (2, 2)
    (MBs outside the rect available with 0)"""
    w, h, qps = 320, 240, [12, 26, 39]
    plan = [([(0, pos[1], 20, pos[1] + 1, 1, 37, -5), (19, 14, 20, 15, 0, 41, 51)], (PSKIP, SPEC)[f], pos)
            for f in range(2)]
    R = random_refs(w, h, 41)
    src = synth(oracle, 1, 2, rw, rh)
    exp, _ = expect_stream(oracle, w, h, [13, 150], plan, rw, rh, src[0], R, qps)
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 2, R)
    apply_plans(b, [plan])
    load(b, [[13, 150]], src)
    check(b.dyn_probe(2, qps, hinted=True), 0, exp)
    b.close()


# 3. eight candidates
def test_eight_candidates(gpu, oracle):
    qps = [0, 10, 20, 26, 30, 36, 44, 51]
    c = case_b(oracle, SPEC)
    exp, _ = case_expect(oracle, c, qps)
    check(probe_case(gpu, c, qps), 0, exp)


# 4. a row wider than 128 MBs, dynamic LDS past 64 KB
def test_wide_row(gpu, oracle):
    """240 x 2 at (0, 1) of a 3840 x 48 picture, 8 candidates: the MBs of a
    row and of the row above resolve in a strided loop (480 > 256), and the
    dynamic LDS is 37 * 240 * 8 = 71040 bytes.  sse of every candidate
    against dyn_sse of eight streams composed at those QPs (k_hdyn_recon, not
    the code under test); bits / nonzero against the helper at two
    candidates"""
    w, h, rw, rh, pos = 3840, 48, 240, 2, (0, 1)
    qps = [0, 10, 20, 26, 30, 36, 44, 51]
    plan = [([(0, 1, 240, 2, 1, 5, -3)], SPEC, pos)]
    R = random_refs(w, h, 91)
    src = synth(oracle, 1, 1, rw, rh)
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 1, R)
    apply_plans(b, [plan])
    load(b, [[7]], src)
    res = b.dyn_probe(1, qps, hinted=True)
    b.close()
    assert res["valid"].all()
    n = make_batch(gpu, w, h, (0, 0, rw, rh), 8, 1, R, slot=2048 * rw * rh, recon=True)
    apply_plans(n, [plan] * 8, qp_of=lambda s, f: qps[s])
    load(n, [[7]] * 8, np.repeat(src, 8, 0))
    n.compose(1)
    assert n.sync() == 0, gpu.last_error()
    for k in range(8):
        assert n.dyn_sse(k, 0) == tuple(int(v) for v in res[0, 0, k]["sse"]), k
    n.close()
    two = [2, 6]
    exp, _ = expect_stream(oracle, w, h, [7], plan, rw, rh, src[0], R, [qps[k] for k in two])
    for i, k in enumerate(two):
        e = exp[0][i]
        assert (int(res[0, 0, k]["bits"]), int(res[0, 0, k]["nonzero"])) == (e["bits"], e["nonzero"]), k
        assert tuple(int(v) for v in res[0, 0, k]["sse"]) == tuple(e["sse"]), k


# 5. both clips
def test_extreme_source(gpu, oracle):
    w, h, rw, rh, qps = 96, 96, 2, 2, [0, 51]
    src = (np.random.default_rng(5).integers(0, 2, (1, 1, 384 * rw * rh)) * 255).astype(np.uint8)
    plan = [([(0, 2, 6, 4, 1, -9, 30)], SPEC, (2, 2))]
    R = random_refs(w, h, 31)
    clips = [0, 0]
    exp, _ = expect_stream(oracle, w, h, [17], plan, rw, rh, src[0], R, qps, clips=clips)
    assert clips[0] > 0 and clips[1] > 0, clips
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 1, R)
    apply_plans(b, [plan])
    load(b, [[17]], src)
    check(b.dyn_probe(1, qps, hinted=True), 0, exp)
    b.close()


# 6. waypoints
def waypoint_case(oracle):
    """64 x 512: the 496 waypoint is made by frame 2, frame 3's hint names it"""
    w, h, rw, rh = 64, 512, 2, 3
    offs = [0, 17, 496, 500]
    plan = [([(0, 20, 4, 23, 2 if f >= 3 else f & 1, (-3, 6, 1, 5)[f], (-40, 9, 20, -33)[f])],
             (SPEC, PSKIP, EXACT, SPEC)[f], (1, 20)) for f in range(4)]
    return w, h, rw, rh, offs, plan, striped_refs(oracle, w, h), synth(oracle, 1, 4, rw, rh)


def test_waypoint_made_inside_the_probe(gpu, oracle):
    w, h, rw, rh, offs, plan, R, src = waypoint_case(oracle)
    qps = [22, 37]
    exp, _ = expect_stream(oracle, w, h, offs, plan, rw, rh, src[0], R, qps)
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 4, R)
    apply_plans(b, [plan])
    load(b, [offs], src)
    check(b.dyn_probe(4, qps, hinted=True), 0, exp)
    b.close()


def test_half_pel_waypoint_chain(gpu, oracle):
    """tests/test_gpu_recon_hint.py's case: a resumed waypoint at an odd
    offset, chroma through a half-pel waypoint step (k_hdyn_probe<true>)"""
    w, h, rw, rh = 64, 1024, 2, 3
    wps = [(501, 2, 1)]
    offs = [600, 777, 505]
    plan = [([(0, 20 + f, 4, 22 + f, 2, (-3, 6, 1)[f], (-40, 9, 200)[f])], (SPEC, PSKIP, EXACT)[f], (1, 20))
            for f in range(3)]
    R = random_refs(w, h, 5)
    src = synth(oracle, 1, 3, rw, rh)
    qps = [18, 33]
    exp, _ = expect_stream(oracle, w, h, offs, plan, rw, rh, src[0], R, qps, waypoints=wps)
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 3, R, waypoints=wps)
    apply_plans(b, [plan])
    load(b, [offs], src)
    check(b.dyn_probe(3, qps, hinted=True), 0, exp)
    b.close()


# 7. per-frame positions, a frame without the rect, experiment mode
def test_positions_and_missing_rect(gpu, oracle):
    w, h, rw, rh, qps = 96, 96, 2, 2, [14, 26, 41]
    offs = [[5, 40, 64], [9, 60, 33]]
    where = {(0, 0): (0, 1), (0, 1): (4, 4), (0, 2): (3, 0), (1, 0): (1, 2), (1, 1): None, (1, 2): (4, 0)}
    plans = [[([(0, 1 + f, 6, 3 + f, (s + f) & 1, 6 - 5 * f, 2 * f - 3)], (EXACT, PSKIP, SPEC)[(s + f) % 3],
               where[(s, f)]) for f in range(3)] for s in range(2)]
    R = random_refs(w, h, 51)
    src = synth(oracle, 2, 3, rw, rh)
    b = make_batch(gpu, w, h, (1, 1, rw, rh), 2, 3, R)
    apply_plans(b, plans)
    load(b, offs, src)
    res = b.dyn_probe(3, qps, hinted=True)
    for s in range(2):
        exp, _ = expect_stream(oracle, w, h, offs[s], plans[s], rw, rh, src[s], R, qps)
        check(res, s, exp)
    assert exp[1][0] is None and res[1, 1, 0]["valid"] == 0
    assert status(gpu, b, 1, 1) == (1, 12345)              # nothing written
    b.close()


def test_experiment_mode(gpu, oracle):
    """a frame whose waypoint NAL replaces the scroll NAL has nothing to
    probe; the frames before it are the composer mode's, which
    test_waypoint_made_inside_the_probe checks against the oracle"""
    w, h, rw, rh, offs, plan, R, src = waypoint_case(oracle)
    plan = [(r, m, p) for r, m, p in plan[:3]] + [([], SPEC, (1, 20))]
    qps = [22, 37]
    out = []
    for mode in (None, gpu.SCROLL_MODE_EXPERIMENT):
        b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 4, R, mode=mode)
        apply_plans(b, [plan])
        load(b, [offs], src)
        out.append(b.dyn_probe(4, qps, hinted=True))
        if mode is not None:
            assert status(gpu, b, 0, 2) == (1, 12345)
        b.close()
    assert list(out[0]["valid"][0, :, 0]) == [1, 1, 1, 1]
    assert list(out[1]["valid"][0, :, 0]) == [1, 1, 0, 1]
    assert (out[1][0, :2] == out[0][0, :2]).all()


# 8. the fallback
def fallback_case(oracle):
    """tests/test_gpu_recon_hint.py::test_fallback's batch"""
    import random
    from dynhelp import random_hints
    w, h, S, F = 320, 240, 2, 3
    mbw, mbh = w // 16, h // 16
    offs = [[20, 130, 233], [7, 61, 200]]
    rng = random.Random(9)
    bad_rect = (2, 2, 9, 7, 2 + 6, 16, -32)                  # waypoint 6: never valid here
    where = {(0, 0): (0, 0), (0, 1): None, (0, 2): (0, 0), (1, 0): None, (1, 1): None, (1, 2): (0, 0)}
    bad = {(1, 0), (1, 2)}
    plans = [[(random_hints(rng, mbw, mbh, [0, 1], 3) + ([bad_rect] if (s, f) in bad else []),
               (EXACT, PSKIP, SPEC)[(s + f) % 3], where[(s, f)]) for f in range(F)] for s in range(S)]
    return w, h, S, F, mbw, mbh, offs, plans, bad, striped_refs(oracle, w, h), synth(oracle, S, F, mbw, mbh)


def test_fallback(gpu, oracle):
    w, h, S, F, mbw, mbh, offs, plans, bad, R, src = fallback_case(oracle)
    qps = [24, 38]
    b = make_batch(gpu, w, h, (0, 0, mbw, mbh), S, F, R, fallback=True)
    apply_plans(b, plans)
    load(b, offs, src)
    res = b.dyn_probe(F, qps, hinted=True)
    for s in range(S):
        exp, _ = expect_stream(oracle, w, h, offs[s], plans[s], mbw, mbh, src[s], R, qps, fallback=True)
        fell = {(s, f) for f in range(F) if exp[f][0] and exp[f][0]["fell"]}
        assert fell == {x for x in bad if x[0] == s}
        check(res, s, exp)                                    # fallen frames: whole pictures, no hint rects
    for s, f in ((0, 1), (1, 1)):                             # dormant, not falling back
        assert res[s, f, 0]["valid"] == 0 and status(gpu, b, s, f) == (1, 12345)
    # the fallback off: the bad frames would fail their stream, the others answer as before
    b.set_fallback(False)
    off = b.dyn_probe(F, qps, hinted=True)
    for s in range(S):
        for f in range(F):
            if (s, f) in bad:
                assert status(gpu, b, s, f) == (gpu.SCROLL_ERR_CONFIG, 12345), (s, f)
                assert off[s, f, 0]["valid"] == 0
            elif (s, f) in ((0, 1), (1, 1)):
                assert status(gpu, b, s, f) == (1, 12345), (s, f)
            else:
                assert status(gpu, b, s, f)[0] == 0 and (off[s, f] == res[s, f]).all(), (s, f)
    b.close()


# 9. nothing is committed
def test_nothing_committed(gpu, oracle):
    w, h, rw, rh = 96, 96, 6, 6
    offs = [5, 40, 64, 17]
    bad_rect = (1, 1, 4, 3, 2 + 5, 8, -16)
    plan = [([(0, 1 + f, 6, 3 + f, f & 1, 6 - 5 * f, 2 * f - 3)] + ([bad_rect] if f == 1 else []),
             (SPEC, PSKIP, EXACT, SPEC)[f], (0, 0)) for f in range(4)]
    R = random_refs(w, h, 61)
    src = synth(oracle, 1, 4, rw, rh)
    want, frames, _ = oracle_hinted(oracle, w, h, offs, plan, rw, rh, src[0], R, fallback=True)
    assert frames[1]["fell"]
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 2, R, recon=True, fallback=True)
    apply_plans(b, [plan], 0, 2)
    load(b, [offs[:2]], src[:, :2])
    b.compose(2)
    assert b.sync() == 0, gpu.last_error()

    def records():
        return ([b.fallback_frame(0, f) for f in range(2)], b.output_size(0), b.nals(0),
                [b.dyn_sse(0, f) for f in range(2)], [b.dyn_recon(0, f) for f in range(2)], bytes(b.config(0)))

    before = records()
    assert before[0] == [0, 1]
    load(b, [offs[2:]], src[:, 2:])                        # the next frames' offsets and source; hints untouched
    res = b.dyn_probe(2, [20, 33], hinted=True)
    assert res["valid"].all()
    assert b.sync() == 0
    assert records() == before
    apply_plans(b, [plan], 2, 2)                           # set_hints changes, then the probe again
    res = b.dyn_probe(2, [20, 33], hinted=True)
    exp, _ = expect_stream(oracle, w, h, offs, plan, rw, rh, src[0], R, [20, 33], fallback=True)
    check(res, 0, exp[2:])
    b.compose(2)
    assert b.sync() == 0, gpu.last_error()
    assert b.output(0) == want                             # or_compose_hint_dyn's continuation
    b.close()


# 10. the probe against a real compose
def test_probe_against_real_compose(gpu, oracle):
    w, h, rw, rh = 96, 96, 3, 3
    qps = [16, 26, 34, 45]
    offs = [5, 40, 64]
    pick = [2, 0, 3]                                         # frame f composes at qps[pick[f]]
    plan = [([(0, 1 + f, 6, 3 + f, f & 1, 6 - 5 * f, 2 * f - 3)], EXACT, (f, 1)) for f in range(3)]
    R = random_refs(w, h, 81)
    src = synth(oracle, 1, 3, rw, rh)
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 3, R, slot=2048 * rw * rh, recon=True)
    apply_plans(b, [plan])
    load(b, [offs], src)
    res = b.dyn_probe(3, qps, hinted=True)
    assert res["valid"].all()
    for f in range(3):
        b.set_dyn_qp_at(0, f, qps[pick[f]])
    b.compose(3)
    assert b.sync() == 0, gpu.last_error()
    want, _, _ = oracle_hinted(oracle, w, h, offs, plan, rw, rh, src[0], R, qp_of=lambda f: qps[pick[f]])
    assert b.output(0) == want
    nals = split_nals(b.output(0))
    assert len(nals) == 3
    other, _ = expect_stream(oracle, w, h, offs, plan, rw, rh, src[0], R, [30])   # C from another QP
    for f in range(3):
        k = pick[f]
        assert b.dyn_sse(0, f) == tuple(int(v) for v in res[0, f, k]["sse"]), f
        got = rbsp_bits(nals[f]) - int(res[0, f, k]["bits"]) - d_of(qps[k], int(res[0, f, k]["nonzero"]))
        assert got == other[f][0]["C"], f
    b.close()


# 11. the contract
def test_contract(gpu, oracle):
    w, h, rect = 96, 96, (1, 1, 2, 2)
    lib, R = gpu.lib, random_refs(w, h, 61)
    q = gpu.u8buf(bytes([26, 30]))
    r = gpu.ScrollDynProbe()
    CONFIG, ARG = gpu.SCROLL_ERR_CONFIG, gpu.SCROLL_ERR_ARG
    hint = [(0, 0, 6, 1, 0, 0, 0)]
    # no dynamic rect; a rect without references
    b0 = gpu.Batch(1, 2, 1 << 20)
    b0.add_stream(gpu.make_config(w, h))
    b0.set_hints(0, 0, hint, SPEC)
    assert lib.scroll_batch_dyn_probe_hinted(b0.h, 2, q, 2, None) == CONFIG
    b0.set_dyn_rect(*rect)
    assert lib.scroll_batch_dyn_probe_hinted(b0.h, 2, q, 2, None) == CONFIG
    b0.close()
    # a splice staged before the rect existed
    b2 = gpu.Batch(1, 2, 8 << 20)
    b2.add_stream(gpu.make_config(w, h))
    b2.set_splice(0, 0, 0, 0, 1, 1, b"\x00\x00\x00\x01\x21\x00")
    b2.set_dyn_rect(*rect)
    b2.set_dyn_refs(R.i420(0), R.i420(1))
    load(b2, [[5, 40]], synth(oracle, 1, 2, 2, 2))
    assert lib.scroll_batch_dyn_probe_hinted(b2.h, 2, q, 2, None) == CONFIG
    assert "splice" in gpu.last_error()
    b2.clear_splices()
    assert lib.scroll_batch_dyn_probe_hinted(b2.h, 2, q, 2, None) == 0
    b2.close()
    b = make_batch(gpu, w, h, rect, 1, 2, R)
    load(b, [[5, 40]], synth(oracle, 1, 2, 2, 2))
    assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, q, 2, None) == CONFIG        # no hints: the plain probe's case
    assert "hints" in gpu.last_error()
    b.set_hints(0, 0, hint, SPEC)
    for nq in (0, 9, -1):
        assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, gpu.u8buf(bytes(9)), nq, None) == ARG
    assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, gpu.u8buf(bytes([26, 52])), 2, None) == ARG
    for nf in (-1, 3):
        assert lib.scroll_batch_dyn_probe_hinted(b.h, nf, q, 2, None) == ARG
    assert lib.scroll_batch_dyn_probe(b.h, 2, q, 2, None) == CONFIG               # the plain probe still refuses hints
    assert "covers the plain dynamic rect" in gpu.last_error()
    assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, q, 2, None) == 0
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 1, 1, ctypes.byref(r)) == 0 and r.bits > 0
    for s, f, k in ((1, 0, 0), (0, 2, 0), (0, 0, 2)):
        assert lib.scroll_batch_dyn_probe_result(b.h, s, f, k, ctypes.byref(r)) == ARG
    assert b.dyn_probe_ms() == -1.0                                                # timing is off
    b.clear_hints()                                        # the plain probe works, the hinted one refuses
    assert lib.scroll_batch_dyn_probe(b.h, 2, q, 2, None) == 0
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 0, ctypes.byref(r)) == 0
    assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, q, 2, None) == CONFIG
    b.set_hints(0, 1, hint, EXACT)
    assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, q, 2, None) == 0
    b.set_dyn_rect(*rect)                                  # drops the results
    assert lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 0, ctypes.byref(r)) == CONFIG
    assert b.dyn_probe_device()[0] is None
    b.close()
