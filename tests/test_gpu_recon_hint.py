"""GPU check of the dynamic rect's reconstruction under UI hints
(scroll_batch_set_dyn_recon_hinted, k_hdyn_recon): the decoded rect and its
squared error of every frame against what the test decoder
(tests/h264_pslice.py, through tests/hreconhelp.py) makes of the emitted NAL
with the oracle's reference samples at each MB's decoded motion.  Exact
equality of every byte and of the three SSE integers; the emitted bytes with
the feature on equal or_compose_hint_dyn's.  At most 2 streams x 6 frames a
test: the Python decoder dominates.  Run on an MI355X: -m gpu."""
import ctypes
import random

import numpy as np
import pytest

from dynhelp import Rect, random_hints, rect_source
from hreconhelp import EXACT, PSKIP, SPEC, _put, make_cfg, oracle_hinted, pred2d
from reconhelp import _regions, oracle_frames, random_refs, sse3, striped_refs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def synth(oracle, S, F, rw, rh, t0=0):
    """[S][F][384 rw rh] of the documented synthetic source"""
    rc = Rect(0, 0, rw, rh, 0)
    return np.stack([np.stack([np.frombuffer(bytes(rect_source(oracle, s, t0 + t, rc)), np.uint8)
                               for t in range(F)]) for s in range(S)])


def make_batch(gpu, w, h, rect, S, F, R, waypoints=(), slot=0, recon=True, hinted=True, fallback=False):
    b = gpu.Batch(S, F, 8 << 20)
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h, waypoints=waypoints))
    b.set_dyn_rect(*rect, slot)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon(True, hinted=hinted)
    if fallback:
        b.set_fallback(True)
    return b


def apply_plans(b, plans, f0=0, n=None, qp_of=None):
    """plans[s][f] = (hint rects, mode, rect origin or None)"""
    for s, plan in enumerate(plans):
        for f, (rects, mode, pos) in enumerate(plan[f0:f0 + n if n else None]):
            b.set_hints(s, f, rects, mode)
            b.set_dyn_rect_at(s, f, *(pos if pos else (-1, -1)))
            if qp_of:
                b.set_dyn_qp_at(s, f, qp_of(s, f0 + f))


def compose(b, offs, src):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])
    b.compose(offs.shape[1])


def expect(oracle, w, h, offs, plans, rw, rh, src, R, **kw):
    """per stream oracle_hinted's (bytes, frames, cfg); qp_of(s, f) -> per stream"""
    qp_of = kw.pop("qp_of", None)
    return [oracle_hinted(oracle, w, h, offs[s], plans[s], rw, rh, src[s], R,
                          qp_of=(lambda f, s=s: qp_of(s, f)) if qp_of else None, **kw) for s in range(len(plans))]


def device_block(gpu, b, s, f):
    """frame f of stream s of the reconstruction buffer, straight from the device"""
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    ptr, ls, lf = b.dyn_recon_device()
    host = np.empty(lf, np.uint8)
    assert hip.hipMemcpy(host.ctypes.data, ptr + s * ls + f * lf, lf, 2) == 0
    return host


def check_frames(b, want, src, rw, rh, f0=0, n=None):
    """every frame's recon bytes and SSE (None where no rect was coded);
    want[s] = oracle_hinted(...), of which the last compose holds frames
    f0 .. f0 + n"""
    for s, (_, frames, _) in enumerate(want):
        for f, d in enumerate(frames[f0:f0 + n if n else None]):
            if d is None:
                assert b.dyn_recon(s, f) is None and b.dyn_sse(s, f) is None, (s, f0 + f)
                continue
            got, rec = b.dyn_recon(s, f), d["rec"]
            assert got is not None and len(got) == len(rec), (s, f0 + f)
            if got != rec:
                k = next(i for i, (x, y) in enumerate(zip(got, rec)) if x != y)
                raise AssertionError(f"stream {s} frame {f0 + f}: recon differs at byte {k} of {len(rec)} "
                                     f"({got[k]} vs {rec[k]}), {sum(x != y for x, y in zip(got, rec))} in all")
            assert b.dyn_sse(s, f) == sse3(src[s][f0 + f], rec, (0, 0, rw, rh)), (s, f0 + f)


def run_case(gpu, oracle, w, h, rw, rh, offs, plans, R, src=None, **kw):
    offs = np.asarray(offs, np.int32)
    S, F = offs.shape
    if src is None:
        src = synth(oracle, S, F, rw, rh)
    want = expect(oracle, w, h, offs, plans, rw, rh, src, R, **kw)
    b = make_batch(gpu, w, h, (0, 0, rw, rh), S, F, R)
    apply_plans(b, plans)
    compose(b, offs, src)
    assert b.sync() == 0, gpu.last_error()
    for s, (data, _, _) in enumerate(want):
        assert b.output(s) == data, f"stream {s}: output bytes differ from or_compose_hint_dyn's with recon on"
    check_frames(b, want, src, rw, rh)
    return b, want


def moving_plans():
    """test 1's hints: stream 0 crosses the 496 waypoint (its later frames
    name it), both streams get a hint with mv_x != 0 over the rect and one
    whose motion leaves the picture; stream 1's frame 2 has no rect"""
    w, h, rw, rh = 256, 720, 3, 2
    mbw, mbh = w // 16, h // 16
    offs = [[100, 480, 496, 497, 500, 620], [0, 37, 250, 700, 720, 333]]
    rng = random.Random(5)
    plans = []
    for s in range(2):
        plan = []
        for f in range(6):
            x0, y0 = rng.randint(0, mbw - rw), rng.randint(1, mbh - rh - 1)
            rects = random_hints(rng, mbw, mbh, [0, 1], 3)
            if f % 3 == 0:      # horizontal motion over the rect's upper row, out of the picture on the left
                rects.append((0, y0, mbw, y0 + 1, s, -(16 * x0 + 21), 3))
            elif f % 3 == 1:    # over its left column, far below the picture
                rects.append((x0, 0, x0 + 1, mbh, 1 - s, 5, 900))
            elif s == 0:        # the waypoint (valid from frame 3 of stream 0)
                rects.append((x0 + 1, y0, x0 + 3, y0 + 2, 2 if f >= 3 else 0, -7, 33))
            pos = None if (s, f) == (1, 2) else (x0, y0)
            plan.append((rects, (EXACT, PSKIP, SPEC)[(f + s) % 3], pos))
        plans.append(plan)
    return w, h, rw, rh, offs, plans


def test_random_hints_moving_rect(gpu, oracle):
    w, h, rw, rh, offs, plans = moving_plans()
    b, want = run_case(gpu, oracle, w, h, rw, rh, offs, plans, striped_refs(oracle, w, h))
    assert want[1][1][2] is None
    assert not device_block(gpu, b, 1, 2).any(), "a frame without the rect keeps its block"
    motions = [m for _, frames, _ in want for d in frames if d for m in d["motion"]]
    assert any(m[0] >= 2 for m in motions) and any(m[1] != 0 for m in motions)
    b.close()


@pytest.mark.parametrize("rw,rh,pos", [(17, 2, (2, 5)), (12, 1, (8, 14)), (1, 1, (19, 14))])
def test_slot_layout_edges(gpu, oracle, rw, rh, pos):
    """17 MBs wide: 34 chroma blocks per row, a second, partly filled chroma
    wave per plane; 12 x 1; one MB in the bottom-right corner whose hint
    motion points off both edges"""
    w, h = 320, 240
    plans = [[([(0, pos[1], 20, pos[1] + 1, 1, 37, -5), (19, 14, 20, 15, 0, 41, 51)], (PSKIP, SPEC)[f], pos)
              for f in range(2)]]
    b, _ = run_case(gpu, oracle, w, h, rw, rh, [[13, 150]], plans, random_refs(w, h, 41))
    b.close()


def test_half_pel_waypoint_chain(gpu, oracle):
    """a resumed waypoint at an odd offset: hints naming it, and the scroll
    layout's own rows past it, predict chroma through a half-pel waypoint
    step (the kernel's second instantiation, chroma_px_any)"""
    w, h, rw, rh = 64, 1024, 2, 3
    wps = [(501, 2, 1)]
    offs = np.array([[600, 777, 505]], np.int32)
    plans = [[([(0, 20 + f, 4, 22 + f, 2, (-3, 6, 1)[f], (-40, 9, 200)[f])], (SPEC, PSKIP, EXACT)[f], (1, 20))
              for f in range(3)]]
    R = random_refs(w, h, 5)
    src = synth(oracle, 1, 3, rw, rh)
    want = expect(oracle, w, h, offs, plans, rw, rh, src, R, waypoints=wps)
    assert any(m[0] == 2 for d in want[0][1] for m in d["motion"])
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 3, R, waypoints=wps)
    apply_plans(b, plans)
    compose(b, offs, src)
    assert b.sync() == 0, gpu.last_error()
    assert b.output(0) == want[0][0]
    check_frames(b, want, src, rw, rh)
    b.close()


def qp_case(oracle):
    """test 3's inputs and expectation (no GPU)"""
    w, h, rw, rh = 96, 96, 2, 2
    qps = [0, 12, 22, 39, 51]
    offs = np.array([[5, 40, 64, 17, 90]], np.int32)
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (1, 5, 384 * rw * rh), dtype=np.uint8)
    src[0, 3] = (rng.integers(0, 2, 384 * rw * rh) * 255).astype(np.uint8)      # QP 39: clips at both ends
    plans = [[([(0, 2, 6, 4, f & 1, (3, -16, 5, -9, 0)[f], (-7, 8, 1, 30, -2)[f])], (EXACT, PSKIP, SPEC)[f % 3],
               (1 + f % 3, 2)) for f in range(5)]]
    R = random_refs(w, h, 31)
    clips = [0, 0]
    want = expect(oracle, w, h, offs, plans, rw, rh, src, R, qp_of=lambda s, f: qps[f], clips=clips)
    return w, h, rw, rh, qps, offs, src, plans, R, clips, want


def test_per_frame_qps(gpu, oracle):
    w, h, rw, rh, qps, offs, src, plans, R, clips, want = qp_case(oracle)
    assert clips[0] > 0 and clips[1] > 0, clips
    for f, d in enumerate(want[0][1]):
        assert d["qps"] == {qps[f]}, (f, d["qps"])
    b = make_batch(gpu, w, h, (0, 0, rw, rh), 1, 5, R, slot=2048 * rw * rh)
    apply_plans(b, plans, qp_of=lambda s, f: qps[f])
    compose(b, offs, src)
    assert b.sync() == 0, gpu.last_error()
    assert b.output(0) == want[0][0]
    check_frames(b, want, src, rw, rh)
    b.close()


def skip_case(oracle):
    """test 4's inputs and expectation (no GPU): frame 1 has no hint rects
    and its source is its own prediction"""
    w, h, rw, rh = 96, 96, 3, 2
    pos = (2, 2)
    offs = np.array([[30, 16]], np.int32)
    R = random_refs(w, h, 71)
    src = synth(oracle, 1, 2, rw, rh)
    cfg = make_cfg(oracle, w, h)
    a_end, ra, mva, rb, mvb = _regions(cfg, 16)
    pred = bytearray(384 * rw * rh)
    rc = Rect(pos[0], pos[1], rw, rh, 0)
    for y in range(pos[1], pos[1] + rh):
        for x in range(pos[0], pos[0] + rw):
            ref, mv = (ra, mva) if y < a_end else (rb, mvb)
            _put(pred, rc, x, y, *pred2d(oracle, cfg, R, ref, 0, mv, x, y))
    src[0, 1] = np.frombuffer(bytes(pred), np.uint8)
    plans = [[([(0, 2, 6, 3, 1, 4, -3)], PSKIP, pos), ([], PSKIP, pos)]]
    want = expect(oracle, w, h, offs, plans, rw, rh, src, R)
    return w, h, rw, rh, offs, src, plans, R, bytes(pred), want


def test_pskip_inside_the_rect(gpu, oracle):
    w, h, rw, rh, offs, src, plans, R, pred, want = skip_case(oracle)
    d = want[0][1][1]
    assert d["skips"] > 0, "no rect MB came out as P_Skip"
    assert d["rec"] == pred == d["pred"]
    b, _ = run_case(gpu, oracle, w, h, rw, rh, offs, plans, R, src=src)
    assert b.dyn_recon(0, 1) == pred and b.dyn_sse(0, 1) == (0, 0, 0)
    b.close()


def test_fallback(gpu, oracle):
    """the whole-picture rect with scroll_batch_set_fallback
    (tests/test_gpu_hintdyn.py::test_fallback_whole_frame_on_inconsistent_hints
    restated, smaller): frames whose hints name a waypoint the frame lacks
    fall back and return whole-picture reconstructions, with or without the
    rect placed; the others return their rect's, or 1 without it"""
    w, h, S, F = 320, 240, 2, 3
    mbw, mbh = w // 16, h // 16
    offs = np.array([[20, 130, 233], [7, 61, 200]], np.int32)
    R = striped_refs(oracle, w, h)
    src = synth(oracle, S, F, mbw, mbh)
    rng = random.Random(9)
    bad_rect = (2, 2, 9, 7, 2 + 6, 16, -32)                  # waypoint 6: never valid here
    where = {(0, 0): (0, 0), (0, 1): None, (0, 2): (0, 0), (1, 0): None, (1, 1): None, (1, 2): (0, 0)}
    bad = {(1, 0), (1, 2)}
    plans = [[(random_hints(rng, mbw, mbh, [0, 1], 3) + ([bad_rect] if (s, f) in bad else []),
               (EXACT, PSKIP, SPEC)[(s + f) % 3], where[(s, f)]) for f in range(F)] for s in range(S)]
    want = expect(oracle, w, h, offs, plans, mbw, mbh, src, R, fallback=True)
    fell = {(s, f) for s in range(S) for f in range(F) if want[s][1][f] and want[s][1][f]["fell"]}
    assert fell == bad
    assert want[0][1][1] is None and want[1][1][1] is None
    b = make_batch(gpu, w, h, (0, 0, mbw, mbh), S, F, R, fallback=True)
    apply_plans(b, plans)
    compose(b, offs, src)
    assert b.sync() == 0, gpu.last_error()
    for s in range(S):
        assert b.output(s) == want[s][0]
        for f in range(F):
            assert b.fallback_frame(s, f) == ((s, f) in fell), (s, f)
    check_frames(b, want, src, mbw, mbh)
    b.close()


def test_chunked_composes_then_plain(gpu, oracle):
    """4 hinted frames composed as 1 + 3: frame f is the f-th frame of the
    last compose; then clear_hints, and the plain path's k_dyn_recon gives
    what tests/test_gpu_recon.py expects of it"""
    w, h, rw, rh = 96, 96, 4, 4
    offs = np.array([[0, 9, 33, 64]], np.int32)
    R = random_refs(w, h, 51)
    src = synth(oracle, 1, 4, rw, rh)
    plans = [[([(0, 1 + f, 6, 3 + f, f & 1, 6 - 5 * f, 2 * f - 3)], (SPEC, PSKIP, EXACT, SPEC)[f], (f % 3, 1))
              for f in range(4)]]
    want = expect(oracle, w, h, offs, plans, rw, rh, src, R)
    b = make_batch(gpu, w, h, (1, 1, rw, rh), 1, 4, R)
    apply_plans(b, plans, 0, 1)
    compose(b, offs[:, :1], src[:, :1])
    assert b.sync() == 0, gpu.last_error()
    check_frames(b, want, src, rw, rh, 0, 1)
    with pytest.raises(RuntimeError):
        b.dyn_recon(0, 1)                      # outside the last compose
    apply_plans(b, plans, 1, 3)
    compose(b, offs[:, 1:], src[:, 1:])
    assert b.sync() == 0, gpu.last_error()
    assert b.output(0) == want[0][0]
    check_frames(b, want, src, rw, rh, 1, 3)
    b.clear_hints()                            # the plain rect at (1, 1) again
    plain = oracle_frames(oracle, w, h, offs[0, :2], (1, 1, rw, rh), src[0, :2], R)
    compose(b, offs[:, :2], src[:, :2])
    assert b.sync() == 0, gpu.last_error()
    for f, (rec, _) in enumerate(plain[1]):
        assert b.dyn_recon(0, f) == rec, f
        assert b.dyn_sse(0, f) == sse3(src[0][f], rec, (1, 1, rw, rh)), f
    b.close()


def test_contract(gpu, oracle):
    w, h, rw, rh = 96, 96, 2, 2
    offs = np.array([[5, 40], [9, 60]], np.int32)
    R = random_refs(w, h, 61)
    src = synth(oracle, 2, 2, rw, rh)
    CONFIG = gpu.SCROLL_ERR_CONFIG
    # without the reconstruction: SCROLL_ERR_CONFIG
    b = make_batch(gpu, w, h, (1, 1, rw, rh), 2, 2, R, recon=False)
    assert gpu.lib.scroll_batch_set_dyn_recon_hinted(b.h, 1) == CONFIG
    assert gpu.lib.scroll_batch_set_dyn_recon_hinted(b.h, 0) == 0
    # the reconstruction on, the opt-in off (the default): hints are refused as before
    b.set_dyn_recon()
    b.set_hints(0, 0, [(0, 0, 6, 1, 0, 0, 0)], SPEC)
    b.set_offsets(offs)
    b.set_dyn_source(src.tobytes(), 2)
    assert gpu.lib.scroll_batch_compose(b.h, 2, None) == CONFIG
    assert "reconstruction" in gpu.last_error()
    b.set_dyn_recon(True, hinted=True)
    with pytest.raises(RuntimeError, match=r"\(-6\)"):      # a splice: SCROLL_ERR_CONFIG
        b.set_splice(0, 0, 0, 0, 1, 1, b"\x00\x00\x00\x01\x21\x00")
    # a splice staged before the rect existed (set_splice refuses one afterwards): the hinted
    # compose refuses it too, and goes through once the splice is cleared
    b2 = gpu.Batch(1, 2, 8 << 20)
    b2.add_stream(gpu.make_config(w, h))
    b2.set_splice(0, 0, 0, 0, 1, 1, b"\x00\x00\x00\x01\x21\x00")
    b2.set_dyn_rect(1, 1, rw, rh, 0)
    b2.set_dyn_refs(R.i420(0), R.i420(1))
    b2.set_dyn_recon(True, hinted=True)
    b2.set_offsets(offs[:1])
    b2.set_dyn_source(src[:1].tobytes(), 2)
    assert gpu.lib.scroll_batch_compose(b2.h, 2, None) == CONFIG
    assert "reconstruction" in gpu.last_error()
    b2.clear_splices()
    plain = [[([], SPEC, (1, 1)), ([], SPEC, (1, 1))]]
    want2 = expect(oracle, w, h, offs[:1], plain, rw, rh, src[:1], R)
    compose(b2, offs[:1], src[:1])
    assert b2.sync() == 0, gpu.last_error()
    assert b2.output(0) == want2[0][0]
    check_frames(b2, want2, src, rw, rh)
    b2.close()
    # stream 1 names a waypoint it lacks, no fallback: it fails, and its accessors say so
    plans = [[([(0, 0, 6, 1, 0, 0, 0)], SPEC, (1, 1)), ([], SPEC, (1, 1))],
             [([], SPEC, (1, 1)), ([(0, 0, 6, 6, 2 + 3, 0, 0)], SPEC, (1, 1))]]
    want = expect(oracle, w, h, offs[:1], plans[:1], rw, rh, src[:1], R)
    apply_plans(b, plans)
    compose(b, offs, src)
    with pytest.raises(RuntimeError, match=r"\(-6\)"):      # before the sync reports it
        b.dyn_recon(1, 0)
    assert gpu.lib.scroll_batch_set_dyn_recon_hinted(b.h, 0) == 0   # the opt-in off before the sync: the status is kept
    assert b.sync() == CONFIG
    for f in range(2):
        with pytest.raises(RuntimeError, match=r"\(-6\)"):  # and after: never stale pixels
            b.dyn_recon(1, f)
        with pytest.raises(RuntimeError, match=r"\(-6\)"):
            b.dyn_sse(1, f)
    check_frames(b, want, src, rw, rh)                      # stream 0 composed normally
    # set_dyn_rect turns both off
    b.set_dyn_rect(1, 1, rw, rh, 0)
    assert b.dyn_recon_device()[0] is None
    assert gpu.lib.scroll_batch_set_dyn_recon_hinted(b.h, 1) == CONFIG
    b.set_dyn_refs(R.i420(0), R.i420(1))
    b.set_dyn_recon()                                       # the reconstruction alone: hints refused again
    b.set_hints(1, 1, [], SPEC)
    b.set_offsets(offs)
    b.set_dyn_source(src.tobytes(), 2)
    assert gpu.lib.scroll_batch_compose(b.h, 2, None) == CONFIG
    b.close()
