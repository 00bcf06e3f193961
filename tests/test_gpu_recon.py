"""GPU check of the dynamic rect's reconstruction (scroll_batch_set_dyn_recon,
k_dyn_recon): the decoded rect and its squared error of every frame against
what the test decoder (tests/h264_pslice.py, through tests/reconhelp.py)
decodes from the emitted NAL with the oracle's reference samples.  Exact
equality of every byte and of the three SSE integers; the emitted bytes
with the reconstruction on equal the oracle's.  Pictures are tiny: the
Python decoder dominates.  Run on an MI355X: -m gpu."""
import math

import numpy as np
import pytest

from dynhelp import Rect, rect_source
from reconhelp import oracle_frames, random_refs, sse3, striped_refs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def synth(oracle, S, F, rect, t0=0):
    """[S][F][384 w h] of the documented synthetic source"""
    rc = Rect(*rect, 0)
    return np.stack([np.stack([np.frombuffer(bytes(rect_source(oracle, s, t0 + t, rc)), np.uint8)
                               for t in range(F)]) for s in range(S)])


def make_batch(gpu, w, h, rect, S, F, R, qps=None, waypoints=(), recon=True):
    b = gpu.Batch(S, F, 8 << 20)
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h, waypoints=waypoints))
    b.set_dyn_rect(*rect)
    for s, q in enumerate(qps or []):
        b.set_dyn_qp(q, stream=s)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon()
    return b


def compose(gpu, b, offs, src):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])
    b.compose(offs.shape[1])
    assert b.sync() == 0, gpu.last_error()


def expect(oracle, w, h, rect, offs, src, R, qps=None, waypoints=(), clips=None):
    """per stream: (its bytes, per frame (decoded rect, prediction))"""
    return [oracle_frames(oracle, w, h, offs[s], rect, src[s], R, qp=(qps[s] if qps else 26),
                          waypoints=waypoints, clips=clips) for s in range(len(offs))]


def check_frames(b, want, src, rect, f0=0):
    """every frame's recon bytes and SSE; want[s] = oracle_frames(...), of
    which the last compose holds frames f0 ..."""
    for s, (_, frames) in enumerate(want):
        for f, (rec, _) in enumerate(frames[f0:]):
            got = b.dyn_recon(s, f)
            assert got is not None and len(got) == len(rec)
            if got != rec:
                k = next(i for i, (x, y) in enumerate(zip(got, rec)) if x != y)
                raise AssertionError(f"stream {s} frame {f0 + f}: recon differs at byte {k} of {len(rec)} "
                                     f"({got[k]} vs {rec[k]}), {sum(x != y for x, y in zip(got, rec))} in all")
            assert b.dyn_sse(s, f) == sse3(src[s][f0 + f], rec, rect), (s, f0 + f)


def run_case(gpu, oracle, w, h, rect, offs, R, src=None, qps=None, waypoints=()):
    offs = np.asarray(offs, np.int32)
    S, F = offs.shape
    if src is None:
        src = synth(oracle, S, F, rect)
    want = expect(oracle, w, h, rect, offs, src, R, qps, waypoints)
    b = make_batch(gpu, w, h, rect, S, F, R, qps, waypoints)
    compose(gpu, b, offs, src)
    for s, (data, _) in enumerate(want):
        assert b.output(s) == data, f"stream {s}: output bytes differ from or_compose_dyn's with recon on"
    check_frames(b, want, src, rect)
    b.close()


def test_edges_and_chroma_fraction(gpu, oracle):
    """rect touching the region seam at odd offsets (1/8-pel chroma
    fractions), random references"""
    w, h = 96, 96
    run_case(gpu, oracle, w, h, (1, 1, 4, 4), [[0, 5, 40, 96], [96, 41, 6, 0]], random_refs(w, h, 11))


def test_waypoint_references(gpu, oracle):
    w, h = 64, 512
    run_case(gpu, oracle, w, h, (1, 20, 2, 6), [[0, 17, 496, 500, 505, 400, 300]], striped_refs(oracle, w, h))


def test_half_pel_chain(gpu, oracle):
    """a resumed waypoint at an odd offset: rows predict chroma through a
    half-pel waypoint step (ROW_GEN, chroma_px_any)"""
    w, h = 64, 1024
    run_case(gpu, oracle, w, h, (1, 20, 2, 12), [[600, 610, 777, 900, 505, 996]], random_refs(w, h, 5),
             waypoints=[(501, 2, 1)])


def test_qp_range_in_one_batch(gpu, oracle):
    w, h = 96, 96
    qps = [0, 12, 22, 39, 51]
    offs = [[5 + s, 40 + 3 * s] for s in range(len(qps))]
    run_case(gpu, oracle, w, h, (1, 1, 4, 4), offs, random_refs(w, h, 21), qps=qps)


def test_clipping(gpu, oracle):
    """a source of random 0 / 255 pixels at QP 40: the decoder clips at both
    ends (asserted on the expectation first)"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    rng = np.random.default_rng(3)
    offs = np.array([[7, 50]], np.int32)
    src = (rng.integers(0, 2, (1, 2, 384 * 16)) * 255).astype(np.uint8)
    R = random_refs(w, h, 31)
    clips = [0, 0]
    want = expect(oracle, w, h, rect, offs, src, R, qps=[40], clips=clips)
    assert clips[0] > 0 and clips[1] > 0, clips
    b = make_batch(gpu, w, h, rect, 1, 2, R, qps=[40])
    compose(gpu, b, offs, src)
    assert b.output(0) == want[0][0]
    check_frames(b, want, src, rect)
    b.close()


@pytest.mark.parametrize("rect", [(0, 1, 12, 2), (11, 0, 1, 4), (0, 1, 17, 2)])
def test_row_loop_and_widths(gpu, oracle, rect):
    """12 MBs wide: 288 blocks per rect row, more than the workgroup's 256
    (the row loops); one MB wide at the right picture edge; 17 MBs wide (a
    272 x 64 picture): 34 chroma blocks per row, a second, partly filled
    chroma wave per plane"""
    w, h = max(192, 16 * (rect[0] + rect[2])), 64
    run_case(gpu, oracle, w, h, rect, [[3, 30]], random_refs(w, h, 41))


def test_chunked_composes(gpu, oracle):
    """6 frames composed as 2 + 4: dyn_recon(s, f) indexes the last
    compose's frames"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    offs = np.array([[0, 9, 18, 33, 64, 96]], np.int32)
    src = synth(oracle, 1, 6, rect)
    R = random_refs(w, h, 51)
    want = expect(oracle, w, h, rect, offs, src, R)
    b = make_batch(gpu, w, h, rect, 1, 6, R)
    compose(gpu, b, offs[:, :2], src[:, :2])
    check_frames(b, [(want[0][0], want[0][1][:2])], src, rect)
    with pytest.raises(RuntimeError):
        b.dyn_recon(0, 2)                      # outside the last compose
    compose(gpu, b, offs[:, 2:], src[:, 2:])
    assert b.output(0) == want[0][0]
    check_frames(b, want, src, rect, f0=2)
    with pytest.raises(RuntimeError):
        b.dyn_sse(0, 4)
    b.close()


def test_contract(gpu, oracle):
    w, h, rect = 96, 96, (1, 1, 4, 4)
    offs = np.array([[5, 40]], np.int32)
    src = synth(oracle, 1, 2, rect)
    R = random_refs(w, h, 61)
    src4 = np.concatenate([src, src], 1)       # two composes of the same two frames
    want = expect(oracle, w, h, rect, np.concatenate([offs, offs], 1), src4, R)
    # without a rect: SCROLL_ERR_CONFIG
    b0 = gpu.Batch(1, 2, 1 << 20)
    b0.add_stream(gpu.make_config(w, h))
    assert gpu.lib.scroll_batch_set_dyn_recon(b0.h, 1) == gpu.SCROLL_ERR_CONFIG
    b0.close()
    b = make_batch(gpu, w, h, rect, 1, 2, R, recon=False)
    assert b.dyn_recon_device()[0] is None
    compose(gpu, b, offs, src)
    with pytest.raises(RuntimeError):          # before set_dyn_recon
        b.dyn_recon(0, 0)
    with pytest.raises(RuntimeError):
        b.dyn_sse(0, 0)
    b.set_dyn_recon()
    ptr, ls, lf = b.dyn_recon_device()
    assert ptr and lf == 384 * 16 and (ls, lf) == b.dyn_source_device()[1:]
    # hints set: the compose refuses instead of leaving stale pictures
    b.set_hints(0, 0, [(0, 0, 6, 1, 0, 0, 0)])
    b.set_offsets(offs)
    assert gpu.lib.scroll_batch_compose(b.h, 2, None) == gpu.SCROLL_ERR_CONFIG
    assert "reconstruction" in gpu.last_error()
    b.clear_hints()
    compose(gpu, b, offs, src)
    check_frames(b, want, src4, rect, f0=2)
    for f in range(2):                          # dyn_psnr agrees with the SSE
        sse, ps = b.dyn_sse(0, f), b.dyn_psnr(0, f)
        for e, n, p in zip(sse, (256 * 16, 64 * 16, 64 * 16), ps):
            assert p == (math.inf if e == 0 else 10 * math.log10(255 * 255 * n / e))
    assert b.output(0) == want[0][0]            # two composes, recon off then on: the oracle's bytes
    b.set_dyn_recon(False)
    assert b.dyn_recon_device()[0] is None
    compose(gpu, b, offs, src)
    with pytest.raises(RuntimeError):
        b.dyn_recon(0, 0)
    b.close()
    # after set_dyn_recon(False) a further compose still emits the oracle's bytes
    b = make_batch(gpu, w, h, rect, 1, 2, R)
    compose(gpu, b, offs, src)
    b.set_dyn_recon(False)
    compose(gpu, b, offs, src)
    assert b.output(0) == want[0][0]
    b.close()
