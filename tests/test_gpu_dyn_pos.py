"""GPU check of the plain dynamic rect placed per stream and per frame
(scroll_batch_set_dyn_rect_moving): k_plan drops the dynamic NAL of a frame
without a rect, k_dyn_rows / k_dyn_code_general / k_dyn_row / k_dyn_static /
k_dyn_epfix / k_dyn_gather / k_dyn_recon / k_dyn_probe / k_dyn_synth take the
frame's own origin from the position table.  Bytes against the CPU assembly
of tests/dynposhelp.py (one whole-stream oracle run per distinct position;
tests/test_dyn_pos_oracle.py pins it), reconstruction and probe against the
oracle helpers selected per position.  Every comparison is exact.  Run on an
MI355X: -m gpu."""
import ctypes
import random

import numpy as np
import pytest

from cschelp import BT601, RGBA, i420_bytes
from dynhelp import Rect, rect_source, split_nals
from dynposhelp import oracle_moving, per_position
from probehelp import oracle_probe
from qpfhelp import cost_of, oracle_qp_frames, pick_np
from reconhelp import random_refs, striped_refs
from test_gpu_dyn import check_equal
from test_gpu_surface import Hip, Surfaces, cut

pytestmark = pytest.mark.gpu

EXACT = 0
# the smallest picture that reaches every edge: 6 x 23 MBs, taller than one
# static row group (16 rows) plus the rect, so nA changes inside it
W, H, RW, RH = 96, 368, 2, 2
EDGES = [(0, 0),                       # no left or top neighbour, nA forced to 1 with no rows above
         (4, 21),                      # right and bottom edge, no group below
         (2, 15), (2, 16), (2, 17),    # across the DYN_STATIC_ROWS seam: nA 1 -> 1 -> 2
         (0, 1)]


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


@pytest.fixture(scope="module")
def hip(gpu):
    return Hip()


def batch(gpu, w, h, S, F, rect, R, mode=0, moving=True, recon=False, debug=0, arena=8 << 20):
    b = gpu.Batch(S, F, arena, mode=mode)
    if debug:
        b.set_debug(debug)
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h))
    b.set_dyn_rect(*rect)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon()
    if moving:
        b.set_dyn_rect_moving()
    return b


def place(b, pos, f0=0, F=None):
    """pos[s][f0 + f] -> entry f of stream s"""
    for s, row in enumerate(pos):
        for f, p in enumerate(row[f0:f0 + F if F else None]):
            b.set_dyn_rect_at(s, f, *(p if p else (-1, -1)))


def load(b, offs, src):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])


def compose_ok(gpu, b, F):
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()


def want_streams(oracle, w, h, offs, rw, rh, pos, src, R, qps=None, mode=0):
    return [oracle_moving(oracle, w, h, offs[s], rw, rh, pos[s], src[s], R, None if qps is None else qps[s],
                          mode=mode)[0] for s in range(len(pos))]


def noise(seed, S, F, rw, rh):
    return np.random.default_rng(seed).integers(0, 256, (S, F, 384 * rw * rh), dtype=np.uint8)


def edge_case():
    """3 streams x 6 frames, the positions different per stream, offsets
    through the 496 waypoint (a waypoint NAL between the scroll NALs)"""
    offs = np.array([[484, 488, 492, 496, 500, 504], [20, 300, 496, 368, 0, 100], [7, 33, 250, 367, 119, 496]],
                    np.int32)
    pos = [EDGES, EDGES[3:] + EDGES[:3], [EDGES[1], EDGES[0], EDGES[5], EDGES[4], EDGES[2], EDGES[3]]]
    return offs, pos


def ep_bytes(nal):
    """emulation-prevention bytes of a NAL: 00 00 03 occurs nowhere else"""
    return nal.count(b"\x00\x00\x03")


@pytest.mark.parametrize("mode,content", [(0, "noise"), (1, "noise"), (0, "synth")])
def test_edges_and_the_static_group_seam(gpu, oracle, mode, content):
    """noise sources on random references (the gather's group seams carry
    dense bits), once in experiment mode; and the synthetic source of each
    frame's position on the striped references, whose NALs hold
    emulation-prevention bytes at this size (asserted on the expectation)"""
    offs, pos = edge_case()
    S, F = offs.shape
    if content == "noise":
        R = random_refs(W, H, 3)
        src = noise(4, S, F, RW, RH)
    else:
        R = striped_refs(oracle, W, H)
        src = np.stack([np.stack([np.frombuffer(bytes(rect_source(oracle, s, t, Rect(*pos[s][t], RW, RH))), np.uint8)
                                  for t in range(F)]) for s in range(S)])
    per = [oracle_moving(oracle, W, H, offs[s], RW, RH, pos[s], src[s], R, mode=mode) for s in range(S)]
    want = [p[0] for p in per]
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, mode=mode)
    place(b, pos)
    if content == "noise":
        load(b, offs, src)
    else:
        b.set_offsets(offs)
        b.dyn_source_synth(F, 0, 0)
    compose_ok(gpu, b, F)
    check_equal(b, want)
    assert mode == 1 or any(len(b.nals(s)) > F for s in range(S))      # waypoint NALs among the scroll NALs
    eps = 0
    for s in range(S):
        for f in range(F):
            info = b.dyn_frame_info(s, f)
            nals = split_nals(per[s][1][f])
            if info is None:                                   # experiment mode: the waypoint NAL alone
                assert mode == 1 and len(nals) == 1, (s, f)
                continue
            assert info[1] == ep_bytes(nals[-1]), (s, f)
            eps += info[1]
    print("EP bytes", eps)
    assert content != "synth" or eps > 0
    b.close()


@pytest.mark.parametrize("flag", ["SCROLL_DEBUG_DYN_STAMPS", "SCROLL_DEBUG_DYN_GATHER1", "SCROLL_DEBUG_DYN_EPWIN"])
def test_debug_forms_keep_the_bytes(gpu, oracle, flag):
    """the stamped instantiations of k_dyn_row (their slots strided by the
    most groups of any placement), the one-chunk gather and the windowed EP
    path take the frame's origin too"""
    offs, pos = edge_case()
    S, F = offs.shape
    pos = [list(p) for p in pos]
    pos[2][0] = None
    R = striped_refs(oracle, W, H)
    src = np.stack([np.stack([np.frombuffer(bytes(rect_source(oracle, s, t, Rect(*(pos[s][t] or (0, 0)), RW, RH))),
                                            np.uint8) for t in range(F)]) for s in range(S)])
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, debug=getattr(gpu, flag))
    place(b, pos)
    b.set_offsets(offs)
    b.dyn_source_synth(F, 0, 0)
    compose_ok(gpu, b, F)
    check_equal(b, want_streams(oracle, W, H, offs, RW, RH, pos, src, R))
    b.close()


def test_frames_without_a_rect(gpu, oracle):
    """no rect in some frames: plain scroll NALs (k_emit) between the dynamic
    ones, no dynamic NAL for dyn_frame_info / dyn_recon / dyn_sse"""
    offs, pos = edge_case()
    S, F = offs.shape
    pos = [list(p) for p in pos]
    pos[0][1] = pos[0][3] = pos[1][0] = pos[2][5] = None       # (0, 3) and (2, 5) are waypoint frames
    pos[1][2:] = [None] * 4                                    # ... and (1, 2): a stream that ends without
    R = random_refs(W, H, 5)
    src = noise(6, S, F, RW, RH)
    want = want_streams(oracle, W, H, offs, RW, RH, pos, src, R)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    place(b, pos)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    check_equal(b, want)
    for s in range(S):
        for f in range(F):
            none = pos[s][f] is None
            assert (b.dyn_frame_info(s, f) is None) == none, (s, f)
            assert (b.dyn_recon(s, f) is None) == none and (b.dyn_sse(s, f) is None) == none, (s, f)
    assert b.dyn_totals()[2] == sum(p is not None for row in pos for p in row)
    b.close()


def test_every_frame_without_a_rect_and_every_frame_at_the_batch_position(gpu, oracle):
    offs, _ = edge_case()
    S, F = offs.shape
    R = random_refs(W, H, 7)
    src = noise(8, S, F, RW, RH)
    rect = (3, 9, RW, RH)
    # the rect off: the reference for "no rect anywhere"
    off = gpu.Batch(S, F, 8 << 20)
    for _ in range(S):
        off.add_stream(gpu.make_config(W, H))
    off.set_offsets(np.ascontiguousarray(offs))
    compose_ok(gpu, off, F)
    b = batch(gpu, W, H, S, F, rect, R)
    place(b, [[None] * F] * S)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    want = want_streams(oracle, W, H, offs, RW, RH, [[None] * F] * S, src, R)
    check_equal(b, want)
    for s in range(S):
        assert b.output(s) == off.output(s), s
    assert b.dyn_totals()[2] == 0
    off.close()
    b.close()
    # the flag on, every position the batch's: the flag-off bytes
    plain = batch(gpu, W, H, S, F, rect, R, moving=False)
    load(plain, offs, src)
    compose_ok(gpu, plain, F)
    b = batch(gpu, W, H, S, F, rect, R)
    place(b, [[rect[:2]] * F] * S)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    check_equal(b, want_streams(oracle, W, H, offs, RW, RH, [[rect[:2]] * F] * S, src, R))
    for s in range(S):
        assert b.output(s) == plain.output(s), s
    plain.close()
    b.close()


@pytest.mark.parametrize("rw,rh,pos", [(5, 1, [(0, 0), (15, 14)]), (17, 2, [(3, 13), (0, 5)])])
def test_row_widths(gpu, oracle, rw, rh, pos):
    """a 5-MB and a 17-MB row: k_dyn_row takes a different number of passes
    per wave"""
    w, h = 320, 240
    offs = np.array([[3, 130], [240, 77]], np.int32)
    P = [pos, pos[::-1]]
    R = random_refs(w, h, 9)
    src = noise(10, 2, 2, rw, rh)
    b = batch(gpu, w, h, 2, 2, (1, 1, rw, rh), R)
    place(b, P)
    load(b, offs, src)
    compose_ok(gpu, b, 2)
    check_equal(b, want_streams(oracle, w, h, offs, rw, rh, P, src, R))
    b.close()


@pytest.fixture(scope="module")
def config3_case(oracle):
    """1280x720 with a 25x25-MB rect, 2 streams x 3 frames at random legal
    positions and in the bottom-right corner: the expectation, computed once"""
    w, h, rw, rh, S, F = 1280, 720, 25, 25, 2, 3
    rng = random.Random(11)
    pos = [[(rng.randint(0, 80 - rw), rng.randint(0, 45 - rh)) for _ in range(F)] for _ in range(S)]
    pos[1][1] = (55, 20)
    offs = np.array([[490, 496, 502], [33, 700, 121]], np.int32)
    R = striped_refs(oracle, w, h)
    src = np.stack([np.stack([np.frombuffer(bytes(rect_source(oracle, s, 5 + t, Rect(*pos[s][t], rw, rh))), np.uint8)
                              for t in range(F)]) for s in range(S)])
    per = [oracle_moving(oracle, w, h, offs[s], rw, rh, pos[s], src[s], R) for s in range(S)]
    return w, h, rw, rh, S, F, pos, offs, R, per


@pytest.mark.parametrize("epcap4", [False, True])
def test_config3_shape_device_synth(gpu, config3_case, epcap4):
    """the source from k_dyn_synth, whose pattern follows each frame's
    position.  Once with SCROLL_DEBUG_DYN_EPCAP4: 4 EP positions kept per
    frame, so these moved frames (hundreds of EP bytes each) go through the
    serial emit path"""
    w, h, rw, rh, S, F, pos, offs, R, per = config3_case
    b = batch(gpu, w, h, S, F, (28, 10, rw, rh), R, arena=16 << 20, debug=gpu.SCROLL_DEBUG_DYN_EPCAP4 if epcap4 else 0)
    place(b, pos)
    b.set_offsets(offs)
    b.dyn_source_synth(F, 0, 5)
    compose_ok(gpu, b, F)
    check_equal(b, [p[0] for p in per])
    for s in range(S):
        for f in range(F):
            want_ep = ep_bytes(split_nals(per[s][1][f])[-1])
            assert want_ep > 4 and b.dyn_frame_info(s, f)[1] == want_ep, (s, f)
    b.close()


def test_per_frame_qps_and_reconstruction(gpu, oracle):
    """QPs 12 and 0 (the general path, 16-bit levels) beside 30 and 51 (int8)
    on four moved frames of one stream: k_dyn_row<true> and <false> in one
    compose at different origins; the decoded rects and their squared errors
    against the test decoder"""
    offs = np.array([[20, 496, 500, 131], [368, 2, 250, 99]], np.int32)
    pos = [[(0, 0), (4, 21), (2, 16), (2, 17)], [(0, 1), None, (2, 15), (3, 9)]]
    qps = [[12, 30, 0, 51], [26, 26, 26, 26]]
    S, F = offs.shape
    R = random_refs(W, H, 13)
    src = noise(14, S, F, RW, RH)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    b.set_dyn_qp_frames(qps[0], stream=0)
    place(b, pos)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    check_equal(b, want_streams(oracle, W, H, offs, RW, RH, pos, src, R, qps=qps))
    for s in range(S):
        frames = per_position(lambda rect: oracle_qp_frames(oracle, W, H, offs[s], rect, src[s], R, qps[s],
                                                            decode=True)[1], pos[s], RW, RH)
        for f, fr in enumerate(frames):
            if fr is None:
                assert b.dyn_recon(s, f) is None and b.dyn_sse(s, f) is None
                continue
            assert b.dyn_recon(s, f) == fr["rec"], (s, f)
            assert b.dyn_sse(s, f) == fr["sse"], (s, f)
    b.close()


def test_probe_and_pick_follow_the_positions(gpu, oracle):
    """the probe's bits / nonzero / squared error at moved positions are the
    oracle's at each frame's position and candidate; probe -> dyn_pick ->
    compose delivers the choices; a frame without a rect gets none"""
    offs = np.array([[20, 496, 500, 131], [368, 2, 250, 99]], np.int32)
    pos = [[(0, 0), (4, 21), (2, 16), (2, 17)], [(0, 1), None, (2, 15), (3, 9)]]
    cand = [12, 26, 39]
    S, F = offs.shape
    R = random_refs(W, H, 15)
    src = noise(16, S, F, RW, RH)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    place(b, pos)
    load(b, offs, src)
    res = b.dyn_probe(F, cand)
    for s in range(S):
        for k, qp in enumerate(cand):
            frames = per_position(lambda rect: oracle_probe(oracle, W, H, offs[s], rect, src[s], R, qp)[1], pos[s],
                                  RW, RH)
            for f, fr in enumerate(frames):
                got = res[s, f, k]
                if fr is None:
                    assert got["valid"] == 0, (s, f, k)
                    continue
                print(f"stream {s} frame {f} cand {k}: bits {got['bits']} / {fr['bits']}, sse "
                      f"{tuple(int(v) for v in got['sse'])} / {fr['sse']}")
                assert got["valid"] == 1, (s, f, k)
                assert (int(got["bits"]), int(got["nonzero"])) == (fr["bits"], fr["nonzero"]), (s, f, k)
                assert tuple(int(v) for v in got["sse"]) == fr["sse"], (s, f, k)
    cost = cost_of(res, cand)
    budget = int(cost[0, 0].min() + cost[0, 0].max()) // 2
    k, qp, st = b.dyn_pick(F, budget)
    per = [[26] * F for _ in range(S)]
    for s in range(S):
        for f in range(F):
            if pos[s][f] is None:
                assert (k[s, f], qp[s, f], st[s, f]) == (-1, -1, 2), (s, f)
                continue
            wk, wst = pick_np(res[s, f], cand, budget)
            assert (k[s, f], st[s, f]) == (wk, wst), (s, f)
            per[s][f] = cand[wk]
    compose_ok(gpu, b, F)
    check_equal(b, want_streams(oracle, W, H, offs, RW, RH, pos, src, R, qps=per))
    for s in range(S):
        for f in range(F):
            if pos[s][f] is not None:
                assert b.dyn_sse(s, f) == tuple(int(v) for v in res[s, f, k[s, f]]["sse"]), (s, f)
    b.close()


def test_source_from_surfaces_at_moved_positions(gpu, hip, oracle):
    """whole-picture surfaces cut at each frame's position, without hints,
    then a compose: the bytes of a batch fed the numpy-cropped,
    numpy-converted pixels through set_dyn_source"""
    S, F = 2, 3
    pos = [[(0, 0), (4, 21), None], [(2, 16), (2, 17), (0, 1)]]
    offs = np.array([[20, 496, 500], [368, 2, 250]], np.int32)
    R = random_refs(W, H, 17)
    sf = Surfaces(hip, S, F, W, H, seed=18)
    src = np.zeros((S, F, 384 * RW * RH), np.uint8)
    for s in range(S):
        for f in range(F):
            if pos[s][f]:
                src[s, f] = np.frombuffer(i420_bytes(cut(sf.img[s, f], *pos[s][f], RW, RH), RGBA, BT601, 0), np.uint8)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    c = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    try:
        place(b, pos)
        place(c, pos)
        b.set_offsets(offs)
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride)
        compose_ok(gpu, b, F)
        load(c, offs, src)
        compose_ok(gpu, c, F)
        check_equal(b, want_streams(oracle, W, H, offs, RW, RH, pos, src, R))
        for s in range(S):
            assert b.output(s) == c.output(s), s
    finally:
        b.close()
        c.close()
        sf.free()


def test_chunks_and_resets(gpu, oracle):
    """entry f applies to frame f of each compose (2 + 2 frames);
    set_dyn_rect resets the positions (and drops the flag with the rect);
    clear_hints after a hinted compose resets them too"""
    offs = np.array([[492, 496, 500, 504, 20, 30], [20, 300, 496, 368, 7, 9]], np.int32)
    S = 2
    R = random_refs(W, H, 19)
    src = noise(20, S, 6, RW, RH)
    two = [[(0, 0), (4, 21)], [(2, 16), None]]
    b = batch(gpu, W, H, S, 2, (1, 1, RW, RH), R)
    place(b, two)
    for c in range(2):
        load(b, offs[:, 2 * c:2 * c + 2], src[:, 2 * c:2 * c + 2])
        compose_ok(gpu, b, 2)
    pos = [two[s] + two[s] for s in range(S)]
    check_equal(b, want_streams(oracle, W, H, offs[:, :4], RW, RH, pos, src[:, :4], R))
    # a hinted compose at these positions, then clear_hints: the batch's position again, the flag still on
    b.set_hints(0, 0, [], EXACT)
    load(b, offs[:, 4:6], src[:, 4:6])
    compose_ok(gpu, b, 2)
    b.clear_hints()
    b.reset_output()
    for s in range(S):                  # (reset_output keeps the streams' frame_num and waypoints: restart them)
        b.set_config(s, gpu.make_config(W, H))
    load(b, offs[:, :2], src[:, :2])
    compose_ok(gpu, b, 2)
    check_equal(b, want_streams(oracle, W, H, offs[:, :2], RW, RH, [[(1, 1)] * 2] * S, src[:, :2], R))
    # moved again, then set_dyn_rect: positions reset, the flag gone with the rect
    place(b, two)
    b.set_dyn_rect(3, 9, RW, RH)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    b.reset_output()
    for s in range(S):
        b.set_config(s, gpu.make_config(W, H))
    load(b, offs[:, :2], src[:, :2])
    compose_ok(gpu, b, 2)
    check_equal(b, want_streams(oracle, W, H, offs[:, :2], RW, RH, [[(3, 9)] * 2] * S, src[:, :2], R))
    b.set_dyn_rect_at(0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="hints"):
        b.compose(2)
    b.close()


def test_same_bytes_as_the_hinted_path(gpu, oracle):
    """GPU against GPU, beside the oracle check: the positions composed under
    hints with empty rect lists in EXACT mode (k_hdyn_code + k_splice_stage)"""
    offs, pos = edge_case()
    S, F = offs.shape
    pos = [list(p) for p in pos]
    pos[1][1] = None
    R = random_refs(W, H, 21)
    src = noise(22, S, F, RW, RH)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    hb = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, moving=False)
    place(b, pos)
    place(hb, pos)
    for s in range(S):
        for f in range(F):
            hb.set_hints(s, f, [], EXACT)
    for x in (b, hb):
        load(x, offs, src)
        compose_ok(gpu, x, F)
    check_equal(b, want_streams(oracle, W, H, offs, RW, RH, pos, src, R))
    for s in range(S):
        assert b.output(s) == hb.output(s), s
    b.close()
    hb.close()


def test_contract(gpu, oracle):
    lib = gpu.lib
    R = random_refs(W, H, 23)
    b0 = gpu.Batch(1, 2, 1 << 20)
    b0.add_stream(gpu.make_config(W, H))
    assert lib.scroll_batch_set_dyn_rect_moving(b0.h, 1) == gpu.SCROLL_ERR_CONFIG     # no rect
    assert "scroll_batch_set_dyn_rect" in gpu.last_error()
    assert lib.scroll_batch_set_dyn_rect_moving(b0.h, 0) == 0
    b0.close()
    offs = np.array([[496, 20]], np.int32)
    src = noise(24, 1, 2, RW, RH)
    b = batch(gpu, W, H, 1, 2, (1, 1, RW, RH), R, moving=False)
    b.set_dyn_rect_at(0, 1, 2, 16)
    load(b, offs, src)
    assert lib.scroll_batch_compose(b.h, 2, None) == gpu.SCROLL_ERR_CONFIG              # flag off: today's refusal
    assert "need UI hints" in gpu.last_error()
    b.set_dyn_rect_moving()
    with pytest.raises(RuntimeError, match="leaves the picture"):
        b.set_dyn_rect_at(0, 0, 5, 0)
    with pytest.raises(RuntimeError, match="leaves the picture"):
        b.set_dyn_rect_at(0, 0, 0, 22)
    compose_ok(gpu, b, 2)
    pos = [[(1, 1), (2, 16)]]
    check_equal(b, want_streams(oracle, W, H, offs, RW, RH, pos, src, R))
    b.set_dyn_rect_moving(False)                               # off again: refused again, nothing committed
    size = b.output_size(0)
    assert lib.scroll_batch_compose(b.h, 2, None) == gpu.SCROLL_ERR_CONFIG
    assert b.sync() == 0 and b.output_size(0) == size
    b.close()
