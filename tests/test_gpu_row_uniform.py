"""k_dyn_row reads its uniform state where it is used: one argument struct in
the kernel-argument segment, the late values (the hand-off's granules, phase
5's row-stage / spill-pool pointers and strides, the rare paths' NAL context)
loaded at the head of their phase, and the stamps / NOPUBLISH state only in a
debug instantiation the launcher picks when either is on.

Every case is byte for byte the oracle's (oracle/dyn_oracle.c through the
helpers of tests/test_gpu_dyn.py, tests/designed.py) and runs twice: with the
product instantiation and, SCROLL_DEBUG_DYN_STAMPS set, with the debug one --
the same expectation both times, so the two give identical bytes.  The cases
are the places a late value is read: the plain path (a), the spill pool with
its pointers changed between two launches (b), the wide bit window with four
tasks per thread (c), several window passes (d), overflow pieces in the token
and the write phase (e), a general-path NAL beside normal ones (f), two
batches with different arguments in flight on two HIP streams (g), a new rect
and QP between the composes of one batch (h).

head_over (an MB head over 128 bits, the path that builds the NAL's HeadCtx
again from the argument segment): no input reaches it.  A head is two
mb_type bits, ref_idx (a bit, or ue of at most 7), the horizontal mvd -- the
predictor's px is always 0 and so is the motion: se(0), one bit -- and
se(vertical mvd), at most 65 bits for any 32-bit value: under 80 bits
whatever the offsets, and k_dyn_rows sets the flag past 128.  So that branch
keeps the code it had, re-deriving what it needs, and no case here runs it.
Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

import designed as dz
from conftest import synthetic_offsets
from dynhelp import OrCfg, Rect, qp_field
from test_gpu_dyn import (check_equal, gpu, gpu_streams, oracle_streams, random_refs,  # noqa: F401
                          striped_refs, synth_source)
from test_gpu_ipcm import Hip

pytestmark = pytest.mark.gpu

DBG = pytest.mark.parametrize("dbg", [False, True], ids=["product", "stamps"])
_want = {}                                  # the oracle's streams per case, made once


def want_of(key, make):
    if key not in _want:
        _want[key] = make()
    return _want[key]


def flag(gpu, dbg):
    return gpu.SCROLL_DEBUG_DYN_STAMPS if dbg else 0


@DBG
def test_a_plain_path_with_waypoints(gpu, oracle, dbg):
    """a 3x2-MB rect at (1, 1) of a 96x96 picture, two streams; stream 0's
    offsets cross 496 (a waypoint NAL between its dynamic ones)"""
    w, h = 96, 96
    rect = Rect(1, 1, 3, 2)
    S, F = 2, 8
    offs = synthetic_offsets(S, F, h)
    offs[0] = 480 + 4 * np.arange(F)
    R = random_refs(w, h, 31)
    src = synth_source(oracle, S, F, rect)
    want = want_of("a", lambda: oracle_streams(oracle, w, h, offs, rect, src, R))
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src, debug=flag(gpu, dbg))
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    nals = b.nals(0)
    assert any(k == 1 and sl == 0 for k, _, _, sl in nals)         # the waypoint
    assert sum(sl == 2 for _, _, _, sl in nals) == F
    b.close()


def spill_case(oracle):
    """the designed extremes (group d, QP 22), the frame of the largest MBs
    twelve times and the four frames once: 16 frames of 2 rect rows, at least
    24 of each stream's 32 rows past their row-stage slot"""
    def make():
        fr = dz.cases(oracle)["d_extremes_qp22"].frames
        c = dz.Case("row_uniform_spill", "d", 22, [fr[3]] * 12 + list(fr))
        return c, oracle_streams(oracle, c.w, c.h, c.offs, c.rect(), c.src, c.R)
    return want_of("b", make)


@DBG
def test_b_spill_pool_grows_between_launches(gpu, oracle, dbg):
    """96 streams of the extremes: 3,072 rect rows, a spill pool of 2,048
    slots and more rows than that past their slot.  The first compose runs
    the pool out (SCROLL_ERR_OVERFLOW, nothing committed) and the batch grows
    it -- the row stage and the spill pool are new allocations -- and the
    second compose, with the new pointers in its argument segment, is exact"""
    c, want2 = spill_case(oracle)
    S = 96
    pick = [k % 2 for k in range(S)]
    b = gpu.Batch(S, c.F, 1 << 20)
    b.set_debug(flag(gpu, dbg))
    for _ in range(S):
        b.add_stream(gpu.make_config(c.w, c.h))
    b.set_dyn_rect(*c.rc)
    b.set_dyn_qp(c.qp)
    b.set_dyn_refs(c.R.i420(0), c.R.i420(1))
    b.set_offsets(np.ascontiguousarray(c.offs[pick]))
    b.set_dyn_source(np.ascontiguousarray(c.src[pick]).tobytes(), c.F)
    b.compose(c.F)
    assert b.sync() == -4, gpu.last_error()                         # SCROLL_ERR_OVERFLOW
    assert "pool ran out" in gpu.last_error() and "grown" in gpu.last_error()   # (no general-path NAL here)
    assert all(b.output_size(s) == 0 for s in range(S))
    b.compose(c.F)
    assert b.sync() == 0, gpu.last_error()
    check_equal(b, [want2[k] for k in pick])
    b.close()


@DBG
def test_c_wide_rect(gpu, oracle, dbg):
    """47x2 MBs in a 752x64 picture: past SCROLL_ROW_WIDE, so four block
    tasks per thread and the wide bit window in dynamic LDS"""
    w, h = 752, 64
    rect = Rect(0, 1, 47, 2)
    S, F = 2, 3
    offs = synthetic_offsets(S, F, h, first_stream=4)
    R = random_refs(w, h, 33)
    src = synth_source(oracle, S, F, rect)
    want = want_of("c", lambda: oracle_streams(oracle, w, h, offs, rect, src, R))
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src, debug=flag(gpu, dbg))
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@DBG
def test_d_several_window_passes(gpu, oracle, dbg):
    """40x2 MBs (the static 896-word window) over random references: every
    frame is more than twice a window, so one of its two rect rows -- they
    hold all but the two static rows' few bits -- takes a second pass"""
    w, h = 640, 64
    rect = Rect(0, 1, 40, 2)
    S, F = 2, 3
    offs = synthetic_offsets(S, F, h, first_stream=7)
    R = random_refs(w, h, 35)
    src = synth_source(oracle, S, F, rect)
    want = want_of("d", lambda: oracle_streams(oracle, w, h, offs, rect, src, R))
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src, debug=flag(gpu, dbg))
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    sizes = [sz for s in range(S) for _, _, sz, sl in b.nals(s) if sl == 2]
    assert len(sizes) == S * F and min(sizes) > 2 * 4 * 896 + 1024, sizes
    b.close()


@DBG
@pytest.mark.parametrize("name", ["c_lengths_qp24", "d_extremes_qp22"])
def test_e_overflow_pieces(gpu, oracle, name, dbg):
    """bodies of 129 to 140 bits (group c) and the extremes' largest blocks:
    M_OVF pieces, counted by ovf_bits in the token phase and written by
    ovf_put in the write phase"""
    c = dz.cases(oracle)[name]
    b, rc = gpu_streams(gpu, c.w, c.h, c.offs, c.rect(), c.R, c.src, debug=flag(gpu, dbg))
    assert rc == 0, gpu.last_error()
    check_equal(b, dz.want_of(oracle, name))
    b.close()


@DBG
def test_f_general_path_nal_beside_normal_ones(gpu, oracle, dbg):
    """a waypoint at an odd offset: stream 0's frames past it predict through
    a half-pel chroma chain (k_dyn_code_general -> k_dyn_row<true>), its frame
    before it and all of stream 1 take the normal instantiation, in the same
    launches"""
    w, h = 64, 1024
    rect = Rect(1, 0, 2, 48)
    wps = [(501, 2, 1)]
    offs = np.array([[40, 600, 610, 777, 505, 996], [10, 21, 32, 43, 54, 65]], np.int32)
    S, F = offs.shape
    R = random_refs(w, h, 5)
    src = synth_source(oracle, S, F, rect)
    want = want_of("f", lambda: oracle_streams(oracle, w, h, offs, rect, src, R, waypoints=wps))
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src, waypoints=wps, debug=flag(gpu, dbg))
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@DBG
def test_g_two_batches_on_two_hip_streams(gpu, oracle, dbg):
    """two batches, different pictures, rects and QPs, composed alternately
    on two non-blocking HIP streams, three composes each without a sync in
    between: each launch carries its own arguments"""
    L = Hip().lib
    L.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.hipStreamCreateWithFlags.restype = ctypes.c_int
    L.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    S, F, N = 2, 4, 3
    geoms = [(96, 96, Rect(1, 1, 3, 2, qp_field(26)), 41), (128, 96, Rect(2, 0, 4, 3, qp_field(31)), 43)]
    streams, batches, wants = [], [], []
    try:
        for k, (w, h, rect, seed) in enumerate(geoms):
            cs = ctypes.c_void_p()
            assert L.hipStreamCreateWithFlags(ctypes.byref(cs), 1) == 0    # hipStreamNonBlocking
            streams.append(cs)
            offs = synthetic_offsets(S, F, h, first_stream=k)
            R = random_refs(w, h, seed)
            src = synth_source(oracle, S, F, rect)
            wants.append(want_of(("g", k), lambda: oracle_streams(oracle, w, h, np.tile(offs, (1, N)), rect,
                                                                  np.tile(src, (1, N, 1)), R)))
            b = gpu.Batch(S, F, 1 << 20)
            b.set_debug(flag(gpu, dbg))
            for _ in range(S):
                b.add_stream(gpu.make_config(w, h))
            b.set_dyn_rect(rect.x0, rect.y0, rect.w, rect.h)
            b.set_dyn_qp(rect.qp)
            b.set_dyn_refs(R.i420(0), R.i420(1))
            b.set_offsets(offs)
            b.set_dyn_source(src.tobytes(), F)
            batches.append(b)
        for _ in range(N):
            for b, cs in zip(batches, streams):
                b.compose(F, stream=cs.value)
        for b, want in zip(batches, wants):
            assert b.sync() == 0, gpu.last_error()
            check_equal(b, want)
    finally:
        for b in batches:
            b.close()
        for cs in streams:
            L.hipStreamDestroy(cs)


def oracle_two_rects(oracle, w, h, offs, parts, R):
    """one stream state through parts = [(rect, src [S][F][...]), ...]: F
    frames with each rect in turn"""
    oracle.or_compose_dyn.restype = ctypes.c_size_t
    buf = (ctypes.c_uint8 * (4 << 20))()
    nwp = ctypes.c_int()
    outs = []
    for s in range(offs.shape[0]):
        cfg = OrCfg()
        oracle.or_cfg_init(ctypes.byref(cfg), w, h)
        cfg.frame_num = 2
        o, t = bytearray(), 0
        for rect, src in parts:
            for f in range(src.shape[1]):
                sp = np.ascontiguousarray(src[s, f])
                n = oracle.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(offs[s, t]), 0, ctypes.byref(rect),
                                          sp.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), ctypes.byref(nwp))
                assert n > 0
                o += bytes(buf[:n])
                t += 1
        outs.append(bytes(o))
    return outs


@DBG
def test_h_new_rect_and_qp_between_composes(gpu, oracle, dbg):
    """one batch: four frames with a 3x2 rect at QP 26, then set_dyn_rect (a
    5x3 rect elsewhere: new geometry, new buffers) and QP 33, four more"""
    w, h = 128, 96
    S, F = 2, 4
    ra, rb = Rect(1, 1, 3, 2, qp_field(26)), Rect(3, 2, 5, 3, qp_field(33))
    offs = synthetic_offsets(S, 2 * F, h, first_stream=3)
    R = random_refs(w, h, 47)
    sa, sb = synth_source(oracle, S, F, ra), synth_source(oracle, S, F, rb, t0=F)
    want = want_of("h", lambda: oracle_two_rects(oracle, w, h, offs, [(ra, sa), (rb, sb)], R))
    b = gpu.Batch(S, F, 1 << 20)
    b.set_debug(flag(gpu, dbg))
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h))
    for k, (rect, src) in enumerate(((ra, sa), (rb, sb))):
        b.set_dyn_rect(rect.x0, rect.y0, rect.w, rect.h)
        b.set_dyn_qp(rect.qp)
        b.set_dyn_refs(R.i420(0), R.i420(1))
        b.set_offsets(np.ascontiguousarray(offs[:, k * F:(k + 1) * F]))
        b.set_dyn_source(src.tobytes(), F)
        b.compose(F)
        assert b.sync() == 0, gpu.last_error()
    check_equal(b, want)
    b.close()
