"""CPU pin of the moving plain rect's definition (tests/dynposhelp.py).

The expected stream of a compose with scroll_batch_set_dyn_rect_moving on is
assembled frame by frame from whole-stream runs of or_compose_dyn with the
uniform rect at each frame's position (and of the scroll oracle for a frame
without a rect).  oracle/splice_oracle.c's or_compose_hint_dyn takes a rect
position per frame by itself; with no hint rects in EXACT mode it codes the
same field, so the two independently written oracles must agree byte for
byte.  Also: the library exports the call.  No GPU needed."""
import ctypes

import numpy as np

from dynhelp import split_nals
from dynposhelp import oracle_moving, per_position, uniform_run
from qpfhelp import oracle_qp_frames
from reconhelp import random_refs, striped_refs
from test_gpu_dyn import oracle_streams
from test_gpu_hintdyn import EXACT, oracle_hintdyn
from dynhelp import Rect

W, H, RW, RH = 96, 368, 2, 2


def case():
    """a waypoint on the way (offset 496: frame 3 carries its waypoint NAL,
    the frames after it predict through it), one frame without a rect, the
    picture's edges and the static-group seam"""
    offs = np.array([[20, 300, 492, 496, 500, 504, 120, 368]], np.int32)
    pos = [(0, 0), (4, 21), None, (2, 15), (2, 16), (2, 17), (0, 1), (3, 9)]
    return offs, pos


def test_assembly_equals_hint_oracle_without_hint_rects(oracle):
    offs, pos = case()
    F = offs.shape[1]
    R = random_refs(W, H, 5)
    src = np.random.default_rng(6).integers(0, 256, (1, F, 384 * RW * RH), dtype=np.uint8)
    want, frames = oracle_moving(oracle, W, H, offs[0], RW, RH, pos, src[0], R)
    nn = [len(split_nals(fr)) for fr in frames]
    assert 2 in nn and 1 in nn, nn                     # a waypoint NAL sits among the scroll NALs
    plan = {(0, f): ([], EXACT, pos[f]) for f in range(F)}
    other = oracle_hintdyn(oracle, W, H, offs, RW, RH, plan, src, R)[0]
    assert want == other
    # experiment mode: the waypoint NAL replaces the frame's scroll NAL in every run
    want1, _ = oracle_moving(oracle, W, H, offs[0], RW, RH, pos, src[0], R, mode=1)
    assert want1 == oracle_hintdyn(oracle, W, H, offs, RW, RH, plan, src, R, compose_mode=1)[0]
    assert want1 != want


def test_uniform_positions_and_no_rect_are_the_existing_oracles(oracle):
    offs, _ = case()
    F = offs.shape[1]
    R = striped_refs(oracle, W, H)
    src = np.random.default_rng(7).integers(0, 256, (1, F, 384 * RW * RH), dtype=np.uint8)
    got, _ = oracle_moving(oracle, W, H, offs[0], RW, RH, [(3, 9)] * F, src[0], R)
    assert got == oracle_streams(oracle, W, H, offs, Rect(3, 9, RW, RH), src, R)[0]
    none, _ = oracle_moving(oracle, W, H, offs[0], RW, RH, [None] * F, src[0], R)
    assert none == b"".join(uniform_run(oracle, W, H, offs[0], None, src[0], R))
    assert none == oracle_streams(oracle, W, H, offs, Rect(0, 0, 0, 0), src, R)[0]


def test_a_frame_does_not_depend_on_the_frames_before_it(oracle):
    """the premise: calling the oracle once per frame with that frame's rect
    (its state advancing through the moved frames) gives the assembly"""
    offs, pos = case()
    F = offs.shape[1]
    R = random_refs(W, H, 8)
    src = np.random.default_rng(9).integers(0, 256, (F, 384 * RW * RH), dtype=np.uint8)
    qps = [12, 30, 26, 0, 51, 22, 21, 26]
    want, frames = oracle_moving(oracle, W, H, offs[0], RW, RH, pos, src, R, qps=qps)
    oracle.or_compose_dyn.restype = ctypes.c_size_t
    from dynhelp import OrCfg, qp_field
    cfg = OrCfg()
    oracle.or_cfg_init(ctypes.byref(cfg), W, H)
    cfg.frame_num = 2
    buf = (ctypes.c_uint8 * (1 << 20))()
    out = bytearray()
    for f in range(F):
        rc = Rect(pos[f][0], pos[f][1], RW, RH, qp_field(qps[f])) if pos[f] else Rect(0, 0, 0, 0, 0)
        sp = np.ascontiguousarray(src[f])
        n = oracle.or_compose_dyn(buf, len(buf), ctypes.byref(cfg), int(offs[0, f]), 0, ctypes.byref(rc),
                                  sp.ctypes.data_as(ctypes.c_void_p) if pos[f] else None, ctypes.byref(R.refs), None)
        out += bytes(buf[:n])
    assert bytes(out) == want
    # the per-frame selection of another helper's frames: the same NALs
    sel = per_position(lambda rect: oracle_qp_frames(oracle, W, H, offs[0], rect, src, R, qps)[1], pos, RW, RH)
    for f in range(F):
        assert (sel[f] is None) == (pos[f] is None)
        if sel[f]:
            assert sel[f]["data"] == frames[f], f


def test_library_exports_the_call(scroll):
    assert hasattr(scroll.lib, "scroll_batch_set_dyn_rect_moving")
    fn = ctypes.CDLL(scroll.lib._name).scroll_batch_set_dyn_rect_moving
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert fn(None, 1) == scroll.SCROLL_ERR_ARG        # no batch: refused before anything touches a device
