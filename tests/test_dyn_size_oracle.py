"""CPU pin of the sized plain rect's definition (tests/dynsizehelp.py).

The expected stream of a compose with frames sized by
scroll_batch_set_dyn_rect_size_at is one or_compose_dyn call per frame with
that frame's rect {x0, y0, w_f, h_f} and its source in the sized layout.
oracle/splice_oracle.c's or_compose_hint_dyn takes a rect per call by itself;
with no hint rects in EXACT mode it codes the same field, so the two
independently written oracles must agree byte for byte.  Also the located
size rule, in numpy, against damagehelp's box, and the library's export.  No
GPU needed."""
import ctypes

import numpy as np
import pytest

from damagehelp import FIT, OVER, locate_np, record_tuple
from dynhelp import OrCfg, Rect, split_nals
from dynposhelp import oracle_moving
from dynsizehelp import locate_sized_np, sized_place, sized_stream, size_word, table_word
from reconhelp import random_refs
from test_gpu_hintdyn import EXACT, hint_array

W, H, RW, RH = 96, 368, 3, 3


def case():
    """offsets through the 496 waypoint (frame 3 carries its waypoint NAL, the
    frames after it predict through it); sizes 1x1, w x 1, 1 x h and full, one
    frame without a rect; the picture's edges and the static-group seam"""
    offs = np.array([20, 300, 492, 496, 500, 504, 120, 368], np.int32)
    rects = [(0, 0, 1, 1), (3, 20, 3, 1), None, (1, 15, 1, 3), (1, 16, 3, 3), (1, 17, 2, 2), (0, 1, 3, 3),
             (3, 9, 1, 1)]
    return offs, rects


def hint_oracle_sized(oracle, offs, rects, src, R, mode=0):
    """or_compose_hint_dyn, no hint rects, EXACT, the frame's rect per call"""
    oracle.or_compose_hint_dyn.restype = ctypes.c_size_t
    buf = (ctypes.c_uint8 * (4 << 20))()
    err = ctypes.c_int()
    c = OrCfg()
    oracle.or_cfg_init(ctypes.byref(c), W, H)
    c.frame_num = 2
    out = bytearray()
    arr, n = hint_array([])
    for f, rc in enumerate(rects):
        r = Rect(*rc, 0) if rc else None
        sp = np.ascontiguousarray(src[f][:384 * rc[2] * rc[3]] if rc else src[f])
        k = oracle.or_compose_hint_dyn(buf, len(buf), ctypes.byref(c), int(offs[f]), mode, arr, n, EXACT,
                                       ctypes.byref(r) if r else None, sp.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.byref(R.refs), ctypes.byref(err))
        assert err.value == 0 and k > 0, (f, err.value)
        out += bytes(buf[:k])
    return bytes(out)


@pytest.mark.parametrize("mode", [0, 1])
def test_assembly_equals_hint_oracle_with_the_frames_rect_per_call(oracle, mode):
    offs, rects = case()
    F = len(offs)
    R = random_refs(W, H, 5)
    src = np.random.default_rng(6).integers(0, 256, (F, 384 * RW * RH), dtype=np.uint8)
    want, frames = sized_stream(oracle, W, H, offs, rects, src, R, mode=mode)
    nn = [len(split_nals(fr)) for fr in frames]
    if mode == 0:
        assert 2 in nn and 1 in nn, nn                 # a waypoint NAL sits among the scroll NALs
    assert want == hint_oracle_sized(oracle, offs, rects, src, R, mode=mode)


def test_every_frame_at_full_size_is_the_moved_rects_assembly(oracle):
    offs, rects = case()
    F = len(offs)
    R = random_refs(W, H, 9)
    src = np.random.default_rng(10).integers(0, 256, (F, 384 * RW * RH), dtype=np.uint8)
    full = [None if rc is None else (rc[0], rc[1], RW, RH) for rc in rects]
    pos = [None if rc is None else rc[:2] for rc in rects]
    assert sized_stream(oracle, W, H, offs, full, src, R)[0] == oracle_moving(oracle, W, H, offs, RW, RH, pos, src,
                                                                             R)[0]
    # ... and every frame at one smaller size is the assembly of a batch with that rect
    small = [None if rc is None else (rc[0], rc[1], 2, 1) for rc in rects]
    src21 = np.ascontiguousarray(src[:, :384 * 2])
    assert sized_stream(oracle, W, H, offs, small, src, R)[0] == oracle_moving(oracle, W, H, offs, 2, 1, pos, src21,
                                                                              R)[0]


# ---- the located size rule ----

MBW, MBH = 12, 23


def damage(mbs):
    m = np.zeros((MBH, MBW), np.uint32)
    for mx, my in mbs:
        m[my, mx] = 1000 + 7 * mx + my
    return m


BOXES = [[(2, 3), (4, 5)],                  # 3 x 3: exactly w x h
         [(2, 3), (5, 5)],                  # one more column
         [(2, 3), (4, 6)],                  # one more row
         [(5, 5)],                          # 1 x 1
         [(11, 22)],                        # the bottom-right MB: the origin clamps to (mbw - w, mbh - h)
         [(10, 4), (11, 4)],                # the right edge
         [(3, 21), (3, 22)],                # the bottom edge
         [(0, 0), (11, 22)]]                # the whole picture


@pytest.mark.parametrize("margin", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("mbs", BOXES)
def test_located_size_rule(mbs, margin):
    w, h = 3, 3
    m = damage(mbs)
    base = locate_np(m, w, h, 0, margin)
    r, rect = locate_sized_np(m, w, h, 0, margin)
    assert base["status"] in (FIT, OVER)
    x0, y0, wf, hf = rect
    # the origin rule is the placed one; the rect stays inside the batch size and the picture
    assert (x0, y0) == (base["x0"], base["y0"]) and 1 <= wf <= w and 1 <= hf <= h
    assert x0 + wf <= MBW and y0 + hf <= MBH
    bw, bh = base["bx1"] - base["bx0"], base["by1"] - base["by0"]
    if base["status"] == FIT:
        # origin-to-box-end: every damaged MB inside, nothing of the box outside
        assert (x0 + wf, y0 + hf) == (base["bx1"], base["by1"])
        assert r["sse_out"] == 0
        assert wf >= bw and hf >= bh                   # (larger only where the origin was clamped)
        assert (wf, hf) == (bw, bh) or x0 < base["bx0"] or y0 < base["by0"]
    else:
        assert wf == w or hf == h                      # the batch size in a dimension that is over
        assert (wf == w) == (base["bx1"] >= x0 + w) and (hf == h) == (base["by1"] >= y0 + h)
    assert r["reserved"] == size_word(wf, hf)
    # everything else as without the size
    keep = [n for n in base if n not in ("reserved", "sse_out")]
    assert [r[n] for n in keep] == [base[n] for n in keep]
    assert r["sse_out"] >= base["sse_out"]              # the sized rect lies inside the batch-sized one
    e = table_word(x0, y0, w, h, wf, hf)
    assert e & 0xff == x0 and (e >> 16) & 0xff == y0 and w - ((e >> 8) & 0xff) == wf and h - (e >> 24) == hf


def test_size_zero_records_are_the_existing_ones():
    for mbs in BOXES:
        m = damage(mbs)
        r = locate_np(m, 3, 3, 0, 1)
        assert r["reserved"] == 0 and record_tuple(r)[7] == 0
    assert sized_place((2, 3, 5, 6), 3, 3, MBW, MBH) == (2, 3, 3, 3)
    assert sized_place((11, 22, 12, 23), 3, 3, MBW, MBH) == (9, 20, 3, 3)
    assert sized_place((5, 5, 6, 6), 3, 3, MBW, MBH) == (5, 5, 1, 1)


def test_library_exports_the_call(scroll):
    assert hasattr(scroll.lib, "scroll_batch_set_dyn_rect_size_at")
    fn = ctypes.CDLL(scroll.lib._name).scroll_batch_set_dyn_rect_size_at
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
    assert fn(None, 0, 0, 1, 1) == scroll.SCROLL_ERR_ARG       # no batch: refused before anything touches a device
