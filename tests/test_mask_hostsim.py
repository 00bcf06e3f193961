"""The rule of the dynamic rect's per-MB source mask (h264-scroll-encoder_amd/
csrc/mask_device.h: k_dyn_mask_diff / k_dyn_mask_fill / k_dyn_mask_rec run it
on the device), compiled for the CPU (tests/hostsim/mask_sim.cpp), against the
numpy restatement of tests/maskhelp.py; and the mask's premise, on the oracle
alone: a source doctored by the helper, through or_compose_dyn and the test
decoder, codes its dropped MBs with coded_block_pattern 0 and leaves the kept
ones as they were.  Every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import h264_pslice as hp
from conftest import PKG, REPO
from damagehelp import frame_states
from maskhelp import KEPT, MASK_DTYPE, NOFRAME, doctor, mask_map_np, mask_np, noisy, paint_mbs, pred_rect, \
    record_np, record_tuple, scroll_nals
from reconhelp import oracle_frames, random_refs

SRC = os.path.join(REPO, "tests", "hostsim", "mask_sim.cpp")
FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(REPO, "tests", "hostsim"), "-I", os.path.join(REPO, "include"),
         "-I", os.path.join(PKG, "csrc")]
DY_MAX, DC_MAX = 256 * 255 * 255, 128 * 255 * 255


@pytest.fixture(scope="module")
def mksim(tmp_path_factory):
    """TEST-ONLY CPU build of mask_device.h; the library lands in pytest's
    temp directory"""
    so = str(tmp_path_factory.mktemp("mksim") / "libmksim.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", *FLAGS, SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32 = ctypes.c_uint32
    lib.mksim_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [u32] * 5 + [ctypes.c_void_p]
    lib.mksim_parts.argtypes = lib.mksim_frame.argtypes
    lib.mksim_parts.restype = u32
    lib.mksim_noframe.argtypes = [ctypes.c_void_p]
    lib.mksim_map.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u32, u32, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.mksim_record_size() == MASK_DTYPE.itemsize == 40 and lib.mksim_rule_size() == 12
    return lib


def check(lib, m, dcb, ty=0, tc=0, grow=0):
    """the serial walk and the kernels' walk against the helper: KEPT bits and record; returns (record, kept)"""
    m = np.ascontiguousarray(m, dtype=np.uint32)
    dcb = np.ascontiguousarray(dcb, dtype=np.uint32)
    h, w = dcb.shape
    want, wmap = record_np(m, dcb, ty, tc, grow)
    for fn in (lib.mksim_frame, lib.mksim_parts):
        got_m, rec = m.copy(), np.zeros(1, MASK_DTYPE)
        rc = fn(got_m.ctypes.data, dcb.ctypes.data, w, h, ty, tc, grow, rec.ctypes.data)
        assert fn is lib.mksim_frame or rc == 0, "the quad's four parts disagree with the whole"
        assert np.array_equal(got_m, wmap), (w, h, ty, tc, grow)
        assert record_tuple(rec[0]) == record_tuple(want), (w, h, ty, tc, grow)
    return want, (wmap[..., 1] & KEPT) != 0


def blank(w, h, *mbs, dy=9, dc=0):
    m = np.zeros((h, w, 2), np.uint32)
    for x, y in mbs:
        m[y, x] = (dy, dc)
    return m, np.zeros((h, w), np.uint32)


def test_random_maps(mksim):
    rng = np.random.default_rng(1)
    for it in range(400):
        w, h = int(rng.integers(1, 21)), int(rng.integers(1, 15))
        m = np.zeros((h, w, 2), np.uint32)
        if it % 5 == 0:
            m[..., 0] = rng.integers(0, DY_MAX + 1, (h, w))
            m[..., 1] = rng.integers(0, DC_MAX + 1, (h, w))
        else:
            for _ in range(int(rng.integers(0, 6))):
                m[int(rng.integers(0, h)), int(rng.integers(0, w))] = (rng.integers(0, 100000), rng.integers(0, 50000))
        dcb = (m[..., 1] * rng.random((h, w))).astype(np.uint32)
        m[..., 1] |= np.where(rng.integers(0, 2, (h, w)) > 0, KEPT, 0).astype(np.uint32)     # stale KEPT bits
        ty = 0 if rng.integers(0, 3) else int(rng.integers(0, 90000))
        tc = 0 if rng.integers(0, 3) else int(rng.integers(0, 45000))
        check(mksim, m, dcb, ty, tc, int(rng.integers(0, 3)))


def test_noframe(mksim):
    a = np.zeros(1, MASK_DTYPE)
    mksim.mksim_noframe(a.ctypes.data)
    assert record_tuple(a[0]) == record_tuple(record_np(None, None)[0]) and a[0]["status"] == NOFRAME


def test_thresholds_are_exclusive(mksim):
    """D = threshold is unchanged, threshold + 1 changed, for each of the two"""
    m, dcb = blank(6, 4)
    m[1, 2] = (1000, 0)
    m[2, 4] = (1001, 0)
    m[0, 0] = (0, 500)
    m[3, 5] = (0, 501)
    dcb[0, 0], dcb[3, 5] = 200, 501
    r, kept = check(mksim, m, dcb, 1000, 500)
    assert r["n_changed"] == 2 and {(x, y) for y, x in np.argwhere(kept)} == {(4, 2), (5, 3)}
    assert r["sse_drop"] == (1000, 200, 300)
    assert check(mksim, m, dcb, 999, 500)[0]["n_changed"] == 3
    assert check(mksim, m, dcb, 1000, 499)[0]["n_changed"] == 3
    assert check(mksim, m, dcb, 1001, 501)[0]["n_changed"] == 0
    assert check(mksim, m, dcb, 1001, 501)[0]["sse_drop"] == (2001, 701, 300)
    # the largest sums a plane can hold stay below the KEPT bit
    m[1, 1] = (DY_MAX, DC_MAX)
    assert check(mksim, m, dcb, DY_MAX, DC_MAX)[0]["n_changed"] == 0
    assert check(mksim, m, dcb, DY_MAX - 1, DC_MAX)[0]["n_changed"] == 1
    assert check(mksim, m, dcb, DY_MAX, DC_MAX - 1)[0]["n_changed"] == 1


@pytest.mark.parametrize("grow", [0, 1, 2])
def test_grow_at_the_four_edges_and_corners(mksim, grow):
    """one changed MB in each corner and at the middle of each edge of a 7 x 5
    rect: the kept block is the (2 grow + 1)^2 neighbourhood clipped at the rect"""
    w, h = 7, 5
    for x, y in [(0, 0), (6, 0), (0, 4), (6, 4), (3, 0), (3, 4), (0, 2), (6, 2), (3, 2)]:
        for dy, dc in [(9, 0), (0, 9)]:
            m, dcb = blank(w, h, (x, y), dy=dy, dc=dc)
            r, kept = check(mksim, m, dcb, 0, 0, grow)
            want = {(i, j) for j in range(max(y - grow, 0), min(y + grow, h - 1) + 1)
                    for i in range(max(x - grow, 0), min(x + grow, w - 1) + 1)}
            assert {(i, j) for j, i in np.argwhere(kept)} == want
            assert r["n_changed"] == 1 and r["n_kept"] == len(want) and r["sse_drop"] == (0, 0, 0)


def test_none_changed_and_all_changed(mksim):
    rng = np.random.default_rng(2)
    w, h = 9, 6
    m = np.stack([rng.integers(1, 5000, (h, w)), rng.integers(1, 3000, (h, w))], -1).astype(np.uint32)
    dcb = m[..., 1] // 3
    for grow in (0, 1, 2):
        r, kept = check(mksim, m, dcb, 5000, 3000, grow)
        assert r["n_changed"] == 0 and r["n_kept"] == 0 and not kept.any()
        assert r["sse_drop"] == (int(m[..., 0].sum()), int(dcb.sum()), int((m[..., 1] - dcb).sum()))
        r, kept = check(mksim, m, dcb, 0, 0, grow)
        assert r["n_changed"] == r["n_kept"] == w * h and kept.all() and r["sse_drop"] == (0, 0, 0)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (17, 1)])
def test_degenerate_rects(mksim, w, h):
    for grow in (0, 1, 2):
        m, dcb = blank(w, h)
        assert check(mksim, m, dcb, 0, 0, grow)[0]["n_kept"] == 0
        m, dcb = blank(w, h, (w - 1, h - 1))
        r, kept = check(mksim, m, dcb, 0, 0, grow)
        assert r["n_changed"] == 1 and r["n_kept"] == min(grow + 1, w * h)


def test_device_map_against_the_helper(mksim):
    rng = np.random.default_rng(3)
    for w, h in [(1, 1), (5, 5), (17, 2)]:
        n = 384 * w * h
        src, pred = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        m, dcb = np.zeros((h, w, 2), np.uint32), np.zeros((h, w), np.uint32)
        mksim.mksim_map(src.ctypes.data, pred.ctypes.data, w, h, m.ctypes.data, dcb.ctypes.data)
        wm, wcb = mask_map_np(src, pred, w, h)
        assert np.array_equal(m, wm) and np.array_equal(dcb, wcb)
    # the extremes: 0 against 255 everywhere
    src, pred = np.zeros(384, np.uint8), np.full(384, 255, np.uint8)
    m, dcb = np.zeros((1, 1, 2), np.uint32), np.zeros((1, 1), np.uint32)
    mksim.mksim_map(src.ctypes.data, pred.ctypes.data, 1, 1, m.ctypes.data, dcb.ctypes.data)
    assert tuple(m[0, 0]) == (DY_MAX, DC_MAX) and dcb[0, 0] == DC_MAX // 2


def test_sanitized_program(tmp_path):
    """mask_sim.cpp as a program of its own under the host sanitizers: every
    entry point over random maps and rects, the two walks compared"""
    exe = str(tmp_path / "mask_sim")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DMASK_SIM_MAIN", *FLAGS, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "checksum" in p.stdout and not p.stderr.strip(), p.stderr


# ------------------------------------------------- the premise, on the oracle
W, H, RECT = 96, 368, (1, 2, 5, 5)
RW, RH = RECT[2:]
# 0; an odd offset; one that tears the rect's MB row 4 between A and B (a_end = 4, 12 rows of it in A); the frame
# that writes the 496 waypoint, and one predicted through it
OFFS = [0, 7, 300, 496, 500]
BLOCK = [(1, 1), (2, 1), (1, 2), (2, 2)]
# +-1 noise: Dy <= 256 and Dc <= 128 in every MB, so these thresholds name exactly the painted MBs
TY, TC = 256, 128
# the rect's QP: low enough that +-1 noise still codes levels (at QP 26 it quantises to nothing and there
# would be no bits to save)
QP = 10


def parse_rect(nal, rect):
    """(x, y) -> (cbp, luma, cdc, cac) of the rect's MBs of a scroll NAL"""
    got = {}

    def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
        if rect[0] <= x < rect[0] + rect[2] and rect[1] <= y < rect[1] + rect[3]:
            got[(x, y)] = (cbp, luma, cdc, cac)

    hp.parse_p_slice(nal, W, H, on_mb=on_mb)
    assert len(got) == rect[2] * rect[3]
    return got


@pytest.fixture(scope="module")
def premise(oracle):
    R = random_refs(W, H, 51)
    rng = np.random.default_rng(52)
    states = frame_states(oracle, W, H, OFFS)
    preds = [pred_rect(oracle, st, R, RECT, off) for st, off in zip(states, OFFS)]
    srcs = [paint_mbs(noisy(p, rng), BLOCK, RW, RH, rng) for p in preds]
    return R, states, preds, srcs


def test_helper_pred_is_the_decoders(oracle, premise):
    """maskhelp.pred_rect over damagehelp.frame_states is the prediction the
    test decoder forms for the NAL or_compose_dyn writes, and a source equal to
    it decodes to itself"""
    R, states, preds, _ = premise
    assert states[4].nwp > 0 and (H - OFFS[2]) // 16 == 4 and (H - OFFS[2]) % 16
    _, frames = oracle_frames(oracle, W, H, OFFS, RECT, preds, R, qp=QP)
    for f, (rec, pred) in enumerate(frames):
        assert pred == preds[f].tobytes(), (f, OFFS[f])
        assert rec == preds[f].tobytes(), (f, OFFS[f])


@pytest.mark.parametrize("grow", [0, 1])
def test_doctored_source_through_the_oracle(oracle, premise, grow):
    R, states, preds, srcs = premise
    res = [mask_np(s, p, RW, RH, TY, TC, grow) for s, p in zip(srcs, preds)]
    for mk, rec, kept, _ in res:
        assert rec["n_changed"] == len(BLOCK) and rec["n_kept"] == (4 if grow == 0 else 16)
    doctored = [r[3] for r in res]
    doct, frames = oracle_frames(oracle, W, H, OFFS, RECT, doctored, R, qp=QP)
    np_ = scroll_nals(oracle, W, H, OFFS, RECT, srcs, R, qp=QP)
    nd_ = scroll_nals(oracle, W, H, OFFS, RECT, doctored, R, qp=QP)
    assert all(n in doct for n in nd_)
    for f, (a, b) in enumerate(zip(np_, nd_)):
        kept, pred = res[f][2], preds[f]
        ma, mb = parse_rect(a, RECT), parse_rect(b, RECT)
        rec = np.frombuffer(frames[f][0], np.uint8)
        # a dropped MB decodes to exactly its prediction: the doctored source there
        assert np.array_equal(doctor(rec, pred, kept, RW, RH), rec), (f, OFFS[f])
        for (x, y), (cbp, luma, cdc, cac) in mb.items():
            if kept[y - RECT[1], x - RECT[0]]:
                assert (luma, cdc, cac) == ma[(x, y)][1:], (f, x, y)
            else:
                assert cbp == 0, (f, x, y)
        assert any(ma[k][0] != 0 for k in ma if not kept[k[1] - RECT[1], k[0] - RECT[0]]), f   # there was something to save
        assert len(b) < len(a), (f, len(a), len(b))
    assert sum(map(len, nd_)) < sum(map(len, np_))
