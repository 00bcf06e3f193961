"""The rule of the dynamic rect's locate (h264-scroll-encoder_amd/csrc/
damage_device.h: k_dmg_rows / k_dyn_damage / k_dyn_place run it on the
device), compiled for the CPU (tests/hostsim/damage_sim.cpp), against the numpy
restatement of tests/damagehelp.py; and the restatement's premise -- its
Ypred is the luma a decoder shows -- against the test decoder.  Every
comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from cschelp import VARIANTS
from damagehelp import DAMAGE_DTYPE, FIT, NOFRAME, NONE, OVER, damage_map_np, frame_states, locate_np, record_tuple, \
    ypred, ypred_frames
from reconhelp import oracle_frames, random_refs

SRC = os.path.join(REPO, "tests", "hostsim", "damage_sim.cpp")
FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(REPO, "tests", "hostsim"), "-I", os.path.join(REPO, "include"),
         "-I", os.path.join(PKG, "csrc")]


@pytest.fixture(scope="module")
def dmsim(tmp_path_factory):
    """TEST-ONLY CPU build of damage_device.h; the library lands in pytest's
    temp directory"""
    so = str(tmp_path_factory.mktemp("dmsim") / "libdmsim.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", *FLAGS, SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32 = ctypes.c_uint32
    lib.dmsim_locate.argtypes = [ctypes.c_void_p] + [u32] * 6 + [ctypes.c_void_p]
    lib.dmsim_parts.argtypes = lib.dmsim_locate.argtypes
    lib.dmsim_parts.restype = u32
    lib.dmsim_noframe.argtypes = [ctypes.c_void_p, ctypes.POINTER(u32)]
    lib.dmsim_ypred.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    lib.dmsim_map.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, u32, u32, u32,
                              ctypes.c_void_p]
    assert lib.dmsim_record_size() == DAMAGE_DTYPE.itemsize == 40
    return lib


def sim(lib, dmap, w, h, mb_sse=0, margin=0):
    """the record through both walks (they must agree) and the position entry"""
    m = np.ascontiguousarray(dmap, dtype=np.uint32)
    mbh, mbw = m.shape
    a, b = np.zeros(1, DAMAGE_DTYPE), np.zeros(1, DAMAGE_DTYPE)
    lib.dmsim_locate(m.ctypes.data, w, h, mbw, mbh, mb_sse, margin, a.ctypes.data)
    e = lib.dmsim_parts(m.ctypes.data, w, h, mbw, mbh, mb_sse, margin, b.ctypes.data)
    assert a.tobytes() == b.tobytes()
    want_e = 0xFFFFFFFF if a[0]["x0"] < 0 else int(a[0]["x0"]) | int(a[0]["y0"]) << 16
    assert e == want_e
    return record_tuple(a[0])


def check(lib, dmap, w, h, mb_sse=0, margin=0):
    want = locate_np(dmap, w, h, mb_sse, margin)
    assert sim(lib, dmap, w, h, mb_sse, margin) == record_tuple(want), (w, h, mb_sse, margin)
    return want


def blank(mbw, mbh, *mbs, v=9):
    m = np.zeros((mbh, mbw), np.uint32)
    for x, y in mbs:
        m[y, x] = v
    return m


def test_random_maps(dmsim):
    rng = np.random.default_rng(1)
    seen = set()
    for it in range(600):
        mbw, mbh = int(rng.integers(1, 41)), int(rng.integers(1, 31))
        w, h = int(rng.integers(1, mbw + 1)), int(rng.integers(1, mbh + 1))
        m = np.zeros((mbh, mbw), np.uint32)
        if it % 7 == 0:
            m[:] = rng.integers(0, 16646401, m.shape)        # up to 256 * 255^2
        else:
            k = int(rng.integers(0, 6))
            y0, x0 = int(rng.integers(0, mbh)), int(rng.integers(0, mbw))
            for _ in range(k):                               # a cluster: FIT and OVER both occur
                y = min(mbh - 1, y0 + int(rng.integers(0, h + 2)))
                x = min(mbw - 1, x0 + int(rng.integers(0, w + 2)))
                m[y, x] = rng.integers(0, 100000)
        mb_sse = 0 if rng.integers(0, 3) else int(rng.integers(0, 50000))
        seen.add(check(dmsim, m, w, h, mb_sse, int(rng.integers(0, 5)))["status"])
    assert seen == {NONE, FIT, OVER}


def test_noframe(dmsim):
    a, e = np.zeros(1, DAMAGE_DTYPE), ctypes.c_uint32()
    dmsim.dmsim_noframe(a.ctypes.data, ctypes.byref(e))
    assert record_tuple(a[0]) == record_tuple(locate_np(None, 2, 2)) and a[0]["status"] == NOFRAME
    assert e.value == 0xFFFFFFFF


@pytest.mark.parametrize("margin", [0, 1, 2, 3, 4])
def test_margin_at_the_four_edges(dmsim, margin):
    """one damaged MB in each corner and at the middle of each edge of a 12 x 9
    picture, a 9 x 9 rect: the grown box is clipped at the picture, and the
    rect is pushed back inside it"""
    mbw, mbh = 12, 9
    for x, y in [(0, 0), (11, 0), (0, 8), (11, 8), (5, 0), (5, 8), (0, 4), (11, 4), (5, 4)]:
        r = check(dmsim, blank(mbw, mbh, (x, y)), 9, 9, 0, margin)
        assert (r["bx0"], r["by0"], r["bx1"], r["by1"]) == (max(x - margin, 0), max(y - margin, 0),
                                                            min(x + 1 + margin, mbw), min(y + 1 + margin, mbh))
        assert r["status"] == FIT and r["x0"] == min(r["bx0"], mbw - 9) and r["y0"] == 0
        assert r["sse_out"] == 0


def test_boxes_at_and_over_the_rect_size(dmsim):
    mbw, mbh, w, h = 20, 15, 4, 3
    for x0, y0 in [(0, 0), (7, 5), (16, 12)]:
        fit = check(dmsim, blank(mbw, mbh, (x0, y0), (x0 + w - 1, y0 + h - 1)), w, h)
        assert fit["status"] == FIT and (fit["x0"], fit["y0"]) == (x0, y0) and fit["sse_out"] == 0
    for dx, dy in [(1, 0), (0, 1)]:
        over = check(dmsim, blank(mbw, mbh, (7, 5), (7 + w - 1 + dx, 5 + h - 1 + dy)), w, h)
        assert over["status"] == OVER and (over["x0"], over["y0"]) == (7, 5)
        assert over["sse_out"] == 9 and over["sse_all"] == 18   # the far MB is what the rect cannot cover
    # the margin alone makes a fitting box too large
    assert check(dmsim, blank(mbw, mbh, (7, 5), (9, 6)), w, h, 0, 0)["status"] == FIT
    assert check(dmsim, blank(mbw, mbh, (7, 5), (9, 6)), w, h, 0, 1)["status"] == OVER
    # two MBs far apart; the whole picture
    assert check(dmsim, blank(mbw, mbh, (0, 0), (19, 14)), w, h)["status"] == OVER
    full = check(dmsim, np.full((mbh, mbw), 3, np.uint32), w, h)
    assert full["status"] == OVER and full["n_mb"] == mbw * mbh and full["sse_out"] == 3 * (mbw * mbh - w * h)


def test_threshold_is_exclusive(dmsim):
    m = blank(8, 6, (3, 2), v=1000)
    m[4, 6] = 1001
    r = check(dmsim, m, 2, 2, mb_sse=1000)
    assert r["n_mb"] == 1 and (r["x0"], r["y0"]) == (6, 4) and r["sse_out"] == 1000 and r["max_sse"] == 1001
    assert check(dmsim, m, 2, 2, mb_sse=999)["n_mb"] == 2
    assert check(dmsim, m, 2, 2, mb_sse=1001)["status"] == NONE
    assert check(dmsim, m, 2, 2, mb_sse=1001)["sse_out"] == 2001


def test_rect_as_large_as_the_picture(dmsim):
    rng = np.random.default_rng(2)
    for mbw, mbh in [(6, 23), (1, 1), (17, 3)]:
        m = rng.integers(0, 5000, (mbh, mbw)).astype(np.uint32)
        for margin in (0, 4):
            r = check(dmsim, m, mbw, mbh, 10, margin)
            assert r["status"] == FIT and (r["x0"], r["y0"]) == (0, 0) and r["sse_out"] == 0


def test_sanitized_program(tmp_path):
    """damage_sim.cpp as a program of its own under the host sanitizers: every
    entry point over random maps and pictures, the two walks compared"""
    exe = str(tmp_path / "damage_sim")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DDAMAGE_SIM_MAIN", *FLAGS, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "checksum" in p.stdout and not p.stderr.strip(), p.stderr


W, H = 32, 368
OFFS = [0, 7, 300, 367, 368, 490, 496, 500, 503]


@pytest.fixture(scope="module")
def premise(oracle):
    R = random_refs(W, H, 31)
    states = frame_states(oracle, W, H, OFFS)
    return R, states, [ypred(oracle, st, R, off) for st, off in zip(states, OFFS)]


def test_helper_ypred_is_what_a_decoder_shows(oracle, premise):
    """offsets through the 496 waypoint, odd ones and ones that are no
    multiple of 16 (the MB row torn between A and B): a whole-picture rect
    coded from a source whose luma is the helper's Ypred decodes to exactly
    that luma (a wrong prediction would leave a residual that QP 26 does not
    carry losslessly), and the decoder's own prediction agrees"""
    R, states, yps = premise
    assert any(s.nwp > 0 for s in states) and all(s is not None for s in states)
    rect = (0, 0, W // 16, H // 16)
    rng = np.random.default_rng(32)
    srcs = [np.concatenate([yp.reshape(-1), rng.integers(0, 256, W * H // 2, dtype=np.uint8)]) for yp in yps]
    _, frames = oracle_frames(oracle, W, H, OFFS, rect, srcs, R)
    for f, (rec, pred) in enumerate(frames):
        assert rec[:W * H] == yps[f].tobytes(), (f, OFFS[f])
        assert pred[:W * H] == yps[f].tobytes(), (f, OFFS[f])


def test_device_rows_against_the_helper(dmsim, oracle, premise):
    """pred_row (regions + luma_row, what k_dmg_rows runs) picks the rows the
    helper samples through or_ref_sample: random references, every row distinct"""
    R, states, yps = premise
    a, b = R.planes[0][0], R.planes[1][0]
    for st, off, yp in zip(states, OFFS, yps):
        wo = np.array(list(st.wp_off), np.int32)
        wv = np.array(list(st.wp_valid), np.int32)
        out = np.zeros((H, W), np.uint8)
        dmsim.dmsim_ypred(W, H, off, st.nwp, wo.ctypes.data, wv.ctypes.data, a.ctypes.data, b.ctypes.data,
                          out.ctypes.data)
        assert np.array_equal(out, yp), off


def test_experiment_mode_names_its_waypoint_frame(oracle):
    R = random_refs(W, H, 33)
    yps = ypred_frames(oracle, W, H, [490, 496, 500], R, mode=1)
    assert [y is None for y in yps] == [False, True, False]
    assert ypred_frames(oracle, W, H, [490, 496, 500], R, mode=0)[1] is not None


def test_device_map_against_the_helper(dmsim):
    rng = np.random.default_rng(34)
    w, h = 48, 32
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yp = rng.integers(0, 256, (h, w), dtype=np.uint8)
    px = np.ascontiguousarray(img).view("<u4").reshape(h, w)
    for fmt, m, full in VARIANTS:
        out = np.zeros((h // 16, w // 16), np.uint32)
        dmsim.dmsim_map(w, h, px.ctypes.data, yp.ctypes.data, fmt, m, full, out.ctypes.data)
        assert np.array_equal(out, damage_map_np(img, yp, fmt, m, full)), (fmt, m, full)
