"""The rule of the offset detector (h264-scroll-encoder_amd/csrc/
detect_device.h: k_det_surf / k_det_refs / k_det_score / k_det_pick run it on
the device), compiled for the CPU (tests/hostsim/detect_sim.cpp), against the
numpy restatement of tests/detecthelp.py; and the premise of the GPU test's
designed cases: in each of them the helper alone finds the true offset.
Every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from cschelp import VARIANTS
from detecthelp import DETECT_DTYPE, EDGE_H, EDGE_RADII, FOUND, GREY, LOW, NO_SCORE, TIED, detect_np, edge_case, \
    estimates, expect, flat_luma, noise_luma, painted, record_tuple, scroll_surface, sig_rows, sig_surface, stacked, \
    tiled_luma, width_case

SRC = os.path.join(REPO, "tests", "hostsim", "detect_sim.cpp")
FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(REPO, "tests", "hostsim"), "-I", os.path.join(REPO, "include"),
         "-I", os.path.join(PKG, "csrc")]


@pytest.fixture(scope="module")
def dtsim(tmp_path_factory):
    """TEST-ONLY CPU build of detect_device.h; the library lands in pytest's
    temp directory"""
    so = str(tmp_path_factory.mktemp("dtsim") / "libdtsim.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", *FLAGS, SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    lib.dtsim_nuse.argtypes = [u32, u32]
    lib.dtsim_nuse.restype = u32
    lib.dtsim_sig_surface.argtypes = [ctypes.c_int, ctypes.c_int, vp, u32, u32, u32, u32, vp]
    lib.dtsim_sig_refs.argtypes = [ctypes.c_int, ctypes.c_int, vp, u32, vp]
    lib.dtsim_detect.argtypes = [vp, vp, u32, u32, ctypes.c_int32, u32, u32, vp, vp]
    lib.dtsim_walk.argtypes = lib.dtsim_detect.argtypes
    assert lib.dtsim_record_size() == DETECT_DTYPE.itemsize == 32 and lib.dtsim_rule_size() == 16
    return lib


def sim_sigs(lib, img, stack, v=GREY, seg_step=1):
    """(sigS [ph][nuse], sigR [2 ph][nuse]) through the device functions"""
    ph, pw = img.shape[:2]
    nu = lib.dtsim_nuse(pw, seg_step)
    px = np.ascontiguousarray(img).view("<u4").reshape(ph, pw)
    st = np.ascontiguousarray(stack, dtype=np.uint8)
    ss, sr = np.zeros((ph, nu), np.uint16), np.zeros((2 * ph, nu), np.uint16)
    lib.dtsim_sig_surface(pw, ph, px.ctypes.data, v[0], v[1], v[2], seg_step, ss.ctypes.data)
    lib.dtsim_sig_refs(pw, 2 * ph, st.ctypes.data, seg_step, sr.ctypes.data)
    return ss, sr


def sim(lib, ss, sr, est, radius, min_match=1):
    """record and scores through the serial and the kernels' walk (they must agree)"""
    ss, sr = np.ascontiguousarray(ss, dtype=np.uint16), np.ascontiguousarray(sr, dtype=np.uint16)
    ph, nu = ss.shape
    out = []
    for f in (lib.dtsim_detect, lib.dtsim_walk):
        rec, sc = np.zeros(1, DETECT_DTYPE), np.zeros(ph + 1, np.uint32)
        f(ss.ctypes.data, sr.ctypes.data, ph, nu, int(est), radius, min_match, sc.ctypes.data, rec.ctypes.data)
        out.append((rec.tobytes(), sc.tobytes()))
    assert out[0] == out[1], "the serial walk and the tiled / tree walk differ"
    return record_tuple(rec[0]), sc


def check(lib, ss, sr, est, radius, min_match=1):
    want, scores = detect_np(np.asarray(ss, np.int64), np.asarray(sr, np.int64), est, radius, min_match)
    got, sc = sim(lib, ss, sr, est, radius, min_match)
    assert np.array_equal(sc, scores), (est, radius)
    assert got == record_tuple(want), (est, radius, min_match)
    return want


@pytest.mark.parametrize("pw,ph,seg_step", [(96, 48, 1), (96, 48, 2), (272, 48, 1), (272, 48, 2), (272, 48, 3),
                                            (320, 240, 1), (320, 240, 2), (320, 240, 3)])
def test_signatures_and_scores_on_random_and_tiled_pictures(dtsim, pw, ph, seg_step):
    """nseg 2, 4 + a 16-wide one and 5; every variant on the surface side"""
    rng = np.random.default_rng(7 * pw + seg_step)
    for kind, v in zip([noise_luma, tiled_luma] * 4, VARIANTS):
        a, b = kind(pw, ph, rng)
        st = stacked(a, b)
        off = int(rng.integers(0, ph + 1))
        img = scroll_surface(st, off, ph, rng, painted("2x2", pw, ph))
        if v != GREY:                                   # a coloured surface: only the signatures are of interest
            img = rng.integers(0, 256, img.shape, dtype=np.uint8)
        ss, sr = sim_sigs(dtsim, img, st, v, seg_step)
        assert np.array_equal(ss, sig_surface(img, v, seg_step)), v
        assert np.array_equal(sr, sig_rows(st, seg_step))
        r = check(dtsim, ss, sr, off + 3, ph, ph * ss.shape[1] // 4)
        if v == GREY:
            assert r["status"] == FOUND and r["off"] == off and r["n_sig"] == ph * len(range(0, -(-pw // 64), seg_step))


def test_every_status_and_min_match_at_the_score(dtsim):
    rng = np.random.default_rng(3)
    pw, ph = 96, 64
    st = stacked(*noise_luma(pw, ph, rng))
    img = scroll_surface(st, 20, ph, rng, painted("2x2", pw, ph))
    ss, sr = sig_surface(img, GREY), sig_rows(st)
    r = check(dtsim, ss, sr, 18, 8)
    assert r["status"] == FOUND and r["off"] == 20 and r["score"] == (ph - 32) * 2 + 32 and r["second"] < r["score"]
    assert check(dtsim, ss, sr, 18, 8, r["score"])["status"] == FOUND
    assert check(dtsim, ss, sr, 18, 8, r["score"] + 1)["status"] == LOW
    # the truth outside the window: nothing agrees
    low = check(dtsim, ss, sr, 40, 8, ph // 2)
    assert low["status"] == LOW and low["score"] < ph // 2
    # noise against noise
    noise = sig_surface(rng.integers(0, 256, img.shape, dtype=np.uint8), GREY)
    assert check(dtsim, noise, sr, 20, ph, ph)["status"] == LOW
    # a flat page
    fs, fr = np.full((ph, 2), 4928), np.full((2 * ph, 2), 4928)
    t = check(dtsim, fs, fr, 30, 8)
    assert t["status"] == TIED and t["score"] == t["second"] == 2 * ph


def test_ties_go_to_the_nearest_then_the_smaller_offset(dtsim):
    ph = 32
    fs, fr = np.full((ph, 1), 100), np.full((2 * ph, 1), 100)
    # every candidate ties: the centre wins, then the offset one below it
    t = check(dtsim, fs, fr, 10, 5)
    assert (t["off"], t["second_off"], t["status"]) == (10, 9, TIED)
    # the centre at the lower end: the runner-up is the one above
    t = check(dtsim, fs, fr, 0, 5)
    assert (t["off"], t["second_off"], t["lo"], t["hi"]) == (0, 1, 0, 5)
    # a page of period 8: offsets 0, 8, 16, 24 and 32 agree equally.  Two peaks
    # at the same distance from the centre: the smaller offset
    sr = (np.arange(2 * ph) % 8).reshape(-1, 1) + 500
    ss = sr[:ph].copy()
    t = check(dtsim, ss, sr, 12, ph)
    assert (t["off"], t["second_off"], t["score"], t["status"]) == (8, 16, ph, TIED)
    t = check(dtsim, ss, sr, 13, ph)
    assert (t["off"], t["second_off"]) == (16, 8)
    # no peak in the window: every score is 0, which ties by distance (and is LOW for any min_match above 0)
    t = check(dtsim, ss, sr, 12, 3, 0)
    assert (t["lo"], t["hi"], t["score"], t["off"], t["second_off"], t["status"]) == (9, 15, 0, 12, 11, TIED)
    assert check(dtsim, ss, sr, 12, 3, 1)["status"] == LOW


def test_window_clipped_and_radius_extremes(dtsim):
    rng = np.random.default_rng(5)
    pw, ph = 64, 48
    st = stacked(*noise_luma(pw, ph, rng))
    for off in (0, 1, ph - 1, ph):
        ss, sr = sig_surface(scroll_surface(st, off, ph, rng), GREY), sig_rows(st)
        for est in (-7, 0, off, ph, ph + 9):
            for radius in (0, 3, ph, ph + 1, 0xFFFFFFFF):
                r = check(dtsim, ss, sr, est, radius)
                c0 = min(max(est, 0), ph)
                assert r["centre"] == c0 and r["lo"] == max(c0 - min(radius, ph), 0)
                assert r["hi"] == min(c0 + min(radius, ph), ph)
                if radius == 0:
                    assert (r["second"], r["second_off"], r["off"]) == (0, -1, c0)
                    assert r["status"] == (FOUND if c0 == off else LOW)
                if radius >= ph:
                    assert (r["lo"], r["hi"]) == (0, ph) and r["off"] == off and r["status"] == FOUND


def test_scores_outside_the_window_are_marked(dtsim):
    rng = np.random.default_rng(6)
    st = stacked(*noise_luma(64, 32, rng))
    ss, sr = sig_surface(scroll_surface(st, 9, 32, rng), GREY), sig_rows(st)
    _, sc = sim(dtsim, ss, sr, 10, 2)
    assert (sc[:8] == NO_SCORE).all() and (sc[13:] == NO_SCORE).all() and (sc[8:13] != NO_SCORE).all()
    assert sc[9] == 32


def test_more_candidates_than_one_group_and_more_rows_than_one_tile(dtsim):
    """368 rows: three row tiles, 369 candidates in two groups of 256; 20 segments: two segment tiles"""
    rng = np.random.default_rng(8)
    ph = EDGE_H
    sr = rng.integers(0, 40, (2 * ph, 20))              # few levels: many chance agreements
    ss = sr[300:300 + ph].copy()
    ss[100:200] = 9999
    r = check(dtsim, ss, sr, 0, ph)
    assert r["off"] == 300 and r["score"] == (ph - 100) * 20 and r["status"] == FOUND and r["second"] > 0


# ---- the premise of tests/test_gpu_detect.py's designed cases ----

@pytest.mark.parametrize("shared", [False, True])
def test_helper_finds_the_truth_in_the_edge_cases(shared):
    lumas, img, truth = edge_case(shared)
    for radius in EDGE_RADII:
        recs, _ = expect(lumas, img, estimates(truth, radius), radius=radius, min_match=EDGE_H * 2 // 4)
        for s, row in enumerate(recs):
            for f, r in enumerate(row):
                assert r["status"] == FOUND and r["off"] == truth[s, f] and r["score"] > r["second"], (radius, s, f)


@pytest.mark.parametrize("pw,ph", [(272, 48), (320, 240)])
def test_helper_finds_the_truth_in_the_width_cases(pw, ph):
    lumas, img, truth = width_case(pw, ph)
    for seg_step in (1, 2, 3):
        recs, _ = expect(lumas, img, estimates(truth, ph), radius=ph, seg_step=seg_step, min_match=ph)
        assert [[r["off"] for r in row] for row in recs] == truth.tolist()
        assert all(r["status"] == FOUND for row in recs for r in row)


def test_helper_on_flat_pictures_ties_throughout():
    a, b = flat_luma(96, 48)
    rng = np.random.default_rng(9)
    img = scroll_surface(stacked(a, b), 5, 48, rng)
    r, sc = detect_np(sig_surface(img, GREY), sig_rows(stacked(a, b)), 7, 48)
    assert r["status"] == TIED and r["score"] == r["second"] == 96 and (sc == 96).all() and r["off"] == 7


def test_sanitized_program(tmp_path):
    """detect_sim.cpp as a program of its own under the host sanitizers: every
    entry point over random pictures, the two walks compared"""
    exe = str(tmp_path / "detect_sim")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DDETECT_SIM_MAIN", *FLAGS, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "checksum" in p.stdout and not p.stderr.strip(), p.stderr
