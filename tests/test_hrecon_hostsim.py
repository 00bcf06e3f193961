"""The prediction fetch of the reconstruction under UI hints
(h264-scroll-encoder_amd/csrc/hrecon_device.h), compiled for the CPU
(tests/hostsim/hrecon_sim.cpp): (a) against the oracle's or_ref_sample
sampling (tests/hreconhelp.py pred2d), (b) with recon_device.h from pixels to
the reconstruction and SSE against what the test decoder makes of
or_hint_dyn_scroll_nal's NAL.  Every comparison is exact."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from dynhelp import OrCfg, Rect, hint_array, qp_field, random_hints
from hreconhelp import EXACT, PSKIP, SPEC, decode_rect_hinted, make_cfg, pred2d
from reconhelp import random_refs, sse3, striped_refs


@pytest.fixture(scope="module")
def hreconsim(tmp_path_factory):
    """TEST-ONLY CPU build of hrecon_device.h (flags and include paths of the
    hostsim fixture); the library lands in pytest's temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("hreconsim") / "libhreconsim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", d,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(d, "hrecon_sim.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def _refbuf(R):
    data = R.i420(0) + R.i420(1)
    return (ctypes.c_uint8 * len(data)).from_buffer_copy(data)


def _wp(cfg):
    return (ctypes.c_int32 * 8)(*cfg.wp_off), (ctypes.c_int32 * 8)(*cfg.wp_valid)


def _check_mb(sim, lib, cfg, R, rb, ref, mvx, mvy, mbx, mby):
    """hsim_pred_mb == pred2d; returns the GEN flag"""
    wo, wv = _wp(cfg)
    py, pu, pv = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    gen = sim.hsim_pred_mb(rb, cfg.w, cfg.h, wo, wv, ref, mvx, mvy, mbx, mby, py, pu, pv)
    ey, eu, ev = pred2d(lib, cfg, R, ref, mvx, mvy, mbx, mby)
    what = (ref, mvx, mvy, mbx, mby)
    assert list(py) == [v for r in ey for v in r], ("luma",) + what
    assert list(pu) == [v for r in eu for v in r], ("Cb",) + what
    assert list(pv) == [v for r in ev for v in r], ("Cr",) + what
    return gen


W, H = 256, 720


@pytest.fixture(scope="module", params=["striped", "random"])
def refs(request, oracle):
    R = striped_refs(oracle, W, H) if request.param == "striped" else random_refs(W, H, 7)
    return R, _refbuf(R)


def test_pred_random_motion(hreconsim, oracle, refs):
    """random (ref, mvx, mvy) on A / B, each parity of both components"""
    R, rb = refs
    cfg = make_cfg(oracle, W, H)
    rng = random.Random(1)
    seen = set()
    for _ in range(40):
        mvx, mvy = rng.randint(-90, 90), rng.randint(-300, 300)
        seen.add((mvx & 1, mvy & 1))
        gen = _check_mb(hreconsim, oracle, cfg, R, rb, rng.randint(0, 1), mvx, mvy,
                        rng.randint(0, W // 16 - 1), rng.randint(0, H // 16 - 1))
        assert gen == 0
    assert len(seen) == 4


def test_pred_leaves_the_picture(hreconsim, oracle, refs):
    """motions that leave the picture on each side and at each corner, from
    the MBs there and from far inside; partly outside columns at every byte
    alignment"""
    R, rb = refs
    cfg = make_cfg(oracle, W, H)
    mbw, mbh = W // 16, H // 16
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx == 0 and sy == 0:
                continue
            mbx = 0 if sx < 0 else (mbw - 1 if sx > 0 else 5)
            mby = 0 if sy < 0 else (mbh - 1 if sy > 0 else 20)
            for mvx, mvy in ((sx * 21, sy * 37), (sx * 8, sy * 8), (sx * 300, sy * 1000), (sx * 5, sy * 2)):
                _check_mb(hreconsim, oracle, cfg, R, rb, (sx + sy) & 1, mvx, mvy, mbx, mby)
            _check_mb(hreconsim, oracle, cfg, R, rb, 0, sx * 8000, sy * 8000, 7, 22)
    for d in range(-20, 4):                                # sliding over the left and the right edge
        _check_mb(hreconsim, oracle, cfg, R, rb, 1, d, 3, 0, 3)
        _check_mb(hreconsim, oracle, cfg, R, rb, 0, -d, -3, mbw - 1, 3)


@pytest.mark.parametrize("waypoints,want_gen", [([(496, 2, 1)], False), ([(496, 2, 1), (500, 3, 1)], False),
                                                ([(501, 2, 1)], True), ([(496, 2, 1), (501, 3, 1)], True)])
def test_pred_waypoint_references(hreconsim, oracle, refs, waypoints, want_gen):
    """waypoint references: a full-pel chain (offsets 496, 496 -> 500) stays
    on the row path; an odd waypoint step (501: half-pel chroma) takes
    chroma_px_any"""
    R, rb = refs
    cfg = make_cfg(oracle, W, H, waypoints)
    rng = random.Random(len(waypoints) * 10 + want_gen)
    gens = 0
    for it in range(30):
        ref = 2 + rng.randrange(len(waypoints))
        mvx, mvy = rng.randint(-40, 40), rng.randint(-400, 400)
        mbx, mby = rng.randint(0, W // 16 - 1), rng.randint(0, H // 16 - 1)
        if it < 4:                                         # and off the picture's corners
            mbx, mby = (0, W // 16 - 1)[it & 1], (0, H // 16 - 1)[it >> 1]
            mvx, mvy = (-9, 9)[it & 1], (-11, 11)[it >> 1]
        gens += _check_mb(hreconsim, oracle, cfg, R, rb, ref, mvx, mvy, mbx, mby)
    assert (gens > 0) == want_gen


@pytest.mark.parametrize("mode", [EXACT, PSKIP, SPEC])
@pytest.mark.parametrize("qp", [0, 12, 22, 26, 39, 51])
def test_pixels_to_recon_vs_decoder(hreconsim, oracle, qp, mode):
    """source pixels and the decoded motion through hsim_recon_rect (the
    fetch, then recon_luma4x4 / recon_chroma8x8) equal what the test decoder
    makes of or_hint_dyn_scroll_nal's NAL; the SSE equals numpy's"""
    w, h, rw, rh = 96, 96, 3, 2
    lib = oracle
    R = random_refs(w, h, 100 + qp)
    rb = _refbuf(R)
    rng = random.Random(qp * 3 + mode)
    cfg = make_cfg(lib, w, h)
    buf = (ctypes.c_uint8 * (1 << 20))()
    err = ctypes.c_int()
    for t in range(2):
        off = rng.randint(0, h)
        rects = random_hints(rng, w // 16, h // 16, [0, 1], nmax=4) + [(1, 1, 4, 3, t, (5, -16)[t], (-7, 40)[t])]
        rc = Rect(rng.randint(0, w // 16 - rw), rng.randint(0, h // 16 - rh), rw, rh, qp_field(qp))
        src = np.random.default_rng(qp * 7 + t).integers(0, 256, 384 * rw * rh, dtype=np.uint8)
        if t:                                               # a mild residual: zero blocks and skips too
            src = np.clip(src.astype(np.int32) // 8 + 100, 0, 255).astype(np.uint8)
        arr, n = hint_array(rects)
        c2 = OrCfg.from_buffer_copy(cfg)
        k = lib.or_hint_dyn_scroll_nal(buf, len(buf), ctypes.byref(c2), off, arr, n, mode, ctypes.byref(rc),
                                       src.ctypes.data_as(ctypes.c_void_p), ctypes.byref(R.refs), ctypes.byref(err))
        assert err.value == 0 and k > 0
        d = decode_rect_hinted(lib, cfg, R, rc, bytes(buf[:k]), w, h, mode)
        assert d["qps"] <= {qp}
        nb = 384 * rw * rh
        out, sse = (ctypes.c_uint8 * nb)(), (ctypes.c_uint64 * 3)()
        wo, wv = _wp(cfg)
        motion = (ctypes.c_int32 * (3 * rw * rh))(*[v for m in d["motion"] for v in m])
        hreconsim.hsim_recon_rect(rb, w, h, wo, wv, motion, rc.x0, rc.y0, rw, rh,
                                  (ctypes.c_uint8 * nb).from_buffer_copy(src.tobytes()), qp, out, sse)
        assert bytes(out) == d["rec"], (qp, mode, t)
        assert tuple(int(v) for v in sse) == sse3(src, d["rec"], (rc.x0, rc.y0, rw, rh)), (qp, mode, t)
