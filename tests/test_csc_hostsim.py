"""The surface entry's conversion rule (h264-scroll-encoder_amd/csrc/
csc_device.h: k_csc runs it on the device), compiled for the CPU
(tests/hostsim/csc_sim.cpp), against a numpy restatement of its table
(tests/cschelp.py) -- exactly -- and against the real-valued matrices: every
output within 0.506 (0.5 of rounding, 3 * 0.5 / 65536 * 255 ~ 0.006 of
coefficient rounding)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from cschelp import (BGRA, BT601, BT709, RGBA, TABLE, VARIANTS, chroma_np, i420_bytes, luma_np, real_chroma,
                     real_luma, rgb_of)

BOUND = 0.506
SIM_SRC = os.path.join(REPO, "tests", "hostsim", "csc_sim.cpp")
INC = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(PKG, "csrc")]


@pytest.fixture(scope="module")
def cscsim(tmp_path_factory):
    """TEST-ONLY CPU build of csc_device.h; the library lands in pytest's temp
    directory"""
    so = str(tmp_path_factory.mktemp("cscsim") / "libcscsim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", *INC, SIM_SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32, vp, sz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
    lib.cssim_luma.argtypes = [u32, u32, u32, vp, sz, vp]
    lib.cssim_chroma.argtypes = [u32, u32, u32, vp, sz, vp, vp]
    lib.cssim_window.argtypes = [u32, u32, u32, vp, sz, u32, u32, vp]
    lib.cssim_divmod.argtypes = [u32, u32, ctypes.POINTER(u32)]
    lib.cssim_divmod.restype = u32
    lib.cssim_coef.argtypes = [u32, u32, u32, ctypes.POINTER(ctypes.c_int32)]
    return lib


def pixels(rgb, fmt, rng):
    """[n][3] R, G, B -> [n][4] u8 in memory order, alpha random (ignored)"""
    rgb = np.asarray(rgb, np.uint8)
    px = np.empty(rgb.shape[:-1] + (4,), np.uint8)
    px[..., :3] = rgb[..., ::-1] if fmt == BGRA else rgb
    px[..., 3] = rng.integers(0, 256, rgb.shape[:-1])
    return np.ascontiguousarray(px)


def sim_luma(lib, v, px):
    px = np.ascontiguousarray(px.reshape(-1, 4))
    y = np.zeros(len(px), np.uint8)
    lib.cssim_luma(*v, px.ctypes.data, len(px), y.ctypes.data)
    return y


def sim_chroma(lib, v, quads):
    quads = np.ascontiguousarray(quads.reshape(-1, 4, 4))
    cb, cr = np.zeros(len(quads), np.uint8), np.zeros(len(quads), np.uint8)
    lib.cssim_chroma(*v, quads.ctypes.data, len(quads), cb.ctypes.data, cr.ctypes.data)
    return cb, cr


@pytest.fixture(scope="module")
def samples():
    """shared inputs: the 52-step lattice (53 values per channel, 0 and 255
    included) plus 10^6 random pixels, and 10^6 random quads plus constant ones"""
    rng = np.random.default_rng(20261021)
    ax = np.round(np.linspace(0, 255, 53)).astype(np.uint8)
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rgb = np.concatenate([lat, rng.integers(0, 256, (1000000, 3), dtype=np.uint8)])
    quads = np.concatenate([rng.integers(0, 256, (1000000, 4, 3), dtype=np.uint8),
                            np.repeat(lat[:, None, :], 4, axis=1)])
    return rng, rgb, quads


@pytest.mark.parametrize("v", VARIANTS)
def test_luma_exact_and_near_real(cscsim, samples, v):
    rng, rgb, _ = samples
    fmt, m, full = v
    px = pixels(rgb, fmt, rng)
    got = sim_luma(cscsim, v, px)
    r, g, b = rgb_of(px, fmt)
    assert np.array_equal(got, luma_np(r, g, b, m, full))
    err = np.abs(got - real_luma(r.astype(float), g.astype(float), b.astype(float), m, full))
    assert err.max() <= BOUND, err.max()


@pytest.mark.parametrize("v", VARIANTS)
def test_chroma_exact_and_near_real(cscsim, samples, v):
    rng, _, quads = samples
    fmt, m, full = v
    px = pixels(quads, fmt, rng)                   # [n][4][4]
    cb, cr = sim_chroma(cscsim, v, px)
    r, g, b = (c.sum(axis=1) for c in rgb_of(px, fmt))
    wcb, wcr = chroma_np(r, g, b, m, full)
    assert np.array_equal(cb, wcb) and np.array_equal(cr, wcr)
    rcb, rcr = real_chroma(r / 4.0, g / 4.0, b / 4.0, m, full)
    assert np.abs(cb - rcb).max() <= BOUND and np.abs(cr - rcr).max() <= BOUND


@pytest.mark.parametrize("fmt", [RGBA, BGRA])
def test_anchor_colours(cscsim, fmt):
    """white, black and the primaries in BT.601 limited range"""
    rng = np.random.default_rng(1)
    want = {(255, 255, 255): (235, 128, 128), (0, 0, 0): (16, 128, 128), (255, 0, 0): (81, 90, 240),
            (0, 255, 0): (145, 54, 34), (0, 0, 255): (41, 240, 110)}
    for rgb, (y, cb, cr) in want.items():
        px = pixels(np.array([rgb] * 4), fmt, rng)
        v = (fmt, BT601, 0)
        assert sim_luma(cscsim, v, px)[0] == y, rgb
        gcb, gcr = sim_chroma(cscsim, v, px)
        assert (gcb[0], gcr[0]) == (cb, cr), rgb


@pytest.mark.parametrize("v", [x for x in VARIANTS if x[2] == 1])
def test_full_range_clamp(cscsim, v):
    """full-range pure blue / red reach 256 before the clamp"""
    rng = np.random.default_rng(2)
    fmt, m, _ = v
    for rgb, which in (((0, 0, 255), 0), ((255, 0, 0), 1)):
        k = TABLE[(m, 1)][1 + which]
        assert (k[0] * 4 * rgb[0] + k[2] * 4 * rgb[2] + (128 << 18) + (1 << 17)) >> 18 == 256
        px = pixels(np.array([rgb] * 4), fmt, rng)
        assert sim_chroma(cscsim, v, px)[which][0] == 255
    grey = pixels(np.array([[77, 77, 77]] * 4), fmt, rng)
    assert [int(c[0]) for c in sim_chroma(cscsim, v, grey)] == [128, 128]


@pytest.mark.parametrize("v", VARIANTS)
def test_header_coefficients(cscsim, v):
    """what csc_device.h's coef() hands the kernel, by byte position: the
    table's values (R and B swapped for BGRA), luma rows summing to 56284 /
    65536, chroma rows to 0, yoff = (16 << 16 limited) + 32768"""
    fmt, m, full = v
    k = (ctypes.c_int32 * 10)()
    cscsim.cssim_coef(fmt, m, full, k)
    k = list(k)
    assert sum(k[0:3]) == (65536 if full else round(65536 * 219 / 255))
    assert k[3] == (0 if full else 16 << 16) + 32768
    assert sum(k[4:7]) == 0 and sum(k[7:10]) == 0
    y, cb, cr = TABLE[(m, full)]
    order = (lambda c: tuple(c[::-1])) if fmt == BGRA else tuple
    assert (tuple(k[0:3]), k[3], tuple(k[4:7]), tuple(k[7:10])) == (order(y[:3]), y[3], order(cb), order(cr))


@pytest.mark.parametrize("v", VARIANTS)
def test_window_by_task_index(cscsim, v):
    """a pitched window walked patch by patch as the kernel walks it (widths
    that are no power of two go through divmod's correction)"""
    rng = np.random.default_rng(3)
    for w, h, pad in ((16, 16, 0), (80, 32, 48), (48, 48, 16)):
        pitch = 4 * w + pad
        src = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
        out = np.zeros(w * h * 3 // 2, np.uint8)
        cscsim.cssim_window(*v, src.ctypes.data, pitch, w, h, out.ctypes.data)
        img = src[:, :4 * w].reshape(h, w, 4)
        assert out.tobytes() == i420_bytes(img, *v)


def test_divmod(cscsim):
    rng = np.random.default_rng(4)
    r = ctypes.c_uint32()
    cases = [(0, 1), (0xFFFFFFFF, 1), (0xFFFFFFFF, 2), (0xFFFFFFFF, 0xFFFFFFFF), (40959999, 10000), (9999, 50)]
    cases += [(int(n), int(d)) for n, d in zip(rng.integers(0, 1 << 32, 20000), rng.integers(1, 1 << 16, 20000))]
    cases += [(int(n), int(d)) for n, d in zip(rng.integers(0, 1 << 32, 20000), rng.integers(1, 1 << 32, 20000))]
    for n, d in cases:
        assert (cscsim.cssim_divmod(n, d, ctypes.byref(r)), r.value) == divmod(n, d), (n, d)


def test_sim_under_host_sanitizers(tmp_path):
    """csc_sim.cpp as a program of its own under ASan + UBSan, on the CPU"""
    exe = str(tmp_path / "csc_sim")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DCSC_SIM_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", *INC, SIM_SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "csc_sim: checksum" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
