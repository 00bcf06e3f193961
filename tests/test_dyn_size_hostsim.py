"""The host and rule code of the dynamic rect sized per frame
(h264-scroll-encoder_amd/csrc/dyn_pos.h: the position table's word, the row
groups of a placement with h_f, the maxima the row stage is sized by;
damage_device.h: place with size), compiled for the CPU
(tests/hostsim/size_sim.cpp), against numpy / brute force and the numpy rule
of tests/dynsizehelp.py.  Every comparison is exact.

k_dyn_row's LDS rests on no monotonicity of the launch's LDS functions, so
there is no sweep of them here: its arrays are prefixes of the launch's (each
a linear function of the width, carved with w_f <= w), and the bit window is
wherever the launch put it (the kernel reads the batch's width for it)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from damagehelp import DAMAGE_DTYPE, locate_np, record_tuple
from dynsizehelp import locate_sized_np, table_word

SRC = os.path.join(REPO, "tests", "hostsim", "size_sim.cpp")
FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(REPO, "tests", "hostsim"), "-I", os.path.join(REPO, "include"),
         "-I", os.path.join(PKG, "csrc")]


@pytest.fixture(scope="module")
def szsim(tmp_path_factory):
    """TEST-ONLY CPU build; the library lands in pytest's temp directory"""
    so = str(tmp_path_factory.mktemp("szsim") / "libszsim.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", *FLAGS, SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    lib.szsim_pack.argtypes = [u32] * 4
    lib.szsim_pack.restype = u32
    lib.szsim_unpack.argtypes = [u32, u32, ctypes.c_void_p]
    lib.szsim_sized_max.argtypes = [ctypes.c_int, ctypes.c_int, u64, u64, ctypes.c_void_p]
    lib.szsim_place.argtypes = [ctypes.c_void_p] + [u32] * 7 + [ctypes.c_void_p]
    lib.szsim_place.restype = u32
    return lib


def unpack(lib, e, mask):
    out = np.zeros(4, np.int32)
    lib.szsim_unpack(e, mask, out.ctypes.data)
    return tuple(int(v) for v in out)


def test_table_word(szsim):
    # an all-zero size field is the word every table held before: x0 | y0 << 16
    for x0, y0 in [(0, 0), (255, 255), (3, 20), (79, 44)]:
        assert szsim.szsim_pack(x0, y0, 0, 0) == x0 | y0 << 16
        assert unpack(szsim, x0 | y0 << 16, 0xff) == (x0, y0, 0, 0)
    # every size of the largest rect beside every origin byte
    rng = np.random.default_rng(1)
    for _ in range(2000):
        x0, y0, dw, dh = (int(v) for v in rng.integers(0, 256, 4))
        e = szsim.szsim_pack(x0, y0, dw, dh)
        assert e == table_word(x0, y0, 256, 256, 256 - dw, 256 - dh)
        assert unpack(szsim, e, 0xff) == (x0, y0, dw, dh)
    # a legal entry is never the "no rect" word: x0 = 255 leaves no room for a rect 255 columns short of 256
    assert szsim.szsim_pack(255, 255, 255, 255) == 0xFFFFFFFF
    # pictures wider than 256 MBs: origins take 16 bits, no sizes
    assert unpack(szsim, 300 | 400 << 16, 0xffff) == (300, 400, 0, 0)


def groups_np(y0, h, mbh, sr):
    na, nb = -(-y0 // sr), -(-(mbh - y0 - h) // sr)
    return max(na, 1) + h + max(nb, 1)


@pytest.mark.parametrize("mbh", [23, 45])
def test_groups_and_region_maxima_against_brute_force(szsim, mbh):
    sr = szsim.szsim_static_rows()
    for h in range(1, mbh + 1):
        for hf in range(1, h + 1):
            for y0 in range(0, mbh - h + 1):
                assert szsim.szsim_groups_at(y0, hf, mbh) == groups_np(y0, hf, mbh, sr), (y0, hf)
        for sw, rw in [(128, 640), (4096, 64), (64, 64)]:
            best = [0, 0, 0]
            for hf in range(1, h + 1):
                for y0 in range(0, mbh - h + 1):
                    n = groups_np(y0, hf, mbh, sr)
                    best = [max(best[0], n), max(best[1], n - hf), max(best[2], (n - hf) * sw + hf * rw)]
            out = np.zeros(3, np.uint64)
            szsim.szsim_sized_max(h, mbh, sw, rw, out.ctypes.data)
            assert [int(v) for v in out] == best, (h, sw, rw)
            # never below what the unsized moving rect is sized by
            assert best[0] >= szsim.szsim_groups_max(h, mbh)


def test_largest_region_is_not_always_the_full_height(szsim):
    """static groups dearer than rect rows: a one-row rect with three static
    groups around it outweighs the full-height rect with two"""
    out = np.zeros(3, np.uint64)
    szsim.szsim_sized_max(23, 23, 4096, 64, out.ctypes.data)
    assert int(out[2]) > 2 * 4096 + 23 * 64
    assert int(out[0]) == 25 and int(out[1]) == 3


def sim(lib, dmap, w, h, mb_sse, margin, size):
    m = np.ascontiguousarray(dmap, dtype=np.uint32)
    mbh, mbw = m.shape
    a = np.zeros(1, DAMAGE_DTYPE)
    e = lib.szsim_place(m.ctypes.data, w, h, mbw, mbh, mb_sse, margin, size, a.ctypes.data)
    assert e != 0xDEAD0000
    return record_tuple(a[0]), e


def test_place_with_size_against_the_numpy_rule(szsim):
    rng = np.random.default_rng(2)
    seen = set()
    for it in range(400):
        mbw, mbh = int(rng.integers(1, 20)), int(rng.integers(1, 30))
        w, h = int(rng.integers(1, mbw + 1)), int(rng.integers(1, mbh + 1))
        m = np.zeros((mbh, mbw), np.uint32)
        for _ in range(int(rng.integers(0, 5))):
            m[rng.integers(0, mbh), rng.integers(0, mbw)] = rng.integers(1, 100000)
        mb_sse, margin = int(rng.integers(0, 2)) * 500, int(rng.integers(0, 5))
        # size = 0: the existing records and entries, byte for byte
        base = locate_np(m, w, h, mb_sse, margin)
        rec0, e0 = sim(szsim, m, w, h, mb_sse, margin, 0)
        assert rec0 == record_tuple(base)
        assert e0 == (0xFFFFFFFF if base["x0"] < 0 else base["x0"] | base["y0"] << 16)
        want, rect = locate_sized_np(m, w, h, mb_sse, margin)
        rec1, e1 = sim(szsim, m, w, h, mb_sse, margin, 1)
        assert rec1 == record_tuple(want), (it, rect)
        assert e1 == (0xFFFFFFFF if rect is None else table_word(rect[0], rect[1], w, h, rect[2], rect[3]))
        seen.add(int(want["status"]))
    assert seen >= {0, 1, 2}


def test_sanitized_program(tmp_path):
    """size_sim.cpp as a program of its own under the host sanitizers"""
    exe = str(tmp_path / "size_sim")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSIZE_SIM_MAIN", *FLAGS, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "checksum" in p.stdout and not p.stderr.strip(), p.stderr
