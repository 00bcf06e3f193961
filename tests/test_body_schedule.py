"""k_dyn_row's CAVLC phase on the CPU (tests/hostsim/body_sim.cpp around
h264-scroll-encoder_amd/csrc/dyn_device.h): cavlc_body_t (the table form with
its lean level loop) against cavlc_body<CapSink, true> -- the 128 body bits,
the length, TotalCoeff, TrailingOnes and ok, all for equality, over the random
blocks of test_hostsim_dyn and blocks built for the loop's edges (the table's
last level and the first past it, int8's last, sixteen trailing-one-sized
levels, escapes in a row so the 64-bit register spills, bodies of exactly 64,
65 and 128 bits, the suffixLength-1 start).

The balanced chunk schedule this file was to pin as well (body_chunk) was
measured and not taken: the body loop keeps its
pass-major order, which has no function of its own to test."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import PKG, REPO
from test_hostsim_dyn import _random_block


@pytest.fixture(scope="module")
def bodysim(tmp_path_factory):
    """TEST-ONLY CPU build of the CAVLC phase's device functions; the library
    lands in pytest's temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("bodysim") / "libbodysim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", d, "-I", os.path.join(PKG, "csrc"),
                    os.path.join(d, "body_sim.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def bodies(lib, coef, maxc):
    ca = (ctypes.c_int * 16)(*(list(coef) + [0] * (16 - len(coef))))
    out = (ctypes.c_uint32 * 18)()
    rc = lib.bsim_bodies(ca, maxc, out)
    return rc, list(out[:9]), list(out[9:])


def check(lib, coef, maxc):
    """both coders on one block -> the reference's (length, ok)"""
    rc, got, want = bodies(lib, coef, maxc)
    assert rc == 0, coef
    assert got == want, (coef, maxc, got, want)
    return want[4], want[7]


def test_body_t_random_blocks(bodysim):
    rng = random.Random(12)
    n = 0
    for it in range(4000):
        mx = rng.choice([16, 15, 4])
        coef = _random_block(rng, mx)
        if mx == 4 or any(c < -128 or c > 127 for c in coef):
            continue
        check(bodysim, coef, mx)
        n += 1
    assert n > 2000


def designed_blocks():
    out = []
    for v in (47, 48, 127, 46, 49, 128 - 256):
        for s in (1, -1):
            if v == -128 and s == -1:
                continue
            x = s * v
            out.append([x])                                     # the first level: class 7
            out.append([x] + [0] * 14 + [1])                    # after one trailing one
            out.append([x, 0, 3, -2, 1, 1, 1])                  # the last level, suffixLength grown
            out.append([5, x, -9, 0, 0, 2, 0, 1, -1, 1, 1])     # in the middle, four trailing +-1
            out.append([x] * 16)                                # every level
            out.append([3] * 10 + [x])                          # TotalCoeff 11, no trailing one
    out.append([1] * 16)
    out.append([-1] * 16)
    out.append([1, -1] * 8)
    out.append([2] * 16)
    # escapes in a row: the 64-bit register spills in the table loop (|v| <= 47)
    # and in the exact one (past it); over 128 bits: ok is false in both coders
    for v in (16, 31, 40, 47, 48, 100, 127, -128):
        for k in (2, 3, 4, 5, 8, 16):
            out.append([v] * k)
            out.append([-v if v != -128 else v] * k + [1, -1, 1][:max(0, min(3, 16 - k))])
    # TotalCoeff 11 (over 10) with 0, 1, 2 trailing ones: suffixLength starts at 1
    out.append([4, 3, -2, 2, 5, -3, 2, 2, -2, 3, 2])
    out.append([4, 3, -2, 2, 5, -3, 2, 2, -2, 3, 0, 0, 1])
    out.append([4, 3, -2, 2, 5, -3, 2, 2, -2, 0, 0, -1, 0, 1])
    out.append([4, 3, -2, 2, 5, -3, 2, 2, 0, 1, 0, -1, 0, 1])   # three: suffixLength 0
    return out


def test_body_t_designed_blocks(bodysim):
    spilled = over = 0
    for coef in designed_blocks():
        for mx in (16, 15):
            if len(coef) > mx:
                continue
            n, ok = check(bodysim, coef, mx)
            spilled += 64 < n <= 128
            over += not ok
    assert spilled > 10 and over > 10


def test_body_t_exact_lengths(bodysim):
    """bodies of exactly 64, 65 and 128 bits (the register full, its first
    spill, the record full) and one bit past each, found among blocks of
    mid-sized levels"""
    rng = random.Random(5)
    want = {63: 0, 64: 0, 65: 0, 66: 0, 127: 0, 128: 0, 129: 0}
    for it in range(60000):
        if all(v >= 3 for v in want.values()):
            break
        mx = rng.choice([16, 15])
        k = rng.randint(4, mx)
        big = rng.choice([3, 6, 12, 24, 47, 60])
        coef = [rng.randint(-big, big) for _ in range(k)] + [0] * (mx - k)
        n, ok = check(bodysim, coef, mx)
        if n in want:
            want[n] += 1
            assert ok == (n <= 128)
    assert all(v >= 3 for v in want.values()), want
