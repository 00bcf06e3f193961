"""The QP probe's device functions (h264-scroll-encoder_amd/csrc/
probe_device.h: a block's CAVLC body length from levels by value, coeff_token
length by nC, the MB-level sum), compiled for the CPU
(tests/hostsim/probe_sim.cpp), against the oracle's coder (or_cavlc_block,
or_dyn_mb_levels_bits, or_compose_dyn's traced MBs).  Every comparison is
exact."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from dynhelp import Rect, rect_source
from probehelp import constant_of, mb_levels_bits, oracle_probe
from reconhelp import random_refs

QPS = [0, 12, 22, 26, 39, 51]


class OrBits(ctypes.Structure):
    _fields_ = [("buf", ctypes.c_void_p), ("cap", ctypes.c_size_t), ("nbits", ctypes.c_size_t)]


@pytest.fixture(scope="module")
def probesim(tmp_path_factory):
    """TEST-ONLY CPU build of probe_device.h (flags and include paths of the
    hostsim fixture); the library lands in pytest's temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("probesim") / "libprobesim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", d,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(d, "probe_sim.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def _mag(rng, kind):
    s = rng.choice((-1, 1))
    if kind == 0:
        return s
    if kind == 1:
        return s * rng.randint(2, 9)          # suffixLength 0 codes 14..29: the prefix-14 escape
    if kind == 2:
        return s * rng.randint(8, 60)
    if kind == 3:
        return s * rng.randint(60, 400)
    if kind == 4:
        return s * rng.randint(400, 2062)     # prefix 15 at every suffixLength
    return s * 2063


def blocks(maxc, seed):
    """empty, sparse, dense, +-1 runs, every escape up to +-2063, and
    TotalCoeff > 10 with fewer than three trailing ones"""
    rng = random.Random(seed)
    yield [0] * maxc
    for v in (1, -1, 2, -2, 8, -8, 15, 16, -16, 17, 2063, -2063):
        for pos in (0, maxc - 1):
            c = [0] * maxc
            c[pos] = v
            yield c
    for n in range(1, maxc + 1):              # +-1 runs of every length, at both ends
        yield [rng.choice((-1, 1)) for _ in range(n)] + [0] * (maxc - n)
        yield [0] * (maxc - n) + [rng.choice((-1, 1)) for _ in range(n)]
    if maxc > 10:                             # the suffixLength-1 start
        for t1 in range(3):
            for tc in range(11, maxc + 1):
                c = [0] * maxc
                pos = sorted(rng.sample(range(maxc), tc))
                for j, p in enumerate(pos):
                    c[p] = rng.choice((-1, 1)) if j >= tc - t1 else _mag(rng, rng.randint(1, 5))
                yield c
    for _ in range(1500):
        c = [0] * maxc
        for p in rng.sample(range(maxc), rng.randint(1, maxc)):
            c[p] = _mag(rng, rng.choice((0, 0, 0, 1, 1, 2, 3, 4, 5)))
        yield c


@pytest.mark.parametrize("maxc", [16, 15, 4])
def test_block_bits(probesim, oracle, maxc):
    """token + body length equals or_cavlc_block's bit count at every nC
    class, TotalCoeff and TrailingOnes agree"""
    ob = (ctypes.c_uint8 * 1024)()
    seen_sl1 = seen_esc = 0
    for coef in blocks(maxc, 7 + maxc):
        nz = [v for v in coef if v]
        t1 = 0
        for v in reversed(nz):
            if t1 == 3 or v not in (1, -1):
                break
            t1 += 1
        seen_sl1 += len(nz) > 10 and t1 < 3
        seen_esc += any(abs(v) > 2000 for v in coef)
        arr = (ctypes.c_int * 16)(*coef, *([0] * (16 - maxc)))
        for nC in ([-1] if maxc == 4 else [0, 1, 2, 3, 4, 7, 8, 16]):
            b = OrBits()
            oracle.or_bits_init(ctypes.byref(b), ob, len(ob))
            tc = oracle.or_cavlc_block(ctypes.byref(b), arr, maxc, nC)
            g = [ctypes.c_int() for _ in range(4)]
            probesim.psim_block(arr, maxc, nC, *[ctypes.byref(v) for v in g])
            assert (g[0].value, g[1].value) == (tc, t1), (coef, nC)
            assert g[2].value + g[3].value == b.nbits, (coef, nC, g[2].value, g[3].value, b.nbits)
    assert seen_esc and (maxc <= 10 or seen_sl1)


def _synth_mb(rng):
    def blk(maxc, dens):
        if rng.random() >= dens:
            return [0] * maxc
        c = [0] * maxc
        for p in rng.sample(range(maxc), rng.randint(1, maxc)):
            c[p] = _mag(rng, rng.choice((0, 0, 1, 2, 3, 4)))
        return c

    kind = rng.choice(("zero", "luma", "dc", "ac", "mixed", "mixed"))
    dl = 0 if kind in ("zero", "dc") else rng.random() + 0.1
    dd = 0 if kind in ("zero", "luma") else 0.8
    da = rng.random() + 0.1 if kind in ("ac", "mixed") else 0
    if kind == "ac":
        dl = rng.choice((0, 0.5))
    return kind, ([blk(16, dl) for _ in range(16)], [blk(4, dd) for _ in range(2)],
                  [[blk(15, da) for _ in range(4)] for _ in range(2)])


def test_mb_bits(probesim, oracle):
    """mb_len against or_dyn_mb_levels_bits: random neighbour TotalCoeffs,
    both availabilities, cbp 0 / luma-only / DC-only / AC MBs"""
    rng = random.Random(4)
    kinds = set()
    for i in range(400):
        kind, lv = _synth_mb(rng)
        al, at = rng.random() < 0.7, rng.random() < 0.7
        tcl = [rng.choice([0, 0, 1, 2, 3, 4, 5, 7, 8, 11, 16]) if k < 16 else rng.randint(0, 15) for k in range(24)]
        tct = [rng.choice([0, 1, 2, 3, 4, 6, 8, 9, 13, 16]) if k < 16 else rng.randint(0, 15) for k in range(24)]
        bits, nz, tco = mb_levels_bits(oracle, lv, tcl, tct, al, at)
        luma, cdc, cac = lv
        nzo, tcs = ctypes.c_int(), (ctypes.c_int * 24)()
        got = probesim.psim_mb((ctypes.c_int * 256)(*[v for b in luma for v in b]),
                               (ctypes.c_int * 8)(*[v for b in cdc for v in b]),
                               (ctypes.c_int * 120)(*[v for p in cac for b in p for v in b]),
                               (ctypes.c_int * 24)(*tcl), (ctypes.c_int * 24)(*tct), int(al), int(at),
                               ctypes.byref(nzo), tcs)
        assert (got, nzo.value) == (bits, nz), (i, kind, al, at)
        any_ac = any(v for p in cac for b in p for v in b)
        any_dc = any(v for p in cdc for v in p)
        kinds.add((any(v for b in luma for v in b), 2 if any_ac else 1 if any_dc else 0, al, at))
        # TotalCoeffs agree wherever the oracle coded the block
        for r in range(24):
            assert tco[r] in (0, tcs[r])
    assert {(False, 0), (True, 0), (False, 1), (False, 2), (True, 2)} <= {k[:2] for k in kinds}
    assert {k[2:] for k in kinds} == {(a, b) for a in (False, True) for b in (False, True)}


@pytest.fixture(scope="module")
def frames96(oracle):
    """the 96 x 96 case at the six QPs: per QP the oracle's frames"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    offs = [5, 40, 96, 0]
    R = random_refs(w, h, 11)
    rc = Rect(*rect, 0)
    srcs = [np.frombuffer(bytes(rect_source(oracle, 0, off, rc)), np.uint8) for off in offs]
    return offs, rect, srcs, {qp: oracle_probe(oracle, w, h, offs, rect, srcs, R, qp)[1] for qp in QPS}


def test_pixels_to_result(probesim, frames96):
    """psim_rect (the coder's levels, the body / token / MB lengths composed
    across the rect, the decoder's half) equals the sums over the oracle's
    traced MBs and the test decoder's squared error"""
    offs, rect, srcs, by_qp = frames96
    n = 384 * rect[2] * rect[3]
    for qp, frames in by_qp.items():
        for t, fr in enumerate(frames):
            sse, bits, nz = (ctypes.c_uint64 * 3)(), ctypes.c_uint32(), ctypes.c_uint32()
            probesim.psim_rect((ctypes.c_uint8 * n).from_buffer_copy(srcs[t].tobytes()),
                               (ctypes.c_uint8 * n).from_buffer_copy(fr["pred"]), rect[2], rect[3], qp, 1, 1,
                               sse, ctypes.byref(bits), ctypes.byref(nz))
            assert (bits.value, nz.value) == (fr["bits"], fr["nonzero"]), (qp, t)
            assert tuple(int(v) for v in sse) == fr["sse"], (qp, t)


def test_rbsp_identity(frames96):
    """RBSP bits before the stop bit = bits(q) + len(se(q - 26)) + C(frame),
    C one constant per frame; the pinned figures of offset 5 at QP 26"""
    offs, _, _, by_qp = frames96
    want = {5: 258, 40: 264, 96: 230, 0: 230}
    for t, off in enumerate(offs):
        cs = {qp: constant_of(by_qp[qp][t], qp) for qp in QPS}
        assert set(cs.values()) == {want[off]}, (off, cs)
    fr = by_qp[26][0]
    assert (fr["bits"], fr["nonzero"], fr["bits"] + 1 + 258) == (31076, 5299, 31335)
