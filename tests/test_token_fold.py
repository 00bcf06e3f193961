"""k_dyn_row's token-first CAVLC body on the CPU (tests/hostsim/token_sim.cpp
around h264-scroll-encoder_amd/csrc/dyn_device.h): cavlc_body_t given nC and
the coeff_token tables against the oracle's whole block at that nC
(or_cavlc_block: coeff_token, then the body) and cavlc_body<CapSink, true>
(the body alone) -- the bits, the length, TotalCoeff, TrailingOnes and which
of the kernel's three forms the piece takes:
  0  token in front: at most 128 bits, the register holds the whole piece;
  1  over 128 bits only with its token: the register's low bits are the whole
     body (it loses top bits only), the kernel keeps that and adds the token
     when it writes the piece;
  2  the body itself over 128 bits: the levels stay, nothing of the register
     is used.
Inputs: the random blocks of test_hostsim_dyn at every coeff_token table,
luma and chroma AC; blocks searched for pieces of exactly 127, 128, 129 bits
and bodies of exactly 128 and 129; pieces that pass 64 bits only with their
token (the 64-bit accumulator spills with the token in it); levels past the
level table (the exact re-code starts from the token again)."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import PKG, REPO
from test_hostsim_dyn import OrBits, _bits, _random_block

NCS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 16]          # tables 0-1, 2-3, 4-7, >= 8


@pytest.fixture(scope="module")
def toksim(tmp_path_factory):
    """TEST-ONLY CPU build of the token-first body; the library lands in
    pytest's temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("toksim") / "libtoksim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", d, "-I", os.path.join(PKG, "csrc"),
                    os.path.join(d, "token_sim.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def oracle_block(oracle, coef, maxc, nC):
    buf = (ctypes.c_uint8 * 1024)()
    b = OrBits()
    oracle.or_bits_init(ctypes.byref(b), buf, len(buf))
    oracle.or_cavlc_block(ctypes.byref(b), (ctypes.c_int * 16)(*(list(coef) + [0] * (16 - len(coef)))), maxc, nC)
    return _bits(buf, 0, int(b.nbits))


def low_bits(o, n):
    """the low n (<= 128) bits of the register hi:lo in out words o[0..3], first bit first"""
    v = o[0] << 96 | o[1] << 64 | o[2] << 32 | o[3]
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def check(lib, oracle, coef, maxc, nC):
    """one block through both coders and the oracle -> (piece bits, body bits, form)"""
    ca = (ctypes.c_int * 16)(*(list(coef) + [0] * (16 - len(coef))))
    out = (ctypes.c_uint32 * 20)()
    assert lib.tsim_piece(ca, maxc, nC, out) == 0, coef
    tok, ref, tl, form = list(out[:9]), list(out[9:18]), out[18], out[19]
    want = oracle_block(oracle, coef, maxc, nC)
    key = (coef, maxc, nC)
    n, nb = tok[4], ref[4]
    assert n == len(want), key                                  # the length counts the token
    assert n - nb == tl and 1 <= tl <= 16, key                  # ... which is the oracle's coeff_token
    assert tok[5:7] == ref[5:7], key                            # TotalCoeff, TrailingOnes
    assert tok[5] == sum(1 for c in coef if c), key
    assert tok[7] == (1 if n <= 128 else 0), key
    assert form == (0 if n <= 128 else (1 if nb <= 128 else 2)), key
    if form == 0:
        assert low_bits(tok, n) == want, key
    elif form == 1:
        assert low_bits(tok, nb) == want[tl:], key
    if nb <= 128:
        assert low_bits(ref, nb) == want[tl:], key              # the reference body is the oracle's too
    return n, nb, form


def test_token_first_random_blocks(toksim, oracle):
    rng = random.Random(12)
    seen = set()
    for it in range(4000):
        mx = rng.choice([16, 15, 4])
        coef = _random_block(rng, mx)
        if mx == 4 or any(c < -128 or c > 127 for c in coef):
            continue
        nC = NCS[it % len(NCS)]
        n, nb, form = check(toksim, oracle, coef, mx, nC)
        seen.add((mx, 0 if nC < 2 else (1 if nC < 4 else (2 if nC < 8 else 3)), nb == 0, form))
    for mx in (16, 15):
        for cls in range(4):
            assert (mx, cls, True, 0) in seen, (mx, cls)        # the token alone
            for form in range(3):
                assert (mx, cls, False, form) in seen, (mx, cls, form)


def test_token_first_exact_lengths(toksim, oracle):
    """pieces of exactly 127, 128 and 129 bits and bodies of exactly 128 and
    129 (each form's last and first length), at every table, found among
    blocks of mid-sized levels"""
    rng = random.Random(5)
    want = {("piece", k, c): 0 for k in (127, 128, 129) for c in range(4)}
    want.update({("body", k, c): 0 for k in (128, 129) for c in range(4)})
    for it in range(200000):
        if all(v >= 2 for v in want.values()):
            break
        mx = rng.choice([16, 15])
        k = rng.randint(4, mx)
        big = rng.choice([3, 6, 12, 24, 47, 60])
        coef = [rng.randint(-big, big) for _ in range(k)] + [0] * (mx - k)
        c = it % 4
        n, nb, form = check(toksim, oracle, coef, mx, [0, 2, 4, 8][c])
        if ("piece", n, c) in want:
            want[("piece", n, c)] += 1
            assert form == (0 if n <= 128 else 1)
        if ("body", nb, c) in want:
            want[("body", nb, c)] += 1
            assert form == (1 if nb <= 128 else 2)
    assert all(v >= 2 for v in want.values()), want


def test_token_in_the_accumulator_spill(toksim, oracle):
    """bodies of at most 64 bits whose piece is over 64: the accumulator
    spills into the 128-bit register only because the token is in it; and
    bodies of 60 to 70 bits either side of it"""
    rng = random.Random(9)
    only_token = near = 0
    for it in range(20000):
        mx = rng.choice([16, 15])
        k = rng.randint(3, 10)
        big = rng.choice([6, 12, 24, 40])
        coef = [rng.randint(-big, big) for _ in range(k)] + [0] * (mx - k)
        nC = NCS[it % len(NCS)]
        n, nb, form = check(toksim, oracle, coef, mx, nC)
        only_token += nb <= 64 < n
        near += 60 <= nb <= 70
    assert only_token > 100 and near > 500, (only_token, near)


def test_token_first_big_levels(toksim, oracle):
    """levels past the level table (|v| > 47): the block is coded again with
    the exact form, from the token on"""
    rng = random.Random(3)
    forms = [0, 0, 0]
    for v in (48, 49, 100, 127, -128, -48):
        for nC in NCS:
            for mx in (16, 15):
                for blk in ([v], [v] + [0] * 13 + [1], [v, 0, 3, -2, 1, 1, 1], [5, v, -9, 0, 0, 2, 0, 1, -1, 1, 1],
                            [3] * 10 + [v], [v] * 3, [v] * 6, [v] * mx,
                            [rng.randint(-3, 3) for _ in range(8)] + [v]):
                    n, nb, form = check(toksim, oracle, blk + [0] * (mx - len(blk)), mx, nC)
                    forms[form] += 1
    # a big level among mid-sized ones: pieces around 128 bits, the middle form too
    for it in range(6000):
        mx = rng.choice([16, 15])
        big = rng.choice((6, 12, 24, 40))
        blk = [rng.randint(-big, big) for _ in range(rng.randint(4, 12))]
        blk.insert(rng.randrange(len(blk) + 1), rng.choice((48, 60, 100, 127, -128, -48)))
        n, nb, form = check(toksim, oracle, blk + [0] * (mx - len(blk)), mx, NCS[it % len(NCS)])
        forms[form] += 1
    assert all(f > 20 for f in forms), forms
