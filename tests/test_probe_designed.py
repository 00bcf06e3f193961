"""The designed corpus (tests/designed.py) through the QP probe's device
functions compiled for the CPU (psim_rect of tests/hostsim/probe_sim.cpp),
against the expectation of tests/designedprobe.py, which is the oracle's
alone; and what that expectation is worth as a yardstick for the GPU tests
(tests/test_gpu_probe_designed.py, test_gpu_hprobe_designed.py,
test_gpu_pos_designed.py): the header's identity holds on it, its traced
levels ask the probe's length functions every hard question (reach), the
hinted yardstick (tests/hprobehelp.py) agrees with it, and a moved rect
leaves the levels alone.  Every comparison is exact.  No GPU."""
import ctypes
import os
import subprocess

import pytest

import designed as dz
import designedprobe as dp
from conftest import PKG, REPO
from dynposhelp import per_position
from hprobehelp import expect_stream
from hreconhelp import EXACT
from probehelp import oracle_probe, rbsp_bits, se_len

ALL = dz.names("a", "a20", "b", "c", "d", "e")


@pytest.fixture(scope="module")
def probesim(tmp_path_factory):
    """TEST-ONLY CPU build of probe_device.h, as tests/test_probe_hostsim.py
    builds it; the library lands in pytest's temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("probesim") / "libprobesim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", d,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(d, "probe_sim.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.mark.parametrize("name", ALL)
def test_psim_rect(probesim, oracle, name):
    """bits, nonzero and the three squared errors of every frame of stream 0
    at every candidate"""
    c = dz.cases(oracle)[name]
    qps = dp.candidates(name)
    assert c.qp in qps and qps.index(c.qp) == ALL.index(name) % len(qps)
    n = 384 * c.rw * c.rh
    bad = []
    for f, per in enumerate(dp.expect(oracle, name, 0)):
        for k, e in enumerate(per):
            sse, bits, nz = (ctypes.c_uint64 * 3)(), ctypes.c_uint32(), ctypes.c_uint32()
            probesim.psim_rect((ctypes.c_uint8 * n).from_buffer_copy(c.src[0, f].tobytes()),
                               (ctypes.c_uint8 * n).from_buffer_copy(e["pred"]), c.rw, c.rh, qps[k], 1, 1,
                               sse, ctypes.byref(bits), ctypes.byref(nz))
            got = (bits.value, nz.value, tuple(int(v) for v in sse))
            if got != (e["bits"], e["nonzero"], tuple(e["sse"])):
                bad.append((f, qps[k], got, (e["bits"], e["nonzero"], tuple(e["sse"]))))
    assert not bad, bad


@pytest.mark.parametrize("name", ALL)
def test_identity(oracle, name):
    """rbsp_bits(nal) - bits - len(se(qp - 26)) is one constant per frame
    over the candidates: the bits are the NAL's, and nothing else in the NAL
    depends on the QP (stream 0, whose expectation test_psim_rect has made)"""
    qps = dp.candidates(name)
    for f, per in enumerate(dp.expect(oracle, name, 0)):
        cs = [rbsp_bits(e["nal"]) - e["bits"] - se_len(q - 26) for q, e in zip(qps, per)]
        assert len(set(cs)) == 1 and cs[0] == per[0]["C"], (f, cs)


@pytest.fixture(scope="module")
def tally(oracle):
    """what the own-QP levels of stream 0 ask of level_len and zeros_len:
    {(suffixLength, escape class)} of groups b and e, the chroma DC levels of
    group e, {(MAXC, TotalCoeff)} and {MAXC with a run_before at zerosLeft >=
    7} of the whole corpus"""
    pairs, cdc, tcs, zl7 = {}, set(), set(), set()
    for name, group in dz.CASE_GROUPS:
        own = dz.cases(oracle)[name].qp
        for fr in dp.frames_at(oracle, dz.cases(oracle)[name], 0, own):
            for maxc, coef in dp.blocks_of(fr["mbs"]):
                if group in ("b", "e"):
                    for code, sl in dp.level_calls(coef):
                        key = (sl, dp.escape_class(code, sl))
                        pairs[key] = pairs.get(key, 0) + 1
                    if group == "e" and maxc == 4:
                        cdc.update(coef)
                z = dp.zeros_calls(coef)
                if z:
                    tcs.add((maxc, z[0]))
                    if any(v >= 7 for v in z[1]):
                        zl7.add(maxc)
    return pairs, cdc, tcs, zl7


def test_reach(tally):
    """the expectation, not the targets, holds every level_len argument pair,
    +-2063 in a chroma DC block, and zeros_len with zerosLeft >= 7 and with
    TotalCoeff MAXC (no total_zeros) and MAXC - 1 for each block kind"""
    pairs, cdc, tcs, zl7 = tally
    print("level_len (suffixLength, class): calls", sorted(pairs.items()))
    assert set(pairs) == {(sl, k) for sl in range(7) for k in range(3)}
    assert 2063 in cdc and -2063 in cdc
    assert {(m, m - d) for m in (16, 15, 4) for d in (0, 1)} <= tcs
    assert {16, 15} <= zl7                    # a chroma DC block has at most 3 zeros
    assert 4 not in zl7


@pytest.mark.parametrize("name", dp.HINTED)
def test_hinted_yardstick(oracle, name):
    """hprobehelp.expect_stream (no hint rects, EXACT, the rect at the corpus
    origin) gives the plain expectation's bits, nonzero and squared errors:
    the test decoder's levels through or_dyn_mb_levels_bits on one side,
    or_compose_dyn's trace on the other"""
    c = dz.cases(oracle)[name]
    qps = dp.three_of(name)
    assert c.qp in qps
    plan = [([], EXACT, (dz.X0, dz.Y0))] * c.F
    hexp, _ = expect_stream(oracle, c.w, c.h, c.offs[0], plan, c.rw, c.rh, c.src[0], c.R, qps)
    exp = dp.expect(oracle, name, 0, qps)
    for f in range(c.F):
        for k in range(len(qps)):
            h, e = hexp[f][k], exp[f][k]
            assert (h["bits"], h["nonzero"], tuple(h["sse"])) == (e["bits"], e["nonzero"], tuple(e["sse"])), (f, k)


@pytest.mark.parametrize("name", dp.MOVED_INT8 + dp.MOVED_GENERAL)
def test_moved_positions_keep_the_levels(oracle, name):
    """the traced levels of every frame at its moved position (x0 0, flush
    right, one row lower) equal the unmoved run's of that designed frame: the
    prediction is the same, so only nC and the tokens change, and what
    DESIGN 4b proves of the corpus holds for the moved bytes.  A difference
    here is a misplaced reference, not a coder's fault"""
    c = dz.cases(oracle)[name]
    m = dp.moved(oracle, name)
    base = dp.frames_at(oracle, c, 0, c.qp)
    for s in range(2):
        frames = per_position(lambda rect: oracle_probe(oracle, m.w, m.h, m.offs[s], rect, m.src[s], m.R, m.qp,
                                                        decode=False)[1], m.pos[s], m.rw, m.rh)
        for f, fr in enumerate(frames):
            if fr is None:
                assert m.pos[s][f] is None
                continue
            got = [mb[3] for mb in fr["mbs"]]
            assert got == [mb[3] for mb in base[m.slot[s][f]]["mbs"]], (s, f, m.pos[s][f])
