"""The reconstruction's device functions (h264-scroll-encoder_amd/csrc/
recon_device.h: dequantisation, chroma DC path, inverse transform, clip, and
the block from pixels to reconstruction), compiled for the CPU
(tests/hostsim/recon_sim.cpp), against the test decoder tests/h264_pslice.py.
Every comparison is exact."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import h264_pslice as hp
from conftest import PKG, REPO
from dynhelp import Rect, rect_source
from reconhelp import oracle_frames, qpc_of, sse3, striped_refs


@pytest.fixture(scope="module")
def reconsim(tmp_path_factory):
    """TEST-ONLY CPU build of recon_device.h (flags and include paths of the
    hostsim fixture); the library lands in pytest's temp directory"""
    d = os.path.join(REPO, "tests", "hostsim")
    so = str(tmp_path_factory.mktemp("reconsim") / "libreconsim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", d,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(d, "recon_sim.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def _levels(rng, n, mag):
    kind = rng.random()
    if kind < 0.2:
        return [0] * n
    if kind < 0.35:
        return [rng.choice((-2063, 2063, 0)) for _ in range(n)]
    out = [0] * n
    for p in rng.sample(range(n), rng.randint(1, n)):
        out[p] = rng.choice((-2063, 2063)) if rng.random() < 0.05 else rng.randint(-mag, mag)
    return out


def _pred_plane(rng, n):
    kind = rng.random()
    if kind < 0.25:
        return [rng.choice((0, 255)) for _ in range(n * n)]
    if kind < 0.4:
        return [rng.choice((0, 1, 2, 253, 254, 255)) for _ in range(n * n)]
    return [rng.randint(0, 255) for _ in range(n * n)]


def test_qpc_table(reconsim):
    for qp in range(52):
        assert reconsim.rsim_qpc(qp) == qpc_of(qp)


@pytest.mark.parametrize("qp", range(52))
def test_recon_mb_from_levels(reconsim, qp):
    """rsim_recon_mb (dequant4x4, chroma_dc, inv4x4, add_clip) equals
    reconstruct_mb at every QP with its QPc: random levels with the +-2063
    clamp and all-zero blocks, random chroma DCs, predictions with 0 and 255
    so both clips fire"""
    rng = random.Random(1000 + qp)
    lo = hi = 0
    for it in range(5):
        mag = (3, 40, 300, 2063, 12)[it]
        luma = [_levels(rng, 16, mag) for _ in range(16)]
        cdc = [_levels(rng, 4, mag) for _ in range(2)]
        cac = [[_levels(rng, 15, mag) for _ in range(4)] for _ in range(2)]
        py, pu, pv = _pred_plane(rng, 16), _pred_plane(rng, 8), _pred_plane(rng, 8)
        rows = lambda v, n: [v[n * i:n * i + n] for i in range(n)]
        ey, eu, ev = hp.reconstruct_mb(luma, cdc, cac, rows(py, 16), rows(pu, 8), rows(pv, 8),
                                       qp=qp, qpc=qpc_of(qp))
        ry, ru, rv = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
        reconsim.rsim_recon_mb((ctypes.c_int * 256)(*[v for b in luma for v in b]),
                               (ctypes.c_int * 8)(*[v for b in cdc for v in b]),
                               (ctypes.c_int * 120)(*[v for pl in cac for b in pl for v in b]),
                               (ctypes.c_uint8 * 256)(*py), (ctypes.c_uint8 * 64)(*pu), (ctypes.c_uint8 * 64)(*pv),
                               qp, ry, ru, rv)
        assert list(ry) == [v for r in ey for v in r], (qp, it)
        assert list(ru) == [v for r in eu for v in r], (qp, it)
        assert list(rv) == [v for r in ev for v in r], (qp, it)
        lo += list(ry).count(0)
        hi += list(ry).count(255)
    assert lo > 0 and hi > 0


@pytest.mark.parametrize("qp", [0, 12, 22, 26, 39, 51])
def test_pixels_to_recon_vs_decoder(reconsim, oracle, qp):
    """source and or_ref_sample prediction through rsim_recon_rect
    (recon_luma4x4 / recon_chroma8x8: the coder's levels, then the decoder's
    half) equals what the test decoder makes of or_compose_dyn's NAL, and the
    squared error equals numpy's"""
    w, h, rect = 96, 96, (1, 1, 4, 4)
    offs = [0, 5, 40, 96]
    R = striped_refs(oracle, w, h)
    rc = Rect(*rect, 0)
    srcs = [np.frombuffer(bytes(rect_source(oracle, 3, t, rc)), np.uint8) for t in range(len(offs))]
    _, frames = oracle_frames(oracle, w, h, offs, rect, srcs, R, qp=qp)
    n = 384 * rect[2] * rect[3]
    for t, (want, pred) in enumerate(frames):
        out = (ctypes.c_uint8 * n)()
        sse = (ctypes.c_uint64 * 3)()
        reconsim.rsim_recon_rect((ctypes.c_uint8 * n).from_buffer_copy(srcs[t].tobytes()),
                                 (ctypes.c_uint8 * n).from_buffer_copy(pred), rect[2], rect[3], qp, out, sse)
        assert bytes(out) == want, (qp, t)
        assert tuple(int(v) for v in sse) == sse3(srcs[t], want, rect), (qp, t)
