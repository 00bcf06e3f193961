"""k_dyn_gather takes the dynamic rect's NALs to the arena in runs of
consecutive 16-byte chunks per thread (two).  The shapes at which a run-based
gather can go wrong, each byte for byte against the CPU restatement
(oracle_streams): runs cut by workgroup ranges, runs over many tiny row
groups, EP bytes dense in a run, every alignment of a NAL's start, and the
window / serial paths beside it.  The seeds were chosen on the CPU so that the
oracle's own bytes have the property each case is about; the property is
asserted on those bytes, so a case cannot silently stop covering it.
Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import designed as dz
from conftest import synthetic_offsets
from dynhelp import qp_field, Rect, split_nals
from test_gpu_dyn import ArrayRefs, check_equal, gpu_streams, oracle_streams, random_refs

pytestmark = pytest.mark.gpu

RUN = 2                                   # chunks per run (GR, dyn_kernels.hip)


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def slice_nals(stream):
    """(offset, bytes) of the stream's slice NALs (nal_unit_type 1: with a
    dynamic rect set, the NALs k_dyn_gather writes)"""
    out, pos = [], 0
    for n in split_nals(stream):
        if len(n) > 5 and (n[4] & 31) == 1:
            out.append((pos, n))
        pos += len(n)
    return out


def ep_offsets(nal):
    """offsets in the NAL (start code included) of its emulation-prevention bytes"""
    out, i = [], nal.find(b"\x00\x00\x03", 5)
    while i >= 0:
        out.append(i + 2)
        i = nal.find(b"\x00\x00\x03", i + 3)
    return out


def ep_chunk_stats(streams, RUN=RUN):
    """over the streams' slice NALs: the most EP bytes in one 16-byte arena
    chunk, and whether some run (RUN chunks, counted from the NAL's first
    chunk as the kernel does) has an EP byte in every chunk"""
    most, full = 0, False
    for st in streams:
        for off, n in slice_nals(st):
            c0 = off >> 4
            per = {}
            for e in ep_offsets(n):
                c = ((off + e) >> 4) - c0
                per[c] = per.get(c, 0) + 1
            if per:
                most = max(most, max(per.values()))
            full = full or any(all(RUN * (c // RUN) + k in per for k in range(RUN)) for c in per)
    return most, full


def small_case(oracle, S, F, seed):
    """64x64, a 2x2-MB rect, random references and source"""
    w, h = 64, 64
    rect = Rect(1, 1, 2, 2)
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, 40, (S, F)).astype(np.int32)
    R = random_refs(w, h, seed + 1)
    src = rng.integers(0, 256, (S, F, 384 * 4)).astype(np.uint8)
    return w, h, rect, offs, R, src, oracle_streams(oracle, w, h, offs, rect, src, R)


def test_runs_cut_by_workgroup_ranges_z16(gpu, oracle):
    """16 NALs: gather_z takes Z = 16, and a ~1.2 KB NAL's ~75 chunks over 16
    workgroups (ranges in whole runs) leave each three runs or none: fewer
    runs than threads everywhere, the NAL's end inside a late workgroup's
    range"""
    w, h, rect, offs, R, src, want = small_case(oracle, 2, 8, 41)
    sizes = [len(n) for st in want for _, n in slice_nals(st)]
    assert len(sizes) == 16 and max(sizes) < 16 * 128, sizes     # under 128 bytes a workgroup
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


def test_runs_with_one_workgroup_per_nal(gpu, oracle):
    """the same geometry with 128 x 16 = 2,048 NAL slots: Z = 1, one
    workgroup walks the whole NAL in runs"""
    w, h, rect, offs, R, src, want = small_case(oracle, 128, 16, 43)
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src, arena=1 << 20)
    if rc == gpu.SCROLL_ERR_OVERFLOW and "grown" in gpu.last_error():
        b.compose(offs.shape[1])          # random references: every NAL on the general path, its pool grown once
        rc = b.sync()
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.parametrize("rect", [(0, 0, 1, 20), (19, 19, 1, 1)])
def test_many_groups_per_run(gpu, oracle, rect):
    """source = prediction (flat references, the source of the same
    colours): no residual, every row group is a few bits, so every run
    crosses several seams -- more slow runs than the workgroup's queue
    holds"""
    w, h = 320, 320
    rc_ = Rect(*rect)
    S, F = 2, 6
    offs = synthetic_offsets(S, F, h, first_stream=5)
    planes = (np.full((h, w), 90, np.uint8), np.full((h // 2, w // 2), 120, np.uint8),
              np.full((h // 2, w // 2), 200, np.uint8))
    R = ArrayRefs([planes, planes])
    n = rc_.w * rc_.h
    one = np.concatenate([np.full(256 * n, 90, np.uint8), np.full(64 * n, 120, np.uint8),
                          np.full(64 * n, 200, np.uint8)])
    src = np.broadcast_to(one, (S, F, 384 * n)).copy()
    want = oracle_streams(oracle, w, h, offs, rc_, src, R)
    # no residual: under a byte per MB of the picture, a rect row group a few bits
    assert max(len(nl) for st in want for _, nl in slice_nals(st)) < (w // 16) * (h // 16), "residual coded"
    b, rc = gpu_streams(gpu, w, h, offs, rc_, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


def dense_case(oracle, qp):
    w, h = 96, 96
    rect = Rect(0, 0, 6, 6, qp_field(qp))
    seed = {0: 23, 12: 3}[qp]             # of seeds 1..39, the first with two EP bytes in a chunk
    rng = np.random.default_rng(seed)
    S, F = 2, 10
    offs = rng.integers(-200, 300, (S, F)).astype(np.int32)
    R = random_refs(w, h, seed + 100)
    src = rng.integers(0, 256, (S, F, 384 * 36)).astype(np.uint8)
    src[:, ::3] = 0                                   # zero pictures: long zero-bit runs
    return w, h, rect, offs, R, src, oracle_streams(oracle, w, h, offs, rect, src, R)


@pytest.fixture(scope="module")
def dense(oracle):
    return {qp: dense_case(oracle, qp) for qp in (0, 12)}


@pytest.mark.parametrize("qp", [0, 12])
def test_ep_bytes_two_in_a_chunk(gpu, oracle, dense, qp):
    """whole-picture rect, random pixels, QP 0 and 12 (long level escapes):
    a chunk with two EP bytes.  Random pixels give 10-40 EP bytes per 15-20 KB
    NAL: none of seeds 1..39 at either QP has a run with an EP byte in each of
    its chunks (searched on the CPU), so that property is pinned on the
    designed EP-dense pictures below"""
    w, h, rect, offs, R, src, want = dense[qp]
    most, _ = ep_chunk_stats(want)
    assert most >= 2, most
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


def designed_case(oracle, name):
    c = dz.cases(oracle)[name]
    return c.w, c.h, c.rect(), c.offs, c.R, c.src, dz.want_of(oracle, name)


@pytest.mark.parametrize("name", ["d_epdense_qp22", "e_epdense_qp12"])
def test_ep_bytes_in_every_chunk_of_a_run(gpu, oracle, name):
    """the designed EP-dense pictures (tests/designed.py: levels on the
    level_prefix 15 escape, 27 zero bits in a row): up to three EP bytes in
    a chunk and runs with EP bytes in every one of their chunks"""
    w, h, rect, offs, R, src, want = designed_case(oracle, name)
    most, full = ep_chunk_stats(want)
    assert most >= 2 and full, (most, full)
    assert ep_chunk_stats(want, 4)[1]     # also of a 64-byte run
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


def test_every_start_alignment(gpu, oracle):
    """one stream whose slice NALs start at every residue mod 16 of the
    arena: the first run's start code and header end at every byte of a
    chunk, also exactly at its end"""
    w, h, rect, offs, R, src, want = small_case(oracle, 1, 64, 40)
    res = {off & 15 for off, _ in slice_nals(want[0])}
    assert res == set(range(16)), sorted(res)
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    b.close()


@pytest.mark.parametrize("flag", ["SCROLL_DEBUG_DYN_EPWIN", "SCROLL_DEBUG_DYN_EPCAP4"])
def test_rare_paths_unchanged(gpu, oracle, flag):
    """an EP-dense case again through the gather's window path (7 positions
    per LDS window: runs cut by window ends) and through emit_serial"""
    w, h, rect, offs, R, src, want = designed_case(oracle, "d_epdense_qp22")
    b, rc = gpu_streams(gpu, w, h, offs, rect, R, src, debug=getattr(gpu, flag))
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    eps = [b.dyn_frame_info(s, t)[1] for s in range(offs.shape[0]) for t in range(offs.shape[1])]
    assert sum(e > 7 for e in eps) >= 2, eps          # the rare path ran
    b.close()
