"""GPU check of the surface entry (scroll_batch_dyn_source_from_surfaces,
scroll_batch_surfaces_to_i420, scroll_batch_set_dyn_refs_device; k_csc):
windows of pitched RGBA / BGRA surfaces in device memory become the dynamic
rect's source or whole I420 pictures, byte for byte what the numpy
restatement of the rule (tests/cschelp.py) gives, for every matrix / range /
byte-order variant; nothing outside the frames' own source blocks is written;
the composed streams equal those of the host-fed path and the oracle's.
Device buffers through ctypes HIP, as tests/test_gpu_ipcm.py.  Run on an
MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from cschelp import BGRA, BT601, BT709, RGBA, VARIANTS, convert, i420_bytes
from dynhelp import Rect, ipcm_file
from reconhelp import ArrayRefs, oracle_frames, random_refs

pytestmark = pytest.mark.gpu

FILL = 0xA5         # the source buffer before a conversion
PAD = 0xFF          # surface bytes that are no pixel of any window's picture


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


class Hip:
    """Device buffers through the HIP runtime libh264scroll itself links"""

    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so.7")
        L = self.lib
        L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        L.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        L.hipFree.argtypes = [ctypes.c_void_p]
        for f in (L.hipMalloc, L.hipMemcpy, L.hipMemset, L.hipFree, L.hipDeviceSynchronize):
            f.restype = ctypes.c_int

    def alloc(self, n):
        p = ctypes.c_void_p()
        assert self.lib.hipMalloc(ctypes.byref(p), n) == 0
        return p.value

    def free(self, p):
        self.lib.hipFree(p)

    def fill(self, p, value, n):
        assert self.lib.hipMemset(p, value, n) == 0
        assert self.lib.hipDeviceSynchronize() == 0

    def write(self, p, data):
        a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0         # host -> device

    def read(self, p, n):
        host = np.empty(n, np.uint8)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(host.ctypes.data, p, n, 2) == 0             # device -> host
        return host


@pytest.fixture(scope="module")
def hip(gpu):
    return Hip()


class Surfaces:
    """[S][F] random pw x ph pictures laid out at the given pitch and strides
    in one host image (every other byte PAD), uploaded to the device"""

    def __init__(self, hip, S, F, pw, ph, pitch=None, fstride=None, sstride=None, seed=1, shared=False):
        rng = np.random.default_rng(seed)
        self.hip, self.pw, self.ph = hip, pw, ph
        self.pitch = pitch or 4 * pw
        self.fstride = fstride if fstride is not None else self.pitch * ph
        self.sstride = 0 if shared else (sstride if sstride is not None else self.fstride * F)
        ns = 1 if shared else S
        self.img = rng.integers(0, 256, (ns, F, ph, pw, 4), dtype=np.uint8)
        if shared:
            self.img = np.broadcast_to(self.img, (S, F, ph, pw, 4))
        self.bytes = (ns - 1) * self.sstride + (F - 1) * self.fstride + (ph - 1) * self.pitch + 4 * pw
        mem = np.full(self.bytes, PAD, np.uint8)
        for s in range(ns):
            for f in range(F):
                at = s * self.sstride + f * self.fstride
                rows = np.lib.stride_tricks.as_strided(mem[at:], (ph, 4 * pw), (self.pitch, 1))
                rows[:] = self.img[s, f].reshape(ph, 4 * pw)
        self.p = hip.alloc(self.bytes)
        hip.write(self.p, mem)

    def free(self):
        self.hip.free(self.p)


def src_state(hip, b):
    """the whole source buffer and its strides"""
    p, ls, lf = b.dyn_source_device()
    return hip.read(p, b.max_streams * ls), ls, lf


def src_fill(hip, b):
    p, ls, _ = b.dyn_source_device()
    hip.fill(p, FILL, b.max_streams * ls)


def expect_src(b, ls, lf, blocks):
    """the source buffer after a conversion over FILL: blocks = {(s, f): bytes}"""
    want = np.full(b.max_streams * ls, FILL, np.uint8)
    for (s, f), data in blocks.items():
        want[s * ls + f * lf:s * ls + f * lf + len(data)] = np.frombuffer(data, np.uint8)
    return want


def cut(img, x0, y0, rw, rh):
    return img[16 * y0:16 * (y0 + rh), 16 * x0:16 * (x0 + rw)]


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: byte {k} is {got[k]}, not {want[k]}; {int((got != want).sum())} differ")


def make_batch(gpu, S, F, pw, ph, rect=None, arena=1 << 20):
    b = gpu.Batch(S, F, arena)
    for _ in range(S):
        b.add_stream(gpu.make_config(pw, ph))
    if rect:
        b.set_dyn_rect(*rect)
    return b


@pytest.mark.parametrize("rect", [(0, 0, 1, 1), (3, 2, 1, 1), (1, 0, 3, 2), (0, 1, 3, 2), (0, 0, 4, 3)])
def test_small_rects_all_variants(gpu, hip, rect):
    """64x48, 3 streams x 4 frames of which 3 are converted: rects at a
    corner, at the right and bottom edges and the whole picture; pitch, frame
    and stream strides padded with 0xFF; source pre-filled with 0xA5"""
    pw, ph, S, F, nfr = 64, 48, 3, 4, 3
    pitch = 4 * pw + 48
    fstride = pitch * ph + 160
    sf = Surfaces(hip, S, F, pw, ph, pitch, fstride, fstride * F + 4096, seed=sum(rect))
    b = make_batch(gpu, S, F, pw, ph, rect)
    try:
        for fmt, m, full in VARIANTS:
            src_fill(hip, b)
            b.dyn_source_from_surfaces(sf.p, nfr, sf.pitch, sf.fstride, sf.sstride, fmt=fmt, matrix=m,
                                       full_range=bool(full))
            got, ls, lf = src_state(hip, b)
            assert lf == 384 * rect[2] * rect[3] and ls >= F * lf
            blocks = {(s, f): i420_bytes(cut(sf.img[s, f], *rect), fmt, m, full) for s in range(S)
                      for f in range(nfr)}
            assert_same(got, expect_src(b, ls, lf, blocks), f"rect {rect} variant {(fmt, m, full)}")
    finally:
        b.close()
        sf.free()


def test_odd_width(gpu, hip):
    """a 5 x 1 MB rect in an 8 x 2 MB picture: 10 column groups per row pair, no divisor of the wave"""
    pw, ph, S, F, rect = 128, 32, 2, 2, (2, 1, 5, 1)
    sf = Surfaces(hip, S, F, pw, ph, 4 * pw + 16, seed=5)
    b = make_batch(gpu, S, F, pw, ph, rect)
    try:
        src_fill(hip, b)
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride, fmt=BGRA, matrix=BT709)
        got, ls, lf = src_state(hip, b)
        blocks = {(s, f): i420_bytes(cut(sf.img[s, f], *rect), BGRA, BT709, 0) for s in range(S) for f in range(F)}
        assert_same(got, expect_src(b, ls, lf, blocks), "5 x 1 rect")
    finally:
        b.close()
        sf.free()


def test_wide_rows_whole_picture(gpu, hip):
    """one 80 x 45 MB whole-picture rect from a 1280x720 surface"""
    pw, ph, rect = 1280, 720, (0, 0, 80, 45)
    sf = Surfaces(hip, 1, 1, pw, ph, seed=6)
    b = make_batch(gpu, 1, 1, pw, ph, rect, arena=4 << 20)
    try:
        src_fill(hip, b)
        b.dyn_source_from_surfaces(sf.p, 1, sf.pitch, sf.fstride, sf.sstride, fmt=RGBA, matrix=BT709, full_range=True)
        got, ls, lf = src_state(hip, b)
        assert_same(got, expect_src(b, ls, lf, {(0, 0): i420_bytes(sf.img[0, 0], RGBA, BT709, 1)}), "1280x720")
    finally:
        b.close()
        sf.free()


def test_shared_surfaces(gpu, hip):
    """stream_stride 0: every stream gets the same source"""
    pw, ph, S, F, rect = 64, 48, 3, 2, (1, 1, 2, 2)
    sf = Surfaces(hip, S, F, pw, ph, seed=7, shared=True)
    b = make_batch(gpu, S, F, pw, ph, rect)
    try:
        src_fill(hip, b)
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, 0)
        got, ls, lf = src_state(hip, b)
        blocks = {(s, f): i420_bytes(cut(sf.img[0, f], *rect), RGBA, BT601, 0) for s in range(S) for f in range(F)}
        assert_same(got, expect_src(b, ls, lf, blocks), "shared surfaces")
        assert np.array_equal(got[:F * lf], got[2 * ls:2 * ls + F * lf])
    finally:
        b.close()
        sf.free()


def test_cropped_mode(gpu, hip):
    """cropped = 1 on surfaces that are the rect itself: the bytes of the
    whole-picture mode cut at the rect"""
    pw, ph, S, F, rect = 64, 48, 2, 2, (1, 1, 3, 2)
    whole = Surfaces(hip, S, F, pw, ph, 4 * pw + 32, seed=8)
    crop = Surfaces(hip, S, F, 16 * rect[2], 16 * rect[3], 4 * 16 * rect[2] + 16, seed=8)
    # the cropped surfaces hold the whole pictures' rect
    mem = np.full(crop.bytes, PAD, np.uint8)
    for s in range(S):
        for f in range(F):
            at = s * crop.sstride + f * crop.fstride
            rows = np.lib.stride_tricks.as_strided(mem[at:], (crop.ph, 4 * crop.pw), (crop.pitch, 1))
            rows[:] = cut(whole.img[s, f], *rect).reshape(crop.ph, 4 * crop.pw)
    hip.write(crop.p, mem)
    b = make_batch(gpu, S, F, pw, ph, rect)
    try:
        src_fill(hip, b)
        b.dyn_source_from_surfaces(whole.p, F, whole.pitch, whole.fstride, whole.sstride, fmt=BGRA)
        a, ls, lf = src_state(hip, b)
        src_fill(hip, b)
        b.dyn_source_from_surfaces(crop.p, F, crop.pitch, crop.fstride, crop.sstride, fmt=BGRA, cropped=True)
        c, _, _ = src_state(hip, b)
        assert_same(c, a, "cropped against whole-picture mode")
        blocks = {(s, f): i420_bytes(cut(whole.img[s, f], *rect), BGRA, BT601, 0) for s in range(S) for f in range(F)}
        assert_same(a, expect_src(b, ls, lf, blocks), "whole-picture mode")
    finally:
        b.close()
        whole.free()
        crop.free()


def test_per_frame_positions(gpu, hip):
    """under hints the rect sits where set_dyn_rect_at put it, per stream and
    frame; a frame with x0 = -1 keeps its block; cropped surfaces skip it too"""
    pw, ph, S, F, rw, rh = 128, 64, 2, 3, 3, 2
    pos = {(0, 0): (0, 0), (0, 1): (5, 2), (0, 2): (2, 1), (1, 0): (4, 0), (1, 1): None, (1, 2): (1, 2)}
    sf = Surfaces(hip, S, F, pw, ph, 4 * pw + 16, seed=9)
    b = make_batch(gpu, S, F, pw, ph, (1, 1, rw, rh))
    try:
        b.set_hints(0, 0, [], gpu.SCROLL_HINT_EXACT)
        for (s, f), p in pos.items():
            b.set_dyn_rect_at(s, f, *(p if p else (-1, -1)))
        for nfr in (F, 2):                  # the table is compact: its row length follows nframes
            src_fill(hip, b)
            b.dyn_source_from_surfaces(sf.p, nfr, sf.pitch, sf.fstride, sf.sstride, matrix=BT709)
            got, ls, lf = src_state(hip, b)
            blocks = {(s, f): i420_bytes(cut(sf.img[s, f], *p, rw, rh), RGBA, BT709, 0) for (s, f), p in pos.items()
                      if p and f < nfr}
            assert_same(got, expect_src(b, ls, lf, blocks), f"per-frame positions, {nfr} frames")
        src_fill(hip, b)
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride, cropped=True)
        got, ls, lf = src_state(hip, b)
        blocks = {(s, f): i420_bytes(cut(sf.img[s, f], 0, 0, rw, rh), RGBA, BT601, 0) for (s, f), p in pos.items() if p}
        assert_same(got, expect_src(b, ls, lf, blocks), "cropped with a frame without the rect")
    finally:
        b.close()
        sf.free()


def test_offsets_beyond_4_gib(gpu, hip):
    """two streams a little over 4 GiB apart in one allocation, only the two
    windows written: stream 1 converts its own pixels"""
    pw, ph, rect = 64, 48, (1, 0, 3, 3)
    pitch, sstride = 4 * pw, (1 << 32) + 65536
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (2, ph, pw, 4), dtype=np.uint8)
    p = hip.alloc(sstride + pitch * ph)
    b = make_batch(gpu, 2, 1, pw, ph, rect)
    try:
        hip.fill(p + 65536, PAD, pitch * ph)       # where a 32-bit stream offset would read
        hip.write(p, img[0])
        hip.write(p + sstride, img[1])
        src_fill(hip, b)
        b.dyn_source_from_surfaces(p, 1, pitch, pitch * ph, sstride)
        got, ls, lf = src_state(hip, b)
        blocks = {(s, 0): i420_bytes(cut(img[s], *rect), RGBA, BT601, 0) for s in range(2)}
        assert_same(got, expect_src(b, ls, lf, blocks), "streams 4 GiB apart")
    finally:
        b.close()
        hip.free(p)


def test_surfaces_to_i420(gpu, hip):
    """whole pictures, padded pitch and picture stride, every variant; bytes
    between the pictures untouched; no dynamic rect needed"""
    w, h, n = 48, 32, 3
    sf = Surfaces(hip, 1, n, w, h, 4 * w + 16, seed=11)
    psz = w * h * 3 // 2
    stride = psz + 64
    out = hip.alloc(n * stride)
    b = gpu.Batch(1, 1, 1 << 20)
    try:
        for fmt, m, full in VARIANTS:
            hip.fill(out, FILL, n * stride)
            b.surfaces_to_i420(n, w, h, sf.p, sf.pitch, sf.fstride, out, stride, fmt=fmt, matrix=m,
                               full_range=bool(full))
            got = hip.read(out, n * stride)
            want = np.full(n * stride, FILL, np.uint8)
            for i in range(n):
                want[i * stride:i * stride + psz] = np.frombuffer(i420_bytes(sf.img[0, i], fmt, m, full), np.uint8)
            assert_same(got, want, f"surfaces_to_i420 {(fmt, m, full)}")
    finally:
        b.close()
        sf.free()
        hip.free(out)


def test_fallback_frames_without_the_rect(gpu, hip):
    """with scroll_batch_set_fallback on, a frame without the rect keeps a
    dormant whole-picture region that is coded from its source block when its
    hints are inconsistent: such frames get their pixels too (converted at
    (0, 0)), whole-picture and cropped; the compose equals one fed by
    set_dyn_source, and the frames that fell back are the ones expected"""
    pw, ph, S, F = 64, 48, 2, 4
    rect, v = (0, 0, pw // 16, ph // 16), (BGRA, BT601, 1)
    bad = [(0, 0, 2, 2, 2 + 6, 16, -32)]            # waypoint 6: a reference no frame here has
    good = [(0, 0, 4, 1, 0, 0, 0)]
    #            placed  hints     falls back
    plan = {(0, 0): (True, good), (0, 1): (False, bad), (0, 2): (False, good), (0, 3): (True, bad),
            (1, 0): (False, bad), (1, 1): (True, []), (1, 2): (True, bad), (1, 3): (False, [])}
    fell = {k for k, (_, rects) in plan.items() if rects is bad}
    R = random_refs(pw, ph, 18)
    offs = np.array([[3, 17, 30, 48], [44, 20, 9, 0]], np.int32)
    sf = Surfaces(hip, S, F, pw, ph, 4 * pw + 16, seed=18)
    blocks = {(s, f): i420_bytes(sf.img[s, f], *v) for s in range(S) for f in range(F)}
    src = b"".join(blocks[(s, f)] for s in range(S) for f in range(F))
    outs = []
    try:
        for feed in ("surfaces", "cropped", "host"):
            b = make_batch(gpu, S, F, pw, ph, rect, arena=4 << 20)
            b.set_dyn_refs(R.i420(0), R.i420(1))
            b.set_fallback(True)
            for (s, f), (placed, rects) in plan.items():
                b.set_hints(s, f, rects, gpu.SCROLL_HINT_SPEC)
                b.set_dyn_rect_at(s, f, *((0, 0) if placed else (-1, -1)))
            b.set_offsets(offs)
            if feed == "host":
                b.set_dyn_source(src, F)
            else:
                src_fill(hip, b)
                b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride, fmt=v[0], matrix=v[1],
                                           full_range=True, cropped=feed == "cropped")
                got, ls, lf = src_state(hip, b)
                assert_same(got, expect_src(b, ls, lf, blocks), f"fallback on, {feed}: every frame converted")
            b.compose(F)
            assert b.sync() == 0, gpu.last_error()
            assert {(s, f) for s in range(S) for f in range(F) if b.fallback_frame(s, f)} == fell
            outs.append([b.output(s) for s in range(S)])
            if feed == "surfaces":
                # without the fallback the same frames keep their bytes
                b.set_fallback(False)
                src_fill(hip, b)
                b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride, fmt=v[0], matrix=v[1],
                                           full_range=True)
                got, ls, lf = src_state(hip, b)
                kept = {k: d for k, d in blocks.items() if plan[k][0]}
                assert_same(got, expect_src(b, ls, lf, kept), "fallback off: frames without the rect skipped")
            b.close()
        assert outs[0] == outs[2], "composed bytes differ from the host-fed batch's"
        assert outs[1] == outs[2], "cropped: composed bytes differ from the host-fed batch's"
        assert all(len(o) > 0 for o in outs[2])
    finally:
        sf.free()


def planes_of(img, v):
    return tuple(convert(img, *v))


def test_compose_equals_host_fed_source(gpu, hip, oracle):
    """a compose after dyn_source_from_surfaces against a second batch fed
    set_dyn_source(numpy-converted): the same bytes, reconstruction and SSE"""
    pw, ph, S, F, rect = 96, 96, 2, 3, (1, 1, 4, 4)
    v = (BGRA, BT709, 0)
    R = random_refs(pw, ph, 12)
    offs = np.array([[0, 5, 40], [96, 41, 6]], np.int32)
    sf = Surfaces(hip, S, F, pw, ph, 4 * pw + 16, seed=12)
    src = b"".join(i420_bytes(cut(sf.img[s, f], *rect), *v) for s in range(S) for f in range(F))
    outs = []
    try:
        for from_surfaces in (True, False):
            b = make_batch(gpu, S, F, pw, ph, rect, arena=8 << 20)
            b.set_dyn_refs(R.i420(0), R.i420(1))
            b.set_dyn_recon()
            b.set_offsets(offs)
            if from_surfaces:
                b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride, fmt=v[0], matrix=v[1])
            else:
                b.set_dyn_source(src, F)
            b.compose(F)
            assert b.sync() == 0, gpu.last_error()
            outs.append(([b.output(s) for s in range(S)],
                         [(b.dyn_recon(s, f), b.dyn_sse(s, f)) for s in range(S) for f in range(F)]))
            b.close()
        assert outs[0][0] == outs[1][0], "composed bytes differ"
        assert outs[0][1] == outs[1][1], "reconstruction or SSE differ"
        assert all(len(o) > 0 for o in outs[0][0])
    finally:
        sf.free()


def test_end_to_end_without_a_host_step(gpu, hip, oracle):
    """64x48: RGBA pictures A, B -> surfaces_to_i420 -> ipcm_files_device ->
    ingest_device; the same I420 -> set_dyn_refs_device; per-frame surfaces ->
    dyn_source_from_surfaces -> compose.  The streams are the oracle's on the
    numpy-converted inputs"""
    w, h, S, F, rect = 64, 48, 2, 4, (1, 1, 2, 1)
    v = (RGBA, BT601, 0)
    ab = Surfaces(hip, 1, 2, w, h, 4 * w + 16, seed=13)
    fr = Surfaces(hip, S, F, w, h, seed=14)
    psz = w * h * 3 // 2
    pstride = (psz + 255) // 256 * 256
    ostride = 2 * pstride + 4096
    d_pics, d_files = hip.alloc(2 * pstride), hip.alloc(2 * ostride)
    offs = np.array([[3, 17, 30, 48], [44, 20, 9, 0]], np.int32)
    b = gpu.Batch(S, F, 4 << 20)
    try:
        b.surfaces_to_i420(2, w, h, ab.p, ab.pitch, ab.fstride, d_pics, pstride)
        sizes = b.ipcm_files_device(2, w, h, d_pics, pstride, d_files, ostride)
        assert b.ingest_device(S, d_files, [0, sizes[0], ostride, sizes[1]] * S) == 0
        b.set_dyn_rect(*rect)
        b.set_dyn_refs_device(d_pics, d_pics + pstride)
        b.dyn_source_from_surfaces(fr.p, F, fr.pitch, fr.fstride, fr.sstride)
        c = b.config(0)
        assert (c.frame_num, c.log2_max_frame_num, c.pic_order_cnt_type, c.deblocking_filter_control_present_flag) == \
            (2, 4, 2, 1)                                    # what oracle_frames composes with
        b.set_offsets(offs)
        b.compose(F)
        assert b.sync() == 0, gpu.last_error()
        pics = [i420_bytes(ab.img[0, k], *v) for k in range(2)]
        files = [ipcm_file(oracle, w, h, p) for p in pics]
        cap = 2 * (len(files[0]) + len(files[1])) + 65536
        buf = (ctypes.c_uint8 * cap)()
        n = oracle.or_composer_run(buf, cap, files[0], len(files[0]), files[1], len(files[1]), 0, 1)
        assert n
        R = ArrayRefs([planes_of(ab.img[0, k], v) for k in range(2)])
        for s in range(S):
            srcs = [np.frombuffer(i420_bytes(cut(fr.img[s, f], *rect), *v), np.uint8) for f in range(F)]
            want = bytes(buf[:n]) + oracle_frames(oracle, w, h, offs[s], rect, srcs, R)[0]
            assert b.output(s) == want, f"stream {s}"
    finally:
        b.close()
        ab.free()
        fr.free()
        hip.free(d_pics)
        hip.free(d_files)


def test_set_dyn_refs_device(gpu, hip, oracle):
    """the same composed bytes as set_dyn_refs on the same pictures: shared,
    then one stream with a pair of its own"""
    pw, ph, S, F, rect = 96, 96, 3, 2, (1, 1, 4, 4)
    R, R2 = random_refs(pw, ph, 15), random_refs(pw, ph, 16)
    psz = pw * ph * 3 // 2
    d = hip.alloc(4 * psz)
    for k, pic in enumerate((R.i420(0), R.i420(1), R2.i420(0), R2.i420(1))):
        hip.write(d + k * psz, pic)
    offs = np.array([[5, 40], [41, 6], [96, 0]], np.int32)
    outs = []
    try:
        for device in (False, True):
            b = make_batch(gpu, S, F, pw, ph, rect, arena=8 << 20)
            b.set_offsets(offs)
            got = []
            for per_stream in (False, True):
                if device:
                    b.set_dyn_refs_device(d + 2 * psz * per_stream, d + 2 * psz * per_stream + psz,
                                          stream=1 if per_stream else -1)
                else:
                    Rk = R2 if per_stream else R
                    b.set_dyn_refs(Rk.i420(0), Rk.i420(1), stream=1 if per_stream else -1)
                b.dyn_source_synth(F)
                b.compose(F, rewind=True)
                assert b.sync() == 0, gpu.last_error()
                got.append([b.output(s) for s in range(S)])
            outs.append(got)
            b.close()
        assert outs[0] == outs[1]
        # the shared pair is what the oracle predicts from
        want = oracle_frames(oracle, pw, ph, offs[0], rect,
                             [np.frombuffer(bytes(src_of(oracle, 0, t, rect)), np.uint8) for t in range(F)], R)[0]
        assert outs[1][0][0] == want
    finally:
        hip.free(d)


def src_of(oracle, s, t, rect):
    from dynhelp import rect_source
    return rect_source(oracle, s, t, Rect(*rect, 0))


def test_contract(gpu, hip, scroll):
    """every refusal returns its code, leaves the source buffer as it was and
    the batch usable; surface_ms is -1 without timing, positive with it"""
    pw, ph, S, F, rect = 64, 48, 2, 2, (1, 1, 2, 2)
    sf = Surfaces(hip, S, F, pw, ph, 4 * pw + 16, seed=17)
    lib, ARG, CONFIG = scroll.lib, scroll.SCROLL_ERR_ARG, scroll.SCROLL_ERR_CONFIG

    def call(b, nframes, **kw):
        a = dict(base=sf.p, pitch=sf.pitch, frame_stride=sf.fstride, stream_stride=sf.sstride, format=RGBA,
                 matrix=BT601, full_range=0, cropped=0)
        a.update(kw)
        s = scroll.ScrollSurfaces(**a)
        return lib.scroll_batch_dyn_source_from_surfaces(b.h, nframes, ctypes.byref(s), None)

    b = make_batch(gpu, S, F, pw, ph)
    try:
        assert call(b, F) == CONFIG                          # no dynamic rect
        assert b.surface_ms() == -1.0
        b.set_dyn_rect(*rect)
        src_fill(hip, b)
        before, _, _ = src_state(hip, b)
        bad = [dict(base=sf.p + 4), dict(pitch=sf.pitch + 8), dict(pitch=4 * pw - 16), dict(pitch=4 * 16 * rect[2]),
               dict(frame_stride=sf.fstride + 4), dict(stream_stride=sf.sstride + 8), dict(format=2), dict(matrix=2),
               dict(full_range=2), dict(cropped=2), dict(base=None)]
        for kw in bad:
            assert call(b, F, **kw) == ARG, kw
            assert scroll.last_error()
        assert call(b, -1) == ARG and call(b, F + 1) == ARG
        assert lib.scroll_batch_dyn_source_from_surfaces(b.h, F, None, None) == ARG
        # cropped surfaces may be as narrow as the rect
        assert call(b, 0, pitch=4 * 16 * rect[2], cropped=1) == 0
        after, _, _ = src_state(hip, b)
        assert_same(after, before, "a refused call wrote to the source")
        d = hip.alloc(4096 + 64)
        s = scroll.ScrollSurfaces(sf.p, sf.pitch, sf.fstride, 0, RGBA, BT601, 0, 0)
        for n, w, h, dp, st in ((1, 24, 16, d, 4096), (1, 16, 8, d, 4096), (-1, 16, 16, d, 4096), (1, 16, 16, d + 8, 4096),
                                (2, 16, 16, d, 4088), (2, 16, 16, d, 256), (1, 16, 16, None, 4096),
                                (1, pw + 16, 16, d, 4096)):
            assert lib.scroll_batch_surfaces_to_i420(b.h, n, w, h, ctypes.byref(s), dp, st, None) == ARG, (n, w, h)
        hip.free(d)
        assert b.surface_ms() == -1.0
        b.enable_timing()
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride)
        ms = b.surface_ms()
        assert ms > 0.0, ms
        got, ls, lf = src_state(hip, b)
        blocks = {(s_, f): i420_bytes(cut(sf.img[s_, f], *rect), RGBA, BT601, 0) for s_ in range(S) for f in range(F)}
        assert_same(got, expect_src(b, ls, lf, blocks), "the batch after the refusals")
        b.enable_timing(False)
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride)
        assert b.surface_ms() == -1.0
    finally:
        b.close()
        sf.free()
