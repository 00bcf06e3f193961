"""GPU check of the plain dynamic rect sized per stream and per frame
(scroll_batch_set_dyn_rect_size_at): every kernel that takes
the frame's origin from the position table takes its size from the same word
-- k_dyn_rows, k_dyn_code_general, k_dyn_row (rows past h_f return at the
head, columns past w_f are no tasks), k_dyn_static / k_dyn_epfix /
k_dyn_gather (more static rows around a shorter rect), k_dyn_recon,
k_dyn_probe (and through it k_dyn_pick), k_dyn_mask_*, k_dyn_synth, k_csc and
k_dyn_place (size = 1).  Bytes against the CPU assembly of
tests/dynsizehelp.py (one or_compose_dyn call per frame with the frame's own
rect; tests/test_dyn_size_oracle.py pins it); reconstruction, probe, mask and
surfaces against the existing helpers run on the frame's own rect.  A sized
frame's source, reconstruction and mask map lie in the sized layout at the
head of the frame's slot; the rest of a slot holds noise here.  Every
comparison is exact.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

import damagehelp
from cschelp import BT601, RGBA, i420_bytes
from damagehelp import FIT, NONE, OVER, damage_map_np, grey_surface, paint, record_tuple, ypred_frames
from dynhelp import Rect, rect_source, split_nals
from dynposhelp import oracle_moving
from dynsizehelp import locate_sized_np, per_rect, sized_stream, sized_streams, table_word
from maskhelp import mask_np, noisy, paint_mbs
from maskhelp import record_tuple as mask_tuple
from probehelp import oracle_probe
from qpfhelp import cost_of, oracle_qp_frames, pick_np
from reconhelp import random_refs, striped_refs
from test_gpu_dyn import check_equal
from test_gpu_mask import preds_of
from test_gpu_surface import Hip, Surfaces, cut

pytestmark = pytest.mark.gpu

EXACT = 0
# 6 x 23 MBs: taller than one static row group (16 rows) plus the rect, so nA changes inside it
W, H, RW, RH = 96, 368, 3, 3
NB = 384 * RW * RH


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


@pytest.fixture(scope="module")
def hip(gpu):
    return Hip()


def batch(gpu, w, h, S, F, rect, R, mode=0, moving=True, recon=False, debug=0, arena=8 << 20):
    b = gpu.Batch(S, F, arena, mode=mode)
    if debug:
        b.set_debug(debug)
    for _ in range(S):
        b.add_stream(gpu.make_config(w, h))
    b.set_dyn_rect(*rect)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon()
    if moving:
        b.set_dyn_rect_moving()
    return b


def place(b, rects, f0=0, F=None):
    """rects[s][f0 + f] = (x0, y0, w_f, h_f) or None -> entry f of stream s"""
    for s, row in enumerate(rects):
        for f, rc in enumerate(row[f0:f0 + F if F else None]):
            b.set_dyn_rect_at(s, f, *(rc[:2] if rc else (-1, -1)))
            if rc:
                b.set_dyn_rect_size_at(s, f, rc[2], rc[3])


def load(b, offs, src):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])


def compose_ok(gpu, b, F):
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()


def noise(seed, S, F, rw=RW, rh=RH):
    return np.random.default_rng(seed).integers(0, 256, (S, F, 384 * rw * rh), dtype=np.uint8)


def ep_bytes(nal):
    return nal.count(b"\x00\x00\x03")


def edge_case():
    """3 streams x 6 frames through the 496 waypoint; sizes 1x1, 3x1, 1x3, 2x2
    and 3x3 mixed per stream and frame; origins (0, 0), (3, 20) and (1, 15 /
    16 / 17) across the static-group seam; frames without a rect mixed in"""
    offs = np.array([[484, 488, 492, 496, 500, 504], [20, 300, 496, 368, 0, 100], [7, 33, 250, 367, 119, 496]],
                    np.int32)
    rects = [[(0, 0, 1, 1), (3, 20, 3, 1), (1, 15, 1, 3), (1, 16, 2, 2), (1, 17, 3, 3), None],
             [(1, 16, 3, 1), None, (0, 0, 3, 3), (3, 20, 1, 1), (1, 15, 2, 2), (1, 17, 1, 3)],
             [(3, 20, 2, 2), (1, 17, 1, 1), (0, 0, 1, 3), None, (1, 16, 3, 3), (1, 15, 3, 1)]]
    return offs, rects


# ---- case 1 ----

@pytest.mark.parametrize("mode", [0, 1])
def test_sizes_edges_and_the_static_group_seam(gpu, oracle, mode):
    offs, rects = edge_case()
    S, F = offs.shape
    R = random_refs(W, H, 3)
    src = noise(4, S, F)
    per = [sized_stream(oracle, W, H, offs[s], rects[s], src[s], R, mode=mode) for s in range(S)]
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, mode=mode)
    place(b, rects)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    check_equal(b, [p[0] for p in per])
    assert mode == 1 or any(len(b.nals(s)) > F for s in range(S))      # waypoint NALs among the scroll NALs
    noframe = set()
    for s in range(S):
        for f in range(F):
            info = b.dyn_frame_info(s, f)
            nals = split_nals(per[s][1][f])
            if rects[s][f] is None:
                assert info is None, (s, f)
            elif info is None:                                 # experiment mode: the waypoint NAL alone
                noframe.add((s, f))
                assert mode == 1 and len(nals) == 1, (s, f)
            else:
                assert info[1] == ep_bytes(nals[-1]), (s, f)
    assert noframe == ({(0, 3), (1, 2), (2, 5)} if mode else set())    # the frames at offset 496
    b.close()


def test_full_size_is_the_moved_rect_and_one_size_is_that_batch(gpu, oracle):
    offs, rects = edge_case()
    S, F = offs.shape
    R = random_refs(W, H, 5)
    src = noise(6, S, F)
    pos = [[None if rc is None else rc[:2] for rc in row] for row in rects]
    # all frames at full size: the parent's moved-rect bytes
    full = [[None if p is None else (*p, RW, RH) for p in row] for row in pos]
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    place(b, full)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    m = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    for s in range(S):
        for f in range(F):
            m.set_dyn_rect_at(s, f, *(pos[s][f] or (-1, -1)))
    load(m, offs, src)
    compose_ok(gpu, m, F)
    check_equal(b, [oracle_moving(oracle, W, H, offs[s], RW, RH, pos[s], src[s], R)[0] for s in range(S)])
    for s in range(S):
        assert b.output(s) == m.output(s), s
    b.close()
    m.close()
    # all frames at 2 x 1: a batch configured with that rect, fed the same sized blocks
    small = [[None if p is None else (*p, 2, 1) for p in row] for row in pos]
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    place(b, small)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    c = batch(gpu, W, H, S, F, (1, 1, 2, 1), R)
    for s in range(S):
        for f in range(F):
            c.set_dyn_rect_at(s, f, *(pos[s][f] or (-1, -1)))
    load(c, offs, np.ascontiguousarray(src[:, :, :384 * 2]))
    compose_ok(gpu, c, F)
    check_equal(b, sized_streams(oracle, W, H, offs, small, src, R))
    for s in range(S):
        assert b.output(s) == c.output(s), s
    b.close()
    c.close()


# ---- case 2 ----

@pytest.mark.parametrize("flags", [("SCROLL_DEBUG_DYN_EPCAP4",), ("SCROLL_DEBUG_DYN_GATHER1", "SCROLL_DEBUG_DYN_EPWIN")])
def test_device_synth_on_striped_references(gpu, oracle, flags):
    """k_dyn_synth writes or_dyn_source's pattern for each frame's own rect;
    on the striped references the NALs hold emulation-prevention bytes
    (asserted on the expectation), kept 4 a frame / through the one-chunk
    gather and the windowed EP path"""
    offs, rects = edge_case()
    S, F = offs.shape
    R = striped_refs(oracle, W, H)
    src = np.zeros((S, F, NB), np.uint8)
    for s in range(S):
        for t in range(F):
            if rects[s][t]:
                v = np.frombuffer(bytes(rect_source(oracle, s, t, Rect(*rects[s][t]))), np.uint8)
                src[s, t, :len(v)] = v
    per = [sized_stream(oracle, W, H, offs[s], rects[s], src[s], R) for s in range(S)]
    debug = 0
    for n in flags:
        debug |= getattr(gpu, n)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, debug=debug)
    place(b, rects)
    b.set_offsets(offs)
    b.dyn_source_synth(F, 0, 0)
    compose_ok(gpu, b, F)
    check_equal(b, [p[0] for p in per])
    eps = 0
    for s in range(S):
        for f in range(F):
            if rects[s][f]:
                want = ep_bytes(split_nals(per[s][1][f])[-1])
                assert b.dyn_frame_info(s, f)[1] == want, (s, f)
                eps += want
    print("EP bytes", eps)
    assert eps > 0
    b.close()


# ---- cases 3 and 4 ----

@pytest.mark.parametrize("w,h,rw,rh,widths", [(320, 240, 17, 5, [1, 5, 16, 17]),
                                               (720, 64, 45, 2, [1, 32, 33, 40, 41, 45])])
def test_row_widths(gpu, oracle, w, h, rw, rh, widths):
    """a 17-MB batch row at widths on both sides of a wave's 16 luma MBs; a
    45-MB batch row (over SCROLL_ROW_WIDE: four tasks a thread, the wide bit
    window of the launch) at widths on both sides of 32 / 40"""
    F = len(widths)
    mbw, mbh = w // 16, h // 16
    rects = [[((3 * i) % (mbw - rw + 1), i % (mbh - rh + 1), wf, 1 + i % rh) for i, wf in enumerate(widths)],
             [(0, mbh - rh, wf, rh) for wf in widths[::-1]]]
    offs = np.array([[(3 + 11 * i) % (h + 1) for i in range(F)], [(h - 5 * i) for i in range(F)]], np.int32)
    R = random_refs(w, h, 9)
    src = noise(10, 2, F, rw, rh)
    b = batch(gpu, w, h, 2, F, (0, 0, rw, rh), R, arena=16 << 20)
    place(b, rects)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    check_equal(b, sized_streams(oracle, w, h, offs, rects, src, R))
    b.close()


# ---- case 5 ----

def qp_case():
    offs = np.array([[20, 496, 500, 131], [368, 2, 250, 99]], np.int32)
    rects = [[(0, 0, 1, 1), (3, 20, 3, 2), (1, 16, 2, 3), (1, 17, 3, 3)], [(0, 1, 2, 2), None, (1, 15, 1, 3), (3, 9, 3, 1)]]
    return offs, rects


def test_per_frame_qps_and_reconstruction(gpu, oracle):
    """QPs 12 and 0 (k_dyn_code_general and k_dyn_row<true, POS>, 16-bit
    levels) beside 30 and 51 (int8) on four sized frames; the decoded rects (in
    the sized layout) and their squared errors against the test decoder"""
    offs, rects = qp_case()
    qps = [[12, 30, 0, 51], [26, 26, 26, 26]]
    S, F = offs.shape
    R = random_refs(W, H, 13)
    src = noise(14, S, F)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    b.set_dyn_qp_frames(qps[0], stream=0)
    place(b, rects)
    load(b, offs, src)
    compose_ok(gpu, b, F)
    check_equal(b, sized_streams(oracle, W, H, offs, rects, src, R, qps=qps))
    for s in range(S):
        frames = per_rect(lambda rc: oracle_qp_frames(oracle, W, H, offs[s], rc,
                                                      np.ascontiguousarray(src[s][:, :384 * rc[2] * rc[3]]), R, qps[s],
                                                      decode=True)[1], rects[s])
        for f, fr in enumerate(frames):
            if fr is None:
                assert b.dyn_recon(s, f) is None and b.dyn_sse(s, f) is None
                continue
            n = 384 * rects[s][f][2] * rects[s][f][3]
            assert b.dyn_recon(s, f)[:n] == fr["rec"], (s, f)
            assert b.dyn_sse(s, f) == fr["sse"], (s, f)
    b.close()


# ---- case 6 ----

def test_probe_and_pick_follow_the_sizes(gpu, oracle):
    offs, rects = qp_case()
    cand = [12, 26, 39]
    S, F = offs.shape
    R = random_refs(W, H, 15)
    src = noise(16, S, F)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    place(b, rects)
    load(b, offs, src)
    res = b.dyn_probe(F, cand)
    for s in range(S):
        for k, qp in enumerate(cand):
            frames = per_rect(lambda rc: oracle_probe(oracle, W, H, offs[s], rc,
                                                      np.ascontiguousarray(src[s][:, :384 * rc[2] * rc[3]]), R, qp)[1],
                              rects[s])
            for f, fr in enumerate(frames):
                got = res[s, f, k]
                if fr is None:
                    assert got["valid"] == 0, (s, f, k)
                    continue
                print(f"stream {s} frame {f} cand {k}: bits {got['bits']} / {fr['bits']}, sse "
                      f"{tuple(int(v) for v in got['sse'])} / {fr['sse']}")
                assert got["valid"] == 1, (s, f, k)
                assert (int(got["bits"]), int(got["nonzero"])) == (fr["bits"], fr["nonzero"]), (s, f, k)
                assert tuple(int(v) for v in got["sse"]) == fr["sse"], (s, f, k)
    cost = cost_of(res, cand)
    budget = int(cost[0, 1].min() + cost[0, 1].max()) // 2
    k, qp, st = b.dyn_pick(F, budget)
    per = [[26] * F for _ in range(S)]
    for s in range(S):
        for f in range(F):
            if rects[s][f] is None:
                assert (k[s, f], qp[s, f], st[s, f]) == (-1, -1, 2), (s, f)
                continue
            wk, wst = pick_np(res[s, f], cand, budget)
            assert (k[s, f], st[s, f]) == (wk, wst), (s, f)
            per[s][f] = cand[wk]
    compose_ok(gpu, b, F)
    check_equal(b, sized_streams(oracle, W, H, offs, rects, src, R, qps=per))
    for s in range(S):
        for f in range(F):
            if rects[s][f] is not None:
                assert b.dyn_sse(s, f) == tuple(int(v) for v in res[s, f, k[s, f]]["sse"]), (s, f)
    b.close()


# ---- case 7 ----

def test_source_from_surfaces_at_sized_frames(gpu, hip, oracle):
    """whole-picture surfaces cropped to 16 w_f x 16 h_f at each frame's origin
    into the sized layout; the rest of the slot keeps what it held"""
    S, F = 2, 3
    rects = [[(0, 0, 1, 1), (3, 20, 3, 2), None], [(1, 16, 2, 3), (1, 17, 3, 3), (0, 1, 1, 3)]]
    offs = np.array([[20, 496, 500], [368, 2, 250]], np.int32)
    R = random_refs(W, H, 17)
    sf = Surfaces(hip, S, F, W, H, seed=18)
    src = noise(19, S, F)
    held = src.copy()
    for s in range(S):
        for f in range(F):
            if rects[s][f]:
                v = np.frombuffer(i420_bytes(cut(sf.img[s, f], *rects[s][f]), RGBA, BT601, 0), np.uint8)
                src[s, f, :len(v)] = v
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    try:
        place(b, rects)
        load(b, offs, held)
        b.dyn_source_from_surfaces(sf.p, F, sf.pitch, sf.fstride, sf.sstride)
        assert b.sync() == 0
        p, ls, lf = b.dyn_source_device()
        got = np.stack([np.stack([hip.read(p + s * ls + f * lf, NB) for f in range(F)]) for s in range(S)])
        assert np.array_equal(got, src)
        compose_ok(gpu, b, F)
        check_equal(b, sized_streams(oracle, W, H, offs, rects, src, R))
    finally:
        b.close()
        sf.free()


# ---- case 8 ----

@pytest.mark.parametrize("grow", [0, 1])
def test_mask_on_sized_frames(gpu, hip, oracle, grow):
    """map, records and doctored source of maskhelp run on each frame's own
    rect (grow dilates inside the sized rect); the composed bytes of the
    doctored source; the sse_drop identity against the reconstruction"""
    S, F = 2, 3
    rects = [[(0, 0, 3, 3), (3, 20, 3, 2), None], [(1, 16, 2, 3), (1, 17, 1, 1), (0, 1, 1, 3)]]
    offs = np.array([[20, 496, 500], [368, 2, 250]], np.int32)
    R = random_refs(W, H, 21)
    preds = preds_of(oracle, W, H, offs, R, lambda s, f: rects[s][f])
    rng = np.random.default_rng(22)
    src = noise(23, S, F)
    for s in range(S):
        for f in range(F):
            if rects[s][f]:
                wf, hf = rects[s][f][2:]
                v = paint_mbs(noisy(preds[s][f], rng, 1), [(wf - 1, 0), (0, hf - 1)][:1 + (s + f) % 2], wf, hf, rng)
                src[s, f, :len(v)] = v
    ty, tc = 600, 300
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    try:
        place(b, rects)
        load(b, offs, src)
        b.dyn_mask(F, ty, tc, grow)
        maps, recs = b.dyn_mask_map(F, RW, RH), b.dyn_mask_result(F)
        p, ls, lf = b.dyn_source_device()
        doctored = src.copy()
        seen = 0
        for s in range(S):
            for f in range(F):
                if rects[s][f] is None:
                    assert recs[s, f]["status"] == 1, (s, f)           # SCROLL_DYN_MASK_NOFRAME
                    continue
                wf, hf = rects[s][f][2:]
                n = 384 * wf * hf
                mk, rec, kept, doc = mask_np(src[s, f, :n], preds[s][f], wf, hf, ty, tc, grow)
                got = maps[s, f].reshape(-1)[:2 * wf * hf].reshape(hf, wf, 2)
                assert np.array_equal(got, mk), (s, f)
                assert mask_tuple(recs[s, f]) == mask_tuple(rec), (s, f)
                doctored[s, f, :n] = doc
                seen += rec["n_changed"]
        assert seen > 0
        got = np.stack([np.stack([hip.read(p + s * ls + f * lf, NB) for f in range(F)]) for s in range(S)])
        assert np.array_equal(got, doctored)
        compose_ok(gpu, b, F)
        check_equal(b, sized_streams(oracle, W, H, offs, rects, doctored, R))
        # dropped MBs decode to their prediction: the frame's error against the
        # ORIGINAL source is the coder's against the doctored one plus sse_drop
        for s in range(S):
            for f in range(F):
                if rects[s][f] is None:
                    continue
                wf, hf = rects[s][f][2:]
                n = 384 * wf * hf
                rec = np.frombuffer(b.dyn_recon(s, f)[:n], np.uint8).astype(np.int64)
                d = (rec - src[s, f, :n].astype(np.int64)) ** 2
                total = (int(d[:256 * wf * hf].sum()), int(d[256 * wf * hf:320 * wf * hf].sum()),
                         int(d[320 * wf * hf:].sum()))
                drop = tuple(int(v) for v in recs[s, f]["sse_drop"])
                assert total == tuple(a + c for a, c in zip(b.dyn_sse(s, f), drop)), (s, f)
    finally:
        b.close()


# ---- case 9 ----

def test_whole_tick_located_and_sized(gpu, hip, oracle):
    """dyn_locate(apply, size) -> dyn_source_from_surfaces -> dyn_mask ->
    dyn_probe -> dyn_pick -> compose on one stream, nothing read back in
    between; the batch rect is the whole 6 x 23 picture and each frame pays
    for the box its damage needs"""
    S, F = 1, 5
    mbw, mbh = W // 16, H // 16
    offs = np.array([[20, 300, 496, 120, 368]], np.int32)
    damage = [[(2, 7)], [(4, 21), (5, 22)], [(0, 0), (5, 22)], [], [(x, y) for y in range(mbh) for x in range(mbw)]]
    R = random_refs(W, H, 25)
    rng = np.random.default_rng(26)
    yps = ypred_frames(oracle, W, H, offs[0], R)
    img = np.stack([np.stack([paint(grey_surface(yps[f], RGBA, rng), damage[f], rng) for f in range(F)])])
    sf = damagehelp.Surfaces(damagehelp.Hip(), img)
    dmaps = [damage_map_np(img[0, f], yps[f], RGBA, BT601, True) for f in range(F)]
    want_rec, rects = zip(*[locate_sized_np(dmaps[f], mbw, mbh, 0, 0) for f in range(F)])
    assert [r["status"] for r in want_rec] == [FIT, FIT, FIT, NONE, FIT]
    # origins stay legal by the batch size, so in a whole-picture batch rect every origin is (0, 0) and a
    # sized rect reaches from there to its box's end
    assert rects[0] == (0, 0, 3, 8) and rects[1] == (0, 0, 6, 23) and rects[2] == (0, 0, 6, 23) and rects[3] is None
    cand = [20, 26, 34]
    b = batch(gpu, W, H, S, F, (0, 0, mbw, mbh), R, recon=True, arena=16 << 20)
    try:
        b.set_offsets(offs)
        b.dyn_locate(sf.p, F, *sf.args(), full_range=True, apply=True, size=True)
        b.dyn_source_from_surfaces(sf.p, F, *sf.args(), full_range=True)
        b.dyn_mask(F, 0, 0, 0)
        lib = gpu.lib
        assert lib.scroll_batch_dyn_probe(b.h, F, (ctypes.c_uint8 * 3)(*cand), 3, None) == 0, gpu.last_error()
        rate = gpu.ScrollDynRate(gpu.SCROLL_DYN_RATE_FRAME, 1 << 30, 0, 0)
        assert lib.scroll_batch_dyn_pick(b.h, F, ctypes.byref(rate), None, None) == 0, gpu.last_error()
        compose_ok(gpu, b, F)
        qp = np.full((S, F), -1, np.int32)
        for f in range(F):
            ka, qa = ctypes.c_int(), ctypes.c_int()
            rc = lib.scroll_batch_dyn_pick_result(b.h, 0, f, ctypes.byref(ka), ctypes.byref(qa))
            assert rc == (2 if rects[f] is None else 0), (f, rc, gpu.last_error())
            qp[0, f] = qa.value
        got = b.dyn_locate_result(F)
        for f in range(F):
            assert record_tuple(got[0, f]) == record_tuple(want_rec[f]), f
        # a generous budget picks the candidate of the smallest error: the lowest QP
        src = np.zeros((S, F, 384 * mbw * mbh), np.uint8)
        for f in range(F):
            if rects[f]:
                v = np.frombuffer(i420_bytes(cut(img[0, f], *rects[f]), RGBA, BT601, 1), np.uint8)
                src[0, f, :len(v)] = v
        preds = preds_of(oracle, W, H, offs, R, lambda s, f: rects[f])
        qps = [[26] * F]
        for f in range(F):
            if rects[f]:
                wf, hf = rects[f][2:]
                n = 384 * wf * hf
                src[0, f, :n] = mask_np(src[0, f, :n], preds[0][f], wf, hf, 0, 0, 0)[3]
                qps[0][f] = int(qp[0, f])
                assert qps[0][f] in cand
        check_equal(b, sized_streams(oracle, W, H, offs, [list(rects)], src, R, qps=qps))
        for f in range(F):
            if rects[f] is None:
                assert b.dyn_recon(0, f) is None
                continue
            fr = oracle_qp_frames(oracle, W, H, offs[0], rects[f],
                                  np.ascontiguousarray(src[0][:, :384 * rects[f][2] * rects[f][3]]), R, qps[0],
                                  decode=True)[1][f]
            assert b.dyn_recon(0, f)[:len(fr["rec"])] == fr["rec"], f
    finally:
        b.close()
        sf.free()


def test_located_sizes_of_two_far_mbs_and_an_over_box(gpu, oracle):
    """batch rect 3 x 3 in the 6 x 23 picture: a 2 x 2 box at (4, 21) (the
    origin clamps to (3, 20)), two far MBs (OVER: the batch size) and one MB;
    records, sse_out outside the sized rect, the table through a read-back"""
    S, F = 1, 3
    mbw, mbh = W // 16, H // 16
    offs = np.array([[20, 300, 120]], np.int32)
    damage = [[(4, 21), (5, 22)], [(0, 0), (5, 22)], [(2, 7)]]
    R = random_refs(W, H, 27)
    rng = np.random.default_rng(28)
    yps = ypred_frames(oracle, W, H, offs[0], R)
    img = np.stack([np.stack([paint(grey_surface(yps[f], RGBA, rng), damage[f], rng) for f in range(F)])])
    sf = damagehelp.Surfaces(damagehelp.Hip(), img)
    dmaps = [damage_map_np(img[0, f], yps[f], RGBA, BT601, True) for f in range(F)]
    want = [locate_sized_np(dmaps[f], RW, RH, 0, 0) for f in range(F)]
    assert [w[0]["status"] for w in want] == [FIT, OVER, FIT]
    assert [w[1] for w in want] == [(3, 20, 3, 3), (0, 0, 3, 3), (2, 7, 1, 1)]
    assert want[1][0]["sse_out"] > 0
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)
    try:
        b.set_offsets(offs)
        b.dyn_locate(sf.p, F, *sf.args(), full_range=True, apply=True, size=True)
        got = b.dyn_locate_result(F)
        for f in range(F):
            assert record_tuple(got[0, f]) == record_tuple(want[f][0]), f
        # the sizes through the host: a source laid out by them composes to the sized bytes
        src = noise(29, S, F)
        b.set_dyn_source(src.tobytes(), F)
        compose_ok(gpu, b, F)
        check_equal(b, sized_streams(oracle, W, H, offs, [[w[1] for w in want]], src, R))
        # size = 0 afterwards: the records of before, the batch size again
        b.dyn_locate(sf.p, F, *sf.args(), full_range=True, apply=True)
        got = b.dyn_locate_result(F)
        for f in range(F):
            assert record_tuple(got[0, f]) == record_tuple(damagehelp.locate_np(dmaps[f], RW, RH, 0, 0)), f
    finally:
        b.close()
        sf.free()


# ---- cases 10 and 11 ----

def test_chunks_and_resets(gpu, oracle):
    """entry f applies to frame f of each compose (2 + 2 frames); clear_hints
    and set_dyn_rect reset sizes together with positions"""
    offs = np.array([[492, 496, 500, 504, 20, 30], [20, 300, 496, 368, 7, 9]], np.int32)
    S = 2
    R = random_refs(W, H, 31)
    src = noise(32, S, 6)
    two = [[(0, 0, 1, 1), (3, 20, 3, 2)], [(1, 16, 2, 3), None]]
    b = batch(gpu, W, H, S, 2, (1, 1, RW, RH), R)
    place(b, two)
    for c in range(2):
        load(b, offs[:, 2 * c:2 * c + 2], src[:, 2 * c:2 * c + 2])
        compose_ok(gpu, b, 2)
    check_equal(b, sized_streams(oracle, W, H, offs[:, :4], [two[s] + two[s] for s in range(S)], src[:, :4], R))
    # hints on with sizes set: refused; clear_hints: the batch's position and size again, the flag still on
    b.set_hints(0, 0, [], EXACT)
    load(b, offs[:, 4:6], src[:, 4:6])
    size = [b.output_size(s) for s in range(S)]
    assert gpu.lib.scroll_batch_compose(b.h, 2, None) == gpu.SCROLL_ERR_CONFIG
    assert "size of its own" in gpu.last_error()
    assert b.sync() == 0 and [b.output_size(s) for s in range(S)] == size
    b.clear_hints()
    b.reset_output()
    for s in range(S):
        b.set_config(s, gpu.make_config(W, H))
    load(b, offs[:, :2], src[:, :2])
    compose_ok(gpu, b, 2)
    check_equal(b, sized_streams(oracle, W, H, offs[:, :2], [[(1, 1, RW, RH)] * 2] * S, src[:, :2], R))
    # sized again, (w, h) restores one entry, then set_dyn_rect: everything reset, the flag gone with the rect
    place(b, two)
    b.set_dyn_rect_size_at(0, 1, RW, RH)
    b.reset_output()
    for s in range(S):
        b.set_config(s, gpu.make_config(W, H))
    load(b, offs[:, :2], src[:, :2])
    compose_ok(gpu, b, 2)
    restored = [[two[0][0], (3, 20, RW, RH)], two[1]]
    check_equal(b, sized_streams(oracle, W, H, offs[:, :2], restored, src[:, :2], R))
    b.set_dyn_rect(3, 9, RW, RH)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    b.reset_output()
    for s in range(S):
        b.set_config(s, gpu.make_config(W, H))
    load(b, offs[:, :2], src[:, :2])
    compose_ok(gpu, b, 2)
    check_equal(b, sized_streams(oracle, W, H, offs[:, :2], [[(3, 9, RW, RH)] * 2] * S, src[:, :2], R))
    assert gpu.lib.scroll_batch_set_dyn_rect_size_at(b.h, 0, 0, 1, 1) == gpu.SCROLL_ERR_CONFIG   # the flag went
    b.close()


# ---- case 12 ----

def test_refusals(gpu, hip, oracle):
    lib = gpu.lib
    R = random_refs(W, H, 33)
    b0 = gpu.Batch(1, 2, 1 << 20)
    b0.add_stream(gpu.make_config(W, H))
    assert lib.scroll_batch_set_dyn_rect_size_at(b0.h, 0, 0, 1, 1) == gpu.SCROLL_ERR_ARG         # no rect
    b0.close()
    offs = np.array([[496, 20]], np.int32)
    src = noise(34, 1, 2)
    b = batch(gpu, W, H, 1, 2, (1, 1, RW, RH), R, moving=False)
    assert lib.scroll_batch_set_dyn_rect_size_at(b.h, 0, 0, 1, 1) == gpu.SCROLL_ERR_CONFIG       # the flag is off
    assert "scroll_batch_set_dyn_rect_moving" in gpu.last_error()
    b.set_dyn_rect_moving()
    for s, f, w, h in [(0, 0, 0, 1), (0, 0, 1, 0), (0, 0, RW + 1, 1), (0, 0, 1, RH + 1), (0, 0, -1, 1), (1, 0, 1, 1),
                       (0, 2, 1, 1), (-1, 0, 1, 1), (0, -1, 1, 1)]:
        assert lib.scroll_batch_set_dyn_rect_size_at(b.h, s, f, w, h) == gpu.SCROLL_ERR_ARG, (s, f, w, h)
    # nothing was set by the refused calls: the batch-sized bytes over pre-filled buffers
    load(b, offs, src)
    compose_ok(gpu, b, 2)
    check_equal(b, sized_streams(oracle, W, H, offs, [[(1, 1, RW, RH)] * 2], src, R))
    # the locate's size word
    sf = Surfaces(hip, 1, 2, W, H, seed=35)
    try:
        for apply, size in [(1, 2), (0, 1)]:
            rule = gpu.ScrollDynLocate(0, 0, apply, size)
            srf = gpu.ScrollSurfaces(sf.p, sf.pitch, sf.fstride, sf.sstride, gpu.SCROLL_SURF_RGBA,
                                     gpu.SCROLL_SURF_BT601, 0, 0)
            assert lib.scroll_batch_dyn_locate(b.h, 2, ctypes.byref(srf), ctypes.byref(rule), None) == \
                gpu.SCROLL_ERR_ARG, (apply, size)
            assert "size" in gpu.last_error()
        # hints with a size set: compose and the hinted probe refuse, nothing committed
        b.set_dyn_rect_size_at(0, 1, 2, 2)
        b.set_hints(0, 0, [], EXACT)
        size = b.output_size(0)
        assert lib.scroll_batch_compose(b.h, 2, None) == gpu.SCROLL_ERR_CONFIG
        assert "size of its own" in gpu.last_error()
        qp = (ctypes.c_uint8 * 1)(26)
        assert lib.scroll_batch_dyn_probe_hinted(b.h, 2, qp, 1, None) == gpu.SCROLL_ERR_CONFIG
        assert "size of its own" in gpu.last_error()
        assert b.sync() == 0 and b.output_size(0) == size
    finally:
        b.close()
        sf.free()


# ---- case 13 ----

def test_destroy_with_a_sized_compose_in_flight(gpu, oracle):
    offs, rects = edge_case()
    S, F = offs.shape
    R = random_refs(W, H, 37)
    b = batch(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    place(b, rects)
    load(b, offs, noise(38, S, F))
    b.compose(F)
    b.close()                                                  # no sync: destroy waits for the launches
    c = batch(gpu, W, H, S, F, (1, 1, RW, RH), R)              # the device is in order afterwards
    place(c, rects)
    src = noise(39, S, F)
    load(c, offs, src)
    compose_ok(gpu, c, F)
    check_equal(c, sized_streams(oracle, W, H, offs, rects, src, R))
    c.close()


# ---- pictures wider than 256 MBs ----

def test_pictures_over_256_mbs_take_no_sizes_and_keep_16_bit_origins(gpu, oracle):
    """257 MBs wide: an origin at x0 = 256 needs the table word's full 16 bits,
    so sizes are refused (SCROLL_ERR_CONFIG) and the moved rect reads its
    entries as it always did -- set from the host, and placed by dyn_locate
    and cropped by dyn_source_from_surfaces at the located entry"""
    w, h, rw, rh = 4112, 64, 1, 2
    S, F = 1, 2
    offs = np.array([[5, 40]], np.int32)
    pos = [[(256, 2), (3, 0)]]
    R = random_refs(w, h, 41)
    src = noise(42, S, F, rw, rh)
    b = batch(gpu, w, h, S, F, (0, 0, rw, rh), R)
    sf = None
    try:
        assert gpu.lib.scroll_batch_set_dyn_rect_size_at(b.h, 0, 0, 1, 1) == gpu.SCROLL_ERR_CONFIG
        assert "256 x 256" in gpu.last_error()
        for f in range(F):
            b.set_dyn_rect_at(0, f, *pos[0][f])
        load(b, offs, src)
        compose_ok(gpu, b, F)
        check_equal(b, [oracle_moving(oracle, w, h, offs[0], rw, rh, pos[0], src[0], R)[0]])
        # located: damage at MB (256, 2) of frame 0 and at (3, 0) and (3, 1) of frame 1
        rng = np.random.default_rng(43)
        yps = ypred_frames(oracle, w, h, offs[0], R)
        damage = [[(256, 2)], [(3, 0), (3, 1)]]
        img = np.stack([np.stack([paint(grey_surface(yps[f], RGBA, rng), damage[f], rng) for f in range(F)])])
        sf = damagehelp.Surfaces(damagehelp.Hip(), img)
        rule = gpu.ScrollDynLocate(0, 0, 1, 1)
        srf = gpu.ScrollSurfaces(sf.p, sf.pitch, sf.fstride, sf.sstride, gpu.SCROLL_SURF_RGBA, gpu.SCROLL_SURF_BT601,
                                 1, 0)
        assert gpu.lib.scroll_batch_dyn_locate(b.h, F, ctypes.byref(srf), ctypes.byref(rule), None) == \
            gpu.SCROLL_ERR_CONFIG
        assert "256 x 256" in gpu.last_error()
        b.reset_output()
        b.set_config(0, gpu.make_config(w, h))
        b.set_offsets(offs)
        b.dyn_locate(sf.p, F, *sf.args(), full_range=True, apply=True)
        b.dyn_source_from_surfaces(sf.p, F, *sf.args(), full_range=True)
        compose_ok(gpu, b, F)
        got = b.dyn_locate_result(F)
        assert [(int(r["x0"]), int(r["y0"]), int(r["status"])) for r in got[0]] == [(256, 2, FIT), (3, 0, FIT)]
        cut_src = np.stack([np.stack([np.frombuffer(i420_bytes(cut(img[0, f], *pos[0][f], rw, rh), RGBA, BT601, 1),
                                                    np.uint8) for f in range(F)])])
        check_equal(b, [oracle_moving(oracle, w, h, offs[0], rw, rh, pos[0], cut_src[0], R)[0]])
    finally:
        b.close()
        if sf:
            sf.free()
