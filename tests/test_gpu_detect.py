"""GPU check of scroll_batch_detect_offsets (k_det_refs, k_det_surf,
k_det_score, k_det_pick): each frame's scroll offset found from renderer
surfaces and the stacked reference pictures.  Scores and records are compared
integer for integer with the numpy restatement of tests/detecthelp.py, which
tests/test_detect_hostsim.py pins (and where the designed cases' premise --
the helper alone finds the truth -- is asserted); and the offsets applied on
the device: detect -> locate -> dyn_source_from_surfaces -> compose from
perturbed estimates against a second batch given the true offsets.  A surface
that must agree with the references exactly is grey (R = G = B = v) in full
range, where its luma is v.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from cschelp import BGRA, BT601, BT709, RGBA, VARIANTS, luma_np, rgb_of
from damagehelp import Hip, Surfaces
from detecthelp import DETECT_DTYPE, EDGE_F, EDGE_H, EDGE_RADII, EDGE_S, EDGE_W, FOUND, GREY, LOW, NO_SCORE, TIED, \
    detect_np, edge_case, estimates, expect, flat_luma, i420, noise_luma, painted, record_tuple, scroll_surface, \
    sig_rows, sig_surface, stacked, width_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


@pytest.fixture(scope="module")
def hip(gpu):
    return Hip()


def make(gpu, w, h, ns, nf, lumas, rect=(0, 0, 2, 2), mode=0, moving=False, recon=False, arena=8 << 20):
    """a batch of ns w x h streams with the dynamic rect and the references: lumas one (A, B) pair (shared) or one per stream"""
    b = gpu.Batch(ns, nf, arena, mode=mode)
    for _ in range(ns):
        b.add_stream(gpu.make_config(w, h))
    b.set_dyn_rect(*rect)
    if len(lumas) == 1:
        b.set_dyn_refs(i420(lumas[0][0]), i420(lumas[0][1]))
    else:
        for s, (ya, yb) in enumerate(lumas):
            b.set_dyn_refs(i420(ya), i420(yb), stream=s)
    if recon:
        b.set_dyn_recon()
    if moving:
        b.set_dyn_rect_moving()
    return b


def detect(b, sf, nframes, v=GREY, **kw):
    b.detect_offsets(sf.p, nframes, *sf.args(), fmt=v[0], matrix=v[1], full_range=bool(v[2]), **kw)


def offsets(b, hip, ns, nf):
    """the device's offsets, [ns][max_frames] of the batch"""
    return hip.read(b.offsets_device_ptr(), 4 * ns * nf).view(np.int32).reshape(ns, nf).copy()


def check(b, nframes, recs, scores):
    got = b.detect_result(nframes)
    for s in range(len(recs)):
        for f in range(nframes):
            sc = b.detect_scores(s, f)
            if not np.array_equal(sc, scores[s, f]):
                o = int(np.argwhere(sc != scores[s, f])[0][0])
                raise AssertionError(f"scores of stream {s} frame {f}: offset {o} has {sc[o]}, not {scores[s, f][o]}")
            assert record_tuple(got[s, f]) == record_tuple(recs[s][f]), (s, f)


@pytest.fixture(scope="module")
def edges():
    return {shared: edge_case(shared) for shared in (False, True)}


@pytest.mark.parametrize("shared", [False, True])
def test_edge_offsets_patterns_centres_and_radii(gpu, hip, edges, shared):
    """96x368: two segments, the second 32 wide; radius 400 searches 369
    candidates, more than one workgroup's 256.  Per-stream references (stream
    1 tiled: a scores curve with many partial agreements) and a shared pair"""
    lumas, img, truth = edges[shared]
    sf = Surfaces(hip, img)
    b = make(gpu, EDGE_W, EDGE_H, EDGE_S, EDGE_F, lumas)
    try:
        for radius in EDGE_RADII:
            est = estimates(truth, radius)
            b.set_offsets(est)
            detect(b, sf, EDGE_F, radius=radius, min_match=EDGE_H * 2 // 4, apply=False)
            recs, scores = expect(lumas, img, est, radius=radius, min_match=EDGE_H * 2 // 4)
            check(b, EDGE_F, recs, scores)
            assert [[r["off"] for r in row] for row in recs] == truth.tolist()
            if radius == 400:
                assert (scores != NO_SCORE).all()
                if not shared:                          # the tiled stream: not two-valued
                    assert len(np.unique(scores[1, 0])) > 8
    finally:
        b.close()
        sf.free()


@pytest.mark.parametrize("pw,ph", [(272, 48), (320, 240)])
def test_partial_segment_widths_and_seg_step(gpu, hip, pw, ph):
    """four segments and a 16-wide one, and five full ones; every seg_step of 1, 2, 3; a padded pitch"""
    lumas, img, truth = width_case(pw, ph)
    sf = Surfaces(hip, img, 4 * pw + 32)
    b = make(gpu, pw, ph, 2, 2, lumas)
    try:
        est = estimates(truth, ph)
        b.set_offsets(est)
        for seg_step in (1, 2, 3):
            detect(b, sf, 2, radius=ph, seg_step=seg_step, min_match=ph, apply=False)
            recs, scores = expect(lumas, img, est, radius=ph, seg_step=seg_step, min_match=ph)
            check(b, 2, recs, scores)
            assert recs[0][0]["n_sig"] == ph * len(range(0, 5, seg_step))
    finally:
        b.close()
        sf.free()


def test_flat_references_tie_and_keep_the_offsets(gpu, hip):
    pw, ph = 96, 48
    lumas = [flat_luma(pw, ph)]
    rng = np.random.default_rng(71)
    img = np.stack([np.stack([scroll_surface(stacked(*lumas[0]), 5, ph, rng) for _ in range(3)]) for _ in range(2)])
    sf = Surfaces(hip, img)
    b = make(gpu, pw, ph, 2, 3, lumas)
    try:
        est = np.array([[0, 7, 48], [20, 21, 22]], np.int32)
        b.set_offsets(est)
        detect(b, sf, 3, radius=6, apply=True)
        recs, scores = expect(lumas, img, est, radius=6)
        check(b, 3, recs, scores)
        assert all(r["status"] == TIED and r["score"] == r["second"] == 2 * ph for row in recs for r in row)
        assert np.array_equal(offsets(b, hip, 2, 3), est), "a TIED frame's offset was written"
    finally:
        b.close()
        sf.free()


def test_noise_surfaces_are_low(gpu, hip):
    pw, ph = 128, 64
    rng = np.random.default_rng(72)
    lumas = [noise_luma(pw, ph, rng)]
    img = rng.integers(0, 256, (2, 2, ph, pw, 4), dtype=np.uint8)
    sf = Surfaces(hip, img)
    b = make(gpu, pw, ph, 2, 2, lumas)
    try:
        est = np.array([[0, 30], [64, 11]], np.int32)
        b.set_offsets(est)
        v = (BGRA, BT709, 0)
        detect(b, sf, 2, v, radius=ph, min_match=ph * 2 // 2, apply=True)
        recs, scores = expect(lumas, img, est, v, radius=ph, min_match=ph * 2 // 2)
        check(b, 2, recs, scores)
        assert all(r["status"] == LOW for row in recs for r in row)
        assert np.array_equal(offsets(b, hip, 2, 2), est), "a LOW frame's offset was written"
    finally:
        b.close()
        sf.free()


def test_every_variant_with_references_converted_from_surfaces(gpu, hip):
    """references made by surfaces_to_i420 from coloured surfaces under the
    same rule; the frames show rows of those surfaces"""
    pw, ph = 128, 48
    rng = np.random.default_rng(73)
    col = rng.integers(0, 256, (2, ph, pw, 4), dtype=np.uint8)            # A and B as surfaces
    stack = col.reshape(2 * ph, pw, 4)
    truth = np.array([[0, 17, 48]], np.int32)
    img = np.stack([np.stack([stack[o:o + ph] for o in truth[0]])])
    img[..., 3] = rng.integers(0, 256, img.shape[:-1])                    # alpha is ignored
    ref_sf = Surfaces(hip, col[None])
    sf = Surfaces(hip, img)
    pic = 3 * pw * ph // 2
    d_pics = hip.alloc(2 * pic)
    b = make(gpu, pw, ph, 1, 3, [noise_luma(pw, ph, rng)])
    try:
        est = truth + np.array([[3, -3, -2]], np.int32)
        b.set_offsets(est)
        for v in VARIANTS:
            b.surfaces_to_i420(2, pw, ph, ref_sf.p, ref_sf.pitch, ref_sf.fstride, d_pics, pic, fmt=v[0], matrix=v[1],
                               full_range=bool(v[2]))
            assert b.sync() == 0
            b.set_dyn_refs_device(d_pics, d_pics + pic)
            detect(b, sf, 3, v, radius=4, apply=False)
            ya, yb = (luma_np(*rgb_of(col[k], v[0]), v[1], v[2]).astype(np.uint8) for k in (0, 1))
            recs, scores = expect([(ya, yb)], img, est, v, radius=4)
            check(b, 3, recs, scores)
            assert [r["off"] for r in recs[0]] == truth[0].tolist(), v
            assert all(r["status"] == FOUND and r["score"] == 2 * ph for r in recs[0])
    finally:
        b.close()
        sf.free()
        ref_sf.free()
        hip.free(d_pics)


def test_padded_strides_and_shared_surfaces(gpu, hip):
    pw, ph = 96, 48
    rng = np.random.default_rng(74)
    lumas = [noise_luma(pw, ph, rng), noise_luma(pw, ph, rng)]
    truth = np.array([[4, 40], [48, 9]], np.int32)
    img = np.stack([np.stack([scroll_surface(stacked(*lumas[s]), int(truth[s, f]), ph, rng) for f in range(2)])
                    for s in range(2)])
    pitch = 4 * pw + 48
    fstride = pitch * ph + 160
    sf = Surfaces(hip, img, pitch, fstride, 2 * fstride + 4096)
    sh = Surfaces(hip, img[:1], pitch, shared=True)
    b = make(gpu, pw, ph, 2, 2, lumas)
    try:
        est = truth + 2
        b.set_offsets(est)
        detect(b, sf, 2, radius=3, apply=False)
        recs, scores = expect(lumas, img, est, radius=3)
        check(b, 2, recs, scores)
        assert [[r["off"] for r in row] for row in recs] == truth.tolist()
        # stream_stride 0: both streams read stream 0's surfaces, each against its own references
        detect(b, sh, 2, radius=3, min_match=ph, apply=False)
        recs, scores = expect(lumas, img[:1], est, radius=3, min_match=ph)
        check(b, 2, recs, scores)
        assert [r["status"] for r in recs[0]] == [FOUND, FOUND] and [r["status"] for r in recs[1]] == [LOW, LOW]
        # fewer frames than the batch holds: frame 1 keeps the last call's record and scores
        detect(b, sf, 1, radius=3, apply=False)
        r1, s1 = expect(lumas, img, est, radius=3)
        check(b, 1, r1, s1)
        got = np.frombuffer(hip.read(b.detect_device()[0], 4 * 32).tobytes(), DETECT_DTYPE).reshape(2, 2)
        assert record_tuple(got[1, 1]) == record_tuple(recs[1][1])
    finally:
        b.close()
        sf.free()
        sh.free()


def test_config3_shape_at_full_radius(gpu, hip):
    """one 1280x720 stream x 2 frames, a 360 x 360 pixel region repainted, every offset searched"""
    pw, ph = 1280, 720
    rng = np.random.default_rng(75)
    lumas = [noise_luma(pw, ph, rng)]
    truth = np.array([[100, 701]], np.int32)
    st = stacked(*lumas[0])
    img = np.stack([np.stack([scroll_surface(st, int(o), ph, rng) for o in truth[0]])])
    reg = img[0, :, 160:520, 448:808, :3]
    reg[:] = (reg.astype(np.int64) + rng.integers(64, 192, reg.shape)) % 256
    sf = Surfaces(hip, img)
    b = make(gpu, pw, ph, 1, 2, lumas, rect=(0, 0, 25, 25), arena=16 << 20)
    try:
        est = np.array([[0, 720]], np.int32)
        b.set_offsets(est)
        detect(b, sf, 2, radius=ph, min_match=ph * 20 // 2, apply=False)
        recs, scores = expect(lumas, img, est, radius=ph, min_match=ph * 20 // 2)
        check(b, 2, recs, scores)
        for f in range(2):
            r = recs[0][f]
            assert r["status"] == FOUND and r["off"] == truth[0, f] and r["n_sig"] == 720 * 20
            # segments 7 .. 12 of 360 rows do not vote (but for a repainted run that keeps its sum by chance)
            assert 0 <= r["score"] - (720 * 20 - 360 * 6) < 20
    finally:
        b.close()
        sf.free()


def test_4k_tiles_over_rows(gpu, hip):
    """3840x2160: 60 segments x 4320 stacked rows of signatures, far more than the LDS holds"""
    pw, ph = 3840, 2160
    rng = np.random.default_rng(76)
    lumas = [noise_luma(pw, ph, rng)]
    img = scroll_surface(stacked(*lumas[0]), 1234, ph, rng, painted("2x2", pw, ph))[None, None]
    sf = Surfaces(hip, img)
    b = make(gpu, pw, ph, 1, 1, lumas, arena=16 << 20)
    try:
        est = np.array([[1240]], np.int32)
        b.set_offsets(est)
        detect(b, sf, 1, radius=8, min_match=ph * 60 // 2, apply=True)
        recs, scores = expect(lumas, img, est, radius=8, min_match=ph * 60 // 2)
        check(b, 1, recs, scores)
        assert recs[0][0]["status"] == FOUND and recs[0][0]["off"] == 1234 and recs[0][0]["score"] >= ph * 60 - 32
        assert offsets(b, hip, 1, 1)[0, 0] == 1234
    finally:
        b.close()
        sf.free()


def test_apply_semantics(gpu, hip):
    """apply = 0 leaves the offsets; apply = 1 changes FOUND frames only
    (frame 1 is noise: LOW); entries from nframes on are kept"""
    pw, ph = 96, 48
    rng = np.random.default_rng(77)
    lumas = [noise_luma(pw, ph, rng)]
    truth = [9, None, 30, 41]
    st = stacked(*lumas[0])
    img = np.stack([np.stack([rng.integers(0, 256, (ph, pw, 4), dtype=np.uint8) if o is None else
                              scroll_surface(st, o, ph, rng) for o in truth])])
    sf = Surfaces(hip, img)
    b = make(gpu, pw, ph, 1, 4, lumas)
    try:
        est = np.array([[11, 20, 28, 44]], np.int32)
        b.set_offsets(est)
        detect(b, sf, 4, radius=4, min_match=ph, apply=False)
        assert np.array_equal(offsets(b, hip, 1, 4), est)
        detect(b, sf, 3, radius=4, min_match=ph, apply=True)
        recs, scores = expect(lumas, img[:, :3], est[:, :3], radius=4, min_match=ph)
        check(b, 3, recs, scores)
        assert [r["status"] for r in recs[0]] == [FOUND, LOW, FOUND]
        assert offsets(b, hip, 1, 4).tolist() == [[9, 20, 30, 44]]
        # the next call starts from the applied offsets
        detect(b, sf, 4, radius=4, min_match=ph, apply=True)
        recs, scores = expect(lumas, img, np.array([[9, 20, 30, 44]], np.int32), radius=4, min_match=ph)
        check(b, 4, recs, scores)
        assert offsets(b, hip, 1, 4).tolist() == [[9, 20, 30, 41]]
    finally:
        b.close()
        sf.free()


@pytest.mark.parametrize("mode,hints", [(0, False), (0, True), (1, False)])
def test_detect_reads_no_stream_state(gpu, hip, mode, hints):
    """with UI hints set and in experiment mode the same records"""
    pw, ph = 96, 48
    rng = np.random.default_rng(78)
    lumas = [noise_luma(pw, ph, rng)]
    img = scroll_surface(stacked(*lumas[0]), 13, ph, rng)[None, None]
    sf = Surfaces(hip, img)
    b = make(gpu, pw, ph, 1, 1, lumas, mode=mode)
    try:
        if hints:
            b.set_hints(0, 0, [], gpu.SCROLL_HINT_EXACT)
        est = np.array([[10]], np.int32)
        b.set_offsets(est)
        detect(b, sf, 1, radius=5, apply=False)
        recs, scores = expect(lumas, img, est, radius=5)
        check(b, 1, recs, scores)
        assert recs[0][0]["off"] == 13
    finally:
        b.close()
        sf.free()


def test_end_to_end_against_true_offsets(gpu, hip):
    """detect(apply) -> locate(apply) -> dyn_source_from_surfaces -> compose
    from estimates off by up to 6 against a batch given the true offsets by
    set_offsets: arena bytes, reconstruction and NAL table.  96x1008, offsets
    through 496: the waypoint NAL follows the detected offsets"""
    pw, ph, ns, nf = 96, 1008, 2, 6
    rng = np.random.default_rng(79)
    lumas = [noise_luma(pw, ph, rng)]
    truth = np.array([[470, 480, 490, 500, 510, 520], [3, 200, 495, 496, 497, 1008]], np.int32)
    st = stacked(*lumas[0])
    img = np.stack([np.stack([scroll_surface(st, int(truth[s, f]), ph, rng, [(2, 30), (3, 30), (2, 31), (3, 31)])
                              for f in range(nf)]) for s in range(ns)])
    sf = Surfaces(hip, img)
    est = truth + np.array([[6, -6, 1, -1, 0, 3], [-3, 5, -5, 2, 6, -6]], np.int32)
    recs, _ = expect(lumas, img, est, radius=6, min_match=ph)
    assert [[r["off"] for r in row] for row in recs] == truth.tolist()
    assert all(r["status"] == FOUND for row in recs for r in row)
    a = make(gpu, pw, ph, ns, nf, lumas, rect=(1, 1, 2, 2), moving=True, recon=True)
    c = make(gpu, pw, ph, ns, nf, lumas, rect=(1, 1, 2, 2), moving=True, recon=True)

    def tick(x):
        x.dyn_locate(sf.p, nf, *sf.args(), full_range=True)
        x.dyn_source_from_surfaces(sf.p, nf, *sf.args(), full_range=True)
        x.compose(nf)
        assert x.sync() == 0, gpu.last_error()
        return ([x.output(s) for s in range(ns)], [x.nals(s) for s in range(ns)],
                [x.dyn_recon(s, f) for s in range(ns) for f in range(nf)])

    try:
        a.set_offsets(est)
        detect(a, sf, nf, radius=6, min_match=ph, apply=True)
        got = tick(a)
        c.set_offsets(truth)
        want = tick(c)
        assert got[1] == want[1], "the NAL tables differ"
        assert got[0] == want[0], "composed bytes differ from the batch given the true offsets"
        assert got[2] == want[2], "reconstructions differ"
        assert np.array_equal(offsets(a, hip, ns, nf), truth)
    finally:
        a.close()
        c.close()
        sf.free()


def test_struct_layout(gpu):
    assert ctypes.sizeof(gpu.ScrollOffsetFound) == 32 == DETECT_DTYPE.itemsize
    assert ctypes.sizeof(gpu.ScrollDetect) == 16
    assert [n for n, _ in gpu.ScrollOffsetFound._fields_] == list(DETECT_DTYPE.names)
    assert [getattr(gpu.ScrollOffsetFound, n).offset for n in DETECT_DTYPE.names] == \
        [DETECT_DTYPE.fields[n][1] for n in DETECT_DTYPE.names]


def test_contract(gpu, hip, scroll):
    """every refusal returns its code and leaves records, scores and offsets
    as they were (pre-filled patterns); detect_ms is -1 without timing"""
    pw, ph = 96, 48
    rng = np.random.default_rng(80)
    lumas = [noise_luma(pw, ph, rng)]
    truth = np.array([[5, 6], [7, 8]], np.int32)
    img = np.stack([np.stack([scroll_surface(stacked(*lumas[0]), int(truth[s, f]), ph, rng) for f in range(2)])
                    for s in range(2)])
    sf = Surfaces(hip, img, 4 * pw + 16)
    lib, ARG, CONFIG = scroll.lib, scroll.SCROLL_ERR_ARG, scroll.SCROLL_ERR_CONFIG

    def call(b, nframes, rule=(4, 1, 1, 1), **kw):
        a = dict(base=sf.p, pitch=sf.pitch, frame_stride=sf.fstride, stream_stride=sf.sstride, format=RGBA,
                 matrix=BT601, full_range=1, cropped=0)
        a.update(kw)
        s = scroll.ScrollSurfaces(**a)
        r = scroll.ScrollDetect(*rule)
        return lib.scroll_batch_detect_offsets(b.h, nframes, ctypes.byref(s), ctypes.byref(r), None)

    b = gpu.Batch(2, 2, 4 << 20)
    try:
        for _ in range(2):
            b.add_stream(gpu.make_config(pw, ph))
        assert call(b, 2) == CONFIG                                  # no dynamic rect
        b.set_dyn_rect(1, 1, 2, 1)
        assert call(b, 2) == CONFIG and "reference pictures" in scroll.last_error()
        assert lib.scroll_batch_detect_device(b.h, None) is None     # nothing allocated by a refusal
        assert lib.scroll_batch_detect_scores_device(b.h, None, None) is None
        rec = scroll.ScrollOffsetFound()
        assert lib.scroll_batch_detect_result(b.h, 0, 0, ctypes.byref(rec)) == CONFIG
        assert b.detect_ms() == -1.0
        b.set_dyn_refs(i420(lumas[0][0]), i420(lumas[0][1]))
        est = truth + 1
        b.set_offsets(est)
        assert call(b, 2, (4, 1, 1, 0)) == 0                         # the first call allocates
        recs, scores = expect(lumas, img, est, radius=4)
        check(b, 2, recs, scores)
        assert b.detect_ms() == -1.0
        pr, ls = b.detect_device()
        ps, ss, fs = b.detect_scores_device()
        assert ls == 2 * 32 and fs == 4 * (ph + 1) and ss == 2 * fs
        hip.fill(pr, 0x5A, 2 * ls)
        hip.fill(ps, 0xA5, 2 * ss)
        bad = [dict(base=sf.p + 4), dict(pitch=sf.pitch + 8), dict(pitch=4 * pw - 16), dict(frame_stride=sf.fstride + 4),
               dict(stream_stride=sf.sstride + 8), dict(format=2), dict(matrix=2), dict(full_range=2), dict(cropped=1),
               dict(cropped=2), dict(base=None)]
        for kw in bad:
            assert call(b, 2, **kw) == ARG, kw
            assert scroll.last_error()
        assert call(b, -1) == ARG and call(b, 3) == ARG
        assert call(b, 2, (4, 0, 1, 1)) == ARG and call(b, 2, (4, 3, 1, 1)) == ARG       # seg_step 0, above nseg = 2
        assert call(b, 2, (4, 1, 1, 2)) == ARG                                           # apply
        s0 = scroll.ScrollSurfaces(sf.p, sf.pitch, sf.fstride, sf.sstride, RGBA, BT601, 1, 0)
        assert lib.scroll_batch_detect_offsets(b.h, 2, ctypes.byref(s0), None, None) == ARG
        assert lib.scroll_batch_detect_offsets(b.h, 2, None, ctypes.byref(scroll.ScrollDetect(4, 1, 1, 1)), None) == ARG
        assert call(b, 0) == 0                                       # no frames: nothing to do, nothing written
        assert (hip.read(pr, 2 * ls) == 0x5A).all(), "a refused call wrote to the records"
        assert (hip.read(ps, 2 * ss) == 0xA5).all(), "a refused call wrote to the scores"
        assert np.array_equal(offsets(b, hip, 2, 2), est), "a refused call wrote an offset"
        assert lib.scroll_batch_detect_result(b.h, 0, 2, ctypes.byref(rec)) == ARG
        assert lib.scroll_batch_detect_result(b.h, 2, 0, ctypes.byref(rec)) == ARG
        # the batch after the refusals, timed; seg_step 2 = nseg is the last one accepted
        b.enable_timing()
        assert call(b, 2, (4, 2, 1, 0)) == 0
        recs2, scores2 = expect(lumas, img, est, radius=4, seg_step=2)
        check(b, 2, recs2, scores2)
        assert b.detect_ms() > 0.0 and 0.0 < b.detect_ms(kernel=True) <= b.detect_ms()
        assert 0.0 < b.detect_ms(score=True) <= b.detect_ms()
        b.enable_timing(False)
        assert call(b, 2, (4, 1, 1, 0)) == 0
        assert b.detect_ms() == -1.0
        # set_dyn_rect drops the buffers
        b.set_dyn_rect(0, 0, 2, 1)
        assert lib.scroll_batch_detect_device(b.h, None) is None
        assert lib.scroll_batch_detect_result(b.h, 0, 0, ctypes.byref(rec)) == CONFIG
    finally:
        b.close()
        sf.free()


def test_pixel_limit(gpu, hip, scroll):
    """65 streams x 64 frames of 3840x2160 are more than 2^35 pixels: refused before anything is read or allocated"""
    pw, ph = 3840, 2160
    ya = np.zeros((ph, pw), np.uint8)
    b = gpu.Batch(65, 64, 1 << 16)
    p = hip.alloc(4 * pw * 16)
    try:
        for _ in range(65):
            b.add_stream(gpu.make_config(pw, ph))
        b.set_dyn_rect(0, 0, 1, 1)
        b.set_dyn_refs(i420(ya), i420(ya))
        s = scroll.ScrollSurfaces(p, 4 * pw, 0, 0, RGBA, BT601, 1, 0)
        r = scroll.ScrollDetect(4, 1, 1, 1)
        assert 65 * 64 * pw * ph > 1 << 35 >= 65 * 63 * pw * ph
        assert scroll.lib.scroll_batch_detect_offsets(b.h, 64, ctypes.byref(s), ctypes.byref(r), None) == \
            scroll.SCROLL_ERR_ARG
        assert "2^35" in scroll.last_error()
        assert scroll.lib.scroll_batch_detect_device(b.h, None) is None
    finally:
        b.close()
        hip.free(p)
