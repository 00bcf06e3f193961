"""GPU check of scroll_batch_dyn_locate (k_dmg_rows, k_dyn_damage,
k_dyn_place): the per-MB damage map between renderer surfaces and the scroll
prediction, the records and the placed positions, integer for integer
against the numpy restatement of tests/damagehelp.py (its Ypred sampled
through the oracle's or_ref_sample; tests/test_damage_hostsim.py pins it
against the test decoder); and the positions applied on the device: locate ->
dyn_source_from_surfaces -> [probe -> pick] -> compose against a second batch
given the helper's positions through set_dyn_rect_at.  A surface that must
match the prediction exactly is grey (R = G = B = v) in full range, where
Ysrc = v; damage is painted over that.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from cschelp import BGRA, BT601, BT709, RGBA, VARIANTS
from damagehelp import DAMAGE_DTYPE, FIT, NOFRAME, NONE, OVER, Hip, Surfaces, damage_map_np, grey_surface, \
    locate_np, paint, position, record_tuple, ypred_frames
from reconhelp import random_refs

pytestmark = pytest.mark.gpu

GREY = (RGBA, BT601, 1)             # the variant under which a grey surface's luma is its grey level
# tests/test_gpu_dyn_pos.py's shape: 6 x 23 MBs, the smallest that reaches every edge and the 496 waypoint
W, H, RW, RH = 96, 368, 2, 2
MBW, MBH = W // 16, H // 16
OFFS = np.array([[484, 488, 492, 496, 500, 504], [20, 300, 496, 368, 0, 100], [7, 33, 250, 367, 119, 496]], np.int32)
S, F = OFFS.shape
# experiment mode: the frame that first reaches 496 writes a waypoint NAL in place of its scroll NAL
NOFRAMES = {(0, 3), (1, 2), (2, 5)}
D = 5                               # the single pixel's luma error
ALL = [(x, y) for y in range(MBH) for x in range(MBW)]
PATTERNS = ["none", "corners", "2x2", "3x1", "far", "whole", "pixel"]
DAMAGE = {"none": [], "corners": [(0, 0), (MBW - 1, 0), (0, MBH - 1), (MBW - 1, MBH - 1)],
          "2x2": [(4, 21), (5, 21), (4, 22), (5, 22)], "3x1": [(1, 9), (2, 9), (3, 9)], "far": [(1, 2), (4, 19)],
          "whole": ALL, "pixel": []}
WANT = {"none": NONE, "corners": OVER, "2x2": FIT, "3x1": OVER, "far": OVER, "whole": OVER, "pixel": FIT}


def pattern_of(s, f):
    return PATTERNS[(s * F + f) % len(PATTERNS)]


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


@pytest.fixture(scope="module")
def hip(gpu):
    return Hip()


def make(gpu, w, h, ns, nf, rect, R, mode=0, moving=True, recon=False, arena=8 << 20):
    b = gpu.Batch(ns, nf, arena, mode=mode)
    for _ in range(ns):
        b.add_stream(gpu.make_config(w, h))
    b.set_dyn_rect(*rect)
    b.set_dyn_refs(R.i420(0), R.i420(1))
    if recon:
        b.set_dyn_recon()
    if moving:
        b.set_dyn_rect_moving()
    return b


def locate(b, sf, nframes, v=GREY, **kw):
    b.dyn_locate(sf.p, nframes, *sf.args(), fmt=v[0], matrix=v[1], full_range=bool(v[2]), **kw)


def source(b, sf, nframes, v=GREY):
    b.dyn_source_from_surfaces(sf.p, nframes, *sf.args(), fmt=v[0], matrix=v[1], full_range=bool(v[2]))


def compose_ok(gpu, b, nframes):
    b.compose(nframes)
    assert b.sync() == 0, gpu.last_error()


def expect(img, yps, v, rw, rh, mb_sse=0, margin=0):
    """(maps [S][F][mbh][mbw], records [S][F]) of the helper; yps[s][f] None: no scroll NAL"""
    ns, nf = len(yps), len(yps[0])
    maps = np.stack([np.stack([damage_map_np(img[s if img.shape[0] > 1 else 0, f], yps[s][f], *v) for f in range(nf)])
                     for s in range(ns)])
    recs = [[locate_np(None if yps[s][f] is None else maps[s, f], rw, rh, mb_sse, margin) for f in range(nf)]
            for s in range(ns)]
    return maps, recs


def check(b, nframes, maps, recs):
    got_m, got_r = b.dyn_damage_map(nframes), b.dyn_locate_result(nframes)
    for s in range(len(recs)):
        for f in range(nframes):
            if not np.array_equal(got_m[s, f], maps[s, f]):
                bad = np.argwhere(got_m[s, f] != maps[s, f])[0]
                raise AssertionError(f"map of stream {s} frame {f}: MB {tuple(bad[::-1])} is "
                                     f"{got_m[s, f][tuple(bad)]}, not {maps[s, f][tuple(bad)]}")
            assert record_tuple(got_r[s, f]) == record_tuple(recs[s][f]), (s, f)


@pytest.fixture(scope="module")
def edge(oracle):
    """per mode: references, every frame's Ypred and the painted surfaces, computed once"""
    R = random_refs(W, H, 41)
    out = {}
    for mode in (0, 1):
        rng = np.random.default_rng(42 + mode)
        yps = [ypred_frames(oracle, W, H, OFFS[s], R, mode) for s in range(S)]
        img = np.empty((S, F, H, W, 4), np.uint8)
        for s in range(S):
            for f in range(F):
                if yps[s][f] is None:
                    img[s, f] = rng.integers(0, 256, (H, W, 4))
                    continue
                img[s, f] = grey_surface(yps[s][f], RGBA, rng)
                name = pattern_of(s, f)
                paint(img[s, f], DAMAGE[name], rng)
                if name == "pixel":             # one pixel of MB (3, 11) off by D
                    v = int(yps[s][f][181, 53])
                    img[s, f, 181, 53, :3] = v + D if v + D <= 255 else v - D
        out[mode] = (R, yps, img)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_map_records_and_positions(gpu, hip, edge, mode):
    """every damage pattern, in composer and experiment mode, at mb_sse 0, D^2 -
    1 and D^2 and with a margin; the NOFRAME frames are the ones named here"""
    R, yps, img = edge[mode]
    none = {(s, f) for s in range(S) for f in range(F) if yps[s][f] is None}
    assert none == (NOFRAMES if mode else set())
    sf = Surfaces(hip, img)
    b = make(gpu, W, H, S, F, (1, 1, RW, RH), R, mode=mode)
    try:
        b.set_offsets(OFFS)
        for mb_sse, margin in [(0, 0), (D * D - 1, 0), (D * D, 0), (0, 2), (0, 4)]:
            locate(b, sf, F, mb_sse=mb_sse, margin=margin)
            maps, recs = expect(img, yps, GREY, RW, RH, mb_sse, margin)
            check(b, F, maps, recs)
            for s in range(S):
                for f in range(F):
                    name, r = pattern_of(s, f), recs[s][f]
                    if (s, f) in none:
                        assert r["status"] == NOFRAME and not maps[s, f].any()
                    elif name == "pixel":
                        assert maps[s, f][11, 3] == D * D and r["sse_all"] == D * D
                        # (grown by a margin, the one MB's box no longer fits the 2 x 2 rect)
                        assert r["status"] == (NONE if mb_sse == D * D else FIT if margin == 0 else OVER)
                        if mb_sse < D * D and margin == 0:
                            assert position(r) == (3, 11) and r["sse_out"] == 0
                    elif margin == 0:
                        assert r["status"] == WANT[name], (s, f, name)
                        assert r["n_mb"] == len(DAMAGE[name])
                        if name == "2x2":
                            assert position(r) == (4, 21) and r["sse_out"] == 0
                        if name in ("3x1", "far", "whole", "corners"):
                            assert r["sse_out"] > 0
    finally:
        b.close()
        sf.free()


@pytest.mark.parametrize("w,h,mbs", [(320, 240, [(15, 7), (16, 7)]), (272, 48, [(16, 0), (0, 2), (15, 1)])])
def test_widths_across_the_span(gpu, hip, oracle, w, h, mbs):
    """20 and 17 MBs per row: a second, partial span of 16 MBs; damage on both sides of the seam"""
    offs = np.array([[3, 130], [h, 77]], np.int32)
    R = random_refs(w, h, 43)
    rng = np.random.default_rng(44)
    yps = [ypred_frames(oracle, w, h, offs[s], R) for s in range(2)]
    img = np.stack([np.stack([paint(grey_surface(yps[s][f], RGBA, rng), mbs if (s + f) % 2 == 0 else mbs[:1], rng)
                              for f in range(2)]) for s in range(2)])
    sf = Surfaces(hip, img, 4 * w + 16)
    b = make(gpu, w, h, 2, 2, (1, 0, 2, 2), R)
    try:
        b.set_offsets(offs)
        locate(b, sf, 2)
        maps, recs = expect(img, yps, GREY, 2, 2)
        check(b, 2, maps, recs)
        assert {(x, y) for y, x in np.argwhere(maps[0, 0] > 0)} == set(mbs)
    finally:
        b.close()
        sf.free()


def test_config3_shape(gpu, hip, oracle):
    """one 1280x720 stream x 2 frames, the 25 x 25 rect, a 360 x 360 pixel
    region changed at MB (28, 10): FIT at (28, 10)"""
    w, h, rw, rh = 1280, 720, 25, 25
    offs = np.array([[100, 100]], np.int32)
    R = random_refs(w, h, 45)
    rng = np.random.default_rng(46)
    yp = ypred_frames(oracle, w, h, offs[0][:1], R)[0]
    yps = [[yp, yp]]                            # the same offset and waypoint table: the same prediction
    img = np.stack([np.stack([grey_surface(yp, RGBA, rng) for _ in range(2)])])
    for f in range(2):
        reg = img[0, f, 160:520, 448:808, :3]
        reg[:] = (reg.astype(np.int64) + rng.integers(64, 192, reg.shape)) % 256
    sf = Surfaces(hip, img)
    b = make(gpu, w, h, 1, 2, (0, 0, rw, rh), R, arena=16 << 20)
    try:
        b.set_offsets(offs)
        locate(b, sf, 2)
        maps, recs = expect(img, yps, GREY, rw, rh)
        check(b, 2, maps, recs)
        for f in range(2):
            assert recs[0][f]["status"] == FIT and position(recs[0][f]) == (28, 10), recs[0][f]
            assert recs[0][f]["n_mb"] == 23 * 23 and recs[0][f]["sse_out"] == 0
    finally:
        b.close()
        sf.free()


@pytest.fixture(scope="module")
def small(oracle):
    """64x48, 2 streams x 2 frames of noise surfaces: every MB damaged, the maps' values matter"""
    w, h = 64, 48
    offs = np.array([[5, 40], [48, 17]], np.int32)
    R = random_refs(w, h, 47)
    yps = [ypred_frames(oracle, w, h, offs[s], R) for s in range(2)]
    img = np.random.default_rng(48).integers(0, 256, (2, 2, h, w, 4), dtype=np.uint8)
    return w, h, offs, R, yps, img


def test_every_variant_padded_strides_and_shared_surfaces(gpu, hip, small):
    w, h, offs, R, yps, img = small
    pitch = 4 * w + 48
    fstride = pitch * h + 160
    sf = Surfaces(hip, img, pitch, fstride, 2 * fstride + 4096)
    sh = Surfaces(hip, img[:1], pitch, shared=True)
    b = make(gpu, w, h, 2, 2, (1, 1, 2, 1), R, moving=False)
    try:
        b.set_offsets(offs)
        for v in VARIANTS:
            locate(b, sf, 2, v, apply=False)
            maps, recs = expect(img, yps, v, 2, 1)
            check(b, 2, maps, recs)
            assert maps.min() > 0
        v = (BGRA, BT709, 0)
        locate(b, sh, 2, v, apply=False, mb_sse=200000)
        maps, recs = expect(img[:1], yps, v, 2, 1, mb_sse=200000)
        check(b, 2, maps, recs)
        # fewer frames than the batch holds: frame 1 keeps the last call's map and record
        locate(b, sf, 1, v, apply=False)
        m2, r2 = expect(img, yps, v, 2, 1)
        check(b, 1, m2, r2)
    finally:
        b.close()
        sf.free()
        sh.free()


def test_offsets_beyond_4_gib(gpu, hip, small):
    """two streams a little over 4 GiB apart in one allocation: stream 1 is compared with its own pixels"""
    w, h, offs, R, yps, img = small
    pitch, sstride = 4 * w, (1 << 32) + 65536
    p = hip.alloc(sstride + pitch * h)
    b = make(gpu, w, h, 2, 1, (1, 1, 2, 1), R, moving=False)
    try:
        hip.fill(p + 65536, 0xFF, pitch * h)        # where a 32-bit stream offset would read
        hip.write(p, img[0, 0])
        hip.write(p + sstride, img[1, 0])
        b.set_offsets(offs[:, :1])
        b.dyn_locate(p, 1, pitch, pitch * h, sstride, apply=False)
        v = (RGBA, BT601, 0)
        maps, recs = expect(img[:, :1], [y[:1] for y in yps], v, 2, 1)
        check(b, 1, maps, recs)
    finally:
        b.close()
        hip.free(p)


def results(b, nframes, recon=True):
    out = [b.output(s) for s in range(b.num_streams)]
    rec = [(b.dyn_frame_info(s, f) is None, b.dyn_recon(s, f) if recon else None, b.dyn_sse(s, f) if recon else None)
           for s in range(b.num_streams) for f in range(nframes)]
    return out, rec


def place(b, pos):
    for s, row in enumerate(pos):
        for f, p in enumerate(row):
            b.set_dyn_rect_at(s, f, *(p if p else (-1, -1)))


def test_apply_end_to_end(gpu, hip, edge):
    """locate -> dyn_source_from_surfaces -> compose on one stream, no host
    step between them, against a batch placed by set_dyn_rect_at at the
    helper's positions: output bytes, reconstruction and SSE; NONE frames carry
    a plain scroll NAL; sse_out is the helper's sum outside the placed rect"""
    R, yps, img = edge[0]
    sf = Surfaces(hip, img)
    maps, recs = expect(img, yps, GREY, RW, RH)
    pos = [[position(r) for r in row] for row in recs]
    assert any(p is None for row in pos for p in row) and (4, 21) in pos[0] + pos[1] + pos[2]
    a = make(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    c = make(gpu, W, H, S, F, (1, 1, RW, RH), R, recon=True)
    try:
        a.set_offsets(OFFS)
        locate(a, sf, F)
        source(a, sf, F)
        compose_ok(gpu, a, F)
        c.set_offsets(OFFS)
        place(c, pos)
        source(c, sf, F)
        compose_ok(gpu, c, F)
        got, want = results(a, F), results(c, F)
        assert got[0] == want[0], "composed bytes differ from the host-placed batch's"
        assert got[1] == want[1], "reconstruction or SSE differ"
        check(a, F, maps, recs)
        for s in range(S):
            for f in range(F):
                none, rec, sse = got[1][s * F + f]
                assert none == (pos[s][f] is None) and (rec is None) == none and (sse is None) == none, (s, f)
                x0, y0 = pos[s][f] or (0, 0)
                inside = 0 if none else int(maps[s, f][y0:y0 + RH, x0:x0 + RW].astype(np.int64).sum())
                assert recs[s][f]["sse_out"] == int(maps[s, f].astype(np.int64).sum()) - inside
        # apply = 0 on the placed batch: another compose of the same frames gives the same bytes
        size = [c.output_size(s) for s in range(S)]
        for x in (a, c):
            x.reset_output()
            for s in range(S):
                x.set_config(s, gpu.make_config(W, H))
        locate(c, sf, F, apply=False, mb_sse=1 << 30)      # (would place nothing)
        source(c, sf, F)
        compose_ok(gpu, c, F)
        assert [c.output_size(s) for s in range(S)] == size and results(c, F)[0] == want[0]
        # locate -> source -> probe -> pick -> compose against the same on the placed batch
        cand = [20, 30, 40]
        picks = []
        for x in (a, c):
            x.reset_output()
            for s in range(S):
                x.set_config(s, gpu.make_config(W, H))
            if x is a:
                locate(x, sf, F)
            source(x, sf, F)
            res = x.dyn_probe(F, cand)
            k, qp, st = x.dyn_pick(F, 4000)
            compose_ok(gpu, x, F)
            picks.append((res.tobytes(), k.tolist(), st.tolist(), results(x, F)))
        assert picks[0] == picks[1]
        valid = np.frombuffer(picks[0][0], res.dtype).reshape(S, F, len(cand))["valid"][:, :, 0]
        assert valid.tolist() == [[int(p is not None) for p in row] for row in pos]
    finally:
        a.close()
        c.close()
        sf.free()


def test_positions_between_host_and_device(gpu, hip, edge):
    """entries from nframes on keep the host's positions; after a locate one
    set_dyn_rect_at changes that frame only; set_dyn_rect and clear_hints
    reset the positions"""
    R, yps, img = edge[0]
    sf = Surfaces(hip, img)
    _, recs = expect(img, yps, GREY, RW, RH)
    pos = [[position(r) for r in row] for row in recs]
    host = [[(0, 1), (2, 16), (4, 21), None, (3, 9), (0, 0)]] * S
    a = make(gpu, W, H, S, F, (1, 1, RW, RH), R)
    c = make(gpu, W, H, S, F, (1, 1, RW, RH), R)

    def restart(x):
        x.reset_output()
        for s in range(S):
            x.set_config(s, gpu.make_config(W, H))

    def run(x):
        x.set_offsets(OFFS)
        source(x, sf, F)
        compose_ok(gpu, x, F)
        return [x.output(s) for s in range(S)]

    try:
        # 1. a locate of 2 of 6 frames over host-set positions
        place(a, host)
        a.set_offsets(OFFS)
        locate(a, sf, 2)
        place(c, [pos[s][:2] + host[s][2:] for s in range(S)])
        assert run(a) == run(c)
        # 2. a locate of all, then one entry set by the host: that frame only
        for x in (a, c):
            restart(x)
        locate(a, sf, F)
        a.set_dyn_rect_at(1, 4, 2, 17)
        mixed = [list(row) for row in pos]
        mixed[1][4] = (2, 17)
        place(c, mixed)
        assert run(a) == run(c)
        # 3. hints turned on after a locate read the located positions; clear_hints resets them
        for x in (a, c):
            restart(x)
        locate(a, sf, F)
        place(c, pos)
        for x in (a, c):
            x.set_hints(0, 0, [], gpu.SCROLL_HINT_EXACT)
        assert run(a) == run(c)
        for x in (a, c):
            x.clear_hints()
            restart(x)
        place(c, [[(1, 1)] * F] * S)
        assert run(a) == run(c)
        # 4. set_dyn_rect after a locate: the new rect's position everywhere, the results gone
        locate(a, sf, F)
        for x in (a, c):
            x.set_dyn_rect(3, 9, RW, RH)
            x.set_dyn_refs(R.i420(0), R.i420(1))
            restart(x)
        assert gpu.lib.scroll_batch_dyn_locate_device(a.h, None) is None
        assert run(a) == run(c)
    finally:
        a.close()
        c.close()
        sf.free()


def test_contract(gpu, hip, small, scroll):
    """every refusal returns its code and leaves results, map and positions as
    they were (pre-filled patterns); locate_ms is -1 without timing"""
    w, h, offs, R, yps, img = small
    sf = Surfaces(hip, img, 4 * w + 16)
    lib, ARG, CONFIG = scroll.lib, scroll.SCROLL_ERR_ARG, scroll.SCROLL_ERR_CONFIG
    v = (RGBA, BT601, 0)

    def call(b, nframes, rule=(0, 0, 0), **kw):
        a = dict(base=sf.p, pitch=sf.pitch, frame_stride=sf.fstride, stream_stride=sf.sstride, format=RGBA,
                 matrix=BT601, full_range=0, cropped=0)
        a.update(kw)
        s = scroll.ScrollSurfaces(**a)
        r = scroll.ScrollDynLocate(rule[0], rule[1], rule[2], 0)
        return lib.scroll_batch_dyn_locate(b.h, nframes, ctypes.byref(s), ctypes.byref(r), None)

    b = gpu.Batch(2, 2, 4 << 20)
    try:
        for _ in range(2):
            b.add_stream(gpu.make_config(w, h))
        assert call(b, 2) == CONFIG                                  # no dynamic rect
        b.set_dyn_rect(1, 1, 2, 1)
        assert call(b, 2) == CONFIG and "reference pictures" in scroll.last_error()
        assert lib.scroll_batch_dyn_locate_device(b.h, None) is None  # nothing allocated by a refusal
        rec = scroll.ScrollDynDamage()
        assert lib.scroll_batch_dyn_locate_result(b.h, 0, 0, ctypes.byref(rec)) == CONFIG
        assert b.dyn_locate_ms() == -1.0
        b.set_dyn_refs(R.i420(0), R.i420(1))
        b.set_offsets(offs)
        assert call(b, 2, (0, 0, 1)) == CONFIG and "moving" in scroll.last_error()   # apply without moving rects
        b.set_dyn_rect_moving()
        b.set_dyn_rect_at(0, 1, 2, 2)
        b.set_dyn_rect_at(1, 0, -1, -1)
        assert call(b, 2, (0, 0, 0)) == 0                            # apply = 0: the first call allocates
        maps, recs = expect(img, yps, v, 2, 1)
        check(b, 2, maps, recs)
        assert b.dyn_locate_ms() == -1.0
        source(b, sf, 2, v)
        compose_ok(gpu, b, 2)
        before = [b.output(s) for s in range(2)]
        # pre-fill results and map, then every refusal
        pr, ls = b.dyn_locate_device()
        pm, ms, mf = b.dyn_damage_map_device()
        assert ls == 2 * DAMAGE_DTYPE.itemsize and mf == 4 * (w // 16) * (h // 16) and ms == 2 * mf
        hip.fill(pr, 0x5A, 2 * ls)
        hip.fill(pm, 0xA5, 2 * ms)
        bad = [dict(base=sf.p + 4), dict(pitch=sf.pitch + 8), dict(pitch=4 * w - 16), dict(frame_stride=sf.fstride + 4),
               dict(stream_stride=sf.sstride + 8), dict(format=2), dict(matrix=2), dict(full_range=2), dict(cropped=1),
               dict(cropped=2), dict(base=None)]
        for kw in bad:
            assert call(b, 2, (0, 0, 1), **kw) == ARG, kw
            assert scroll.last_error()
        assert call(b, -1) == ARG and call(b, 3) == ARG
        assert call(b, 2, (0, 5, 1)) == ARG and call(b, 2, (0, 0, 2)) == ARG
        s0 = scroll.ScrollSurfaces(sf.p, sf.pitch, sf.fstride, sf.sstride, RGBA, BT601, 0, 0)
        assert lib.scroll_batch_dyn_locate(b.h, 2, ctypes.byref(s0), None, None) == ARG
        assert lib.scroll_batch_dyn_locate(b.h, 2, None, ctypes.byref(scroll.ScrollDynLocate()), None) == ARG
        b.set_hints(0, 0, [], gpu.SCROLL_HINT_EXACT)
        assert call(b, 2, (0, 0, 1)) == CONFIG and "hints" in scroll.last_error()
        b.clear_hints()                                              # (resets the positions: set again)
        b.set_dyn_rect_at(0, 1, 2, 2)
        b.set_dyn_rect_at(1, 0, -1, -1)
        assert call(b, 0, (0, 0, 1)) == 0                            # no frames: nothing to do, nothing written
        assert (hip.read(pr, 2 * ls) == 0x5A).all(), "a refused call wrote to the records"
        assert (hip.read(pm, 2 * ms) == 0xA5).all(), "a refused call wrote to the map"
        b.reset_output()
        for s in range(2):
            b.set_config(s, gpu.make_config(w, h))
        source(b, sf, 2, v)
        compose_ok(gpu, b, 2)
        assert [b.output(s) for s in range(2)] == before, "a refused call moved a position"
        # the batch after the refusals, timed
        b.enable_timing()
        locate(b, sf, 2, v, apply=False)
        check(b, 2, maps, recs)
        assert b.dyn_locate_ms() > 0.0 and 0.0 < b.dyn_locate_ms(kernel=True) <= b.dyn_locate_ms()
        b.enable_timing(False)
        locate(b, sf, 2, v, apply=False)
        assert b.dyn_locate_ms() == -1.0
    finally:
        b.close()
        sf.free()
