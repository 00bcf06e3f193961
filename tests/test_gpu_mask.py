"""GPU check of scroll_batch_dyn_mask (k_dyn_mask_diff, k_dyn_mask_fill,
k_dyn_mask_rec): the per-MB map between the dynamic rect's source and the
prediction a decoder forms for it, the keep decision, the records and the
doctored source, integer for integer and byte for byte against the numpy
restatement of tests/maskhelp.py (its prediction sampled through the oracle's
or_ref_sample; tests/test_mask_hostsim.py pins it against the test decoder);
the composed bytes against or_compose_dyn on the helper's doctored source; and
the mask inside the device-side tick.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

import h264_pslice as hp
from cschelp import BT601, RGBA
from damagehelp import Hip, Surfaces, frame_states, grey_surface, locate_np, paint, position, ypred_frames
from damagehelp import damage_map_np
from dynhelp import split_nals
from dynposhelp import oracle_moving, per_position
from maskhelp import KEPT, MASK_DTYPE, NOFRAME, OK, doctor, mask_np, noisy, paint_mbs, planes, pred_rect, \
    record_np, record_tuple
from probehelp import constant_of, oracle_probe, se_len
from reconhelp import oracle_frames, random_refs, sse3

pytestmark = pytest.mark.gpu

# tests/test_gpu_dyn_pos.py's picture: 6 x 23 MBs, the smallest that reaches the 496 waypoint
W, H, RECT = 96, 368, (1, 2, 5, 5)
RW, RH = RECT[2:]
# offset 0, odd ones, 300 (the rect's MB row 4 torn between A and B), through the 496 waypoint
OFFS = np.array([[484, 488, 492, 496, 500, 504], [0, 300, 496, 368, 7, 100], [7, 33, 250, 367, 119, 496]], np.int32)
S, F = OFFS.shape
# experiment mode: the frame that first reaches 496 writes a waypoint NAL in place of its scroll NAL
NOFRAMES = {(0, 3), (1, 2), (2, 5)}
D = 5                               # the single pixel's error: Dy = 25
BLOCK = [(1, 1), (2, 1), (1, 2), (2, 2)]
AMP = 2                             # the noise: Dy <= 1024, Dc <= 512 per MB
TY, TC = 256 * AMP * AMP, 128 * AMP * AMP
PATTERNS = ["noise", "pixel", "chroma", "block"]
NB = 384 * RW * RH
MAXT = 0xFFFFFFFF


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


def make(gpu, w, h, ns, nf, rect, refs, mode=0, moving=False, recon=False, qp=None, waypoints=(), arena=8 << 20):
    """refs: one ArrayRefs for every stream, or a list of one per stream"""
    b = gpu.Batch(ns, nf, arena, mode=mode)
    for _ in range(ns):
        b.add_stream(gpu.make_config(w, h, waypoints=waypoints))
    b.set_dyn_rect(*rect)
    if qp is not None:
        b.set_dyn_qp(qp)
    if isinstance(refs, list):
        for s, R in enumerate(refs):
            b.set_dyn_refs(R.i420(0), R.i420(1), stream=s)
    else:
        b.set_dyn_refs(refs.i420(0), refs.i420(1))
    if recon:
        b.set_dyn_recon()
    if moving:
        b.set_dyn_rect_moving()
    return b


def load(b, offs, src):
    offs = np.ascontiguousarray(offs, dtype=np.int32)
    b.set_offsets(offs)
    b.set_dyn_source(np.ascontiguousarray(src).tobytes(), offs.shape[1])


def device_source(b, hip, ns, nf, nbytes):
    p, ls, lf = b.dyn_source_device()
    return np.stack([np.stack([hip.read(p + s * ls + f * lf, nbytes) for f in range(nf)]) for s in range(ns)])


def compose_ok(gpu, b, nframes):
    b.compose(nframes)
    assert b.sync() == 0, gpu.last_error()


def expect(src, preds, rw, rh, ty=0, tc=0, grow=0):
    """per (s, f): (map with KEPT bits, record, kept, doctored source) of the helper; preds[s][f] None: no dynamic NAL"""
    out = []
    for s in range(len(preds)):
        row = []
        for f in range(len(preds[s])):
            if preds[s][f] is None:
                row.append((np.zeros((rh, rw, 2), np.uint32), record_np(None, None)[0], None, src[s][f]))
            else:
                row.append(mask_np(src[s][f], preds[s][f], rw, rh, ty, tc, grow))
        out.append(row)
    return out


def check(b, nframes, want, rw, rh):
    got_m, got_r = b.dyn_mask_map(nframes, rw, rh), b.dyn_mask_result(nframes)
    for s in range(len(want)):
        for f in range(nframes):
            wm, wr = want[s][f][:2]
            if not np.array_equal(got_m[s, f], wm):
                bad = np.argwhere(got_m[s, f] != wm)[0]
                raise AssertionError(f"map of stream {s} frame {f}: MB ({bad[1]}, {bad[0]}) word {bad[2]} is "
                                     f"{got_m[s, f][tuple(bad)]:#x}, not {wm[tuple(bad)]:#x}")
            assert record_tuple(got_r[s, f]) == record_tuple(wr), (s, f, got_r[s, f], wr)


def sources(preds, rw, rh, rng):
    """[S][F][384 rw rh]: per frame one of PATTERNS over its prediction (random where there is none)"""
    ns, nf = len(preds), len(preds[0])
    src = np.empty((ns, nf, 384 * rw * rh), np.uint8)
    for s in range(ns):
        for f in range(nf):
            p = preds[s][f]
            if p is None:
                src[s, f] = rng.integers(0, 256, src.shape[2])
                continue
            name = pattern_of(s, f)
            if name == "noise":
                src[s, f] = noisy(p, rng, AMP)
            elif name == "block":
                src[s, f] = paint_mbs(noisy(p, rng, AMP), BLOCK, rw, rh, rng)
            elif name == "pixel":                   # one luma sample of MB (3, 4) off by D
                src[s, f] = p
                y = planes(src[s, f], rw, rh)[0]
                v = int(y[16 * 4 + 5, 16 * 3 + 9])
                y[16 * 4 + 5, 16 * 3 + 9] = v + D if v + D <= 255 else v - D
            else:                                   # chroma only: Cr of MB (4, 0) repainted, Dy = 0 everywhere
                src[s, f] = p
                cr = planes(src[s, f], rw, rh)[2][0:8, 32:40]
                cr[:] = (cr.astype(np.int64) + rng.integers(64, 192, cr.shape)) % 256
    return src


def preds_of(oracle, w, h, offs, R, rect_of, mode=0, waypoints=()):
    """[S][F] predictions; R one ArrayRefs or a list per stream; rect_of(s, f) -> rect or None"""
    out = []
    for s in range(len(offs)):
        Rs = R[s] if isinstance(R, list) else R
        states = frame_states(oracle, w, h, offs[s], mode, waypoints)
        out.append([None if st is None or rect_of(s, f) is None else pred_rect(oracle, st, Rs, rect_of(s, f), off)
                    for f, (st, off) in enumerate(zip(states, offs[s]))])
    return out


@pytest.fixture(scope="module")
def edge(oracle):
    """per mode: references, every frame's prediction and source, computed once"""
    R = random_refs(W, H, 61)
    out = {}
    for mode in (0, 1):
        preds = preds_of(oracle, W, H, OFFS, R, lambda s, f: RECT, mode)
        out[mode] = (R, preds, sources(preds, RW, RH, np.random.default_rng(62 + mode)))
    return out


RULES = [(0, 0, 0), (D * D - 1, 0, 0), (D * D, 0, 0), (TY, TC, 0), (TY, TC, 1), (TY, TC, 2), (MAXT, 0, 1)]


@pytest.mark.parametrize("mode", [0, 1])
def test_map_and_records(gpu, hip, edge, mode):
    """check 4: every pattern in composer and experiment mode under every rule,
    apply = 0; the NOFRAME frames are the ones named here; the source stays"""
    R, preds, src = edge[mode]
    none = {(s, f) for s in range(S) for f in range(F) if preds[s][f] is None}
    assert none == (NOFRAMES if mode else set())
    b = make(gpu, W, H, S, F, RECT, R, mode=mode)
    try:
        load(b, OFFS, src)
        for ty, tc, grow in RULES:
            b.dyn_mask(F, ty, tc, grow, apply=False)
            want = expect(src, preds, RW, RH, ty, tc, grow)
            check(b, F, want, RW, RH)
            for s in range(S):
                for f in range(F):
                    mk, rec, kept, _ = want[s][f]
                    name = pattern_of(s, f)
                    if (s, f) in none:
                        assert rec["status"] == NOFRAME and not mk.any()
                        continue
                    assert rec["status"] == OK
                    if name == "pixel":
                        assert mk[4, 3, 0] == D * D and int(mk[..., 0].sum()) == D * D and not (mk[..., 1] & 0x7FFFFFFF).any()
                        assert rec["n_changed"] == (1 if ty < D * D else 0)
                    if name == "chroma":
                        assert not mk[..., 0].any() and (mk[0, 4, 1] & 0x7FFFFFFF) > TC
                        assert rec["n_changed"] == 1 and kept[0, 4]
                    if name == "block" and (ty, tc) == (TY, TC):
                        assert rec["n_changed"] == len(BLOCK) and rec["n_kept"] == (4, 16, 25)[grow]
                    if name == "noise" and (ty, tc) == (TY, TC):
                        assert rec["n_changed"] == 0 and rec["n_kept"] == 0
                        assert rec["sse_drop"] == sse3(src[s][f], preds[s][f], RECT)
        assert np.array_equal(device_source(b, hip, S, F, NB), src), "apply = 0 wrote to the source"
    finally:
        b.close()


def run_apply(gpu, hip, oracle, w, h, rect, offs, refs, src, preds, rule, qp=26, waypoints=()):
    """check 5 on one batch: the doctored source, the composed bytes against
    or_compose_dyn on it, the reconstruction at the dropped MBs and the
    squared-error identity"""
    ns, nf = offs.shape
    rw, rh = rect[2:]
    want = expect(src, preds, rw, rh, *rule)
    b = make(gpu, w, h, ns, nf, rect, refs, recon=True, qp=qp, waypoints=waypoints)
    try:
        load(b, offs, src)
        b.dyn_mask(nf, *rule)
        check(b, nf, want, rw, rh)
        doct = np.stack([np.stack([want[s][f][3] for f in range(nf)]) for s in range(ns)])
        got = device_source(b, hip, ns, nf, 384 * rw * rh)
        assert np.array_equal(got, doct), "the source after the mask is not the helper's doctored source"
        recs = b.dyn_mask_result(nf)
        # a second call with the same rule: the source stays, nothing is left to drop
        b.dyn_mask(nf, *rule)
        assert np.array_equal(device_source(b, hip, ns, nf, 384 * rw * rh), doct)
        again = b.dyn_mask_result(nf)
        for s in range(ns):
            for f in range(nf):
                assert tuple(again[s, f]["sse_drop"]) == (0, 0, 0)
                assert (again[s, f]["n_changed"], again[s, f]["n_kept"]) == (recs[s, f]["n_changed"], recs[s, f]["n_kept"])
        compose_ok(gpu, b, nf)
        for s in range(ns):
            Rs = refs[s] if isinstance(refs, list) else refs
            data, frames = oracle_frames(oracle, w, h, offs[s], rect, doct[s], Rs, qp=qp, waypoints=waypoints)
            assert b.output(s) == data, f"stream {s}: composed bytes differ from or_compose_dyn's on the doctored source"
            for f in range(nf):
                kept, pred = want[s][f][2], preds[s][f]
                rec = np.frombuffer(b.dyn_recon(s, f), np.uint8)
                assert rec.tobytes() == frames[f][0]
                assert np.array_equal(doctor(rec, pred, kept, rw, rh), rec), (s, f)     # dropped MBs: the prediction
                total = tuple(a + int(d) for a, d in zip(b.dyn_sse(s, f), recs[s, f]["sse_drop"]))
                assert total == sse3(src[s][f], rec, rect), (s, f)
    finally:
        b.close()
    return want


def test_apply_end_to_end(gpu, hip, oracle, edge):
    R, preds, src = edge[0]
    want = run_apply(gpu, hip, oracle, W, H, RECT, OFFS, R, src, preds, (TY, TC, 1))
    assert any(0 < want[s][f][1]["n_kept"] < RW * RH for s in range(S) for f in range(F))


@pytest.mark.parametrize("w,h,rect", [(320, 240, (19, 1, 1, 3)), (320, 240, (1, 0, 17, 2)), (320, 240, (0, 12, 20, 3))])
def test_widths_and_per_stream_references(gpu, hip, oracle, w, h, rect):
    """rects of 1, 17 and 20 MBs per row (a second, partial span of 16 MBs; the
    5-MB rect is the tests' above), each stream with references of its own;
    changed MBs on both sides of the span seam"""
    offs = np.array([[3, 130], [h, 77]], np.int32)
    refs = [random_refs(w, h, 63), random_refs(w, h, 64)]
    rw, rh = rect[2:]
    preds = preds_of(oracle, w, h, offs, refs, lambda s, f: rect)
    rng = np.random.default_rng(65)
    mbs = [(min(15, rw - 1), 0), (min(16, rw - 1), rh - 1), (0, rh - 1)]
    src = np.stack([np.stack([paint_mbs(noisy(preds[s][f], rng, AMP), mbs if (s + f) % 2 else mbs[:1], rw, rh, rng)
                              for f in range(2)]) for s in range(2)])
    want = run_apply(gpu, hip, oracle, w, h, rect, offs, refs, src, preds, (TY, TC, 1 if rw > 1 else 0))
    assert want[0][1][1]["n_changed"] == len(set(mbs))


def test_half_pel_chain(gpu, hip, oracle):
    """a resumed waypoint at an odd offset: rows predict chroma through a
    half-pel waypoint step (ROW_GEN: the kernels' second instantiation,
    chroma_pred_any).  That a row sets ROW_GEN is taken on the waypoint
    table's word, as in the project's other half-pel tests; nothing here
    observes which instantiation ran.  Should k_dyn_rows stop listing such a
    frame, the map would show it: the first instantiation skips those rows
    and the second would never see them, so their entries would keep the
    zeroes of a fresh batch"""
    w, h, rect, wps = 64, 1024, (1, 20, 2, 12), [(501, 2, 1)]
    offs = np.array([[600, 777, 996]], np.int32)
    R = random_refs(w, h, 66)
    preds = preds_of(oracle, w, h, offs, R, lambda s, f: rect, waypoints=wps)
    rng = np.random.default_rng(67)
    src = np.stack([np.stack([paint_mbs(noisy(p, rng, AMP), [(1, 3), (0, 11)], 2, 12, rng) for p in preds[0]])])
    run_apply(gpu, hip, oracle, w, h, rect, offs, R, src, preds, (TY, TC, 0), waypoints=wps)


def test_keep_all_and_drop_all(gpu, hip, oracle):
    """check 6: thresholds (0, 0) on a source that differs everywhere keep every
    MB and change no byte; maximal thresholds drop every MB and the frame's
    rect is coded without residual"""
    offs = np.array([[7, 300]], np.int32)
    R = random_refs(W, H, 68)
    preds = preds_of(oracle, W, H, offs, R, lambda s, f: RECT)
    src = np.stack([np.stack([(p.astype(np.int64) + 1 + (p.astype(np.int64) > 200) * -2).astype(np.uint8)
                              for p in preds[0]])])
    assert all((src[0, f] != preds[0][f]).all() for f in range(2))
    b = make(gpu, W, H, 1, 2, RECT, R, recon=True)
    try:
        load(b, offs, src)
        b.dyn_mask(2, 0, 0, 0)
        check(b, 2, expect(src, preds, RW, RH), RW, RH)
        assert (b.dyn_mask_result(2)["n_kept"] == RW * RH).all()
        assert np.array_equal(device_source(b, hip, 1, 2, NB), src)
        b.dyn_mask(2, MAXT, MAXT, 2)
        want = expect(src, preds, RW, RH, MAXT, MAXT, 2)
        check(b, 2, want, RW, RH)
        assert (b.dyn_mask_result(2)["n_kept"] == 0).all()
        assert np.array_equal(device_source(b, hip, 1, 2, NB), np.stack([np.stack(preds[0])]))
        compose_ok(gpu, b, 2)
        nals = split_nals(b.output(0))
        assert len(nals) == 2
        for f, nal in enumerate(nals):
            seen = []

            def on_mb(x, y, ref, mvd, cbp, luma, cdc, cac):
                if RECT[0] <= x < RECT[0] + RW and RECT[1] <= y < RECT[1] + RH:
                    seen.append(cbp)

            hp.parse_p_slice(nal, W, H, on_mb=on_mb)
            assert seen == [0] * (RW * RH), (f, seen)
            assert b.dyn_recon(0, f) == preds[0][f].tobytes() and b.dyn_sse(0, f) == (0, 0, 0)
            assert tuple(int(v) for v in b.dyn_mask_result(2)[0, f]["sse_drop"]) == sse3(src[0, f], preds[0][f], RECT)
    finally:
        b.close()


def raw_tick(gpu, b, nframes, cand, frame_bits, rule):
    """dyn_mask -> dyn_probe -> dyn_pick -> compose through the C calls, nothing read back in between"""
    lib = gpu.lib
    r = gpu.ScrollDynMaskRule(rule[0], rule[1], rule[2], 1)
    assert lib.scroll_batch_dyn_mask(b.h, nframes, ctypes.byref(r), None) == 0, gpu.last_error()
    assert lib.scroll_batch_dyn_probe(b.h, nframes, gpu.u8buf(bytes(cand)), len(cand), None) == 0, gpu.last_error()
    rate = gpu.ScrollDynRate(gpu.SCROLL_DYN_RATE_FRAME, int(frame_bits), 0, 0)
    assert lib.scroll_batch_dyn_pick(b.h, nframes, ctypes.byref(rate), None, None) == 0, gpu.last_error()
    b.compose(nframes)
    assert b.sync() == 0, gpu.last_error()


def probe_results(gpu, b, ns, nframes, nq):
    out = {}
    r = gpu.ScrollDynProbe()
    for s in range(ns):
        for f in range(nframes):
            for k in range(nq):
                rc = gpu.lib.scroll_batch_dyn_probe_result(b.h, s, f, k, ctypes.byref(r))
                out[(s, f, k)] = None if rc == 1 else (rc, tuple(r.sse), r.bits, r.nonzero)
    return out


def outputs(b, ns, nf):
    return ([b.output(s) for s in range(ns)], [b.dyn_frame_info(s, f) for s in range(ns) for f in range(nf)],
            b.dyn_qp_frames(nf).tolist())


def test_moving_rect_and_the_tick(gpu, hip, oracle, edge):
    """check 7: the mask at set_dyn_rect_at's positions, frames without a rect
    included; then mask -> probe -> pick -> compose without a host step
    against a batch that is given the helper's doctored source and stepped
    from the host: probe results, picks, frame sizes and bytes agree"""
    R = edge[0][0]
    pos = [[(1, 2), (0, 0), None, (1, 18), (0, 9), (1, 2)], [(1, 3), None, (0, 17), (1, 2), (0, 5), (1, 11)],
           [None, (1, 2), (1, 6), (0, 18), (1, 0), (0, 13)]]

    def rect_of(s, f):
        return None if pos[s][f] is None else pos[s][f] + (RW, RH)

    preds = preds_of(oracle, W, H, OFFS, R, rect_of)
    src = sources(preds, RW, RH, np.random.default_rng(69))
    rule, cand = (TY, TC, 1), [20, 30, 40]
    want = expect(src, preds, RW, RH, *rule)
    doct = np.stack([np.stack([want[s][f][3] for f in range(F)]) for s in range(S)])
    a = make(gpu, W, H, S, F, RECT, R, moving=True)
    c = make(gpu, W, H, S, F, RECT, R, moving=True)
    try:
        for x in (a, c):
            for s in range(S):
                for f in range(F):
                    x.set_dyn_rect_at(s, f, *(pos[s][f] or (-1, -1)))
        load(a, OFFS, src)
        raw_tick(gpu, a, F, cand, 3000, rule)
        check(a, F, want, RW, RH)
        assert [want[s][f][1]["status"] for s in range(S) for f in range(F)] == \
            [NOFRAME if pos[s][f] is None else OK for s in range(S) for f in range(F)]
        assert np.array_equal(device_source(a, hip, S, F, NB), doct)
        load(c, OFFS, doct)
        c.dyn_probe(F, cand)
        c.dyn_pick(F, 3000)
        compose_ok(gpu, c, F)
        assert probe_results(gpu, a, S, F, len(cand)) == probe_results(gpu, c, S, F, len(cand))
        assert outputs(a, S, F) == outputs(c, S, F)
    finally:
        a.close()
        c.close()


def test_the_whole_tick_after_a_locate(gpu, hip, oracle, edge):
    """check 7: dyn_locate(apply = 1) -> dyn_source_from_surfaces -> dyn_mask ->
    dyn_probe -> dyn_pick -> compose on one stream, nothing read back in
    between.  The surfaces are grey (their luma is the prediction's) with
    painted MBs; their chroma is 128 against random references, so the rule
    (0, maximal, 1) drops the unpainted MBs by their luma and the fill
    rewrites their chroma: bytes that really differ.  What the source step
    makes of the surfaces is learnt from a second batch run before.  Against
    the helper at the located positions: map, records, doctored source; the
    probe's bits and non-zero levels at every candidate against the oracle's
    trace of the doctored source; the composed bytes against or_compose_dyn on
    it at the picked QPs; and the probe's bits at the picked candidate against
    the compose's dyn_frame_info through the header's identity, RBSP bits = C
    + len(se(q - 26)) + bits + the stop bit, C from the oracle at another
    candidate"""
    R = edge[0][0]
    rng = np.random.default_rng(70)
    grey = (RGBA, BT601, 1)
    rule, cand, budget = (0, MAXT, 1), [24, 36], 6000
    yps = [ypred_frames(oracle, W, H, OFFS[s], R) for s in range(S)]
    dmg = [[[[(2, 5), (3, 6)], [], [(0, 20), (1, 21)]][(s + f) % 3] for f in range(F)] for s in range(S)]
    img = np.stack([np.stack([paint(grey_surface(yps[s][f], RGBA, rng), dmg[s][f], rng) for f in range(F)])
                    for s in range(S)])
    pos = [[position(locate_np(damage_map_np(img[s, f], yps[s][f], *grey), RW, RH)) for f in range(F)] for s in range(S)]
    assert {p for row in pos for p in row} == {None, (1, 5), (0, 18)}
    preds = preds_of(oracle, W, H, OFFS, R, lambda s, f: None if pos[s][f] is None else pos[s][f] + (RW, RH))
    sf = Surfaces(hip, img)
    kw = dict(fmt=grey[0], matrix=grey[1], full_range=True)
    c = make(gpu, W, H, S, F, RECT, R, moving=True)
    try:
        c.set_offsets(OFFS)
        c.dyn_locate(sf.p, F, *sf.args(), **kw)
        c.dyn_source_from_surfaces(sf.p, F, *sf.args(), **kw)
        src = device_source(c, hip, S, F, NB)           # what the source step makes of the surfaces
    finally:
        c.close()
    want = expect(src, preds, RW, RH, *rule)
    doct = np.stack([np.stack([want[s][f][3] for f in range(F)]) for s in range(S)])
    for s in range(S):
        for f in range(F):
            if pos[s][f] is not None:
                x0, y0 = pos[s][f]
                mk, rec, kept, _ = want[s][f]
                assert {(x + x0, y + y0) for y, x in np.argwhere(mk[..., 0] > 0)} <= set(dmg[s][f])
                assert 0 < rec["n_changed"] <= len(dmg[s][f]) and rec["n_kept"] < RW * RH and rec["sse_drop"][1] > 0
                assert (doct[s, f] != src[s, f]).any()
    a = make(gpu, W, H, S, F, RECT, R, moving=True)
    try:
        a.set_offsets(OFFS)
        a.dyn_locate(sf.p, F, *sf.args(), **kw)
        a.dyn_source_from_surfaces(sf.p, F, *sf.args(), **kw)
        raw_tick(gpu, a, F, cand, budget, rule)
        check(a, F, want, RW, RH)
        assert np.array_equal(device_source(a, hip, S, F, NB), doct)
        got = probe_results(gpu, a, S, F, len(cand))
        qps = a.dyn_qp_frames(F)
        picked = 0
        for s in range(S):
            qs = [int(q) if q >= 0 else 26 for q in qps[s]]
            assert a.output(s) == oracle_moving(oracle, W, H, OFFS[s], RW, RH, pos[s], doct[s], R, qs)[0], s
            trace = [per_position(lambda r, q=q: oracle_probe(oracle, W, H, OFFS[s], r, doct[s], R, q, decode=False)[1],
                                  pos[s], RW, RH) for q in cand]
            for f in range(F):
                info = a.dyn_frame_info(s, f)
                if pos[s][f] is None:
                    assert info is None and all(got[(s, f, k)] is None for k in range(len(cand))), (s, f)
                    continue
                for k in range(len(cand)):
                    assert got[(s, f, k)][0] == 0 and got[(s, f, k)][2:] == (trace[k][f]["bits"], trace[k][f]["nonzero"])
                assert qps[s, f] in cand, (s, f, qps[s, f])
                k = cand.index(int(qps[s, f]))
                C = constant_of(trace[1 - k][f], cand[1 - k])
                assert info[0] == (C + se_len(cand[k] - 26) + got[(s, f, k)][2] + 1 + 7) // 8, (s, f, info)
                picked += 1
        assert picked == sum(p is not None for row in pos for p in row)
    finally:
        a.close()
        sf.free()


def test_a_rect_wider_than_64_mbs(gpu, hip, oracle):
    """80 MBs per rect row (a 1280-wide picture's whole width): five spans, so
    k_dyn_mask_fill's waves take a second span; changed MBs on both sides of
    MB 64 and at both ends"""
    w, h, rect = 1280, 48, (0, 1, 80, 2)
    offs = np.array([[3, 20]], np.int32)
    R = random_refs(w, h, 73)
    preds = preds_of(oracle, w, h, offs, R, lambda s, f: rect)
    rng = np.random.default_rng(74)
    mbs = [(0, 0), (63, 0), (64, 1), (79, 1)]
    src = np.stack([np.stack([paint_mbs(noisy(p, rng, AMP), mbs, 80, 2, rng) for p in preds[0]])])
    want = run_apply(gpu, hip, oracle, w, h, rect, offs, R, src, preds, (TY, TC, 1))
    assert want[0][0][1]["n_changed"] == 4 and want[0][0][1]["n_kept"] == 2 * (2 + 4 + 2)


def test_config3_shape(gpu, hip, oracle):
    """one 1280x720 stream x 2 frames, the 25 x 25 rect at (28, 10): a 5 x 5-MB
    block changed in a noisy source"""
    w, h, rect = 1280, 720, (28, 10, 25, 25)
    offs = np.array([[100, 100]], np.int32)
    R = random_refs(w, h, 71)
    rng = np.random.default_rng(72)
    p = pred_rect(oracle, frame_states(oracle, w, h, offs[0][:1])[0], R, rect, 100)
    preds = [[p, p]]                            # the same offset and waypoint table: the same prediction
    blk = [(x, y) for y in range(9, 14) for x in range(14, 19)]
    src = np.stack([np.stack([paint_mbs(noisy(p, rng, 1), blk, 25, 25, rng) for _ in range(2)])])
    want = expect(src, preds, 25, 25, 256, 128, 1)
    b = make(gpu, w, h, 1, 2, rect, R, arena=16 << 20)
    try:
        load(b, offs, src)
        b.dyn_mask(2, 256, 128, 1)
        check(b, 2, want, 25, 25)
        for f in range(2):
            assert want[0][f][1]["n_changed"] == 25 and want[0][f][1]["n_kept"] == 49
        assert np.array_equal(device_source(b, hip, 1, 2, 384 * 625),
                              np.stack([np.stack([want[0][f][3] for f in range(2)])]))
    finally:
        b.close()


def test_contract(gpu, hip, oracle, edge, scroll):
    """check 8: every refusal returns its code and leaves records and map as
    they were (pre-filled patterns); set_dyn_rect frees the buffers; a batch
    that never calls the mask composes what it composed before; mask_ms is -1
    without timing"""
    R, preds, src = edge[0]
    lib, ARG, CONFIG = scroll.lib, scroll.SCROLL_ERR_ARG, scroll.SCROLL_ERR_CONFIG

    def call(b, nframes, ty=0, tc=0, grow=0, apply=1):
        r = scroll.ScrollDynMaskRule(ty, tc, grow, apply)
        return lib.scroll_batch_dyn_mask(b.h, nframes, ctypes.byref(r), None)

    b = gpu.Batch(S, F, 8 << 20)
    try:
        for _ in range(S):
            b.add_stream(gpu.make_config(W, H))
        assert call(b, F) == CONFIG                                  # no dynamic rect
        b.set_dyn_rect(*RECT)
        assert call(b, F) == CONFIG and "reference pictures" in scroll.last_error()
        assert lib.scroll_batch_dyn_mask_device(b.h, None) is None   # nothing allocated by a refusal
        assert lib.scroll_batch_dyn_mask_map_device(b.h, None, None) is None
        rec = scroll.ScrollDynMask()
        assert lib.scroll_batch_dyn_mask_result(b.h, 0, 0, ctypes.byref(rec)) == CONFIG
        assert b.dyn_mask_ms() == -1.0
        b.set_dyn_refs(R.i420(0), R.i420(1))
        # never masked: the bytes of a plain compose, for the comparison below
        load(b, OFFS, src)
        compose_ok(gpu, b, F)
        before = [b.output(s) for s in range(S)]
        assert before[0] == oracle_frames(oracle, W, H, OFFS[0], RECT, src[0], R)[0]
        assert lib.scroll_batch_dyn_mask_device(b.h, None) is None

        def restart():
            b.reset_output()
            for s in range(S):
                b.set_config(s, gpu.make_config(W, H))

        restart()
        assert call(b, F, apply=0) == 0                              # the first call allocates
        want = expect(src, preds, RW, RH)
        check(b, F, want, RW, RH)
        assert lib.scroll_batch_dyn_mask_result(b.h, S, 0, ctypes.byref(rec)) == ARG
        assert lib.scroll_batch_dyn_mask_result(b.h, 0, F, ctypes.byref(rec)) == ARG
        # pre-fill records and map, then every refusal
        pr, ls = b.dyn_mask_device()
        pm, ms, mf = b.dyn_mask_map_device()
        assert ls == F * MASK_DTYPE.itemsize and mf == 8 * RW * RH and ms == F * mf
        hip.fill(pr, 0x5A, S * ls)
        hip.fill(pm, 0xA5, S * ms)
        assert call(b, -1) == ARG and call(b, F + 1) == ARG
        assert call(b, F, grow=3) == ARG and call(b, F, apply=2) == ARG
        assert lib.scroll_batch_dyn_mask(b.h, F, None, None) == ARG
        b.set_hints(0, 0, [], gpu.SCROLL_HINT_EXACT)
        assert call(b, F) == CONFIG and "hints" in scroll.last_error()
        b.clear_hints()
        assert call(b, 0) == 0                                       # no frames: nothing to do, nothing written
        assert (hip.read(pr, S * ls) == 0x5A).all(), "a refused call wrote to the records"
        assert (hip.read(pm, S * ms) == 0xA5).all(), "a refused call wrote to the map"
        assert np.array_equal(device_source(b, hip, S, F, NB), src), "a refused call wrote to the source"
        compose_ok(gpu, b, F)
        assert [b.output(s) for s in range(S)] == before, "a report-only mask changed the composed bytes"
        # timed
        restart()
        b.enable_timing()
        assert call(b, F, apply=0) == 0
        check(b, F, want, RW, RH)
        assert b.dyn_mask_ms() > 0.0 and 0.0 < b.dyn_mask_ms(kernel=True) <= b.dyn_mask_ms()
        b.enable_timing(False)
        assert call(b, F, apply=0) == 0
        assert b.dyn_mask_ms() == -1.0
        # set_dyn_rect drops the buffers and the results
        b.set_dyn_rect(*RECT)
        assert lib.scroll_batch_dyn_mask_device(b.h, None) is None
        assert lib.scroll_batch_dyn_mask_result(b.h, 0, 0, ctypes.byref(rec)) == CONFIG
    finally:
        b.close()                                                    # destroy after a mask: its buffers go with the batch
    b = make(gpu, W, H, S, F, RECT, R)
    load(b, OFFS, src)
    b.dyn_mask(F, TY, TC, 1)
    b.close()                                                        # with the mask's launches still in flight
