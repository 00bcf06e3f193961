"""GPU check of what the batch's side passes share (csrc/batch_pass.hip): the
QP probe, the pick, the locate, the mask and the detect keep their last run in
one record and answer their result calls, their timing getters and a dropped
rect alike.  The messages are literals of the library's source as it stood
before the passes shared that code.  Every case is 2 streams of 2 frames of a
96x48 picture with a 2x1-MB rect.  Run on an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

from damagehelp import Hip, Surfaces
from detecthelp import i420, noise_luma

pytestmark = pytest.mark.gpu

PW, PH, S, F, RECT = 96, 48, 2, 2, (1, 1, 2, 1)
NB = 384 * RECT[2] * RECT[3]
QPS = [26, 30]
OFFS = np.array([[5, 6], [7, 8]], np.int32)


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


@pytest.fixture(scope="module")
def hip(gpu):
    return Hip()


@pytest.fixture(scope="module")
def data(hip):
    """references, the rect's source and whole-picture surfaces, all noise; shared and left unchanged"""
    rng = np.random.default_rng(90)
    ya, yb = noise_luma(PW, PH, rng)
    src = rng.integers(0, 256, (S, F, NB), dtype=np.uint8)
    sf = Surfaces(hip, rng.integers(0, 256, (S, F, PH, PW, 4), dtype=np.uint8))
    yield (i420(ya), i420(yb)), src, sf
    sf.free()


def make(gpu, data, refs=True):
    b = gpu.Batch(S, F, 4 << 20)
    for _ in range(S):
        b.add_stream(gpu.make_config(PW, PH))
    b.set_dyn_rect(*RECT)
    if refs:
        ready(b, data)
    return b


def ready(b, data):
    """what set_dyn_rect dropped: references, offsets, source"""
    b.set_dyn_refs(*data[0])
    b.set_offsets(OFFS)
    b.set_dyn_source(data[1][:, :F].tobytes(), F)


class Pass:
    """one side pass: how it runs, the result calls that name a frame, its device getter, its timing getters"""

    def __init__(self, run, results, device=None, ms=None, parts=()):
        self.run, self.results, self.device, self.ms, self.parts = run, results, device, ms, parts


def passes(scroll, data):
    lib, sf = scroll.lib, data[2]
    u32 = (ctypes.c_uint32 * (PH + 1 + 2 * RECT[2] * RECT[3] + (PW // 16) * (PH // 16)))()
    k, qp = ctypes.c_int(), ctypes.c_int()
    probe_rec, locate_rec = scroll.ScrollDynProbe(), scroll.ScrollDynDamage()
    mask_rec, detect_rec = scroll.ScrollDynMask(), scroll.ScrollOffsetFound()

    def probe(b, n):
        assert lib.scroll_batch_dyn_probe(b.h, n, scroll.u8buf(bytes(QPS)), len(QPS), None) == 0

    def pick(b, n):
        probe(b, n)
        rate = scroll.ScrollDynRate(scroll.SCROLL_DYN_RATE_FRAME, 1 << 20, 0, 0)
        assert lib.scroll_batch_dyn_pick(b.h, n, ctypes.byref(rate), None, None) == 0

    def locate(b, n):
        b.dyn_locate(sf.p, n, *sf.args(), full_range=True, apply=False)

    def mask(b, n):
        b.dyn_mask(n, apply=False)

    def detect(b, n):
        b.detect_offsets(sf.p, n, *sf.args(), full_range=True, radius=4, apply=False)

    return [
        Pass(probe,
             {"scroll_batch_dyn_probe_result":
              lambda b, s, f: lib.scroll_batch_dyn_probe_result(b.h, s, f, 1, ctypes.byref(probe_rec))},
             lambda b: lib.scroll_batch_dyn_probe_device(b.h, None, None), lambda b: b.dyn_probe_ms()),
        Pass(pick,
             {"scroll_batch_dyn_pick_result":
              lambda b, s, f: lib.scroll_batch_dyn_pick_result(b.h, s, f, ctypes.byref(k), ctypes.byref(qp))}),
        Pass(locate,
             {"scroll_batch_dyn_locate_result":
              lambda b, s, f: lib.scroll_batch_dyn_locate_result(b.h, s, f, ctypes.byref(locate_rec)),
              "scroll_batch_dyn_damage_map": lambda b, s, f: lib.scroll_batch_dyn_damage_map(b.h, s, f, u32)},
             lambda b: lib.scroll_batch_dyn_locate_device(b.h, None), lambda b: b.dyn_locate_ms(),
             (lambda b: b.dyn_locate_ms(kernel=True),)),
        Pass(mask,
             {"scroll_batch_dyn_mask_result":
              lambda b, s, f: lib.scroll_batch_dyn_mask_result(b.h, s, f, ctypes.byref(mask_rec)),
              "scroll_batch_dyn_mask_map": lambda b, s, f: lib.scroll_batch_dyn_mask_map(b.h, s, f, u32)},
             lambda b: lib.scroll_batch_dyn_mask_device(b.h, None), lambda b: b.dyn_mask_ms(),
             (lambda b: b.dyn_mask_ms(kernel=True),)),
        Pass(detect,
             {"scroll_batch_detect_result":
              lambda b, s, f: lib.scroll_batch_detect_result(b.h, s, f, ctypes.byref(detect_rec)),
              "scroll_batch_detect_scores": lambda b, s, f: lib.scroll_batch_detect_scores(b.h, s, f, u32)},
             lambda b: lib.scroll_batch_detect_device(b.h, None), lambda b: b.detect_ms(),
             (lambda b: b.detect_ms(kernel=True), lambda b: b.detect_ms(score=True))),
    ]


NOUNS = ["probe", "pick", "locate", "mask", "detect"]

# per result call: "nothing to read", and "outside the last run" for (stream 0, frame 1) and (stream 2, frame 0)
MESSAGES = {
    "scroll_batch_dyn_probe_result": (
        "scroll_batch_dyn_probe_result: no probe to read (scroll_batch_dyn_probe; scroll_batch_set_dyn_rect drops it)",
        "scroll_batch_dyn_probe_result: stream 0 / frame 1 / candidate 1 outside the last probe",
        "scroll_batch_dyn_probe_result: stream 2 / frame 0 / candidate 1 outside the last probe"),
    "scroll_batch_dyn_pick_result": (
        "scroll_batch_dyn_pick_result: no pick to read (scroll_batch_dyn_pick; scroll_batch_set_dyn_rect drops it)",
        "scroll_batch_dyn_pick_result: stream 0 / frame 1 outside the last pick",
        "scroll_batch_dyn_pick_result: stream 2 / frame 0 outside the last pick"),
    "scroll_batch_dyn_locate_result": (
        "scroll_batch_dyn_locate_result: no locate to read (scroll_batch_dyn_locate; scroll_batch_set_dyn_rect "
        "drops it)",
        "scroll_batch_dyn_locate_result: stream 0 / frame 1 outside the last locate",
        "scroll_batch_dyn_locate_result: stream 2 / frame 0 outside the last locate"),
    "scroll_batch_dyn_damage_map": (
        "scroll_batch_dyn_damage_map: no locate to read (scroll_batch_dyn_locate; scroll_batch_set_dyn_rect drops it)",
        "scroll_batch_dyn_damage_map: stream 0 / frame 1 outside the last locate",
        "scroll_batch_dyn_damage_map: stream 2 / frame 0 outside the last locate"),
    "scroll_batch_dyn_mask_result": (
        "scroll_batch_dyn_mask_result: no mask to read (scroll_batch_dyn_mask; scroll_batch_set_dyn_rect drops it)",
        "scroll_batch_dyn_mask_result: stream 0 / frame 1 outside the last mask",
        "scroll_batch_dyn_mask_result: stream 2 / frame 0 outside the last mask"),
    "scroll_batch_dyn_mask_map": (
        "scroll_batch_dyn_mask_map: no mask to read (scroll_batch_dyn_mask; scroll_batch_set_dyn_rect drops it)",
        "scroll_batch_dyn_mask_map: stream 0 / frame 1 outside the last mask",
        "scroll_batch_dyn_mask_map: stream 2 / frame 0 outside the last mask"),
    "scroll_batch_detect_result": (
        "scroll_batch_detect_result: no detect to read (scroll_batch_detect_offsets; scroll_batch_set_dyn_rect "
        "drops it)",
        "scroll_batch_detect_result: stream 0 / frame 1 outside the last detect",
        "scroll_batch_detect_result: stream 2 / frame 0 outside the last detect"),
    "scroll_batch_detect_scores": (
        "scroll_batch_detect_scores: no detect to read (scroll_batch_detect_offsets; scroll_batch_set_dyn_rect "
        "drops it)",
        "scroll_batch_detect_scores: stream 0 / frame 1 outside the last detect",
        "scroll_batch_detect_scores: stream 2 / frame 0 outside the last detect"),
}


@pytest.mark.parametrize("which", range(5), ids=NOUNS)
def test_refusals(gpu, data, which):
    """a result call before any run, outside the last run and after
    set_dyn_rect: the code and the whole message"""
    p = passes(gpu, data)[which]
    ARG, CONFIG = gpu.SCROLL_ERR_ARG, gpu.SCROLL_ERR_CONFIG

    def nothing(b):
        for who, call in p.results.items():
            assert call(b, 0, 0) == CONFIG
            assert gpu.last_error() == MESSAGES[who][0]
        if p.device:
            assert p.device(b) is None

    b = make(gpu, data)
    try:
        nothing(b)
        p.run(b, 1)
        for who, call in p.results.items():
            assert call(b, 0, 0) >= 0
            for (s, f), text in zip(((0, 1), (2, 0)), MESSAGES[who][1:]):
                assert call(b, s, f) == ARG
                assert gpu.last_error() == text
        if p.device:
            assert p.device(b)
        b.set_dyn_rect(*RECT)
        nothing(b)
        ready(b, data)
        p.run(b, F)                                                  # and the pass runs again on the new rect
        for call in p.results.values():
            assert call(b, S - 1, F - 1) >= 0
    finally:
        b.close()


def test_probe_candidate_range(gpu, data):
    b = make(gpu, data)
    try:
        passes(gpu, data)[0].run(b, 1)
        r = gpu.ScrollDynProbe()
        assert gpu.lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 2, ctypes.byref(r)) == gpu.SCROLL_ERR_ARG
        assert gpu.last_error() == \
            "scroll_batch_dyn_probe_result: stream 0 / frame 0 / candidate 2 outside the last probe"
    finally:
        b.close()


@pytest.mark.parametrize("which", [0, 2, 3, 4], ids=["probe", "locate", "mask", "detect"])
def test_timing(gpu, data, which):
    """-1 before a run and after an untimed one; a timed run's spans are
    positive and its parts no longer than the whole"""
    p = passes(gpu, data)[which]
    b = make(gpu, data)
    try:
        spans = (p.ms,) + p.parts
        assert all(ms(b) == -1.0 for ms in spans)
        p.run(b, F)
        assert all(ms(b) == -1.0 for ms in spans)
        b.enable_timing()
        p.run(b, F)
        total = p.ms(b)
        assert total > 0.0
        for part in p.parts:
            assert 0.0 < part(b) <= total
        b.enable_timing(False)
        p.run(b, F)
        assert all(ms(b) == -1.0 for ms in spans)
    finally:
        b.close()


def test_surface_timing(gpu, data):
    sf = data[2]
    b = make(gpu, data)
    try:
        assert b.surface_ms() == -1.0
        b.dyn_source_from_surfaces(sf.p, F, *sf.args())
        assert b.surface_ms() == -1.0
        b.enable_timing()
        b.dyn_source_from_surfaces(sf.p, F, *sf.args())
        assert b.surface_ms() > 0.0
        b.enable_timing(False)
        b.dyn_source_from_surfaces(sf.p, F, *sf.args())
        assert b.surface_ms() == -1.0
    finally:
        b.close()


def test_probe_of_no_frames_is_a_last_probe(gpu, data):
    """the probe stores its run before it launches anything: a pick of 0 frames may follow a probe of 0 frames"""
    lib = gpu.lib
    rate = gpu.ScrollDynRate(gpu.SCROLL_DYN_RATE_FRAME, 1 << 20, 0, 0)
    b = make(gpu, data)
    try:
        assert lib.scroll_batch_dyn_pick(b.h, 0, ctypes.byref(rate), None, None) == gpu.SCROLL_ERR_CONFIG
        assert lib.scroll_batch_dyn_probe(b.h, 0, gpu.u8buf(bytes(QPS)), len(QPS), None) == 0
        assert lib.scroll_batch_dyn_pick(b.h, 0, ctypes.byref(rate), None, None) == 0
        assert lib.scroll_batch_dyn_pick(b.h, 1, ctypes.byref(rate), None, None) == gpu.SCROLL_ERR_CONFIG
        r = gpu.ScrollDynProbe()
        assert lib.scroll_batch_dyn_probe_result(b.h, 0, 0, 0, ctypes.byref(r)) == gpu.SCROLL_ERR_ARG
        assert b.dyn_probe_ms() == -1.0
    finally:
        b.close()


def test_retired_debug_bit_changes_no_dry_plan(gpu, data):
    """SCROLL_DEBUG_DYN_NOCAVLC is retired (no kernel reads it) and has the
    value of k_plan's PLAN_SIZE flag: the probe's and the mask's state pass
    must not see it.  A k_plan that saw it would skip its state phase and leave
    the pass's NalDesc / DynFrame / PlanPending as they were: unwritten in a
    fresh batch, the previous offsets' after set_offsets.  So the flag is set
    before a fresh batch's first probe and mask, its offsets then change, and
    both takes are compared with those of a second fresh batch without it"""
    moved = OFFS[::-1] + 20

    def taken(b):
        res = b.dyn_probe(F, QPS)
        b.dyn_mask(F, apply=False)
        return res, b.dyn_mask_result(F), b.dyn_mask_map(F, RECT[2], RECT[3])

    def takes(flag):
        b = make(gpu, data)
        try:
            if flag:
                b.set_debug(flag)
            first = taken(b)
            b.set_offsets(moved)
            return first, taken(b)
        finally:
            b.close()

    plain, flagged = takes(0), takes(gpu.SCROLL_DEBUG_DYN_NOCAVLC)
    for take in plain:
        assert (take[0]["valid"] == 1).all() and (take[0]["bits"] > 0).all()
    # the premise: the moved offsets change what the state pass leaves behind
    assert plain[0][0].tobytes() != plain[1][0].tobytes() or plain[0][2].tobytes() != plain[1][2].tobytes()
    for a, c in zip(plain[0] + plain[1], flagged[0] + flagged[1]):
        assert a.dtype == c.dtype and a.tobytes() == c.tobytes()
