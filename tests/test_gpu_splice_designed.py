"""GPU parity of the pre-encoded MB splice on the designed corpus
(tests/splicedesign.py): k_splice_parse, k_splice_lanes and k_splice_stage
against the CPU restatement (or_compose_splice) byte for byte, on external
slices written from explicit coefficients, motion and QPs.
tests/test_splice_designed_oracle.py proves on the CPU that the corpus holds
every table entry, class pair, level triple, phase and limit these tests rely
on.  Stream s of a case splices its pictures in slice shape s, so one compose
reads a case on all three parse routes.  Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import splicedesign as sd
from test_gpu_splice import gpu_streams, plan_from, check_equal

pytestmark = pytest.mark.gpu

EXACT, PSKIP, SPEC = 0, 1, 2


@pytest.fixture(scope="module")
def gpu(scroll):
    if scroll.device_count() < 1:
        pytest.fail("no gfx950 device: " + scroll.last_error())
    return scroll


def _run(gpu, oracle, w, h, frames, offs, debug=0):
    _, want = plan_from(oracle, w, h, offs, frames)
    b, rc = gpu_streams(gpu, w, h, offs, frames, debug=debug)
    assert rc == 0, gpu.last_error()
    check_equal(b, want)
    for (s, f), (_, _, sp) in frames.items():
        assert b.splice_status(s, f) == 0, (s, f)
    b.close()


@pytest.mark.parametrize("mode", [EXACT, PSKIP, SPEC])
@pytest.mark.parametrize("name", sd.names())
def test_designed_case(gpu, oracle, name, mode):
    """each case in its slice shapes (one stream each) and each hint mode"""
    case = sd.cases()[name]
    _run(gpu, oracle, case.w, case.h, sd.frames_of(oracle, case, mode), sd.offsets_of(case))


@pytest.mark.parametrize("name", sd.names(refused=True))
def test_refused_frame_fails_its_stream_alone(gpu, oracle, scroll, name):
    """|mv| = 16384 and a level_prefix 16 code, in each slice shape: the
    oracle's status on both parsers, nothing committed; a stream without it
    composes"""
    case = sd.cases()[name]
    frames = sd.frames_of(oracle, case, SPEC)
    S = len(case.shapes) + 1
    offs = sd.offsets_of(case, S)
    b, rc = gpu_streams(gpu, case.w, case.h, offs, frames)
    assert rc == scroll.SCROLL_ERR_CONFIG
    for s in range(S - 1):
        assert b.splice_status(s, 0) == case.pics[0].status == scroll.SCROLL_SPLICE_ERR_SYNTAX, s
        assert b.output_size(s) == 0, s
    _, want = plan_from(oracle, case.w, case.h, offs[S - 1:], {})
    assert b.output(S - 1) == want[0]
    b.close()


def test_ep_dense_host_bytes_with_and_without_start_code(gpu, oracle):
    """the emulation-prevention case as host bytes: its one-slice pictures, one
    with and one without the Annex-B start code"""
    case = sd.cases()["e_epdense"]
    frames = sd.frames_of(oracle, case, SPEC, shapes=("one",))
    r, m, (x0, y0, w, h, nal) = frames[(0, 1)]
    assert nal[:4] == b"\x00\x00\x00\x01"
    frames[(0, 1)] = (r, m, (x0, y0, w, h, nal[4:]))
    _run(gpu, oracle, case.w, case.h, frames, sd.offsets_of(case, 1))


@pytest.mark.parametrize("align", [1, 10])
def test_ep_dense_by_device_pointer(gpu, oracle, align):
    """the same pictures, every shape, by device pointer at two alignments
    modulo 16: k_splice_unesc's 16-byte lines cut the 00 00 03 triples at
    other places than the host copy's"""
    from test_gpu_ipcm import Hip
    case = sd.cases()["e_epdense"]
    frames = sd.frames_of(oracle, case, SPEC)
    offs = sd.offsets_of(case)
    _, want = plan_from(oracle, case.w, case.h, offs, frames)
    total = sum(len(sp[4]) + 32 for (_, _, sp) in frames.values())
    dev = Hip().buf(total + 64, fill=0xA5)
    pos, specs = 0, []
    for (s, t), (_, _, sp) in sorted(frames.items()):
        nal = bytes(sp[4])
        pos = ((pos + 15) & ~15) + align
        dev.write(pos, nal)
        specs.append((s, t, sp[0], sp[1], sp[2], sp[3], dev.p + pos, len(nal)))
        pos += len(nal)
    S, F = offs.shape
    b = gpu.Batch(S, F, 16 << 20)
    for _ in range(S):
        b.add_stream(gpu.make_config(case.w, case.h))
    b.set_splices_device(specs)
    b.set_offsets(offs)
    b.compose(F)
    assert b.sync() == 0, gpu.last_error()
    check_equal(b, want)
    assert {sp[6] % 16 for sp in specs} == {align}
    b.close()
    dev.free()


def test_ep_dense_through_the_dynamic_emit(gpu, oracle, scroll):
    """the composed NALs' own emulation prevention with the EP list capped at
    4: every NAL goes through k_dyn_emit"""
    case = sd.cases()["e_epdense"]
    _run(gpu, oracle, case.w, case.h, sd.frames_of(oracle, case, PSKIP), sd.offsets_of(case),
         debug=scroll.SCROLL_DEBUG_DYN_EPCAP4)


def test_mixed_shapes_in_one_compose(gpu, oracle):
    """frames of different slice shapes in one compose, a frame without a
    splice between them: the lanes' list and the wave-uniform list are both
    non-empty in one launch"""
    pics = sd.cases()["w_walk"].pics + sd.cases()["l_levels"].pics[:1]
    order = [("one", "rows", "two"), ("rows", "two", "one"), ("two", "one", "rows")]
    frames = {}
    for s, shapes in enumerate(order):
        for t in range(6):
            if t % 2:
                continue                                   # no splice in the odd frames
            p = pics[(t // 2 + s) % len(pics)]
            frames[(s, t)] = ([], (EXACT, PSKIP, SPEC)[(s + t // 2) % 3],
                              (p.at[0], p.at[1], p.W, p.H, p.nal(oracle, shapes[t // 2])))
    offs = np.array([[30 + 2 * t + s for t in range(6)] for s in range(3)], np.int32)
    _run(gpu, oracle, 320, 256, frames, offs)
