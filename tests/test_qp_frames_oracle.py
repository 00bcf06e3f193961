"""The premise the per-frame QP of the plain dynamic rect rests on
(tests/test_gpu_qp_frames.py): prediction is from the static pictures only,
so frame f's dynamic NAL out of an or_compose_dyn run with a QP per frame is
frame f's NAL of the run with every frame at that QP.  Oracle only."""
from probehelp import oracle_probe, synth
from qpfhelp import oracle_qp_frames
from reconhelp import random_refs


def test_frame_nal_is_the_uniform_runs(oracle):
    w, h, rect = 96, 96, (1, 1, 4, 4)
    qps, offs = [12, 30, 0, 51], [0, 5, 40, 96]
    R = random_refs(w, h, 11)
    src = synth(oracle, 1, len(offs), rect)[0]
    mixed, frames = oracle_qp_frames(oracle, w, h, offs, rect, src, R, qps)
    nals = set()
    for f, qp in enumerate(qps):
        uniform = oracle_probe(oracle, w, h, offs, rect, src, R, qp, decode=False)[1]
        assert frames[f]["nal"] == uniform[f]["nal"], (f, qp)
        # ... and it is that QP's NAL, not another's: the four runs differ in this frame
        nals.add(uniform[f]["nal"])
        others = [oracle_probe(oracle, w, h, offs, rect, src, R, q, decode=False)[1][f]["nal"]
                  for q in qps if q != qp]
        assert frames[f]["nal"] not in others
    assert len(nals) == len(qps)
    assert mixed == b"".join(fr["data"] for fr in frames)
