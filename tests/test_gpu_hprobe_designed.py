"""k_hdyn_probe (probe_row of csrc/probe_block.h) on the designed corpus
(tests/designed.py): the rect under hints without hint rects, EXACT, one MB
row lower in the odd frames whose offset pays for it
(test_gpu_designed.hinted_plan), three candidates a case with the case's own
QP among them at a different index per case, both streams, and one case at
eight.  bits, nonzero and the squared errors against tests/hprobehelp.py,
integer-exact; tests/test_probe_designed.py pins that yardstick to the plain
one on these cases.  Run on an MI355X: -m gpu."""
import numpy as np
import pytest

import designed as dz
import designedprobe as dp
from hprobehelp import check, expect_stream
from reconhelp import ArrayRefs
from test_gpu_designed import SLOT, hinted_plan
from test_gpu_dyn import gpu  # noqa: F401
from test_gpu_hprobe import apply_plans, load, make_batch

pytestmark = pytest.mark.gpu


def run(gpu, oracle, name, qps):
    c = dz.cases(oracle)[name]
    assert c.qp in qps
    offs, plan_, _ = hinted_plan(c)
    plans = [[plan_[(s, f)] for f in range(c.F)] for s in range(2)]
    if c.F > 1:
        assert any(p[2][1] != dz.Y0 for p in plan_.values())
    h = c.h + 16                                      # room for the rect one row lower
    R = ArrayRefs([tuple(np.pad(p, ((0, 16 if k == 0 else 8), (0, 0)), constant_values=128)
                         for k, p in enumerate(c.R.planes[0]))] * 2)
    exp = [expect_stream(oracle, c.w, h, offs[s], plans[s], c.rw, c.rh, c.src[s], R, qps)[0] for s in range(2)]
    b = make_batch(gpu, c.w, h, c.rc, 2, c.F, R, slot=SLOT * c.rw * c.rh)
    apply_plans(b, plans)
    load(b, offs, c.src)
    res = b.dyn_probe(c.F, qps, hinted=True)
    b.close()
    assert res.shape == (2, c.F, len(qps))
    for s in range(2):
        check(res, s, exp[s])


@pytest.mark.parametrize("name", dp.HINTED)
def test_hinted_probe(gpu, oracle, name):
    run(gpu, oracle, name, dp.three_of(name))


def test_hinted_probe_eight_candidates(gpu, oracle):
    qps = dp.candidates("c_lengths_qp24")
    assert len(qps) == 8
    run(gpu, oracle, "c_lengths_qp24", qps)
