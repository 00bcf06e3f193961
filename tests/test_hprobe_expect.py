"""CPU checks behind the hinted QP probe (scroll_batch_dyn_probe_hinted,
DESIGN.md §3j "Under UI hints"): the expectation helper (tests/hprobehelp.py:
or_compose_hint_dyn + the test decoder + or_dyn_mb_levels_bits) pinned on two
designed cases, the identity
    rbsp_bits(NAL) = bits(q) + D(q) + C(frame),
    D(q) = len(se(q - 26)) - 1 if nonzero(q) > 0 else 0,
with its P_Skip caveat, and the new entry point's presence in the header, the
library and the Python wrapper.  No GPU."""
import inspect
import subprocess

import pytest

from hprobehelp import QPS6, case_a, case_b, case_expect
from hreconhelp import EXACT, PSKIP, SPEC

# case A: (bits, nonzero) per position and QP 0 / 12 / 22 / 26 / 39 / 51, the same in every mode
CASE_A = [[(23081, 1529), (15998, 1517), (11080, 1470), (9362, 1413), (5460, 1072), (2159, 370)],
          [(23077, 1531), (16046, 1510), (11178, 1443), (9420, 1390), (5513, 1045), (2245, 404)],
          [(23243, 1530), (16072, 1512), (11204, 1455), (9382, 1410), (5522, 1056), (2378, 436)]]
CASE_A_C = {EXACT: [481, 481, 481], SPEC: [481, 481, 481], PSKIP: [461, 455, 455]}
# case B: (bits, nonzero, PSKIP skips, PSKIP C) per QP; 26 and 39 as 51
CASE_B = [(9850, 1806, 0, 205), (3594, 657, 0, 205), (25, 1, 5, 177), (6, 0, 6, 169), (6, 0, 6, 169),
          (6, 0, 6, 169)]


@pytest.mark.parametrize("mode", [EXACT, PSKIP, SPEC])
def test_case_a(oracle, mode):
    exp, _ = case_expect(oracle, case_a(oracle, mode))
    for f in range(3):
        assert [(e["bits"], e["nonzero"]) for e in exp[f]] == CASE_A[f], f
        assert [e["C"] for e in exp[f]] == [CASE_A_C[mode][f]] * len(QPS6), f     # constant: the identity
        assert all(e["skips"] == 0 for e in exp[f])


@pytest.mark.parametrize("mode", [EXACT, PSKIP, SPEC])
def test_case_b(oracle, mode):
    exp, _ = case_expect(oracle, case_b(oracle, mode))
    assert [(e["bits"], e["nonzero"]) for e in exp[0]] == [t[:2] for t in CASE_B]
    if mode == PSKIP:
        assert [(e["skips"], e["C"]) for e in exp[0]] == [t[2:] for t in CASE_B]
        c0 = exp[0][0]["C"]
        for e in exp[0]:           # equal before an MB skips, strictly an upper bound once one does
            assert (e["C"] == c0) if e["skips"] == 0 else (e["C"] < c0)
    else:
        assert [e["C"] for e in exp[0]] == [273] * len(QPS6)
        assert all(e["skips"] == 0 for e in exp[0])


def test_entry_point_declared_exported_and_wrapped(scroll):
    assert "scroll_batch_dyn_probe_hinted" in scroll.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", scroll.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "scroll_batch_dyn_probe_hinted" in exported
    assert "hinted" in inspect.signature(scroll.Batch.dyn_probe).parameters
