"""h264scroll.pick_qp on hand-made probe results: the smallest total squared
error among the candidates that fit, ties, nothing fits, masked frames."""
import numpy as np

import h264scroll as hs

QPS = [20, 26, 32, 38]


def _res(rows):
    """rows: [frames][candidates] of (sse3, bits, valid)"""
    r = np.zeros((1, len(rows), len(QPS)), dtype=hs._probe_dtype())
    for f, row in enumerate(rows):
        for k, (sse, bits, valid) in enumerate(row):
            r[0, f, k] = (sse, bits, 0, valid)
    return r


def test_pick_qp():
    rows = [
        # the error falls with the bits: the best that fits 1000 bits is QP 26
        [((10, 1, 1), 1500, 1), ((20, 2, 2), 900, 1), ((40, 4, 4), 500, 1), ((80, 8, 8), 100, 1)],
        # nothing fits
        [((1, 0, 0), 5000, 1), ((2, 0, 0), 4000, 1), ((3, 0, 0), 3000, 1), ((4, 0, 0), 2000, 1)],
        # a tie in the total error (30 = 10 + 10 + 10): the fewer bits win
        [((30, 0, 0), 800, 1), ((10, 10, 10), 700, 1), ((0, 0, 30), 700, 1), ((99, 0, 0), 10, 1)],
        # a frame without a dynamic NAL
        [((0, 0, 0), 0, 0)] * 4,
        # exactly at the limit fits; a better candidate that is masked does not count
        [((1, 1, 1), 1000, 0), ((5, 5, 5), 1000, 1), ((9, 9, 9), 999, 1), ((9, 9, 9), 1, 1)],
    ]
    got = hs.pick_qp(_res(rows), QPS, 1000)
    assert got.dtype == np.int32 and got.shape == (1, 5)
    assert got.tolist() == [[26, -1, 26, -1, 26]]
    # everything fits: the smallest error
    assert hs.pick_qp(_res(rows), QPS, 1 << 30).tolist() == [[20, 20, 26, -1, 26]]
    # a plain array without the valid field, one frame
    r = np.zeros((4,), dtype=[("sse", np.uint64, 3), ("bits", np.uint32), ("nonzero", np.uint32)])
    r["bits"] = [40, 30, 20, 10]
    r["sse"][:, 0] = [1, 2, 3, 4]
    assert int(hs.pick_qp(r, QPS, 25)) == 32
    # sums past 2^32 per plane stay ordered
    big = _res([[((1 << 40, 0, 0), 1, 1), ((1 << 40, 0, 1), 1, 1), (((1 << 40) - 1, 0, 0), 2, 1), ((1 << 41, 0, 0), 1, 1)]])
    assert hs.pick_qp(big, QPS, 10).tolist() == [[32]]
