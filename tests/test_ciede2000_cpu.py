"""CPU: the numpy restatement of CIEDE2000 (tests/ciede2000_ref.py) against the 34 published pairs of Sharma, Wu and Dalal,
its Lab of black and white, and the package's host-built level table against the restatement's linearisation."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_ref as R  # noqa: E402


def test_reference_reproduces_the_published_pairs_in_both_orders():
    """the table holds four decimals: 5e-5 of rounding, 5.1e-5 asked"""
    lab1, lab2, want = R.SHARMA[:, 0:3].T, R.SHARMA[:, 3:6].T, R.SHARMA[:, 6]
    for a, b in ((lab1, lab2), (lab2, lab1)):
        got = R.delta_e(a, b)
        assert np.abs(got - want).max() <= 5.1e-5, np.abs(got - want).max()


def test_level_table_equals_the_reference_linearisation_bit_for_bit():
    from hvi_cidnet_amd import metrics as M
    t = M.ciede2000_tables()
    assert t.shape == (256,) and t.dtype == np.float64
    assert np.array_equal(t, R.linearize(np.arange(256) / 255.0))
    assert t[0] == 0.0 and t[255] == 1.0 and np.all(np.diff(t) > 0)
    assert 10 / 255.0 < 0.04045 < 11 / 255.0 and t[10] == (10 / 255.0) / 12.92                    # either side of the threshold
    assert abs(t[11] - ((11 / 255.0 + 0.055) / 1.055) ** 2.4) < 1e-17
    assert M.ciede2000_tables() is t and not t.flags.writeable


def test_reference_lab_of_black_and_white():
    black = R.rgb2lab(np.zeros((3, 1), dtype=np.uint8))[:, 0]
    assert np.array_equal(black, np.zeros(3))
    white = R.rgb2lab(np.full((3, 1), 255, dtype=np.uint8))[:, 0]
    assert abs(white[0] - 100.0) <= 1e-12


def test_plan_query_contract():
    """cidnet_metric_ciede2000_plan (host only): blocks x pixels cover the image exactly once, the workspace is one double per
    block, and bad arguments are the library's errors with nothing written"""
    import ctypes
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    q, ws = L.raw("cidnet_metric_ciede2000_plan"), L.raw("cidnet_metric_ciede2000_ws_bytes")
    for h, w in ((1, 1), (7, 13), (32, 32), (33, 67), (400, 600), (1024, 1025)):
        out = (ctypes.c_int * 4)(-7, -7, -7, -7)
        assert q(h, w, out, 3) == 0 and out[3] == -7
        blocks, per, lds = out[0], out[1], out[2]
        assert per % 4 == 0 and blocks * per >= h * w > (blocks - 1) * per and 0 < lds <= 64 * 1024
        assert ws(3, h, w) == 3 * blocks * 8
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    for bad in ((0, 8), (8, 0), (-1, 8)):
        assert q(*bad, out, 3) == -1 and ws(1, *bad) == 0
    assert q(8, 8, None, 3) == -1 and q(8, 8, out, 2) == -1
    assert q(65536, 65536, out, 3) == -2 and ws(0, 8, 8) == 0
    assert list(out) == [-7] * 4
