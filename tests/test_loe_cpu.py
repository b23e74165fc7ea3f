"""CPU: the LOE oracle against itself (the histogram identity equals the pairwise definition), the sampler's contract
(metrics.loe_grid), the launch-plan query of the library (cidnet_metric_loe_plan: host only, no device is touched), and the
public surface that needs no device."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loe_ref as R  # noqa: E402

SHAPES = [(1, 1), (7, 13), (33, 67), (50, 78)]
_PLAN_FIELDS = ("rows", "cols", "blocks_per_image", "samples_per_block", "counter_bits", "lds_bytes")


def _pairs(h, w, seed):
    """(name, low, out) uint8 (3,h,w): random pairs; Le = 255 - L; a four-level L against random Le"""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    out = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    yield "random", low, out
    yield "inverted", low, 255 - np.repeat(low.max(axis=0, keepdims=True), 3, axis=0)
    four = (rng.integers(0, 4, (1, h, w)) * 80).astype(np.uint8)
    yield "four levels", np.repeat(four, 3, axis=0), out


@pytest.mark.parametrize("h,w", SHAPES)
def test_histogram_identity_equals_the_definition(h, w):
    for name, low, out in _pairs(h, w, 100 * h + w):
        for sample in (None, 50, 5):
            assert R.by_hist(low, out, sample) == R.brute(low, out, sample), (name, h, w, sample)


def test_oracle_on_cases_known_by_hand():
    one = np.full((3, 1, 1), 9, np.uint8)
    assert R.brute(one, one, None) == (0, 1)
    ramp = np.repeat(np.arange(12, dtype=np.uint8).reshape(1, 3, 4) * 20, 3, axis=0)
    assert R.brute(ramp, ramp, None) == (0, 12)
    # 12 distinct levels reversed: every ordered pair of distinct samples flips, the 12 pairs (x, x) do not
    assert R.brute(ramp, 255 - ramp, None) == (12 * 11, 12)
    # a constant low image against two levels, 5 and 7 samples: U(L) = 1 everywhere, U(Le) = 0 for the 5 * 7 (small, large) pairs
    two = np.zeros((3, 3, 4), np.uint8)
    two.reshape(3, -1)[:, 5:] = 200
    assert R.brute(np.full((3, 3, 4), 50, np.uint8), two, None) == (35, 12)


def test_loe_grid_contract():
    from hvi_cidnet_amd import metrics as M
    assert M.loe_grid(101, 157, 50) == (2, 50, 78)
    assert M.loe_grid(149, 100, 50) == (2, 74, 50)
    assert M.loe_grid(30, 40, 50) == (1, 30, 40)
    assert M.loe_grid(101, 157, None) == (1, 101, 157)
    assert M.loe_grid(400, 600) == (8, 50, 75)                             # sample defaults to 50
    for h, w, s in [(101, 157, 50), (149, 100, 50), (30, 40, 50), (7, 13, None), (1, 1, 50), (1024, 1024, 50)]:
        assert M.loe_grid(h, w, s) == R.grid(h, w, s)
        step, rows, cols = M.loe_grid(h, w, s)
        assert 1 <= step <= min(h, w) and (rows - 1) * step < h and (cols - 1) * step < w
    for bad in [(0, 5, 50), (5, 0, 50), (5, 5, 0)]:
        with pytest.raises(ValueError):
            M.loe_grid(*bad)


def _plan(h, w, step, n=8):
    """cidnet_metric_loe_plan -> (status, {field: value}); the buffer is prefilled so that unwritten fields show"""
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_int * 8)(*([-7] * 8))
    rc = _lib.lib().raw("cidnet_metric_loe_plan")(h, w, step, buf, n)
    vals = list(buf)
    if rc == 0:
        assert vals[6:] == [-7, -7]                                        # never past its own fields
    else:
        assert vals == [-7] * 8                                            # nothing is written on an error
    return rc, dict(zip(_PLAN_FIELDS, vals))


def test_plan_query_contract():
    from hvi_cidnet_amd import metrics as M
    for h, w, sample in [(1, 1, None), (7, 13, None), (30, 40, 50), (101, 157, 50), (149, 100, 50), (400, 600, 50),
                         (400, 600, None), (256, 257, None), (1024, 1024, None), (1024, 1024, 50), (4000, 6000, None),
                         (128, 128, None), (128, 129, None)]:
        step, rows, cols = M.loe_grid(h, w, sample)
        rc, p = _plan(h, w, step)
        what = (h, w, sample, p)
        assert rc == 0, what
        assert (p["rows"], p["cols"]) == (rows, cols), what
        assert p["blocks_per_image"] >= 1 and p["samples_per_block"] >= 1, what
        assert p["blocks_per_image"] * p["samples_per_block"] >= rows * cols, what
        assert (p["blocks_per_image"] - 1) * p["samples_per_block"] < rows * cols, what      # no block without a sample
        assert p["counter_bits"] in (16, 32) and p["samples_per_block"] < 2 ** p["counter_bits"], what
        assert 0 <= p["lds_bytes"] <= 160 * 1024, what
        if p["counter_bits"] == 16:
            assert p["lds_bytes"] == 65536 * 2, what                       # the whole joint histogram, 16 bits a bin
    assert _plan(256, 257, 1)[1]["blocks_per_image"] > 1                   # what tests/test_loe_gpu.py's cap case relies on


def test_plan_query_bad_arguments():
    for h, w, step in [(0, 8, 1), (8, 0, 1), (-3, 8, 1), (8, 8, 0), (8, 8, -1), (8, 9, 9), (9, 8, 9)]:
        assert _plan(h, w, step)[0] == -1, (h, w, step)                    # CIDNET_ERR_ARG
    assert _plan(8, 9, 8)[0] == 0                                          # step == min(h, w) is a 1 x 1 grid
    assert _plan(8, 8, 1, n=5)[0] == -1                                    # too small a buffer: nothing written
    assert _plan(8, 8, 1, n=6)[0] == 0
    from hvi_cidnet_amd import _lib
    assert _lib.lib().raw("cidnet_metric_loe_plan")(8, 8, 1, None, 6) == -1
    assert _plan(40000, 40000, 1)[0] == -2                                 # CIDNET_ERR_SHAPE: more than 2^30 samples


def test_workspace_query_and_argument_checks_need_no_device():
    """the size query, and every refusal of the launcher that is decided before anything is launched"""
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    assert L.raw("cidnet_metric_loe_ws_bytes")(1) == 65536 * 4
    assert L.raw("cidnet_metric_loe_ws_bytes")(3) == 3 * 65536 * 4
    f = L.raw("cidnet_metric_loe_u8")
    p = ctypes.c_void_p(4096)                                              # never dereferenced: every call below is refused
    ws = 3 * 65536 * 4
    assert f(None, p, 1, 8, 8, 1, p, p, p, ws, None) == -1
    assert f(p, None, 1, 8, 8, 1, p, p, p, ws, None) == -1
    assert f(p, p, 1, 8, 8, 1, None, p, p, ws, None) == -1
    assert f(p, p, 1, 8, 8, 1, p, None, p, ws, None) == -1
    assert f(p, p, 1, 8, 8, 1, p, p, None, ws, None) == -1
    for B, h, w, step in [(0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 0), (1, 8, 9, 9)]:
        assert f(p, p, B, h, w, step, p, p, p, ws, None) == -1, (B, h, w, step)
    assert f(p, p, 3, 8, 8, 1, p, p, p, ws - 1, None) == -3                # CIDNET_ERR_WS


def test_unpaired_result_defaults_to_no_loe():
    from hvi_cidnet_amd import metrics as M
    r = M.UnpairedResult(alpha=1.0, niqe=4.0)
    assert math.isnan(r.loe) and "loe" not in r.per_image
    assert M.UnpairedResult(alpha=1.0, niqe=4.0, loe=7.5).loe == 7.5


def test_loe_is_exported_and_refuses_cpu_tensors():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    assert P.loe is M.loe and P.loe_counts is M.loe_counts and P.loe_grid is M.loe_grid
    a = torch.zeros((1, 3, 8, 8), dtype=torch.uint8)
    for fn in (P.loe, P.loe_counts):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, a)
