"""GPU: CIEDE2000 on the device (csrc/ciede2000.hip through metrics.ciede2000_lab / ciede2000_map / ciede2000) against the numpy
restatement of tests/ciede2000_ref.py.

Tolerance against the restatement: 1e-9 absolute on every pixel of the map and on every mean.  Values are at most 128 and fp64
eps is 2.2e-16; away from the hue discontinuities the formula's conditioning is at most about 1e3, which gives about 3e-11, and
the same formula under two fp64 CPU math libraries differs by at most 4.4e-13 on random 400 x 600 pairs: the bar leaves three
decades over that.  Every image case first asserts that its inputs stay at least 1e-6 degrees away from the 180 degree
hue-difference discontinuity, so no pixel is left out of a comparison.  The observed maxima are printed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ciede2000_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
EDGE = 1e-6


def _rand(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _plan(h, w):
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_int * 3)()
    assert _lib.lib().raw("cidnet_metric_ciede2000_plan")(h, w, buf, 3) == 0
    return dict(zip(("blocks", "per_block", "lds"), buf))


def _tree(v):
    """the block tree of include/cidnet_hip.h over 256 values: per wave of 64 the butterfly, then the four waves in order"""
    v = np.asarray(v, dtype=np.float64).reshape(4, 64)
    for half in (32, 16, 8, 4, 2, 1):
        v = v[:, :half] + v[:, half:2 * half]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def fixed_order_mean(dmap):
    """(h,w) fp64 map -> the mean as the header documents the reduction"""
    d = np.asarray(dmap, dtype=np.float64).ravel()
    n = d.size
    blocks = -(-n // 1024)
    d = np.concatenate([d, np.zeros(blocks * 1024 - n)]).reshape(blocks, 256, 4)
    slots = []
    for x in range(blocks):
        t = np.zeros(256)
        for k in range(4):
            t = t + d[x, :, k]
        slots.append(_tree(t))
    slots = np.concatenate([slots, np.zeros(-(-blocks // 256) * 256 - blocks)]).reshape(-1, 256)
    t = np.zeros(256)
    for row in slots:
        t = t + row
    return _tree(t) / float(n)


def _check(dev, restored, gt, gt_mean=False, what=""):
    """uint8 numpy (B,3,h,w) pairs: the map and the mean of every image against the restatement -> (map, mean) as numpy"""
    from hvi_cidnet_amd import metrics as M
    for a, g in zip(restored, gt):
        assert R.hue_edge_distance(a, g, gt_mean) >= EDGE, what
    ta, tg = torch.from_numpy(np.ascontiguousarray(restored)).to(dev), torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
    dmap, mean = M.ciede2000_map(ta, tg, gt_mean), M.ciede2000(ta, tg, gt_mean)
    assert dmap.dtype == torch.float64 and mean.dtype == torch.float64 and dmap.device == ta.device
    assert tuple(dmap.shape) == (restored.shape[0],) + restored.shape[2:] and tuple(mean.shape) == (restored.shape[0],)
    dmap, mean = dmap.cpu().numpy(), mean.cpu().numpy()
    want = np.stack([R.image_map(a, g, gt_mean) for a, g in zip(restored, gt)])
    e_map = np.abs(dmap - want).max()
    e_mean = max(abs(mean[i] - want[i].mean()) for i in range(len(want)))
    print(f"ciede2000 {what} {restored.shape} gt_mean={gt_mean}: max |map - ref| = {e_map:.3e}, max |mean - ref| = {e_mean:.3e}")
    assert e_map <= TOL and e_mean <= TOL, (what, e_map, e_mean)
    return dmap, mean


def test_sharma_pairs_through_the_device(dev):
    from hvi_cidnet_amd import metrics as M
    lab1 = torch.from_numpy(np.ascontiguousarray(R.SHARMA[:, 0:3])).to(dev)
    lab2 = torch.from_numpy(np.ascontiguousarray(R.SHARMA[:, 3:6])).to(dev)
    want = R.SHARMA[:, 6]
    for a, b, ra, rb in ((lab1, lab2, R.SHARMA[:, 0:3].T, R.SHARMA[:, 3:6].T), (lab2, lab1, R.SHARMA[:, 3:6].T, R.SHARMA[:, 0:3].T)):
        got = M.ciede2000_lab(a, b).cpu().numpy()
        ref = R.delta_e(ra, rb)
        worst = 0.0
        for i in range(34):
            if i + 1 in R.SHARMA_ON_THE_EDGE:             # |h1' - h2'| is exactly 180 in real arithmetic: rounding picks the branch
                other = want[R.SHARMA_ON_THE_EDGE[i + 1] - 1]
                assert min(abs(got[i] - want[i]), abs(got[i] - other)) <= 5.1e-5, (i + 1, got[i])
                continue
            assert abs(got[i] - want[i]) <= 5.1e-5, (i + 1, got[i], want[i])
            assert abs(got[i] - ref[i]) <= TOL, (i + 1, got[i], ref[i])
            worst = max(worst, abs(got[i] - ref[i]))
        print(f"ciede2000_lab: max |device - ref| over the 32 pairs off the edge = {worst:.3e}")
    assert M.ciede2000_lab(lab1[:0], lab2[:0]).shape == (0,)
    with pytest.raises(RuntimeError, match=r"fp64 \(n,3\)"):
        M.ciede2000_lab(lab1.float(), lab2.float())


def test_tails_and_addressing(dev):
    p = _plan(33, 67)
    per = p["per_block"]
    assert p["blocks"] == -(-33 * 67 // per) and per % 4 == 0
    sizes = [(1, 1), (7, 13), (33, 67),
             (per // 32, 32),                              # exactly one full block
             (1, per + 1),                                 # a single pixel for the last block
             (3, 2 * per // 3 + 1),                        # an odd width: rows start at every alignment, a ragged last group
             (5, 4 * 61 + 3)]                              # a width that is no multiple of 4
    assert _plan(*sizes[3])["blocks"] == 1 and per // 32 * 32 == per
    assert _plan(*sizes[4])["blocks"] == 2 and sizes[6][1] % 4 == 3
    for i, (h, w) in enumerate(sizes):
        a, g = _rand(20 + i, 2, 3, h, w), _rand(40 + i, 2, 3, h, w)
        dmap, mean = _check(dev, a, g, what=f"{h}x{w}")
        for b in range(2):
            assert mean[b] == fixed_order_mean(dmap[b]), (h, w, b)


def _chart():
    """16 x 256: the 256 greys; the primaries, secondaries, black, white and levels 10 / 11 (either side of the 0.04045
    threshold); dark colours whose linear values and XYZ stay under the 0.008856 threshold; and random colours"""
    rng = np.random.default_rng(77)
    img = np.zeros((3, 16, 256), dtype=np.uint8)
    img[:, 0] = np.arange(256, dtype=np.uint8)
    fixed = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255),
             (10, 10, 10), (11, 11, 11), (10, 11, 10), (11, 10, 11), (10, 0, 0), (0, 11, 0), (0, 0, 11), (255, 10, 11)]
    img[:, 1] = np.array(fixed * 16, dtype=np.uint8).T
    img[:, 2:6] = rng.integers(0, 23, (3, 4, 256), dtype=np.uint8)           # level 22 -> 0.0080 linear: every f() is linear
    img[:, 6:8] = rng.integers(0, 64, (3, 2, 256), dtype=np.uint8)           # across the threshold of f()
    img[:, 8:] = rng.integers(0, 256, (3, 8, 256), dtype=np.uint8)
    return img


def _plane_sweep():
    """256 x 256: red = row, green = column, blue fixed"""
    img = np.empty((3, 256, 256), dtype=np.uint8)
    img[0] = np.arange(256, dtype=np.uint8)[:, None]
    img[1] = np.arange(256, dtype=np.uint8)[None, :]
    img[2] = 96
    return img


def test_colour_coverage(dev):
    from hvi_cidnet_amd import metrics as M
    sweep = _plane_sweep()
    mid = np.empty_like(sweep)
    mid[0], mid[1], mid[2] = 131, 117, 140
    _check(dev, sweep[None], mid[None], what="sweep vs mid colour")
    chart = _chart()
    black, white = np.zeros_like(chart), np.full_like(chart, 255)
    fwd = _check(dev, np.stack([chart, chart, chart]), np.stack([black, white, chart]), what="chart vs black / white / itself")
    assert fwd[0][0].min() >= 0 and fwd[0][0, 1, 6] == 0.0                    # black against black
    bwd = _check(dev, np.stack([black, white]), np.stack([chart, chart]), what="black / white vs chart")
    assert np.abs(fwd[0][:2] - bwd[0]).max() <= TOL and np.abs(fwd[1][:2] - bwd[1]).max() <= TOL       # symmetric within the bar
    for img in (chart, sweep, _rand(3, 3, 33, 67)):                           # identical images: exactly 0.0 everywhere
        t = torch.from_numpy(img).to(dev)
        assert torch.count_nonzero(M.ciede2000_map(t, t.clone())).item() == 0
        assert M.ciede2000(t, t.clone()).cpu().tolist() == [0.0]
    a, g = _rand(5, 1, 3, 33, 67), _rand(6, 1, 3, 33, 67)
    ab, ba = _check(dev, a, g, what="a vs g"), _check(dev, g, a, what="g vs a")
    assert np.abs(ab[0] - ba[0]).max() <= TOL and abs(ab[1][0] - ba[1][0]) <= TOL


def test_gt_mean(dev):
    rng = np.random.default_rng(11)
    h, w = 33, 67
    a = np.stack([rng.integers(0, 256, (3, h, w)), rng.integers(40, 140, (3, h, w)), rng.integers(100, 256, (3, h, w))]).astype(np.uint8)
    g = np.stack([rng.integers(0, 256, (3, h, w)), rng.integers(150, 256, (3, h, w)), rng.integers(0, 120, (3, h, w))]).astype(np.uint8)
    import metrics_ref as MR
    scaled = MR.gt_mean_image(a[1], g[1])
    assert (scaled == 255).mean() > 0.2                                        # image 1: much brighter gt, many values clip
    assert int(MR.gray(g[2]).sum()) < int(MR.gray(a[2]).sum())                 # image 2: scale < 1
    _, mean = _check(dev, a, g, gt_mean=True, what="gt mean")
    _, plain = _check(dev, a, g, what="plain")
    assert all(abs(mean[i] - plain[i]) > 1e-3 for i in range(3))
    for i in range(3):
        assert abs(mean[i] - R.mean_delta_e(a[i], g[i], gt_mean=True)) <= TOL


def test_determinism_and_batch_independence(dev):
    from hvi_cidnet_amd import metrics as M
    h, w = 40, 131                                                             # six blocks, a ragged last one
    assert _plan(h, w)["blocks"] == 6
    a, g = torch.from_numpy(_rand(8, 3, 3, h, w)).to(dev), torch.from_numpy(_rand(9, 3, 3, h, w)).to(dev)
    for gt_mean in (False, True):
        m1, m2 = M.ciede2000(a, g, gt_mean), M.ciede2000(a, g, gt_mean)
        d1, d2 = M.ciede2000_map(a, g, gt_mean), M.ciede2000_map(a, g, gt_mean)
        assert torch.equal(m1, m2) and torch.equal(d1, d2)
        for i in range(3):
            assert torch.equal(M.ciede2000(a[i], g[i], gt_mean), m1[i:i + 1])   # (3,h,w) inputs, alone
            assert torch.equal(M.ciede2000_map(a[i:i + 1], g[i:i + 1], gt_mean), d1[i:i + 1])
            assert m1[i].item() == fixed_order_mean(d1[i].cpu().numpy())
            assert abs(m1[i].item() - d1[i].mean().item()) <= TOL


def test_errors(dev):
    from hvi_cidnet_amd import _lib
    from hvi_cidnet_amd import metrics as M
    a = torch.from_numpy(_rand(1, 1, 3, 12, 12)).to(dev)

    def message(fn, *args):
        with pytest.raises(RuntimeError) as e:
            fn(*args)
        return str(e.value)
    bad = ((a.float(), a), (a, a.float()), (a.cpu(), a), (a, a.cpu()), (a, a[..., :11]), (a[0, :2], a[0, :2]))
    for fn in (M.ciede2000, M.ciede2000_map):
        for args in bad:                                                       # the checks and the messages of psnr_ssim
            assert message(fn, *args) == message(M.psnr_ssim, *args).replace("psnr / ssim", "ciede2000 / ciede2000_map")
    assert "take uint8 images (got torch.float32" in message(M.ciede2000, a.float(), a)
    assert "no CPU fallback" in message(M.ciede2000, a.cpu(), a) and "differ" in message(M.ciede2000, a, a[..., :11])
    q = _lib.lib().raw("cidnet_metric_ciede2000_plan")
    out = (ctypes.c_int * 3)(-7, -7, -7)
    for args in ((0, 8, out, 3), (8, -1, out, 3), (8, 8, None, 3), (8, 8, out, 2)):
        assert q(*args) == -1
    assert q(65536, 65536, out, 3) == -2 and list(out) == [-7] * 3
