"""GPU: metrics.evaluate(ciede2000=True) -- the two CIEDE2000 columns equal metrics.ciede2000 of the separately quantized output
bit for bit (at batch size 1 and 2, per value of an alpha sweep, from the resized output under resize=True, on two ranks), and
ciede2000=False returns exactly what the call returned before the argument existed.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_harness import in_child as _in_child, model as _model, two_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
# two images that pad to 40 x 56 with different crops, then two of 32 x 48
SIZES = [(36, 52), (33, 50), (32, 48), (32, 48)]
KEYS = ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")
LKEYS = ("lpips", "lpips_gt_mean")
CKEYS = ("ciede2000", "ciede2000_gt_mean")


def _pairs(seed=13, sizes=SIZES, gt_sizes=None):
    rng = np.random.default_rng(seed)
    pairs = []
    for i, (h, w) in enumerate(sizes):
        low = torch.from_numpy(rng.random((3, h, w), dtype=np.float32) * 0.6 + 0.05)
        gh, gw = (h, w) if gt_sizes is None else gt_sizes[i]
        if (gh, gw) == (h, w):
            gt = np.clip(low.numpy() * 1.5 + rng.normal(0, 0.05, (3, h, w)), 0, 1)
        else:
            gt = rng.random((3, gh, gw))
        pairs.append((low, torch.from_numpy((gt * 255).astype(np.uint8))))
    return pairs


def _quantized(model, pairs, alpha=1.0, **attrs):
    """the model's own output per image (batch 1), quantized by to_uint8 on its own"""
    import hvi_cidnet_amd as P
    t = model.trans
    old = (model.training, t.gated, t.alpha_s, t.gated2, t.alpha)
    model.eval()
    t.gated, t.alpha_s, t.gated2, t.alpha = attrs.get("gated", False), 1.3, attrs.get("gated2", False), alpha
    out = []
    with torch.no_grad():
        for low, _ in pairs:
            x, (h, w) = P.pad_to_multiple(low.unsqueeze(0).cuda(), 8)
            out.append(P.metrics.to_uint8(model(x), (h, w)))
    model.train(old[0])
    t.gated, t.alpha_s, t.gated2, t.alpha = old[1:]
    return out


def _expected(qs, pairs, resize=False):
    import hvi_cidnet_amd as P
    out = {k: [] for k in CKEYS}
    for q, (_, g) in zip(qs, pairs):
        g = g.unsqueeze(0).cuda()
        if resize:
            q = P.metrics.resize_u8(q, g.shape[-2:])
        out["ciede2000"].append(P.ciede2000(q, g).item())
        out["ciede2000_gt_mean"].append(P.ciede2000(q, g, gt_mean=True).item())
    return out


def test_columns_equal_ciede2000_of_the_quantized_output(dev):
    _in_child(_case_columns)


def _case_columns():
    import hvi_cidnet_amd as P
    m, pairs = _model(), _pairs()
    want = _expected(_quantized(m, pairs, gated=True), pairs)
    assert all(v > 0 for k in CKEYS for v in want[k]) and want["ciede2000"] != want["ciede2000_gt_mean"]
    before = P.evaluate(m, pairs, gated=True, batch_size=2)
    off = P.evaluate(m, pairs, gated=True, batch_size=2, ciede2000=False)
    assert off == before and tuple(off.per_image) == KEYS                  # the same keys, in the same order, the same values
    assert math.isnan(off.ciede2000) and math.isnan(off.ciede2000_gt_mean)
    assert off.ciede2000 is P.metrics.EvalResult.ciede2000 and off.ciede2000_gt_mean is P.metrics.EvalResult.ciede2000_gt_mean
    for bs in (1, 2):
        res = P.evaluate(m, pairs, gated=True, batch_size=bs, ciede2000=True)
        assert tuple(res.per_image) == KEYS + CKEYS
        for k in CKEYS:
            assert res.per_image[k] == want[k], (bs, k)
            assert getattr(res, k) == sum(res.per_image[k]) / len(pairs)
        for k in KEYS:                                                       # the other columns are untouched
            assert res.per_image[k] == before.per_image[k] and getattr(res, k) == getattr(before, k)
        assert math.isnan(res.lpips)
    assert m.trans.alpha == 1.0 and m.training


def test_alpha_sweep_scores_every_value(dev):
    _in_child(_case_sweep)


def _case_sweep():
    import hvi_cidnet_amd as P
    m, pairs = _model(), _pairs()
    alphas = [0.8, 1.0]
    sweep = P.evaluate(m, pairs, gated2=True, alpha=alphas, batch_size=2, ciede2000=True)
    assert [r.alpha for r in sweep] == alphas
    for a, r in zip(alphas, sweep):
        want = _expected(_quantized(m, pairs, alpha=a, gated2=True), pairs)
        for k in CKEYS:
            assert r.per_image[k] == want[k], (a, k)
    assert sweep[0].per_image["ciede2000"] != sweep[1].per_image["ciede2000"]


def test_resized_output_is_what_is_scored(dev):
    _in_child(_case_resize)


def _case_resize():
    import hvi_cidnet_amd as P
    m = _model()
    pairs = _pairs(sizes=[(36, 52), (32, 48)], gt_sizes=[(45, 61), (32, 48)])
    res = P.evaluate(m, pairs, gated=True, resize=True, ciede2000=True)
    assert res.resized == [0] and tuple(res.per_image) == KEYS + CKEYS
    want = _expected(_quantized(m, pairs, gated=True), pairs, resize=True)
    for k in CKEYS:
        assert res.per_image[k] == want[k], k


def test_key_order_with_lpips(dev):
    _in_child(_case_order)


def _case_order():
    import hvi_cidnet_amd as P
    m, pairs = _model(), _pairs(sizes=SIZES[2:])
    both = P.evaluate(m, pairs, gated=True, lpips=P.LpipsParams.random(), ciede2000=True)
    assert tuple(both.per_image) == KEYS + LKEYS + CKEYS
    alone = P.evaluate(m, pairs, gated=True, ciede2000=True)
    for k in CKEYS:
        assert both.per_image[k] == alone.per_image[k] and getattr(both, k) == getattr(alone, k)
    assert both.lpips > 0
    sized = P.evaluate(m, pairs, gated=True, lpips=P.LpipsParams.random(), ciede2000=True, resize=True)
    assert sized.resized == [] and tuple(sized.per_image) == KEYS + LKEYS + CKEYS


def test_the_gt_mean_scale_is_formed_once_per_scored_batch(dev):
    _in_child(_case_scale_once)


def _case_scale_once():
    """PSNR/SSIM, LPIPS and CIEDE2000 under GT mean share one scale: the launcher runs once per scored batch and alpha"""
    import collections
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    counts, call = collections.Counter(), L.call

    def counting(name, *args):
        counts[name] += 1
        return call(name, *args)
    L.call = counting
    m, pairs, prm = _model(), _pairs(), P.LpipsParams.random()
    # batch_size=2 over SIZES: the first two images pad alike but are cropped apart, so each is scored alone; the last two
    # are one batch
    scored = 3
    res = P.evaluate(m, pairs, gated=True, batch_size=2, lpips=prm, ciede2000=True)
    assert tuple(res.per_image) == KEYS + LKEYS + CKEYS
    assert counts["cidnet_metric_gt_mean_scale"] == scored
    assert counts["cidnet_metric_psnr_ssim"] == 2 * scored and counts["cidnet_metric_ciede2000_u8"] == 2 * scored
    counts.clear()
    alphas = [0.8, 1.0]
    sweep = P.evaluate(m, pairs, gated2=True, alpha=alphas, batch_size=2, lpips=prm, ciede2000=True)
    assert [r.alpha for r in sweep] == alphas
    assert counts["cidnet_metric_gt_mean_scale"] == len(alphas) * scored
    assert counts["cidnet_metric_psnr_ssim"] == 2 * len(alphas) * scored


def test_two_ranks_shard_the_evaluation(dev):
    """two ranks sharing the GPU over gloo: both return exactly the single-process values"""
    got = two_ranks(_case_three)
    ref = _in_child(_case_three)
    assert got[0] == ref and got[1] == ref
    assert all(v > 0 for v in ref[5]["ciede2000"])


def _case_three():
    import hvi_cidnet_amd as P
    r = P.evaluate(_model(), _pairs(sizes=SIZES[:3]), gated=True, batch_size=1, ciede2000=True)
    return (r.alpha, r.psnr, r.ssim, r.ciede2000, r.ciede2000_gt_mean, r.per_image)
