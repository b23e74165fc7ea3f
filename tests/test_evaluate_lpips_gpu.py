"""GPU: metrics.evaluate(lpips=) -- the LPIPS columns equal metrics.lpips of the separately quantized output bit for bit (at
batch size 1 and 2, per value of an alpha sweep, from the resized output under resize=True), and lpips=None returns exactly
what the call returned before the argument existed.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402

pytestmark = pytest.mark.gpu
# two images that pad to 40 x 56 with different crops, then two of 32 x 48: every one at least 31 x 31
SIZES = [(36, 52), (33, 50), (32, 48), (32, 48)]
KEYS = ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")
LKEYS = ("lpips", "lpips_gt_mean")


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


def _expected(qs, pairs, prm, resize=False):
    import hvi_cidnet_amd as P
    out = {k: [] for k in LKEYS}
    for q, (_, g) in zip(qs, pairs):
        g = g.unsqueeze(0).cuda()
        if resize:
            q = P.metrics.resize_u8(q, g.shape[-2:])
        out["lpips"].append(P.lpips(q, g, prm).item())
        out["lpips_gt_mean"].append(P.lpips(q, g, prm, gt_mean=True).item())
    return out


def test_columns_equal_lpips_of_the_quantized_output(dev):
    _in_child(_case_columns)


def _case_columns():
    import hvi_cidnet_amd as P
    m, pairs, prm = _model(), _pairs(), P.LpipsParams.random()
    want = _expected(_quantized(m, pairs, gated=True), pairs, prm)
    assert all(v > 0 for k in LKEYS for v in want[k]) and want["lpips"] != want["lpips_gt_mean"]
    before = P.evaluate(m, pairs, gated=True, batch_size=2)
    none = P.evaluate(m, pairs, gated=True, batch_size=2, lpips=None)
    assert none == before and tuple(none.per_image) == KEYS                # the same keys, in the same order, the same values
    assert math.isnan(none.lpips) and math.isnan(none.lpips_gt_mean)
    for bs in (1, 2):
        res = P.evaluate(m, pairs, gated=True, batch_size=bs, lpips=prm)
        assert tuple(res.per_image) == KEYS + LKEYS
        for k in LKEYS:
            assert res.per_image[k] == want[k], (bs, k)
            assert getattr(res, k) == sum(res.per_image[k]) / len(pairs)
        for k in KEYS:                                                       # the other columns are untouched
            assert res.per_image[k] == before.per_image[k] and getattr(res, k) == getattr(before, k)
    with pytest.raises(ValueError, match="31 x 31"):
        P.evaluate(m, _pairs(sizes=[(24, 40)]), lpips=prm)
    with pytest.raises(ValueError, match="neither file is shipped"):
        P.evaluate(m, pairs, lpips="alex.pth")
    assert m.trans.alpha == 1.0 and m.training


def test_paths_load_the_parameters(dev, tmp_path):
    _in_child(_case_paths, str(tmp_path))


def _case_paths(tmp):
    import hvi_cidnet_amd as P
    prm = P.LpipsParams.random(seed=5)
    alex = {f"features.{i}.{n}": t for l, i in enumerate((0, 3, 6, 8, 10))
            for n, t in (("weight", prm.weights[l]), ("bias", prm.biases[l]))}
    heads = {f"lin{l}.model.1.weight": prm.heads[l].view(1, -1, 1, 1) for l in range(5)}
    paths = (os.path.join(tmp, "alexnet.pth"), os.path.join(tmp, "alex.pth"))
    torch.save(alex, paths[0])
    torch.save(heads, paths[1])
    m, pairs = _model(), _pairs(sizes=SIZES[2:])
    a, b = P.evaluate(m, pairs, lpips=paths), P.evaluate(m, pairs, lpips=prm)
    assert a == b and a.lpips > 0


def test_alpha_sweep_scores_every_value(dev):
    _in_child(_case_sweep)


def _case_sweep():
    import hvi_cidnet_amd as P
    m, pairs, prm = _model(), _pairs(), P.LpipsParams.random()
    alphas = [0.8, 1.0]
    sweep = P.evaluate(m, pairs, gated2=True, alpha=alphas, batch_size=2, lpips=prm)
    assert [r.alpha for r in sweep] == alphas
    for a, r in zip(alphas, sweep):
        want = _expected(_quantized(m, pairs, alpha=a, gated2=True), pairs, prm)
        for k in LKEYS:
            assert r.per_image[k] == want[k], (a, k)
    assert sweep[0].per_image["lpips"] != sweep[1].per_image["lpips"]
    assert sweep == [P.evaluate(m, pairs, gated2=True, alpha=a, batch_size=2, lpips=prm) for a in alphas]


def test_resized_output_is_what_is_scored(dev):
    _in_child(_case_resize)


def _case_resize():
    import hvi_cidnet_amd as P
    m, prm = _model(), P.LpipsParams.random()
    pairs = _pairs(sizes=[(36, 52), (32, 48)], gt_sizes=[(45, 61), (32, 48)])
    res = P.evaluate(m, pairs, gated=True, resize=True, lpips=prm)
    assert res.resized == [0] and tuple(res.per_image) == KEYS + LKEYS
    want = _expected(_quantized(m, pairs, gated=True), pairs, prm, resize=True)
    for k in LKEYS:
        assert res.per_image[k] == want[k], k
