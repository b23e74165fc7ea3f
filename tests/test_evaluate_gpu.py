"""GPU: metrics.evaluate (eval.py + measure.py on the device) -- per-image values equal the fp64 restatement applied to
the model's own output, the model is left as it was found, alpha sweeps run the trunk once per batch, the MSSA / TNSM
variants, evaluation between training steps, and data-parallel sharding over two ranks.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cidnet_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as R  # noqa: E402
from evaluate_harness import in_child as _in_child, model as _model, two_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
# four images that pad to 40 x 56 (three different crops), then two of 32 x 48
SIZES = [(36, 52), (36, 52), (33, 50), (40, 56), (32, 48), (32, 48)]


def _pairs(seed=9, sizes=SIZES):
    """(low fp32 (3,h,w) on the CPU, gt in one of the accepted forms) and the gt as uint8 (3,h,w) numpy"""
    rng = np.random.default_rng(seed)
    pairs, gts = [], []
    for i, (h, w) in enumerate(sizes):
        low = torch.from_numpy(rng.random((3, h, w), dtype=np.float32) * 0.6 + 0.05)
        gt = np.clip(low.numpy() * 1.5 + rng.normal(0, 0.05, (3, h, w)), 0, 1)
        gt8 = (gt * 255).astype(np.uint8)
        form = i % 3
        if form == 0:
            g = np.ascontiguousarray(gt8.transpose(1, 2, 0))              # HWC uint8, as PIL / numpy give it
        elif form == 1:
            g = torch.from_numpy(gt8)                                      # CHW uint8 tensor
        else:
            g = torch.from_numpy(gt8).float().div(255)                     # ToTensor() image
        pairs.append((low, g))
        gts.append(gt8)
    return pairs, gts


def _restated(model, pairs, gts, gamma, gated, alpha_s, gated2, alpha):
    """the model's own output per image (batch 1), quantized on the host, measured by the restatement"""
    import hvi_cidnet_amd as P
    t = model.trans
    old = (model.training, t.gated, t.alpha_s, t.gated2, t.alpha)
    model.eval()
    t.gated, t.alpha_s, t.gated2, t.alpha = gated, alpha_s, gated2, alpha
    out = {k: [] for k in ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")}
    with torch.no_grad():
        for (low, _), g in zip(pairs, gts):
            x, (h, w) = P.pad_to_multiple(low.unsqueeze(0).cuda(), 8)
            y = model(x ** gamma)
            y = y[0] if isinstance(y, tuple) else y
            q = R.quantize(y[0].cpu().numpy(), h, w)
            for gm, sfx in ((False, ""), (True, "_gt_mean")):
                out["psnr" + sfx].append(R.psnr(q, g, gt_mean=gm))
                out["ssim" + sfx].append(R.ssim(q, g, gt_mean=gm))
    model.train(old[0])
    t.gated, t.alpha_s, t.gated2, t.alpha = old[1:]
    return out


def _assert_close(res, ref):
    for k in ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean"):
        tol = 1e-6 if k.startswith("psnr") else 1e-10
        d = np.abs(np.array(res.per_image[k]) - np.array(ref[k])).max()
        assert d <= tol, (k, d)
        assert getattr(res, k) == sum(res.per_image[k]) / len(res.per_image[k])


@pytest.mark.parametrize("cfg", [dict(gamma=1.0, gated=False, alpha_s=1.3, gated2=False, alpha=1.0),
                                 dict(gamma=1.4, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)])
def test_evaluate_matches_the_restatement_and_restores_the_model(dev, cfg):
    _in_child(_case_restatement_and_restore, cfg)


def _case_restatement_and_restore(cfg):
    import hvi_cidnet_amd as P
    m = _model()
    pairs, gts = _pairs()
    t = m.trans
    t.gated, t.alpha_s, t.gated2, t.alpha = False, 1.1, False, 0.7
    m.train()
    m.HV_LCA1.eval()                                                        # a mixed-mode module tree comes back as it was
    modes = [mod.training for mod in m.modules()]
    k_state = (t._this_k_host, t._this_k_dev)
    res = P.evaluate(m, pairs, **cfg)
    assert isinstance(res, P.metrics.EvalResult) and res.alpha == cfg["alpha"]
    assert [mod.training for mod in m.modules()] == modes
    assert (t.gated, t.alpha_s, t.gated2, t.alpha) == (False, 1.1, False, 0.7)
    assert (t._this_k_host, t._this_k_dev) == k_state
    assert res.names == list(range(len(pairs)))
    _assert_close(res, _restated(m, pairs, gts, **cfg))


def test_batch_sizes_agree(dev):
    """batch_size 1 and 4 (the first four images pad to one size with three different crops): the per-image values agree
    bit for bit -- every kernel of the forward treats the samples of a batch independently"""
    _in_child(_case_batch_sizes)


def _case_batch_sizes():
    import hvi_cidnet_amd as P
    m = _model()
    pairs, _ = _pairs()
    r1 = P.evaluate(m, pairs, gamma=1.2, gated=True, batch_size=1)
    r4 = P.evaluate(m, pairs, gamma=1.2, gated=True, batch_size=4)
    for k in ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean"):
        a, b = np.array(r1.per_image[k]), np.array(r4.per_image[k])
        assert np.abs(a - b).max() <= (1e-3 if k.startswith("psnr") else 1e-5), k
        assert np.array_equal(a, b), (k, a - b)


def test_alpha_sweep_runs_the_trunk_once(dev):
    _in_child(_case_alpha_sweep)


def _case_alpha_sweep():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib
    m = _model()
    pairs, _ = _pairs(sizes=[(40, 56)] * 4)
    alphas = [0.8, 0.84, 1.0]
    single = [P.evaluate(m, pairs, gated2=True, alpha=a, batch_size=2) for a in alphas]
    L = _lib.lib()
    seen = {}
    orig = L.call

    def spy(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return orig(name, *args)
    L.call = spy
    try:
        sweep = P.evaluate(m, pairs, gated2=True, alpha=alphas, batch_size=2)
    finally:
        L.call = orig
    assert seen["cidnet_hvit_fwd"] == 2                                    # one trunk per batch of two
    assert seen["cidnet_phvit_fwd"] == 2 * len(alphas)
    assert seen["cidnet_metric_to_uint8"] == 2 * len(alphas)
    assert [r.alpha for r in sweep] == alphas
    for a, b in zip(sweep, single):
        assert a == b
    assert m.trans.alpha == 1.0 and m.training


@pytest.mark.parametrize("cls_name", ["CIDNet_MSSA", "CIDNet_TNSM"])
def test_variants(dev, cls_name):
    _in_child(_case_variant, cls_name)


def _case_variant(cls_name):
    import hvi_cidnet_amd as P
    m = _model(cls_name)
    pairs, gts = _pairs(sizes=SIZES[:3])
    cfg = dict(gamma=1.0, gated=False, alpha_s=1.3, gated2=True, alpha=0.85)
    res = P.evaluate(m, pairs, batch_size=2, **cfg)
    _assert_close(res, _restated(m, pairs, gts, **cfg))
    sweep = P.evaluate(m, pairs, batch_size=2, **{**cfg, "alpha": [0.85]})    # the factored trunk + PHVIT
    assert sweep[0] == res
    assert m.training


def test_uint8_low_scores_like_its_totensor_image(dev):
    """a uint8 HWC low image is converted as ToTensor() converts it on the host (a true division by 255), on every level"""
    _in_child(_case_uint8_low)


def _case_uint8_low():
    import hvi_cidnet_amd as P
    m = _model()
    h, w = SIZES[0]
    (_, gt), = _pairs(sizes=SIZES[:1])[0]
    low8 = np.random.default_rng(3).permutation(np.arange(h * w * 3) % 256).astype(np.uint8).reshape(h, w, 3)
    as_float = torch.from_numpy(low8).permute(2, 0, 1).float().div(255)
    assert P.evaluate(m, [(low8, gt)], gamma=1.3) == P.evaluate(m, [(as_float, gt)], gamma=1.3)


@pytest.mark.parametrize("use_graph", [False, True])
def test_evaluation_between_training_steps(dev, use_graph):
    """2 steps, evaluate(trainer.model), 2 steps == 4 steps bit for bit: the evaluation leaves the prepared weights, the
    captured graph and the back-pressure state alone"""
    _in_child(_case_between_training_steps, use_graph)


def _case_between_training_steps(use_graph):
    dev = torch.device("cuda:0")
    from hvi_cidnet_amd import evaluate
    from hvi_cidnet_amd.dp import DataParallelTrainer
    shape = (2, 3, 32, 48)
    batches = [(O.synthetic_batch(71 + i, shape).to(dev), O.synthetic_batch(81 + i, shape).to(dev)) for i in range(4)]
    pairs, _ = _pairs(sizes=SIZES[:3])
    finals = []
    for with_eval in (False, True):
        tr = DataParallelTrainer(_model(), lr=1e-3, n_buckets=3, use_graph=use_graph)
        losses = [float(tr.step(x, gt).item()) for x, gt in batches[:2]]
        if with_eval:
            res = evaluate(tr.model, pairs, gated=True, alpha=[0.9, 1.0], batch_size=2)
            assert len(res) == 2 and all(np.isfinite(r.psnr) for r in res)
            assert tr.model.training
        losses += [float(tr.step(x, gt).item()) for x, gt in batches[2:]]
        torch.cuda.synchronize()
        finals.append((losses, tr.flat_p.clone(), tr.flat_g.clone()))
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1])
    assert torch.equal(finals[0][2], finals[1][2])


@pytest.mark.timeout(600)
def test_two_ranks_shard_the_evaluation(dev):
    """two ranks sharing the GPU over gloo: rank r measures images i % 2 == r, and both return exactly the
    single-process per-image values and means"""
    got = two_ranks(_case_sweep_of_five)
    ref = _in_child(_case_sweep_of_five)
    assert got[0] == ref and got[1] == ref


def _case_sweep_of_five():
    import hvi_cidnet_amd as P
    pairs, _ = _pairs(sizes=SIZES[:5])
    res = P.evaluate(_model(), pairs, gated=True, alpha=[0.9, 1.0], batch_size=1)
    return [(r.alpha, r.psnr, r.ssim, r.psnr_gt_mean, r.ssim_gt_mean, r.per_image) for r in res]
