"""GPU: metrics.evaluate_unpaired (eval.py --unpaired + measure_niqe_bris.py on the device) -- per-image NIQE equals the
numpy restatement (tests/niqe_ref.py) applied to the model's own output quantized independently here, within the score
bar of tests/test_niqe_gpu.py (10 x niqe.npz: score_perturb); the model is left as it was found; alpha sweeps run the
trunk once per batch; the MSSA / TNSM variants; two ranks equal one.

Every case runs in a fresh spawned process, as in tests/test_evaluate_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import metrics_ref as QR  # noqa: E402
import niqe_ref as R  # noqa: E402
from evaluate_harness import in_child as _in_child, model as _model, two_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
PARAMS = os.path.join(HERE, "golden", "niqe_pris_params.npz")
# three images that pad to 200 x 296 (three different crops; the first needs no padding), then two of 192 x 288
SIZES = [(200, 296), (197, 290), (194, 295), (192, 288), (192, 288)]


def _bar():
    with np.load(os.path.join(HERE, "golden", "niqe.npz")) as z:
        return 10 * float(z["score_perturb"])


def _images(seed=9, sizes=SIZES):
    """low-light scenes with structure and grain, fp32 (3,h,w) on the CPU; every third one as a uint8 HWC array"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([0.35 + 0.25 * np.sin(9 * xx + c) * np.cos(7 * yy - c) for c in range(3)])
        img = np.clip(base + rng.normal(0, 0.06, (3, h, w)), 0.02, 0.9)
        u8 = (img * 255).astype(np.uint8)
        if i % 3 == 2:
            out.append(np.ascontiguousarray(u8.transpose(1, 2, 0)))
        else:
            out.append(torch.from_numpy(u8).float().div(255))
    return out


def _as_f32(img):
    if isinstance(img, np.ndarray):
        return torch.from_numpy(img).permute(2, 0, 1).float().div(255)
    return img


def _restated(model, images, gamma, alpha):
    """the model's own output per image (batch 1), quantized on the host, scored by the restatement"""
    import hvi_cidnet_amd as P
    with np.load(PARAMS) as z:
        mu, cov, win = z["mu_pris_param"], z["cov_pris_param"], z["gaussian_window"]
    t = model.trans
    old = (model.training, t.gated, t.alpha_s, t.gated2, t.alpha)
    model.eval()
    t.gated2, t.alpha = True, alpha
    out = []
    with torch.no_grad():
        for img in images:
            x, (h, w) = P.pad_to_multiple(_as_f32(img).unsqueeze(0).cuda(), 8)
            y = model(x ** gamma)
            y = y[0] if isinstance(y, tuple) else y
            out.append(R.niqe(QR.quantize(y[0].cpu().numpy(), h, w), mu, cov, win))
    model.train(old[0])
    t.gated, t.alpha_s, t.gated2, t.alpha = old[1:]
    return out


def _assert_close(res, ref):
    got, want = np.array(res.per_image["niqe"]), np.array(ref)
    print("niqe per image:", got.tolist(), "restatement:", want.tolist(), "max |diff|", np.abs(got - want).max())
    assert np.isfinite(want).all(), want
    assert np.abs(got - want).max() <= _bar(), (got, want)
    assert res.niqe == sum(res.per_image["niqe"]) / len(res.per_image["niqe"])


@pytest.mark.parametrize("cfg", [dict(gamma=1.0, alpha=1.0, batch_size=1), dict(gamma=1.3, alpha=0.85, batch_size=2)])
def test_evaluate_unpaired_matches_the_restatement_and_restores_the_model(dev, cfg):
    _in_child(_case_restatement_and_restore, cfg)


def _case_restatement_and_restore(cfg):
    import hvi_cidnet_amd as P
    m = _model()
    images = _images()
    t = m.trans
    t.gated, t.alpha_s, t.gated2, t.alpha = True, 1.1, False, 0.7
    m.train()
    m.HV_LCA1.eval()                                                        # a mixed-mode module tree comes back as it was
    modes = [mod.training for mod in m.modules()]
    k_state = (t._this_k_host, t._this_k_dev)
    res = P.evaluate_unpaired(m, images, PARAMS, **cfg)                     # the parameter file by path
    assert isinstance(res, P.metrics.UnpairedResult) and res.alpha == cfg["alpha"]
    assert [mod.training for mod in m.modules()] == modes
    assert (t.gated, t.alpha_s, t.gated2, t.alpha) == (True, 1.1, False, 0.7)
    assert (t._this_k_host, t._this_k_dev) == k_state
    assert res.names == list(range(len(images)))
    # evaluate_unpaired leaves trans.gated as it finds it (eval.py --unpaired sets gated2 and alpha only)
    ref = _restated(m, images, cfg["gamma"], cfg["alpha"])
    _assert_close(res, ref)


def test_batch_sizes_agree(dev):
    _in_child(_case_batch_sizes)


def _case_batch_sizes():
    import hvi_cidnet_amd as P
    m = _model()
    images = _images()
    prm = P.load_niqe_params(PARAMS)
    r1 = P.evaluate_unpaired(m, images, prm, alpha=0.9, gamma=1.2, batch_size=1)
    r3 = P.evaluate_unpaired(m, images, prm, alpha=0.9, gamma=1.2, batch_size=3)
    assert r1.per_image["niqe"] == r3.per_image["niqe"] and r1.niqe == r3.niqe


def test_alpha_sweep_runs_the_trunk_once(dev):
    _in_child(_case_alpha_sweep)


def _case_alpha_sweep():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib
    m = _model()
    images = _images(sizes=[(192, 288)] * 4)
    prm = P.load_niqe_params(PARAMS)
    alphas = [0.8, 0.9, 1.0]
    single = [P.evaluate_unpaired(m, images, prm, alpha=a, batch_size=2) for a in alphas]
    L = _lib.lib()
    seen = {}
    orig = L.call

    def spy(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return orig(name, *args)
    L.call = spy
    try:
        sweep = P.evaluate_unpaired(m, images, prm, alpha=alphas, batch_size=2)
    finally:
        L.call = orig
    assert seen["cidnet_hvit_fwd"] == 2                                    # one trunk per batch of two
    assert seen["cidnet_phvit_fwd"] == 2 * len(alphas)
    assert seen["cidnet_metric_to_uint8"] == 2 * len(alphas)
    assert seen["cidnet_metric_niqe_features"] == 2 * len(alphas)
    assert [r.alpha for r in sweep] == alphas
    for a, b in zip(sweep, single):
        assert a == b
    assert m.trans.alpha == 1.0 and m.training and not m.trans.gated2
    _assert_close(sweep[1], _restated(m, images, 1.0, 0.9))


@pytest.mark.parametrize("cls_name", ["CIDNet_MSSA", "CIDNet_TNSM"])
def test_variants(dev, cls_name):
    _in_child(_case_variant, cls_name)


def _case_variant(cls_name):
    import hvi_cidnet_amd as P
    m = _model(cls_name)
    images = _images(sizes=SIZES[:3])
    res = P.evaluate_unpaired(m, images, PARAMS, alpha=0.85, batch_size=2)
    _assert_close(res, _restated(m, images, 1.0, 0.85))
    sweep = P.evaluate_unpaired(m, images, PARAMS, alpha=[0.85], batch_size=2)      # the factored trunk + PHVIT
    assert sweep[0] == res
    assert m.training


def test_small_images_are_refused(dev):
    _in_child(_case_small)


def _case_small():
    import hvi_cidnet_amd as P
    m = _model()
    with pytest.raises(ValueError, match="96 x 96"):
        P.evaluate_unpaired(m, [torch.rand(3, 64, 128)], PARAMS)
    with pytest.raises(ValueError, match="niqe_pris_params.npz"):
        P.evaluate_unpaired(m, [torch.rand(3, 96, 96)], None)
    assert m.training


@pytest.mark.timeout(600)
def test_two_ranks_shard_the_evaluation(dev):
    """two ranks sharing the GPU over gloo: rank r scores images i % 2 == r, and both return exactly the single-process
    per-image values and means"""
    got = two_ranks(_case_sweep_of_all)
    ref = _in_child(_case_sweep_of_all)
    assert got[0] == ref and got[1] == ref


def _case_sweep_of_all():
    import hvi_cidnet_amd as P
    res = P.evaluate_unpaired(_model(), _images(), PARAMS, alpha=[0.9, 1.0], batch_size=1)
    return [(r.alpha, r.niqe, r.per_image) for r in res]
