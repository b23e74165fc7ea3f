"""CPU: the host side of LPIPS (hvi-cidnet_amd/metrics.py: LpipsParams, load_lpips_params, the size rule, the launchers'
shape checks, which return before any launch) and the properties of the restatement the GPU tests are measured against."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402

import hvi_cidnet_amd as P  # noqa: E402
from hvi_cidnet_amd import _lib, metrics as M  # noqa: E402

IDX = (0, 3, 6, 8, 10)


def _state_dicts(prm, prefix="features."):
    alex, heads = {}, {}
    for l, i in enumerate(IDX):
        alex[f"{prefix}{i}.weight"] = prm.weights[l].clone()
        alex[f"{prefix}{i}.bias"] = prm.biases[l].clone()
        heads[f"lin{l}.model.1.weight"] = prm.heads[l].clone().view(1, -1, 1, 1)
    alex["classifier.1.bias"] = torch.zeros(4)                    # a key of the full model that the loader has no use for
    return alex, heads


def _save(tmp_path, alex, heads, tag=""):
    a, h = str(tmp_path / f"alexnet{tag}.pth"), str(tmp_path / f"alex{tag}.pth")
    torch.save(alex, a)
    torch.save(heads, h)
    return a, h


def _same(p, q):
    return all(torch.equal(a, b) for ts, us in ((p.weights, q.weights), (p.biases, q.biases), (p.heads, q.heads))
               for a, b in zip(ts, us))


@pytest.mark.parametrize("prefix", ["features.", ""])
def test_load_reproduces_the_tensors_in_both_key_forms(tmp_path, prefix):
    prm = P.LpipsParams.random(seed=3)
    got = P.load_lpips_params(*_save(tmp_path, *_state_dicts(prm, prefix)))
    assert isinstance(got, P.LpipsParams) and _same(got, prm)
    assert [tuple(h.shape) for h in got.heads] == [(64,), (192,), (384,), (256,), (256,)]


def test_load_names_every_missing_key_and_wrong_shape(tmp_path):
    prm = P.LpipsParams.random(seed=3)
    alex, heads = _state_dicts(prm)
    for n, key in enumerate([k for k in alex if k.startswith("features.")]):
        a, h = _save(tmp_path, {k: v for k, v in alex.items() if k != key}, heads, f"_m{n}")
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            P.load_lpips_params(a, h)
        a, h = _save(tmp_path, {**alex, key: alex[key][1:]}, heads, f"_s{n}")
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + ".*shape"):
            P.load_lpips_params(a, h)
    for n, key in enumerate(list(heads)):
        a, h = _save(tmp_path, alex, {k: v for k, v in heads.items() if k != key}, f"_hm{n}")
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            P.load_lpips_params(a, h)
        a, h = _save(tmp_path, alex, {**heads, key: heads[key].view(-1)}, f"_hs{n}")
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + ".*shape"):
            P.load_lpips_params(a, h)
    with pytest.raises(ValueError, match="neither file is shipped"):
        P.load_lpips_params(None, None)


def test_random_params_are_reproducible_and_documented():
    a, b, c = P.LpipsParams.random(), P.LpipsParams.random(seed=19), P.LpipsParams.random(seed=20)
    assert _same(a, b) and not _same(a, c)
    for l, (m, cin, k, *_rest) in enumerate(R.LAYERS):
        assert tuple(a.weights[l].shape) == (m, cin, k, k) and a.weights[l].dtype == torch.float32
        bound = math.sqrt(6.0 / (k * k * cin))
        assert a.weights[l].abs().max() <= bound and a.weights[l].abs().max() > 0.9 * bound
        assert a.biases[l].abs().max() <= 0.05
        assert a.heads[l].min() >= 0 and a.heads[l].max() < 2.0 / m
    doc = P.LpipsParams.random.__doc__
    assert "NOT the trained metric" in doc and "nothing outside tests" in doc
    with pytest.raises(Exception):                                 # frozen
        a.weights = ()
    with pytest.raises(ValueError, match="weight 0"):
        P.LpipsParams((a.weights[0][:, :, :5, :5],) + a.weights[1:], a.biases, a.heads)


def test_smallest_image_is_31_by_31():
    for h, w in ((30, 31), (31, 30), (5, 400)):
        with pytest.raises(ValueError, match="31 x 31"):
            P.lpips_feature_sizes(h, w)
    assert P.lpips_feature_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert P.lpips_feature_sizes(400, 600) == [(99, 149), (49, 74), (24, 36), (24, 36), (24, 36)]
    prm = P.LpipsParams.random()
    for h, w in ((31, 31), (31, 47), (35, 67), (97, 131)):         # the restatement's own shapes are what the rule says
        f = R.features(torch.zeros((1, 3, h, w), dtype=torch.float64), prm, torch.float32)
        assert [tuple(t.shape[-2:]) for t in f] == P.lpips_feature_sizes(h, w)
    with pytest.raises(RuntimeError):                              # and below the minimum it has no window to pool
        R.features(torch.zeros((1, 3, 30, 31), dtype=torch.float64), prm, torch.float32)


def test_launchers_check_shapes_on_the_host():
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                       # never dereferenced: every call returns before a launch
    assert L.raw("cidnet_metric_lpips_ws_floats")(2, 400, 600) == 2 * 2 * 5 * ((99 * 149 + 31) // 32)
    assert L.raw("cidnet_metric_lpips_ws_floats")(1, 30, 31) == 0 and L.raw("cidnet_metric_lpips_ws_floats")(0, 64, 64) == 0
    assert L.raw("cidnet_metric_gt_mean_scale_ws_floats")(3, 400, 600) == 2 * 3 * 15 * 2
    sizes = (ctypes.c_int * 10)()
    assert L.raw("cidnet_lpips_feature_sizes")(31, 30, sizes) == -2
    assert L.raw("cidnet_lpips_feature_sizes")(31, 31, None) == -1
    conv = L.raw("cidnet_lpips_conv_relu")
    assert conv(p, p, p, p, 1, 64, 3, 64, 64, 7, 2, 3, None) == -2          # not one of the three layer shapes
    assert conv(p, p, p, p, 1, 48, 3, 64, 64, 11, 4, 2, None) == -2         # M is no multiple of 64
    assert conv(p, p, p, p, 1, 64, 3, 6, 64, 11, 4, 2, None) == -2          # the padded input is under the window
    assert conv(p, p, p, p, 70000, 64, 3, 64, 64, 11, 4, 2, None) == -2
    assert conv(None, p, p, p, 1, 64, 3, 64, 64, 11, 4, 2, None) == -1
    assert L.raw("cidnet_lpips_maxpool3s2")(p, p, 4, 2, 9, None) == -2
    layer = L.raw("cidnet_metric_lpips_layer")
    assert layer(p, p, p, p, 10 ** 6, 0, 1, 64, 7, 7, 30, 31, None) == -2   # image under the minimum
    assert layer(p, p, p, p, 10 ** 6, 1, 1, 64, 3, 3, 31, 31, None) == -2   # layer 1 has 192 channels
    assert layer(p, p, p, p, 10 ** 6, 0, 1, 64, 7, 8, 31, 31, None) == -2   # not the layer's size for this image
    assert layer(p, p, p, p, 10 ** 6, 5, 1, 64, 7, 7, 31, 31, None) == -2
    assert layer(p, p, p, p, 1, 0, 1, 64, 7, 7, 31, 31, None) == -3
    assert L.raw("cidnet_metric_lpips_finish")(p, 10 ** 6, p, p, 1, 31, 30, None) == -2
    assert L.raw("cidnet_metric_lpips_finish")(p, 1, p, p, 1, 31, 31, None) == -3
    assert L.raw("cidnet_metric_lpips_ingest")(p, None, None, 1, 31, 31, None) == -1
    assert L.raw("cidnet_metric_gt_mean_scale")(p, p, p, p, 1, 1, 31, 31, None) == -3
    assert L.raw("cidnet_metric_gt_mean_scale")(p, p, p, p, 10 ** 9, 70000, 31, 31, None) == -2     # gridDim.y


def test_cpu_tensors_are_refused():
    prm = P.LpipsParams.random()
    q = torch.zeros((1, 3, 31, 31), dtype=torch.uint8)
    for fn in (lambda: P.lpips(q, q, prm), lambda: P.lpips_layers(q, q, prm), lambda: P.lpips_features(q, prm)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    with pytest.raises(ValueError, match="neither file is shipped"):
        P.lpips(q, q, None)


def test_eval_result_defaults_and_exports():
    r = M.EvalResult(alpha=1.0, psnr=1.0, ssim=1.0, psnr_gt_mean=1.0, ssim_gt_mean=1.0)
    assert math.isnan(r.lpips) and math.isnan(r.lpips_gt_mean) and "lpips" not in r.per_image
    for name in ("LpipsParams", "load_lpips_params", "lpips", "lpips_layers", "lpips_features", "lpips_feature_sizes"):
        assert name in P.__all__ and getattr(P, name) is getattr(M, name)


def test_restatement_properties():
    """identical inputs give exactly 0, the arguments commute, GT mean enters as a float image, and the fp32 run of the
    restatement stays within fp32 rounding of the fp64 one (the distance the GPU tests' bars are multiples of)"""
    prm = P.LpipsParams.random()
    restored, gt = R.images(2, 48, 70, seed=4)
    u0, u1 = R.as_u(restored), R.as_u(gt)
    assert torch.equal(R.score(u1, u1, prm), torch.zeros(2, dtype=torch.float64))
    a, b = R.layers(u0, u1, prm), R.layers(u1, u0, prm)
    assert torch.equal(a, b) and a.shape == (2, 5) and (a > 0).all()
    assert torch.equal(R.score(u0, u1, prm), a.sum(dim=1))
    assert 1e-3 < a.sum(dim=1).min() and a.sum(dim=1).max() < 5e-2
    us = R.rescaled(restored, gt)
    assert us.dtype == torch.float64 and not torch.equal(us, us.round()) and us.max() <= 255.0
    c = R.layers(us, u1, prm)
    assert not torch.equal(c, a)
    a32 = R.layers(u0, u1, prm, torch.float32)
    assert a32.dtype == torch.float32
    assert ((a32.double() - a).abs() / a).max() < 1e-5
    assert np.array_equal(R.images(2, 48, 70, seed=4)[0], restored)
