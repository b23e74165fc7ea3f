"""GPU: the LPIPS kernels (csrc/lpips.hip) against the fp64 run of the plain-torch restatement tests/lpips_ref.py -- the
five taps, the five layer terms and the score, without and with the GT-mean rescale -- and the properties lpips() promises.

The bars are measured here, per quantity: the fp32 run of the same restatement on the CPU stands at some distance from its
fp64 run on the same inputs; eight times that distance is the bar (the margin covers another summation order and the
2^-25 terms a split product may drop), with a floor of 1e-5 because the distance can come out near zero by luck: the fp32
unit roundoff 6e-8 times sqrt(3456), the longest dot product, is 3.5e-6 per layer, and five layers in sequence stay under
1e-5.  The comparison is relative, per layer as well as in total, so that no layer hides behind the first; a wrong tap,
border pixel or channel moves a layer term by orders of magnitude more.  Feature maps use max|delta| / max|f|."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402

import hvi_cidnet_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu
# (B, h, w): the minimum height (deepest maps 1 x 1, both pools floor) | stride 4 divides exactly in both axes | a batch |
# ragged in every stage | the evaluation's size
SHAPES = [(2, 31, 47), (1, 35, 67), (3, 64, 96), (1, 97, 131), (1, 400, 600)]
FLOOR, MARGIN = 1e-5, 8.0


@functools.lru_cache(maxsize=None)
def _params():
    return P.LpipsParams.random()


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """computed once per shape and shared, read-only: the inputs, and per variant (gt_mean False / True) the restatement's
    taps of the restored image and of the ground truth in fp64 and fp32, and its layer terms in both"""
    B, h, w = shape
    restored, gt = R.images(B, h, w, seed=h * 1000 + w)
    prm = _params()
    u1 = R.as_u(gt)
    g64, g32 = R.features(u1, prm, torch.float64), R.features(u1, prm, torch.float32)
    out = {"restored": restored, "gt": gt, "gt64": g64, "gt32": g32}
    for gm in (False, True):
        u0 = R.rescaled(restored, gt) if gm else R.as_u(restored)
        f64, f32 = R.features(u0, prm, torch.float64), R.features(u0, prm, torch.float32)
        out[gm] = {"f64": f64, "f32": f32, "l64": R.layers_from(f64, g64, prm), "l32": R.layers_from(f32, g32, prm).double()}
    return out


def _bar(ref32, ref64):
    """-> (the bar, the relative distance of the fp32 restatement from the fp64 one): the distance times the margin, not
    under the floor"""
    d32 = float(((ref32 - ref64).abs() / ref64.abs()).max())
    return max(MARGIN * d32, FLOOR), d32


def _dev_images(ref, dev):
    return torch.from_numpy(ref["restored"]).to(dev), torch.from_numpy(ref["gt"]).to(dev)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_features_match_the_fp64_restatement(dev, shape):
    ref = _reference(shape)
    q, g = _dev_images(ref, dev)
    B = shape[0]
    scale = torch.from_numpy(np.array([(int(R.metrics_ref.gray(b).sum()) / (shape[1] * shape[2]))
                                       / (int(R.metrics_ref.gray(a).sum()) / (shape[1] * shape[2]))
                                       for a, b in zip(ref["restored"], ref["gt"])], dtype=np.float64)).to(dev)
    runs = [("gt", P.lpips_features(g, _params()), ref["gt64"], ref["gt32"]),
            ("restored", P.lpips_features(q, _params()), ref[False]["f64"], ref[False]["f32"]),
            ("rescaled", P.lpips_features(q, _params(), scale=scale), ref[True]["f64"], ref[True]["f32"])]
    assert P.lpips_feature_sizes(*shape[1:]) == [tuple(t.shape[-2:]) for t in ref["gt64"]]
    for what, got, f64, f32 in runs:
        assert len(got) == 5
        for l in range(5):
            assert got[l].dtype == torch.float32 and tuple(got[l].shape) == tuple(f64[l].shape) and got[l].shape[0] == B
            top = float(f64[l].abs().max())
            d32 = float((f32[l].double() - f64[l]).abs().max()) / top
            bar = max(MARGIN * d32, FLOOR)
            err = float((got[l].cpu().double() - f64[l]).abs().max()) / top
            print(f"features {shape} {what} tap {l}: err {err:.3e} bar {bar:.3e} (fp32 restatement {d32:.3e})")
            assert err <= bar, (what, l, err, bar)


@pytest.mark.parametrize("gt_mean", [False, True], ids=["plain", "gt_mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layers_and_score_match_the_fp64_restatement(dev, shape, gt_mean):
    ref = _reference(shape)
    q, g = _dev_images(ref, dev)
    l64, l32 = ref[gt_mean]["l64"], ref[gt_mean]["l32"]
    layers = P.lpips_layers(q, g, _params(), gt_mean=gt_mean)
    score = P.lpips(q, g, _params(), gt_mean=gt_mean)
    assert layers.dtype == torch.float64 and tuple(layers.shape) == (shape[0], 5) and layers.is_cuda
    assert score.dtype == torch.float64 and tuple(score.shape) == (shape[0],) and score.is_cuda
    layers, score = layers.cpu(), score.cpu()
    assert torch.equal(score, ((((layers[:, 0] + layers[:, 1]) + layers[:, 2]) + layers[:, 3]) + layers[:, 4]))
    for l in range(5):
        bar, d32 = _bar(l32[:, l], l64[:, l])
        err = float(((layers[:, l] - l64[:, l]).abs() / l64[:, l]).max())
        print(f"layer {shape} gt_mean={gt_mean} term {l}: err {err:.3e} bar {bar:.3e} (fp32 restatement {d32:.3e}) "
              f"share {float((l64[:, l] / l64.sum(1)).mean()):.3f}")
        assert err <= bar, (l, err, bar)
    s64, s32 = l64.sum(dim=1), l32.sum(dim=1)
    bar, d32 = _bar(s32, s64)
    err = float(((score - s64).abs() / s64).max())
    print(f"score {shape} gt_mean={gt_mean}: {s64.tolist()} err {err:.3e} bar {bar:.3e} (fp32 restatement {d32:.3e})")
    assert err <= bar, (err, bar)
    assert 1e-3 < float(s64.min()) and float(s64.max()) < 5e-2


def test_identical_images_score_exactly_zero(dev):
    _, gt = R.images(2, 64, 96, seed=1)
    g = torch.from_numpy(gt).to(dev)
    for gm in (False, True):
        assert torch.equal(P.lpips(g, g.clone(), _params(), gt_mean=gm).cpu(), torch.zeros(2, dtype=torch.float64))
        assert torch.equal(P.lpips_layers(g, g.clone(), _params(), gt_mean=gm).cpu(), torch.zeros((2, 5), dtype=torch.float64))


def test_calls_are_bit_identical_and_independent_of_the_batch(dev):
    restored, gt = R.images(3, 97, 131, seed=2)
    q, g = torch.from_numpy(restored).to(dev), torch.from_numpy(gt).to(dev)
    for gm in (False, True):
        a = P.lpips(q, g, _params(), gt_mean=gm)
        b = P.lpips(q, g, _params(), gt_mean=gm)
        assert torch.equal(a, b)
        alone = P.lpips(q[1:2], g[1:2], _params(), gt_mean=gm)
        assert alone.item() == a[1].item() and alone.item() > 0
        assert torch.equal(P.lpips_layers(q[1], g[1], _params(), gt_mean=gm)[0], P.lpips_layers(q, g, _params(), gt_mean=gm)[1])
    swapped = P.lpips(g, q, _params())                               # the arguments commute
    assert torch.equal(swapped, P.lpips(q, g, _params()))


def test_bad_inputs_raise_the_documented_errors(dev):
    prm = _params()
    ok = torch.zeros((1, 3, 31, 31), dtype=torch.uint8, device=dev)
    assert P.lpips(ok, ok, prm).item() == 0.0
    for h, w in ((30, 31), (31, 30)):
        small = torch.zeros((1, 3, h, w), dtype=torch.uint8, device=dev)
        with pytest.raises(ValueError, match="31 x 31"):
            P.lpips(small, small, prm)
        with pytest.raises(ValueError, match="31 x 31"):
            P.lpips_features(small, prm)
    with pytest.raises(RuntimeError, match=r"expected \(B,3,H,W\)"):
        P.lpips(ok[0, 0], ok[0, 0], prm)
    with pytest.raises(RuntimeError, match=r"expected \(B,3,H,W\)"):
        P.lpips(ok[:, :2], ok[:, :2], prm)
    with pytest.raises(RuntimeError, match="uint8"):
        P.lpips(ok.float(), ok, prm)
    with pytest.raises(RuntimeError, match="differ"):
        P.lpips(ok, torch.zeros((1, 3, 31, 32), dtype=torch.uint8, device=dev), prm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.lpips(ok.cpu(), ok, prm)
    with pytest.raises(RuntimeError, match="float64"):
        P.lpips_features(ok, prm, scale=torch.ones(1, device=dev))
