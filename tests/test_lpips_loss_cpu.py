"""CPU: the restatement of the LPIPS training loss (tests/lpips_loss_ref.py) -- its hand-written backward against fp64
autograd of its own forward, the all-zero-pixel convention -- and the argument errors of LPIPSLoss / CIDNetLoss that need no
device."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_loss_ref as LR  # noqa: E402
import lpips_ref as R  # noqa: E402

import hvi_cidnet_amd as P  # noqa: E402


def _pair(B, h, w, seed=1):
    restored, gt = R.images(B, h, w, seed=seed)
    return torch.from_numpy(restored).float() / 255, torch.from_numpy(gt).float() / 255


# 31 x 31: the minimum | 38 x 66: the last row and column are under no window of the first layer | 35 x 47: ragged pools
@pytest.mark.parametrize("h,w", [(31, 31), (38, 66), (35, 47)])
def test_hand_written_backward_equals_fp64_autograd(h, w):
    prm = P.LpipsParams.random()
    x, gt = _pair(2, h, w)
    # the leaf is v = 2 x - 1 as fp32 forms it, widened: d/dx = 2 d/dv exactly, and no gradient is rounded to fp32 on the way
    v = (2.0 * x - 1.0).double().requires_grad_(True)
    f0 = LR.taps(LR.scaling(v), prm)
    for f in f0:                                                   # the premise: no feature pixel is all zero
        assert bool(((f * f).sum(dim=1) > 0).all())
    value = LR.loss_from_taps(f0, LR.taps(LR.ingest(gt, torch.float64), prm), prm, 0.7)
    want = 2.0 * torch.autograd.grad(value, v)[0]
    got_value, got = LR.loss_and_grad(x, gt, prm, torch.float64, 0.7)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert abs(float(got_value) - float(value.detach())) <= 1e-14 * abs(float(value.detach()))
    # fp64 sums in another order: 1e-12 of the gradient's size is 1e4 roundoffs
    assert float((got - want).norm() / want.norm()) < 1e-12
    if (h - 7) % 4 == 3 and (w - 7) % 4 == 3:
        assert torch.count_nonzero(got[:, :, -1, :]) == 0 and torch.count_nonzero(got[:, :, :, -1]) == 0
        assert torch.count_nonzero(got[:, :, -2, :]) > 0


def test_pieces_equal_autograd():
    """the distance derivative, the pool rule and both data gradients one by one, fp64"""
    gen = torch.Generator().manual_seed(3)
    f0 = torch.rand((2, 64, 3, 5), generator=gen, dtype=torch.float64).requires_grad_(True)
    f1 = torch.rand((2, 64, 3, 5), generator=gen, dtype=torch.float64)
    head = torch.rand(64, generator=gen)
    val = 0.25 * (((LR.R._normalize(f0) - LR.R._normalize(f1)) ** 2) * head.double().view(1, -1, 1, 1)).sum()
    (want,) = torch.autograd.grad(val, f0)
    assert torch.allclose(LR.dist_bwd(f0.detach(), f1, head, 0.25), want, rtol=1e-11, atol=1e-15)
    # pool: ties, zeros and an all-zero plane decide like ATen
    for H, W in ((3, 3), (7, 7), (8, 6), (15, 15)):
        x = LR.tap_like((2, 3, H, W), seed=H * 16 + W, zero_plane=1).double().requires_grad_(True)
        y = F.max_pool2d(x, 3, 2)
        gy = torch.rand(y.shape, generator=gen, dtype=torch.float64)
        (want,) = torch.autograd.grad(y, x, gy)
        got = LR.pool_bwd(x.detach(), gy)
        assert torch.allclose(got, want, rtol=1e-14, atol=0)
        zero = got.reshape(-1, H, W)[1]
        assert torch.equal(zero[0:2 * y.shape[-2]:2, 0:2 * y.shape[-1]:2], gy.reshape(-1, *y.shape[-2:])[1])   # top-left elements
    for (h, w) in ((31, 31), (38, 66), (33, 36)):
        x = torch.rand((1, 3, h, w), generator=gen, dtype=torch.float64).requires_grad_(True)
        wt = torch.rand((64, 3, 11, 11), generator=gen, dtype=torch.float64)
        y = F.conv2d(x, wt, stride=4, padding=2)
        dy = torch.rand(y.shape, generator=gen, dtype=torch.float64)
        (want,) = torch.autograd.grad(y, x, dy)
        assert torch.allclose(LR.conv1_dgrad(dy, wt, h, w), want, rtol=1e-11, atol=1e-13)
    x = torch.rand((1, 64, 4, 3), generator=gen, dtype=torch.float64).requires_grad_(True)
    wt = torch.rand((192, 64, 5, 5), generator=gen, dtype=torch.float64)
    y = F.conv2d(x, wt, padding=2)
    dy = torch.rand(y.shape, generator=gen, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, dy)
    assert torch.allclose(LR.conv_dgrad_s1(dy, wt, 2), want, rtol=1e-11, atol=1e-13)


def test_all_zero_pixel_convention():
    """a pixel whose f0 is all zero gets gradient 0 in every channel and nothing anywhere is NaN, where autograd gives NaN;
    a ground-truth pixel that is all zero is nothing special"""
    gen = torch.Generator().manual_seed(5)
    f0 = torch.rand((1, 64, 2, 2), generator=gen, dtype=torch.float64)
    f1 = torch.rand((1, 64, 2, 2), generator=gen, dtype=torch.float64)
    f0[0, :, 0, 1] = 0.0
    f1[0, :, 1, 0] = 0.0
    head = torch.rand(64, generator=gen)
    g = LR.dist_bwd(f0, f1, head, 1.0)
    assert torch.isfinite(g).all()
    assert torch.count_nonzero(g[0, :, 0, 1]) == 0
    assert torch.count_nonzero(g[0, :, 1, 0]) == 64 and torch.count_nonzero(g[0, :, 0, 0]) == 64
    fa = f0.clone().requires_grad_(True)
    val = (((LR.R._normalize(fa) - LR.R._normalize(f1)) ** 2) * head.double().view(1, -1, 1, 1)).sum()
    (auto,) = torch.autograd.grad(val, fa)
    assert torch.isnan(auto[0, :, 0, 1]).all()                    # what the convention replaces
    keep = torch.ones((2, 2), dtype=torch.bool)
    keep[0, 1] = False
    assert torch.allclose(g[0][:, keep], auto[0][:, keep], rtol=1e-11, atol=1e-15)
    assert torch.count_nonzero(LR.dist_bwd(f0, f0.clone(), head, 1.0)) == 0


def test_loss_modules_raise_without_a_device():
    prm = P.LpipsParams.random()
    small = torch.zeros((1, 3, 30, 40))
    with pytest.raises(ValueError, match="31 x 31"):
        P.LPIPSLoss(prm)(small, small)
    with pytest.raises(ValueError, match="neither file is shipped"):
        P.LPIPSLoss(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.LPIPSLoss(prm)(torch.zeros((1, 3, 31, 31)), torch.zeros((1, 3, 31, 31)))
    with pytest.raises(RuntimeError, match=r"\(B,3,H,W\)"):
        P.LPIPSLoss(prm)(torch.zeros((1, 3, 31, 31)), torch.zeros((1, 3, 31, 32)))

    class _Model:
        HVIT = staticmethod(lambda t: t)
    with pytest.raises(ValueError, match="neither file is shipped"):
        P.CIDNetLoss(_Model(), lpips_weight=0.1)
    base = P.CIDNetLoss(_Model())
    assert base.lpips is None and P.CIDNetLoss(_Model(), lpips_weight=0.0).lpips is None
    assert isinstance(P.CIDNetLoss(_Model(), lpips_weight=0.1, lpips_params=prm).lpips, P.LPIPSLoss)
