"""GPU: the metric kernels (csrc/metrics.hip through hvi_cidnet_amd.metrics) against the fp64 restatement of
tests/metrics_ref.py -- quantization bit for bit, PSNR within 1e-6 dB, SSIM within 1e-10, with and without the GT-mean
rescale -- and their reproducibility (bit-identical repeated calls, an image's values independent of its batch)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
PSNR_TOL, SSIM_TOL = 1e-6, 1e-10


def _pair(rng, shape, kind="noisy"):
    """(restored, gt) uint8 (3,h,w) with realistic structure: a smooth gradient scene plus texture, the restored image a
    darker / brighter noisy copy (so the GT-mean scale is not 1)"""
    _, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = np.stack([120 + 90 * np.sin(5 * xx + c) * yy for c in range(3)]) + rng.normal(0, 25, shape)
    gt = np.clip(base, 0, 255).astype(np.uint8)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8), gt
    gain = {"noisy": 0.8, "dark": 0.3, "bright": 1.6}[kind]
    restored = np.clip(gt.astype(np.float64) * gain + rng.normal(0, 12, shape), 0, 255).astype(np.uint8)
    return restored, gt


def _check(rs, gs, dev):
    a = torch.from_numpy(np.stack(rs)).to(dev)
    g = torch.from_numpy(np.stack(gs)).to(dev)
    for gm in (False, True):
        p, s = (t.cpu().numpy() for t in P_M().psnr_ssim(a, g, gt_mean=gm))
        p1, s1 = P_M().psnr(a, g, gt_mean=gm).cpu().numpy(), P_M().ssim(a, g, gt_mean=gm).cpu().numpy()
        assert np.array_equal(p, p1) and np.array_equal(s, s1)        # one-metric calls: the same values
        for i, (r_, g_) in enumerate(zip(rs, gs)):
            rp, rs_ = R.psnr(r_, g_, gt_mean=gm), R.ssim(r_, g_, gt_mean=gm)
            assert abs(p[i] - rp) <= PSNR_TOL, (i, gm, p[i], rp)
            assert abs(s[i] - rs_) <= SSIM_TOL, (i, gm, s[i], rs_)


def P_M():
    from hvi_cidnet_amd import metrics
    return metrics


def test_to_uint8_bit_equal_to_torch(dev):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 24, 40, generator=g) * 1.4 - 0.2                 # negatives and values above 1
    k = torch.arange(256, dtype=torch.float32) / 255                        # right at the k/255 boundaries ...
    edge = torch.cat([k, torch.nextafter(k, torch.full_like(k, 2.0)), torch.nextafter(k, torch.full_like(k, -1.0)),
                      torch.tensor([0.0, -0.0, 1.0, -1e-30, 1e-30, 1.0000001, 3.0, -5.0])])
    flat = x.view(-1)
    flat[:edge.numel()] = edge
    flat[-edge.numel():] = edge.flip(0)
    ref = torch.clamp(x, 0, 1).mul(255).byte()
    M = P_M()
    q = M.to_uint8(x.to(dev))
    assert q.dtype == torch.uint8 and torch.equal(q.cpu(), ref)
    qc = M.to_uint8(x.to(dev), size=(19, 33))                              # padded -> cropped
    assert tuple(qc.shape) == (2, 3, 19, 33) and torch.equal(qc.cpu(), ref[:, :, :19, :33])
    q3 = M.to_uint8(x[1].to(dev), size=(7, 40))
    assert torch.equal(q3.cpu(), ref[1, :, :7])


@pytest.mark.parametrize("shape", [(3, 11, 11), (3, 37, 51), (3, 400, 600), (3, 1024, 1024)])
def test_psnr_ssim_match_the_restatement(dev, shape):
    rng = np.random.default_rng(shape[1] * 7 + shape[2])
    r, g = _pair(rng, shape)
    _check([r], [g], dev)


def test_mixed_batch_matches_the_restatement(dev):
    rng = np.random.default_rng(11)
    pairs = [_pair(rng, (3, 48, 70), kind) for kind in ("dark", "bright", "random")]
    _check([p[0] for p in pairs], [p[1] for p in pairs], dev)


def test_identical_images(dev):
    M = P_M()
    rng = np.random.default_rng(12)
    a = torch.from_numpy(np.stack([_pair(rng, (3, 40, 56))[1] for _ in range(2)])).to(dev)
    for gm in (False, True):
        p, s = M.psnr_ssim(a, a.clone(), gt_mean=gm)
        assert torch.equal(s.cpu(), torch.ones(2, dtype=torch.float64))
        assert np.allclose(p.cpu().numpy(), 10 * math.log10(65025 / 1e-8), rtol=0, atol=1e-9)


def test_reproducible_and_batch_independent(dev):
    M = P_M()
    rng = np.random.default_rng(13)
    pairs = [_pair(rng, (3, 96, 136), kind) for kind in ("noisy", "dark", "random", "bright")]
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    g = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    for gm in (False, True):
        first = [t.clone() for t in M.psnr_ssim(a, g, gt_mean=gm)]
        again = M.psnr_ssim(a, g, gt_mean=gm)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        for i in range(4):
            alone = M.psnr_ssim(a[i:i + 1], g[i:i + 1], gt_mean=gm)
            assert torch.equal(alone[0], first[0][i:i + 1]) and torch.equal(alone[1], first[1][i:i + 1])
        sub = M.psnr_ssim(a[1:3], g[1:3], gt_mean=gm)
        assert torch.equal(sub[0], first[0][1:3]) and torch.equal(sub[1], first[1][1:3])


def _host_scale(restored, gt):
    """the device's expression on np.float64: both gray sums are integers below 2^53, so each side does the same three
    correctly rounded divisions and the comparison needs no tolerance"""
    n = np.float64(restored.shape[1] * restored.shape[2])
    ta, tb = np.float64(int(R.gray(restored).sum())), np.float64(int(R.gray(gt).sum()))
    with np.errstate(all="ignore"):
        return (tb / n) / (ta / n)


@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 11, 11), (3, 37, 51), (3, 128, 128), (3, 113, 145), (3, 400, 600)])
def test_gt_mean_scale_is_bit_equal_to_the_host(dev, shape):
    """128 x 128 is exactly one 16384-pixel chunk of the gray sum, 113 x 145 = 16385 a second chunk of one pixel"""
    r, g = _pair(np.random.default_rng(shape[1] * 7 + shape[2]), shape)
    s = P_M().gt_mean_scale(torch.from_numpy(r).to(dev), torch.from_numpy(g).to(dev))
    assert s.dtype == torch.float64 and tuple(s.shape) == (1,) and s.device.type == "cuda"
    assert np.array_equal(s.cpu().numpy(), np.array([_host_scale(r, g)]))


def test_gt_mean_scale_batch_and_black_images(dev):
    M = P_M()
    rng = np.random.default_rng(14)
    pairs = [_pair(rng, (3, 48, 70), kind) for kind in ("dark", "bright", "random")]
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    g = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    s = M.gt_mean_scale(a, g)
    want = np.array([_host_scale(r_, g_) for r_, g_ in pairs])
    assert len(set(want.tolist())) == 3 and np.array_equal(s.cpu().numpy(), want)
    assert torch.equal(M.gt_mean_scale(a[1:2], g[1:2]), s[1:2])           # an image's scale does not depend on its batch
    black = np.zeros((3, 48, 70), dtype=np.uint8)
    rs, gs = [black, black], [pairs[0][1], black]                          # x / 0 = inf, 0 / 0 = NaN
    s = M.gt_mean_scale(torch.from_numpy(np.stack(rs)).to(dev), torch.from_numpy(np.stack(gs)).to(dev)).cpu().numpy()
    want = np.array([_host_scale(r_, g_) for r_, g_ in zip(rs, gs)])
    assert np.isposinf(want[0]) and np.isnan(want[1]) and np.array_equal(s, want, equal_nan=True)


def _mixed_batch():
    rng = np.random.default_rng(11)                                        # test_mixed_batch_matches_the_restatement's
    pairs = [_pair(rng, (3, 48, 70), kind) for kind in ("dark", "bright", "random")]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.parametrize("images", [lambda: tuple(x[None] for x in _pair(np.random.default_rng(37 * 7 + 51), (3, 37, 51))),
                                    _mixed_batch], ids=["37x51", "mixed"])
def test_a_given_scale_is_the_gt_mean_call(dev, images):
    M = P_M()
    a, g = (torch.from_numpy(x).to(dev) for x in images())
    s = M.gt_mean_scale(a, g)
    own, given = M.psnr_ssim(a, g, gt_mean=True), M.psnr_ssim(a, g, scale=s)
    assert torch.equal(own[0], given[0]) and torch.equal(own[1], given[1])
    assert torch.equal(M.psnr(a, g, gt_mean=True), given[0]) and torch.equal(M.ssim(a, g, gt_mean=True), given[1])
    assert torch.equal(M.psnr_ssim(a, g, scale=s, want_ssim=False)[0], given[0])
    assert torch.equal(M.psnr_ssim(a, g, scale=s, want_psnr=False)[1], given[1])
    assert not torch.equal(M.psnr_ssim(a, g)[0], given[0])                 # and a scale implies GT mean
    B = a.shape[0]
    for bad in (s.float(), torch.ones(B + 1, dtype=torch.float64, device=dev), s[:, None]):
        with pytest.raises(RuntimeError, match=rf"psnr_ssim: scale must be \({B},\) float64 \(got"):
            M.psnr_ssim(a, g, scale=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.psnr_ssim(a, g, scale=s.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.gt_mean_scale(a.cpu(), g)
    with pytest.raises(RuntimeError, match="uint8"):
        M.gt_mean_scale(a.float(), g.float())
    with pytest.raises(RuntimeError, match="differ"):
        M.gt_mean_scale(a, g[:, :, :, :20])


def test_shape_checks(dev):
    M = P_M()
    a = torch.zeros(1, 3, 10, 40, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="11 x 11"):
        M.ssim(a, a)
    assert M.psnr(a, a).shape == (1,)                                      # PSNR alone has no minimum size
    with pytest.raises(RuntimeError, match="uint8"):
        M.psnr(a.float(), a.float())
    with pytest.raises(RuntimeError, match="differ"):
        M.psnr(a, a[:, :, :, :20])


def test_uint8_input_is_divided_by_255(dev):
    """the input converter on all 256 levels: a uint8 HWC array and a uint8 CHW tensor become, bit for bit, what ToTensor()
    computes on the host.  (`t.float().div(255)` on the device multiplies by fl(1/255) instead: DESIGN.md 6.1)"""
    M = P_M()
    a = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    want = torch.from_numpy(a).permute(2, 0, 1).float().div(255)
    for img in (a, torch.from_numpy(a).permute(2, 0, 1).contiguous()):
        got = M._image_f32(img, dev)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 16, 16)
        assert torch.equal(got.cpu(), want)
