"""GPU: the LPIPS training loss (csrc/lpips_loss.hip, ops.LpipsLossFn, losses.LPIPSLoss, CIDNetLoss(lpips_weight=)) stage by
stage and end to end against tests/lpips_loss_ref.py.

Every stage is compared with fp64 torch on the same fp32 inputs, so every mask and argmax is decided on identical values.
The bars:
  * ingest, its backward, the pool backward against the fixed-order restatement: bit-equal.
  * pool backward against fp64 autograd: the fp32 sum of at most four terms, 3 roundings of 2^-24 on the sum of magnitudes.
  * distance backward: fp64 arithmetic rounded once to fp32 -- 2^-24 per element; the bar is 2^-23 on the relative L2 error
    (another summation order in fp64 is 1e-16 and does not show), over the batch as one vector: at P = 1 the image with the
    all-zero pixel has an all-zero gradient and no norm to divide by.
  * convolution data gradients and everything end to end: the rule of tests/test_lpips_gpu.py -- MARGIN = 8 times the distance
    of the fp32 CPU restatement from the fp64 one, not under FLOOR = 1e-5, on the relative L2 error per image."""
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_loss_ref as LR  # noqa: E402
import lpips_ref as R  # noqa: E402

import hvi_cidnet_amd as P  # noqa: E402
from hvi_cidnet_amd import ops  # noqa: E402
from hvi_cidnet_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-5, 8.0
E2E_SHAPES = [(31, 31), (38, 66), (64, 64), (67, 95)]


@functools.lru_cache(maxsize=None)
def _params():
    return P.LpipsParams.random()


def _call(name, *args):
    lib().call(name, *[ops._p(a) if isinstance(a, torch.Tensor) else a for a in args], ops._stream())
    torch.cuda.synchronize()


def _rel_l2(got, want):
    """the relative L2 error per image, the worst image"""
    B = want.shape[0]
    d = (got.double() - want.double()).reshape(B, -1).norm(dim=1)
    return float((d / want.double().reshape(B, -1).norm(dim=1)).max())


def _bar(ref32, ref64):
    d32 = _rel_l2(ref32, ref64)
    return max(MARGIN * d32, FLOOR), d32


def _pair(B, h, w, seed=1):
    restored, gt = R.images(B, h, w, seed=seed)
    return torch.from_numpy(restored).float() / 255, torch.from_numpy(gt).float() / 255


@functools.lru_cache(maxsize=None)
def _e2e_reference(h, w):
    """computed once per shape and shared, read-only: the inputs, and the restatement's loss and gradient in fp64 and fp32"""
    x, gt = _pair(2, h, w)
    v64, g64 = LR.loss_and_grad(x, gt, _params(), torch.float64)
    v32, g32 = LR.loss_and_grad(x, gt, _params(), torch.float32)
    return x, gt, v64, g64, v32, g32


# ---- stage by stage -------------------------------------------------------------------------------------------------------
def test_ingest_and_its_backward_are_bit_equal_to_fp32_torch(dev):
    gen = torch.Generator().manual_seed(2)
    x = torch.rand((2, 3, 33, 37), generator=gen) * 1.5 - 0.25          # beyond [0, 1]: nothing clamps
    shift = torch.tensor(R.SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(R.SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    z = torch.empty_like(x, device=dev)
    _call("cidnet_lpips_ingest_f32", x.to(dev), z, 2, 33, 37)
    assert torch.equal(z.cpu(), ((2.0 * x - 1.0) - shift) / scale)
    g = torch.randn((2, 3, 33, 37), generator=gen)
    gx = torch.empty_like(g, device=dev)
    _call("cidnet_lpips_ingest_f32_bwd", g.to(dev), gx, 2, 33, 37)
    assert torch.equal(gx.cpu(), (g / scale) * 2.0)


def _dgrad_weights(w, stride, dev):
    m, c, k, _ = w.shape
    n = lib().raw("cidnet_lpips_dgrad_weights_floats")(m, c, k, stride)
    assert n == (m * c * k * k if stride == 1 else 121 * m * 4)
    wt = torch.empty(n, dtype=torch.float32, device=dev)
    _call("cidnet_lpips_dgrad_weights", w.to(dev), wt, m, c, k, stride)
    return wt


def _conv_dgrad_case(dev, layer, H, W, seed):
    """layer's data gradient for an input of H x W -> (device result for B = 2, fp64 and fp32 CPU gradients, device inputs)"""
    m, c, k, stride, pad, _ = R.LAYERS[layer]
    w = _params().weights[layer]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gen = torch.Generator().manual_seed(seed)
    dy = torch.randn((2, m, Ho, Wo), generator=gen)
    want = {}
    for dt in (torch.float64, torch.float32):
        x = torch.zeros((2, c, H, W), dtype=dt, requires_grad=True)
        (want[dt],) = torch.autograd.grad(F.conv2d(x, w.to(dt), stride=stride, padding=pad), x, dy.to(dt))
    wt = _dgrad_weights(w, stride, dev)
    dyd = dy.to(dev)
    got = torch.full((2, c, H, W), float("nan"), device=dev)
    _call("cidnet_lpips_conv_dgrad", dyd, wt, None, None, got, 2, m, c, H, W, k, stride, pad)
    return got, want[torch.float64], want[torch.float32], (dyd, wt, (m, c, k, stride, pad))


def _check_conv_dgrad(got, w64, w32, what):
    bar, d32 = _bar(w32, w64)
    err = _rel_l2(got.cpu(), w64)
    print(f"conv dgrad {what}: err {err:.3e} bar {bar:.3e} (fp32 torch {d32:.3e})")
    assert err <= bar, (what, err, bar)


# 31: 7 x 7 outputs | 67 x 95: 16 x 23 = 368 outputs | 38 x 66: (h - 7) mod 4 = (w - 7) mod 4 = 3, the last row and column are
# under no window
@pytest.mark.parametrize("h,w", [(31, 31), (67, 95), (38, 66)])
def test_first_layer_data_gradient(dev, h, w):
    got, w64, w32, (dyd, wt, (m, c, k, stride, pad)) = _conv_dgrad_case(dev, 0, h, w, seed=h)
    _check_conv_dgrad(got, w64, w32, (0, h, w))
    if (h, w) == (38, 66):
        g = got.cpu()
        assert torch.count_nonzero(w64[:, :, -1, :]) == 0 and torch.count_nonzero(w64[:, :, :, -1]) == 0
        assert torch.count_nonzero(g[:, :, -1, :]) == 0 and torch.count_nonzero(g[:, :, :, -1]) == 0
    alone = torch.empty((1, c, h, w), device=dev)
    _call("cidnet_lpips_conv_dgrad", dyd, wt, None, None, alone, 1, m, c, h, w, k, stride, pad)
    assert torch.equal(alone[0], got[0])                              # image 0 of two = image 0 alone


# feature sizes: one pixel | one tile | 35 pixels | 72 pixels: two tiles, the second ragged
@pytest.mark.parametrize("H,W", [(1, 1), (3, 3), (7, 5), (9, 8)])
@pytest.mark.parametrize("layer", [1, 2, 3, 4])
def test_stride_one_data_gradients(dev, layer, H, W):
    got, w64, w32, (dyd, wt, (m, c, k, stride, pad)) = _conv_dgrad_case(dev, layer, H, W, seed=10 * layer + H)
    _check_conv_dgrad(got, w64, w32, (layer, H, W))
    alone = torch.empty((1, c, H, W), device=dev)
    _call("cidnet_lpips_conv_dgrad", dyd, wt, None, None, alone, 1, m, c, H, W, k, stride, pad)
    assert torch.equal(alone[0], got[0])
    # the masked epilogue: dx = tap > 0 ? dx + addend : 0, with the same accumulators
    tap = LR.tap_like((2, c, H, W), seed=layer).to(dev)
    add = torch.randn((2, c, H, W), generator=torch.Generator().manual_seed(layer)).to(dev)
    fused = torch.empty_like(got)
    _call("cidnet_lpips_conv_dgrad", dyd, wt, tap, add, fused, 2, m, c, H, W, k, stride, pad)
    assert torch.equal(fused, torch.where(tap > 0, got + add, torch.zeros_like(got)))


@pytest.mark.parametrize("H,W", [(3, 3), (7, 7), (8, 6), (15, 15)])
def test_pool_backward(dev, H, W):
    x = LR.tap_like((2, 5, H, W), seed=H * 16 + W, zero_plane=3)       # exact zeros, plateaus, an all-zero plane
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    gy = torch.randn((2, 5, Ho, Wo), generator=torch.Generator().manual_seed(H))
    got = torch.full(x.shape, float("nan"), device=dev)
    _call("cidnet_lpips_maxpool3s2_bwd", x.to(dev), gy.to(dev), None, got, 10, H, W)
    got = got.cpu()
    assert torch.equal(got, LR.pool_bwd(x, gy))                         # the fixed-order restatement, fp32
    xa = x.double().requires_grad_(True)
    (want,) = torch.autograd.grad(F.max_pool2d(xa, 3, 2), xa, gy.double())
    mag = LR.pool_bwd(x.double(), gy.double().abs())                    # the sum of the magnitudes that meet in an element
    assert bool(((got.double() - want).abs() <= 3 * 2.0 ** -24 * mag).all())
    if H % 2 == 0:
        assert torch.count_nonzero(got[:, :, -1, :]) == 0               # even sizes: the last row and column are uncovered
    if W % 2 == 0:
        assert torch.count_nonzero(got[:, :, :, -1]) == 0
    zero = got.reshape(-1, H, W)[3]                                     # an all-zero plane: every window's top-left element
    assert torch.equal(zero[0:2 * Ho:2, 0:2 * Wo:2], gy.reshape(-1, Ho, Wo)[3])
    add = torch.randn(x.shape, generator=torch.Generator().manual_seed(W))
    fused = torch.empty(x.shape, device=dev)
    _call("cidnet_lpips_maxpool3s2_bwd", x.to(dev), gy.to(dev), add.to(dev), fused, 10, H, W)
    assert torch.equal(fused.cpu(), torch.where(x > 0, got + add, torch.zeros_like(got)))


@pytest.mark.parametrize("P_", [1, 9, 33])
@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_distance_backward(dev, C, P_):
    gen = torch.Generator().manual_seed(C + P_)
    f0 = torch.relu(torch.randn((2, C, P_, 1), generator=gen) + 0.3)
    f1 = torch.relu(torch.randn((2, C, P_, 1), generator=gen) + 0.3)
    f0[1, :, P_ // 2, 0] = 0.0                                          # a pixel with f0 == 0 in every channel
    f1[0, :, P_ - 1, 0] = 0.0                                           # and one with f1 == 0
    head = torch.rand(C, generator=gen) * (2.0 / C)
    weight = 0.7
    want = LR.dist_bwd(f0.double(), f1.double(), head, weight / (2 * P_))
    got = torch.full(f0.shape, float("nan"), device=dev)
    _call("cidnet_lpips_layer_bwd", f0.to(dev), f1.to(dev), head.to(dev), got, ctypes.c_float(weight), 0, 2, C, P_)
    got = got.cpu()
    assert torch.isfinite(got).all()
    assert torch.count_nonzero(got[1, :, P_ // 2, 0]) == 0
    assert torch.count_nonzero(got[0, :, P_ - 1, 0]) > 0
    coef = float(torch.tensor(weight, dtype=torch.float32)) / weight    # the entry takes the weight as fp32
    err = _rel_l2(got.reshape(1, -1), (want * coef).reshape(1, -1))
    print(f"distance backward C {C} P {P_}: err {err:.3e} bar {2.0 ** -23:.3e}")
    assert err <= 2.0 ** -23
    masked = torch.empty_like(got, device=dev)
    _call("cidnet_lpips_layer_bwd", f0.to(dev), f1.to(dev), head.to(dev), masked, ctypes.c_float(weight), 1, 2, C, P_)
    assert torch.equal(masked.cpu(), torch.where(f0 > 0, got, torch.zeros_like(got)))
    same = torch.full(f0.shape, float("nan"), device=dev)
    _call("cidnet_lpips_layer_bwd", f0.to(dev), f0.clone().to(dev), head.to(dev), same, ctypes.c_float(weight), 0, 2, C, P_)
    assert torch.count_nonzero(same) == 0                               # f0 == f1: exactly 0 everywhere


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _run(x, gt, dev, weight=1.0):
    xd = x.to(dev).requires_grad_(True)
    loss = P.LPIPSLoss(_params(), loss_weight=weight)(xd, gt.to(dev))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    return loss.detach().cpu(), xd.grad.detach().cpu()


@pytest.mark.parametrize("h,w", E2E_SHAPES)
def test_loss_and_gradient_match_the_fp64_restatement(dev, h, w):
    x, gt, v64, g64, v32, g32 = _e2e_reference(h, w)
    loss, grad = _run(x, gt, dev)
    assert torch.isfinite(g64).all() and torch.isfinite(grad).all()
    vbar = max(MARGIN * abs(float(v32) - float(v64)) / float(v64), FLOOR)
    verr = abs(float(loss) - float(v64)) / float(v64)
    gbar, d32 = _bar(g32, g64)
    gerr = _rel_l2(grad, g64)
    print(f"lpips loss {h} x {w}: loss {float(v64):.6e} err {verr:.3e} bar {vbar:.3e}; gradient err {gerr:.3e} bar {gbar:.3e} "
          f"(fp32 restatement {d32:.3e})")
    assert verr <= vbar, (verr, vbar)
    assert gerr <= gbar, (gerr, gbar)
    assert float(v64) > 1e-3


def test_loss_agrees_with_the_metric(dev):
    """x = u / 255: the loss is the mean of metrics.lpips of the 8-bit pair (the two ingests differ by fp32 roundings of x)"""
    restored, gt = R.images(2, 64, 64, seed=1)
    q, g = torch.from_numpy(restored).to(dev), torch.from_numpy(gt).to(dev)
    want = float(P.lpips(q, g, _params()).mean())
    with torch.no_grad():
        got = float(P.LPIPSLoss(_params())(q.float() / 255, g.float() / 255))
    x, gtf, v64, _, v32, _ = _e2e_reference(64, 64)
    bar = max(MARGIN * abs(float(v32) - float(v64)) / float(v64), FLOOR)
    err = abs(got - want) / want
    print(f"loss vs metric: {got:.8e} vs {want:.8e} err {err:.3e} bar {bar:.3e}")
    assert err <= bar


def test_identical_images_give_exactly_zero(dev):
    x, _ = _pair(2, 64, 64)
    loss, grad = _run(x, x.clone(), dev)
    assert float(loss) == 0.0 and torch.count_nonzero(grad) == 0


def test_calls_are_bit_identical_and_the_batch_only_scales(dev):
    x, gt = _pair(2, 67, 95)
    a, b = _run(x, gt, dev), _run(x, gt, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _, alone = _run(x[:1], gt[:1], dev)
    assert torch.equal(a[1][0], alone[0] * 0.5) and torch.count_nonzero(alone) > 0


# ---- integration ----------------------------------------------------------------------------------------------------------
def _model(dev, chans=(12, 12, 24, 48)):
    from oracle import cidnet_oracle as O
    m = P.CIDNet(channels=list(chans))
    p = O.make_params(21, channels=chans)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


def _step(m, loss_fn, x, gt):
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.retain_grad()
    loss = loss_fn(out, gt)
    loss.backward()
    grads = {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None}
    return loss.detach().clone(), out.grad.detach().clone(), out.detach(), grads


def test_cidnet_loss_term(dev):
    from oracle import cidnet_oracle as O
    x = O.synthetic_batch(31, (2, 3, 32, 48)).to(dev)
    gt = O.synthetic_batch(32, (2, 3, 32, 48)).to(dev)
    m = _model(dev)
    m.two_streams = False
    base = _step(m, P.CIDNetLoss(m), x, gt)
    off = _step(m, P.CIDNetLoss(m, lpips_weight=0.0), x, gt)
    assert torch.equal(base[0], off[0]) and torch.equal(base[1], off[1])      # the default objective did not move
    assert len(base[3]) > 50 and base[3].keys() == off[3].keys()
    for n, g in base[3].items():                                              # nor any parameter's gradient
        assert torch.equal(g, off[3][n]), n
    wgt = 0.3
    on = _step(m, P.CIDNetLoss(m, lpips_weight=wgt, lpips_params=_params()), x, gt)
    out = on[2].clone().requires_grad_(True)
    term = P.LPIPSLoss(_params(), loss_weight=wgt)(out, gt)
    term.backward()
    assert float(term.detach()) > 0
    # fp32 summation: one more addend to a loss of a few units, one more to every gradient element
    assert abs(float(on[0]) - (float(base[0]) + float(term))) <= 4 * 2.0 ** -24 * abs(float(on[0]))
    want = base[1].double() + out.grad.double()
    assert float((on[1].double() - want).abs().max()) <= 4 * 2.0 ** -24 * float((base[1].abs() + out.grad.abs()).max())


def test_trainer_steps_with_the_term_eager_and_captured(dev):
    from oracle import cidnet_oracle as O
    from hvi_cidnet_amd.dp import DataParallelTrainer
    shape = (2, 3, 64, 64)
    batches = [(O.synthetic_batch(51 + i, shape).to(dev), O.synthetic_batch(61 + i, shape).to(dev)) for i in range(2)]
    res = []
    for use_graph in (False, True):
        m = _model(dev)
        prm = P.LpipsParams.random()                                    # fresh: nothing of it is on the device yet
        assert not prm._dev and not prm._dgrad
        loss_fn = P.CIDNetLoss(m, lpips_weight=0.5, lpips_params=prm)
        assert len(prm._dev) == 1 and len(prm._dgrad) == 1              # built on the model's device: prepared before any step
        tr = DataParallelTrainer(m, lr=1e-3, n_buckets=3, use_graph=use_graph, loss_fn=loss_fn)
        losses = [float(tr.step(x, gt).item()) for x, gt in batches]
        torch.cuda.synchronize()
        res.append((losses, tr.flat_g.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_prepare_and_the_second_backward(dev):
    """.to(device) prepares the parameters there; a second backward through the same graph is a clear error"""
    prm = P.LpipsParams.random()
    crit = P.LPIPSLoss(prm).to(dev)
    assert len(prm._dev) == 1 and len(prm._dgrad) == 1
    x, gt = _pair(1, 31, 31)
    xd = x.to(dev).requires_grad_(True)
    loss = crit(xd, gt.to(dev))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="freed by the first backward"):
        loss.backward()
