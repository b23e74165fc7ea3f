"""References, fixtures and criteria of tests/test_loss_kernels_gpu.py; nothing here touches a GPU, and
tests/test_loss_kernels_cpu.py checks on the host that the fixtures measure what they claim and that the criteria can be met.

References are fp64 CPU torch: the oracle's ssim_loss / edge_loss / tnsm_noise_losses with autograd, and plain torch expressions
for the vgg.hip and train.hip pieces.  `E32` of a quantity is the deviation of the SAME oracle evaluated in fp32 on the CPU from its
fp64 evaluation: what a correct fp32 implementation may lose on that input.

`ssim_kernel_restated` is a numpy fp32 restatement of csrc/ssim.hip in the kernel's own order (dy outer, dx inner,
wgt = g[dy] * g[dx], five running sums, the A / B / C maps, their three filtered maps, gs * (fa + 2 x fb + y fc)), with the FMA
either emulated (an fp64 product-sum rounded once) or left out.  The reduction tree of the loss is not restated: the S map is summed
per 16 x 64 tile and then over the tiles, in fp32.  It runs only on the host, to show that a correct fp32 implementation of this
algorithm meets the content criteria.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cidnet_oracle as O

F32, F64 = torch.float32, torch.float64
f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------
SSIM_LOSS_ATOL = 2e-6                  # tests/test_losses_gpu.py: |loss - ref| <= 2e-6
SSIM_GRAD_RTOL, SSIM_GRAD_ATOL = 1e-4, 1e-10
E32_FACTOR = 8                         # content cases: the plain criterion + 8 x the fp32 oracle's own deviation
SSIM_WEIGHT, SSIM_UPSTREAM = 0.5, 3.0


def ssim_loss_bound(e32=0.0):
    return SSIM_LOSS_ATOL + E32_FACTOR * e32


def ssim_grad_bound(ref64, e32=0.0):
    return SSIM_GRAD_RTOL * ref64.abs().max().item() + SSIM_GRAD_ATOL + E32_FACTOR * e32


def gen(*seed):
    s = 0
    for v in seed:
        s = s * 1009 + int(v)
    return torch.Generator().manual_seed(s)


def ids(cases):
    return ["x".join(map(str, c)) if isinstance(c, (tuple, list)) else str(c) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# A. SSIM
# ---------------------------------------------------------------------------------------------------------------------
SSIM_HW = [(1, 1), (3, 4), (5, 130), (6, 63), (15, 64), (16, 65), (17, 128), (33, 129)]
SSIM_GEOMETRY = [(b, c, h, w) for h, w in SSIM_HW for b, c in ((1, 1), (2, 3))] + [(1, 4, 2, 9), (8, 4, 33, 129)]
SSIM_CONTENT_SHAPES = [(1, 3, 33, 71), (2, 1, 24, 36)]
SSIM_CONTENT = ["flat_one", "flat_09_08", "const_07_03", "const_07_07", "identical", "ramp", "uint8", "signed"]
# the cases whose fp32 oracle itself misses the plain criterion (asserted on the host)
SSIM_ILL_CONDITIONED = ["flat_one", "flat_09_08", "const_07_03"]


def ssim_blocks(shape):
    b, c, h, w = shape
    return b * c * (-(-h // 16)) * (-(-w // 64))


def ssim_noise_pair(shape):
    g = gen(11, *shape)
    x = torch.rand(shape, generator=g)
    y = (0.7 * x + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)
    return x, y


def ssim_content_pair(kind, shape):
    """fp32 (x, y) of a content case; patches are the central half of the plane inside a white-noise frame"""
    b, c, h, w = shape
    g = gen(13, SSIM_CONTENT.index(kind), *shape)
    x = torch.rand(shape, generator=g)
    y = (0.7 * x + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)
    r0, r1, c0, c1 = h // 4, h - h // 4, w // 4, w - w // 4
    if kind == "flat_one":
        x[..., r0:r1, c0:c1] = 1.0
        y[..., r0:r1, c0:c1] = 1.0
    elif kind == "flat_09_08":
        x[..., r0:r1, c0:c1] = 0.9
        y[..., r0:r1, c0:c1] = 0.8
    elif kind == "const_07_03":
        x, y = torch.full(shape, 0.7), torch.full(shape, 0.3)
    elif kind == "const_07_07":
        x, y = torch.full(shape, 0.7), torch.full(shape, 0.7)
    elif kind == "identical":
        y = x.clone()
    elif kind == "ramp":
        u = torch.linspace(0, 1, h).view(1, 1, h, 1)
        v = torch.linspace(0, 1, w).view(1, 1, 1, w)
        x = (0.5 + 0.4 * torch.sin(3 * u + 2 * v)).expand(shape).contiguous()
        y = (x + 0.02 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif kind == "uint8":
        x = torch.round(x * 255) / 255
        y = torch.round(y * 255) / 255
    elif kind == "signed":
        x, y = 2 * x - 1, 2 * y - 1
    else:
        raise KeyError(kind)
    return x.float().contiguous(), y.float().contiguous()


def ssim_oracle(x, y, dtype, weight=SSIM_WEIGHT, upstream=SSIM_UPSTREAM):
    """(loss, d/dx, d/dy of upstream * loss) of the oracle evaluated in `dtype` on the CPU, returned as fp64"""
    a, b = x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)
    loss = O.ssim_loss(a, b, weight)
    (upstream * loss).backward()
    return loss.detach().double().item(), a.grad.double(), b.grad.double()


def with_e32(fn, *inputs):
    """fn(*inputs, dtype) -> (loss, grad, ...): -> (the fp64 results, E32 of each: |fp32 - fp64|, max over a tensor)"""
    r64, r32 = fn(*inputs, F64), fn(*inputs, F32)
    e = [abs(a - b) if isinstance(a, float) else (a - b).abs().max().item() for a, b in zip(r32, r64)]
    return r64, e


@functools.lru_cache(maxsize=None)
def ssim_geometry_ref(shape):
    x, y = ssim_noise_pair(shape)
    return x, y, ssim_oracle(x, y, F64)


@functools.lru_cache(maxsize=None)
def ssim_content_ref(kind, shape):
    """x, y, (loss64, gx64, gy64), (E32 of the loss, of gx, of gy)"""
    x, y = ssim_content_pair(kind, shape)
    r64, e32 = with_e32(ssim_oracle, x, y)
    return x, y, r64, e32


def kernel_gauss():
    """make_gauss of csrc/ssim.hip: exp in double rounded to fp32, an fp32 running sum, an fp32 division"""
    g = np.array([f32(math.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5))) for i in range(11)], dtype=f32)
    s = f32(0)
    for v in g:
        s = f32(s + v)
    return (g / s).astype(f32)


def _mac(acc, w, v, fma):
    """acc + w * v in fp32: fused (one rounding of the fp64 product-sum) or as two fp32 operations"""
    if fma:
        return (acc.astype(np.float64) + np.float64(w) * v.astype(np.float64)).astype(f32)
    return (acc + (f32(w) * v).astype(f32)).astype(f32)


def _filter(maps, g, fma):
    """the kernel's 121-tap loop over zero-padded planes: maps (K, P, H, W) fp32 -> their filtered planes"""
    k, p, h, w = maps.shape
    pad = np.zeros((k, p, h + 10, w + 10), f32)
    pad[:, :, 5:5 + h, 5:5 + w] = maps
    acc = np.zeros_like(maps)
    for dy in range(11):
        for dx in range(11):
            wgt = f32(g[dy] * g[dx])
            acc = _mac(acc, wgt, pad[:, :, dy:dy + h, dx:dx + w], fma)
    return acc


def _ssim_fwd_restated(x, y, g, fma):
    xx, yy, xy = (x * x).astype(f32), (y * y).astype(f32), (x * y).astype(f32)
    m1, m2, e11, e22, e12 = _filter(np.stack([x, y, xx, yy, xy]), g, fma)

    def msub(e, a, b):                 # e - a * b
        if fma:
            return (e.astype(np.float64) - a.astype(np.float64) * b.astype(np.float64)).astype(f32)
        return (e - (a * b).astype(f32)).astype(f32)

    C1, C2 = f32(f32(0.01) * f32(0.01)), f32(f32(0.03) * f32(0.03))
    two = f32(2)
    s1, s2, s12 = msub(e11, m1, m1), msub(e22, m2, m2), msub(e12, m1, m2)
    N1, N2 = two * m1 * m2 + C1, two * s12 + C2
    D1, D2 = m1 * m1 + m2 * m2 + C1, s1 + s2 + C2
    inv = f32(1) / (D1 * D2)
    S = N1 * N2 * inv
    A = (two * m2 * N2 - two * m2 * N1) * inv - S * two * m1 / D1 + S * two * m1 / D2
    B = -S / D2
    C = two * N1 * inv
    assert all(a.dtype == f32 for a in (S, A, B, C))
    return S, A, B, C


def ssim_kernel_restated(x, y, weight=SSIM_WEIGHT, upstream=SSIM_UPSTREAM, fma=True):
    """x, y (B, C, H, W) fp32 tensors -> (loss, gx, gy) as csrc/ssim.hip computes them, in numpy fp32 on the host"""
    shape = tuple(x.shape)
    b, c, h, w = shape
    xn, yn = x.numpy().reshape(b * c, h, w).astype(f32), y.numpy().reshape(b * c, h, w).astype(f32)
    g = kernel_gauss()
    n = b * c * h * w
    gs = f32(f32(-f32(weight) / f32(n)) * f32(upstream))
    out = []
    loss = None
    for p, q in ((xn, yn), (yn, xn)):
        S, A, B, C = _ssim_fwd_restated(p, q, g, fma)
        if loss is None:
            part = [S[:, r:r + 16, s:s + 64].reshape(b * c, -1).sum(1, dtype=f32) for r in range(0, h, 16) for s in range(0, w, 64)]
            tot = np.concatenate(part).sum(dtype=f32)
            loss = float(f32((f32(1) - tot * f32(f32(1) / f32(n))) * f32(weight)))
        fa, fb, fc = _filter(np.stack([A, B, C]), g, fma)
        grad = gs * (fa + f32(2) * p * fb + q * fc)
        assert grad.dtype == f32
        out.append(torch.from_numpy(grad.reshape(shape)).double())
    return loss, out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------
# B. L1
# ---------------------------------------------------------------------------------------------------------------------
L1_N = [1, 2, 3, 5, 1023, 1025]
L1_WRAP_SHAPE = (1, 3, 593, 591)       # 1,051,389 elements > 1024 * 256 * 4, n & 3 == 1
L1_OFFSETS = [1, 2, 3]
L1_LOSS_RTOL = 2e-6


def l1_pair(n, quantised=False, seed=0):
    g = gen(21, n, seed)
    if quantised:                      # sixteen levels: one element in sixteen is an exact tie
        return (torch.randint(0, 16, (n,), generator=g) / 16.0).float(), (torch.randint(0, 16, (n,), generator=g) / 16.0).float()
    return torch.rand(n, generator=g), torch.rand(n, generator=g)


def l1_ref(x, y):
    """fp64 loss; the exact fp32 gradient wrt x: sign(x - y) * fp32(1 / n)"""
    n = x.numel()
    inv = (torch.ones((), dtype=F32) / torch.tensor(float(n), dtype=F32))
    return (x.double() - y.double()).abs().mean().item(), torch.sign(x - y) * inv


# ---------------------------------------------------------------------------------------------------------------------
# C. edge loss
# ---------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(1, 3, 419, 421), (1, 1, 1, 1), (1, 2, 1, 7), (2, 1, 6, 1), (1, 3, 3, 2)]   # the first: 529,197 > 2048 * 256
EDGE_CONST_SHAPES = [(1, 3, 33, 71), (2, 1, 6, 5)]
EDGE_WEIGHT, EDGE_UPSTREAM = 50.0, 0.5


def edge_pair(shape):
    g = gen(31, *shape)
    x = torch.rand(shape, generator=g)
    return x, (0.6 * x + 0.4 * torch.rand(shape, generator=g)).clamp(0, 1)


def edge_const_pair(shape):
    """x - y = 0.25 exactly in fp32: y on a 2^-10 grid in [0, 0.75)"""
    y = torch.randint(0, 768, shape, generator=gen(32, *shape)).float() / 1024.0
    x = y + 0.25
    assert torch.equal(x - y, torch.full(shape, 0.25))
    return x, y


def edge_oracle(x, y, dtype, weight=EDGE_WEIGHT, upstream=EDGE_UPSTREAM):
    a, b = x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)
    loss = O.edge_loss(a, b, weight)
    (upstream * loss).backward()
    return loss.detach().double().item(), a.grad.double(), b.grad.double()


@functools.lru_cache(maxsize=None)
def edge_ref(shape):
    x, y = edge_pair(shape)
    return x, y, edge_oracle(x, y, F64)


# ---------------------------------------------------------------------------------------------------------------------
# D. vgg.hip
# ---------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 2, 2), (2, 3, 5, 7), (1, 2, 6, 9), (1, 1, 3, 2), (2, 1, 2051, 2049)]   # the last: 2,099,200 windows > 8192 * 256
POOL_KINDS = ["noise", "relu", "dup"]
BIAS_RELU_SHAPES = [(1, 3, 1), (2, 5, 7), (1, 2, 257 * 257), (3, 64, 30)]
RELU_BWD_N = [1, 3, 1026, 4194307]     # the last: > 4096 * 256 * 4, n & 3 == 3
NORM_HW = [1, 35, 593 * 591]           # the last at B = 1: 1,051,389 > 4096 * 256
NORM_RTOL = 5e-7
MSE_N = [1, 3, 1022, 1051389]          # the last: > 1024 * 256 * 4, n & 3 == 1
MSE_LOSS_RTOL, MSE_GRAD_RTOL = 2e-6, 2e-7
PERCEPTUAL_SHAPES = [(1, 3, 16, 16), (1, 3, 35, 51)]


def pool_input(kind, shape):
    g = gen(41, POOL_KINDS.index(kind), *shape)
    if kind == "noise":
        return torch.randn(shape, generator=g)
    if kind == "relu":                 # post-ReLU: half exact zeros, so one window in sixteen ties at 0 in all four
        return torch.randn(shape, generator=g).clamp_min(0)
    return torch.randint(0, 4, shape, generator=g).float() / 4.0       # four levels: four windows in ten have a tied maximum


def pool_ref(x, gy):
    """F.max_pool2d in fp64 on the same values, and the routing of gy (the first maximum in scan order takes it)"""
    a = x.double().requires_grad_(True)
    y = F.max_pool2d(a, 2, 2)
    (gx,) = torch.autograd.grad(y, a, gy.double())
    return y.detach().float(), gx.float()


def vgg_norm_ref(x, range_norm):
    a = x.double().requires_grad_(True)
    v = (a + 1) / 2 if range_norm else a
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=F64).view(1, 3, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=F64).view(1, 3, 1)
    return ((v - mean) / std), a


def mse_ref(a, b, weight):
    x = a.double().requires_grad_(True)
    loss = F.mse_loss(x, b.double()) * weight
    (g,) = torch.autograd.grad(loss, x)
    return loss.item(), g


# ---------------------------------------------------------------------------------------------------------------------
# E. hvi_grad_sum, scale
# ---------------------------------------------------------------------------------------------------------------------
HVI_COMBOS = [c for c in ((a, b, d) for a in (1, 0) for b in (1, 0) for d in (1, 0)) if any(c)]      # (ga, gc, gi) present
HVI_HW = [1, 3, 4, 37 * 41, 933333]    # the last at B = 3: 2,100,006 quads > 8192 * 256, HW & 3 == 1
SCALE_N = [1, 3, 1026, 4194307]        # the last: > 4096 * 256 * 4
SCALE_OFFSETS = [1, 2, 3]


def hvi_grad_sum_ref(ga, gc, gi, B, HW):
    """fp32 (ga + gc) + gi on plane 2, ga + gc elsewhere; a missing term is 0"""
    z = torch.zeros(B, 3, HW)
    out = (ga if ga is not None else z) + (gc if gc is not None else z)
    if gi is not None:
        out = out.clone()
        out[:, 2] = out[:, 2] + gi[:, 0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# F. TNSM noise loss
# ---------------------------------------------------------------------------------------------------------------------
TNSM_WRAP_SHAPES = [(1, 1, 513, 513), (1, 3, 513, 513)]      # 263,169 pixels > 1024 * 256
TNSM_TIE_SHAPES = [(2, 3, 33, 47), (1, 1, 40, 64)]
TNSM_WEIGHT, TNSM_UPSTREAM = 0.7, 2.0
TNSM_LEVELS = 1023                     # 10-bit maps: a neighbour pair ties once in 1023
TNSM_NEAR = 1e-6
TNSM_MASK_KEEPS = 0.99


def tnsm_inputs(shape, quantised=False):
    b, c, h, w = shape
    g = gen(51, int(quantised), *shape)
    nm, out = torch.rand(shape, generator=g), torch.rand((b, 3, h, w), generator=g)
    im = (0.6 * out + 0.4 * torch.rand((b, 3, h, w), generator=g)).clamp(0, 1)
    if quantised:
        nm, out, im = (torch.round(t * TNSM_LEVELS) / TNSM_LEVELS for t in (nm, out, im))
    else:                              # keep nm - target away from 0, where fp32 and fp64 may take different signs
        tgt = 1.0 - torch.sigmoid((out.double() - im.double()).abs().mean(1, keepdim=True))
        nm = torch.where((nm.double() - tgt).abs() < 1e-5, nm + 1e-3, nm)
    return nm.float().contiguous(), out.float().contiguous(), im.float().contiguous()


def tnsm_oracle(nm, out, im, weight=TNSM_WEIGHT, upstream=TNSM_UPSTREAM):
    a, b = nm.double().requires_grad_(True), out.double().requires_grad_(True)
    c, s = O.tnsm_noise_losses(a, b, im.double())
    loss = weight * (c + s)
    (upstream * loss).backward()
    return loss.item(), a.grad, b.grad


@functools.lru_cache(maxsize=None)
def tnsm_ref(shape, quantised=False):
    nm, out, im = tnsm_inputs(shape, quantised)
    return nm, out, im, tnsm_oracle(nm, out, im)


def tnsm_masks(nm, out, im):
    """Per gradient entry, the |.| arguments of the fp64 reference it depends on: for d/d noise_map its own nm - target and its up
    to four neighbour differences; for d/d output_rgb its own out - im and the nm - target of every channel of its pixel.
    -> (strict_nm, strict_out, near_nm, near_out): `strict` keeps the entries with no argument within 1e-6 of 0 (exact ties
    excluded), `near` drops only the entries with 0 < |nm - target| < 1e-6: exact ties have sign 0 on both sides."""
    nm, out, im = nm.double(), out.double(), im.double()
    tgt = 1.0 - torch.sigmoid((out - im).abs().mean(1, keepdim=True))
    e = nm - tgt
    dx, dy = nm[..., :, :-1] - nm[..., :, 1:], nm[..., :-1, :] - nm[..., 1:, :]
    d = out - im

    def masks(bad, bad_diff):
        b_e, b_dx, b_dy, b_d = bad(e), bad_diff(dx), bad_diff(dy), bad_diff(d)
        m = b_e.clone()
        m[..., :, :-1] |= b_dx
        m[..., :, 1:] |= b_dx
        m[..., :-1, :] |= b_dy
        m[..., 1:, :] |= b_dy
        return ~m, ~(b_d | b_e.any(1, keepdim=True))

    def close(t):
        return t.abs() < TNSM_NEAR

    # a difference of two fp32 inputs has the same sign in fp32 as in fp64 (the subtraction is correctly rounded and cannot
    # reach 0 from a non-zero value), so of the arguments only nm - target, whose target is computed, can change sign
    s_nm, s_out = masks(close, close)
    n_nm, n_out = masks(lambda t: close(t) & (t != 0), lambda t: torch.zeros_like(t, dtype=torch.bool))
    return s_nm, s_out, n_nm, n_out


# ---------------------------------------------------------------------------------------------------------------------
# the whole perceptual loss: fixtures that stay off the kinks
# ---------------------------------------------------------------------------------------------------------------------
# d/dx of the VGG stack is discontinuous where a pre-activation crosses 0 (the ReLU mask) and where the two largest values of a
# pooling window cross (the routing).  A fixture with a pre-activation closer to 0 than fp32 rounding of a 2304-term sum cannot
# be compared: with the seeds of tests/test_losses_gpu.py, (1, 3, 35, 51) has conv3_1[132, 4, 9] = 6.3e-6 where the fp32 CPU
# evaluation of that layer is itself off by up to 7.5e-6, and the one unit's mask moves 2 % of max|grad| over a 24 x 24 patch.
# So each shape takes the first seed pair (151 + 2k, 152 + 2k) whose `kink_margin` is at least KINK_MARGIN: every ReLU
# pre-activation, and every gap between the two largest values of a pooling window with a positive maximum, at least that
# many times the largest deviation of the fp32 CPU evaluation of its layer from fp64.  Decided from the reference alone.
KINK_MARGIN = 4.0
PERCEPTUAL_LAYER_WEIGHTS = {"conv1_2": 1, "conv2_2": 1, "conv3_4": 0.5, "conv4_4": 2}
PERCEPTUAL_SEEDS = {(1, 3, 16, 16): (151, 152), (1, 3, 35, 51): (159, 160)}       # margins 16.8 and 5.3; (35, 51) at 151: 0.85


def perceptual_convs(crit):
    """{name: (weight, bias)} in fp64 of a PerceptualLoss module's frozen VGG stack"""
    net = crit.vgg.vgg_net
    return {n: (getattr(net, n).weight.detach().cpu().double(), getattr(net, n).bias.detach().cpu().double())
            for n in O.VGG19_NAMES if n != "pool" and hasattr(net, n)}


def perceptual_pair(shape, seeds):
    x = O.synthetic_batch(seeds[0], shape) * 2 - 1
    return x, (0.6 * x + 0.4 * (O.synthetic_batch(seeds[1], shape) * 2 - 1))


def kink_margin(x, convs, last="conv4_4"):
    """convs: {name: (weight, bias)} fp64.  -> min over the ReLU layers and pools in front of `last` of distance-to-kink / E32"""
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=F64).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=F64).view(1, 3, 1, 1)
    t = ((x.double() + 1) / 2 - mean) / std
    t32 = (((x + 1) / 2) - mean.float()) / std.float()
    margin, e32 = float("inf"), 0.0
    for name in O.VGG19_NAMES[:O.VGG19_NAMES.index(last)]:
        if name == "pool":
            h, w = t.shape[2] // 2 * 2, t.shape[3] // 2 * 2
            win = t[:, :, :h, :w].unfold(2, 2, 2).unfold(3, 2, 2).reshape(*t.shape[:2], h // 2, w // 2, 4)
            top = win.topk(2, -1).values
            gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
            margin = min(margin, gap.min().item() / e32)
            t, t32 = F.max_pool2d(t, 2, 2), F.max_pool2d(t32, 2, 2)
            continue
        w_, b_ = convs[name]
        pre, pre32 = F.conv2d(t, w_, b_, padding=1), F.conv2d(t32, w_.float(), b_.float(), padding=1)
        e32 = (pre32.double() - pre).abs().max().item()
        margin = min(margin, pre.abs().min().item() / e32)
        t, t32 = F.relu(pre), F.relu(pre32)
    return margin
