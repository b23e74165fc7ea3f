"""Plain-torch restatement of the LPIPS (AlexNet) training loss, forward and hand-written backward, from the definition in
include/cidnet_hip.h ("LPIPS training loss"), with the dtype of the arithmetic as a parameter like tests/lpips_ref.py:
torch.float64 is the yardstick of the GPU tests, torch.float32 the same restatement in the kernels' storage precision, whose
distance from fp64 sets the bars.  Runs on the CPU.

    x, gt:    fp32 (B,3,h,w) in [0, 1] (any range is taken)
    ingest:   v = 2 x - 1 in fp32, then (v - shift) / scale in `dtype`; backward (g / scale) * 2
    features: the five post-ReLU taps (lpips_ref.LAYERS)
    loss:     weight / B * sum_b sum_l d_l(b)
    backward: the gradient rules of the header -- ReLU mask on the stored value, pool gradient to the first maximum in scan
              order and summed in window scan order, the distance derivative with 0 at an all-zero pixel, the stride-4 data
              gradient as a gather over the at most 3 x 3 windows that reach a pixel"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402

EPS = 1e-10


def _consts(dtype):
    shift = torch.tensor(R.SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    scale = torch.tensor(R.SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return shift, scale


def scaling(v):
    """lpips' scaling layer in v's dtype"""
    shift, scale = _consts(v.dtype)
    return (v - shift) / scale


def ingest(x, dtype):
    return scaling((2.0 * x.to(torch.float32) - 1.0).to(dtype))


def ingest_bwd(g):
    _, scale = _consts(g.dtype)
    return (g / scale) * 2.0


def taps(z, params):
    """z: the ingested image -> the five post-ReLU taps, in z's dtype"""
    out, x = [], z
    for l, (_, _, _, stride, pad, pooled) in enumerate(R.LAYERS):
        if pooled:
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, params.weights[l].to(z.dtype), params.biases[l].to(z.dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def loss_from_taps(f0, f1, params, weight=1.0):
    return weight * R.layers_from(f0, f1, params).sum(dim=1).mean()


def loss(x, gt, params, dtype=torch.float64, weight=1.0):
    """differentiable in x through torch's autograd (NaN where a feature pixel of x is all zero)"""
    return loss_from_taps(taps(ingest(x, dtype), params), taps(ingest(gt, dtype), params), params, weight)


def dist_bwd(f0, f1, head, coef):
    """d/df0 of coef * sum_p sum_c head_c (n0_c - n1_c)^2, n = f / (s + eps), s = sqrt(sum_c f_c^2); 0 in every channel of a
    pixel whose f0 is all zero"""
    s0 = torch.sqrt((f0 * f0).sum(dim=1, keepdim=True))
    s1 = torch.sqrt((f1 * f1).sum(dim=1, keepdim=True))
    dn = 2.0 * head.to(f0.dtype).view(1, -1, 1, 1) * (f0 / (s0 + EPS) - f1 / (s1 + EPS)) * coef
    dot = (dn * f0).sum(dim=1, keepdim=True)
    dead = s0 == 0
    back = dot / torch.where(dead, torch.ones_like(s0), s0 * (s0 + EPS) ** 2)
    return torch.where(dead, torch.zeros_like(f0), dn / (s0 + EPS) - f0 * back)


def pool_first_max(x):
    """-> (planes..., Ho, Wo) int64: the position 0..8 (row-major in the window) of each 3 x 3 stride-2 window's first maximum;
    a later value replaces the maximum only when strictly greater"""
    H, W = x.shape[-2:]
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1

    def at(k):
        return x[..., k // 3:k // 3 + 2 * Ho - 1:2, k % 3:k % 3 + 2 * Wo - 1:2]
    m = at(0).clone()
    arg = torch.zeros(m.shape, dtype=torch.int64)
    for k in range(1, 9):
        up = at(k) > m
        m = torch.where(up, at(k), m)
        arg = torch.where(up, torch.full_like(arg, k), arg)
    return arg


def pool_bwd(x, gy):
    """the backward of max_pool2d(x, 3, 2) by the header's rule: every window's gradient to its first maximum, an element's
    windows added in window scan order in gy's dtype (a fixed order: the kernel's result bit for bit)"""
    H, W = x.shape[-2:]
    arg = pool_first_max(x)
    Ho, Wo = arg.shape[-2:]
    gx = torch.zeros(x.shape, dtype=gy.dtype).reshape(-1, H, W)
    arg, g = arg.reshape(-1, Ho, Wo), gy.reshape(-1, Ho, Wo)
    planes = torch.arange(gx.shape[0])
    for oy in range(Ho):
        for ox in range(Wo):
            a = arg[:, oy, ox]
            gx[planes, 2 * oy + a // 3, 2 * ox + a % 3] += g[:, oy, ox]
    return gx.reshape(x.shape)


def conv_dgrad_s1(dy, w, pad):
    """stride 1: the convolution of dy with the flipped weights, M and C exchanged, same padding"""
    return F.conv2d(dy, w.to(dy.dtype).flip(2, 3).transpose(0, 1).contiguous(), padding=pad)


def conv1_dgrad(dy, w, h, w_in):
    """the 11 x 11 stride-4 pad-2 layer as a gather: with q = i + 2 the windows that reach row i are oy = q // 4 - j at kernel
    row ky = q % 4 + 4 j, j = 0..2, where 0 <= oy < Ho and ky <= 10"""
    Ho, Wo = dy.shape[-2:]
    w = w.to(dy.dtype)
    qy, qx = torch.arange(h) + 2, torch.arange(w_in) + 2
    dx = torch.zeros((dy.shape[0], w.shape[1], h, w_in), dtype=dy.dtype)
    for jy in range(3):
        oy, ky = qy // 4 - jy, qy % 4 + 4 * jy
        oky = (oy >= 0) & (oy < Ho) & (ky <= 10)
        for jx in range(3):
            ox, kx = qx // 4 - jx, qx % 4 + 4 * jx
            okx = (ox >= 0) & (ox < Wo) & (kx <= 10)
            wg = w[:, :, ky.clamp(0, 10)[:, None], kx.clamp(0, 10)[None, :]]                 # (M,C,h,w)
            dg = dy[:, :, oy.clamp(0, Ho - 1)[:, None], ox.clamp(0, Wo - 1)[None, :]]        # (B,M,h,w)
            ok = (oky[:, None] & okx[None, :]).to(dy.dtype)
            dx += torch.einsum("mchw,bmhw->bchw", wg, dg) * ok
    return dx


def conv_dgrad(dy, w, stride, pad, h, w_in):
    return conv1_dgrad(dy, w, h, w_in) if stride == 4 else conv_dgrad_s1(dy, w, pad)


def loss_and_grad(x, gt, params, dtype=torch.float64, weight=1.0):
    """-> (loss, d loss / d x) by the hand-written chain, all in `dtype`"""
    B, _, h, w = x.shape
    with torch.no_grad():
        f0, f1 = taps(ingest(x, dtype), params), taps(ingest(gt, dtype), params)
        value = loss_from_taps(f0, f1, params, weight)

        def dist(l):
            P = f0[l].shape[-2] * f0[l].shape[-1]
            return dist_bwd(f0[l], f1[l], params.heads[l], weight / (B * P))
        d = dist(4) * (f0[4] > 0)
        for l in range(4, 0, -1):
            _, _, _, stride, pad, pooled = R.LAYERS[l]
            dx = conv_dgrad(d, params.weights[l], stride, pad, *f0[l].shape[-2:])
            if pooled:
                dx = pool_bwd(f0[l - 1], dx)
            d = (dx + dist(l - 1)) * (f0[l - 1] > 0)
        dz = conv_dgrad(d, params.weights[0], 4, 2, h, w)
        return value, ingest_bwd(dz)


def tap_like(shape, seed, zero_plane=None):
    """fp32 planes built like post-ReLU taps: about half exact zeros, plateaus of equal positive values (quantized to eighths),
    optionally one all-zero plane"""
    gen = torch.Generator().manual_seed(seed)
    t = torch.relu(torch.randn(shape, generator=gen))
    t = torch.round(t * 8.0) / 8.0
    if zero_plane is not None:
        t.reshape(-1, *shape[-2:])[zero_plane] = 0.0
    return t.to(torch.float32)
