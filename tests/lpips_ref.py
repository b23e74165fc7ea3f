"""Plain-torch restatement of lpips.LPIPS(net='alex') (version 0.1, lpips=True, spatial=False, eval mode), written from the
definition in include/cidnet_hip.h (LPIPS, steps 1-5), with the dtype of the arithmetic as a parameter: torch.float64 is
the yardstick of the GPU tests, torch.float32 the same restatement in the kernels' storage precision, whose distance from
fp64 sets the tests' bars.  The lpips package and torchvision's weights are not dependencies; the parameters are an
LpipsParams (hvi-cidnet_amd/metrics.py).  Runs on the CPU.

    u:        (B,3,h,w) float64 tensor of 8-bit values (or of clip(u s, 0, 255) under GT mean: rescaled())
    ingest:   x = u / 127.5 - 1 in fp64, rounded once to fp32, then (x - shift) / scale in `dtype` (the constants are the fp32
              ones, widened)
    features: five taps of AlexNet, each after its ReLU
    layers:   d_l = mean over pixels of sum_c w_l[c] (n(f0) - n(f1))^2, n(f) = f / (sqrt(sum_c f^2) + 1e-10) -> (B,5)
    score:    sum_l d_l -> (B,)"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref  # noqa: E402

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (out channels, in channels, kernel, stride, padding, a 3 x 3 stride-2 max pool first)
LAYERS = ((64, 3, 11, 4, 2, False), (192, 64, 5, 1, 2, True), (384, 192, 3, 1, 1, True), (256, 384, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))


def as_u(images_u8):
    """uint8 (B,3,h,w) numpy array or tensor -> float64 tensor"""
    return torch.as_tensor(np.asarray(images_u8)).to(torch.float64)


def rescaled(restored_u8, gt_u8):
    """GT mean: float64 (B,3,h,w) clip(restored * s, 0, 255), s formed as metrics_ref forms it; not re-quantized"""
    return torch.from_numpy(np.stack([metrics_ref.gt_mean_image(np.asarray(r), np.asarray(g))
                                      for r, g in zip(restored_u8, gt_u8)]))


def ingest(u, dtype):
    x = (u.to(torch.float64) / 127.5 - 1.0).to(torch.float32).to(dtype)
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def features(u, params, dtype=torch.float64):
    x = ingest(u, dtype)
    out = []
    for l, (_, _, _, stride, pad, pooled) in enumerate(LAYERS):
        if pooled:
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, params.weights[l].to(dtype), params.biases[l].to(dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def _normalize(f):
    return f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + 1e-10)


def layers_from(f0, f1, params):
    cols = []
    for l in range(5):
        d = (_normalize(f0[l]) - _normalize(f1[l])) ** 2
        w = params.heads[l].to(d.dtype).view(1, -1, 1, 1)
        cols.append((d * w).sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(cols, dim=1)


def layers(u0, u1, params, dtype=torch.float64):
    return layers_from(features(u0, params, dtype), features(u1, params, dtype), params)


def score(u0, u1, params, dtype=torch.float64):
    return layers(u0, u1, params, dtype).sum(dim=1)


def images(B, h, w, seed=0):
    """The inputs of the GPU tests -> (restored, gt) uint8 (B,3,h,w) arrays.  The ground truth is a horizontal ramp mixed with
    uniform noise, so that it has structure and every tap matters; the restored image is that x 0.8 plus Gaussian noise of
    sigma 12, clipped."""
    rng = np.random.default_rng(seed)
    ramp = np.broadcast_to(np.linspace(0.0, 255.0, w), (B, 3, h, w))
    gt = np.clip(0.6 * ramp + 0.4 * rng.uniform(0.0, 255.0, (B, 3, h, w)), 0, 255).astype(np.uint8)
    restored = np.clip(gt.astype(np.float64) * 0.8 + rng.normal(0.0, 12.0, gt.shape), 0, 255).astype(np.uint8)
    return restored, gt
