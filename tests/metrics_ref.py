"""Independent fp64 numpy restatement of the evaluation metrics (hvi-cidnet_amd/metrics.py), written from their
definitions: PSNR 10 log10(255^2 / (MSE + 1e-8)); SSIM with the 11 x 11 Gaussian window (sigma 1.5) on the valid region,
C1 = (0.01 255)^2, C2 = (0.03 255)^2, per-plane mean then the mean of the planes; the GT-mean rescale with the BT.601
fixed-point gray.  The reference's measure.py needs cv2 (not a dependency here), so this restatement is not pinned to it
bit for bit; cv2's gray conversion is the only part that could round differently (by one level per pixel).
Images are uint8 (3,h,w) numpy arrays."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2


def gaussian_1d(n=11, sigma=1.5):
    d = np.arange(n, dtype=np.float64) - (n - 1) / 2
    g = np.exp(-(d * d) / (2 * sigma * sigma))
    return g / g.sum()


def gaussian_window(n=11, sigma=1.5):
    g = gaussian_1d(n, sigma)
    return np.outer(g, g)


def filter_valid(x):
    """sum over the 11 x 11 window of x (2-D, fp64), valid region only -> (h-10, w-10); the window is an outer product, so
    rows then columns"""
    g = gaussian_1d()
    t = sliding_window_view(x, 11, axis=0) @ g                  # (h-10, w)
    return sliding_window_view(t, 11, axis=1) @ g               # (h-10, w-10)


def gray(img):
    """(3,h,w) uint8 -> (h,w) int64: (4899 R + 9617 G + 1868 B + 8192) >> 14"""
    r, g, b = (img[i].astype(np.int64) for i in range(3))
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14


def gt_mean_image(restored, gt):
    """fp64 (3,h,w): clip(restored * mean(gray(gt)) / mean(gray(restored)), 0, 255), the means formed as numpy does"""
    n = restored.shape[1] * restored.shape[2]
    s = (int(gray(gt).sum()) / n) / (int(gray(restored).sum()) / n)
    return np.clip(restored.astype(np.float64) * s, 0, 255)


def ssim_plane(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    mu1, mu2 = filter_valid(a), filter_valid(b)
    s1 = filter_valid(a * a) - mu1 * mu1
    s2 = filter_valid(b * b) - mu2 * mu2
    s12 = filter_valid(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float(m.mean())


def ssim(restored, gt, gt_mean=False):
    a = gt_mean_image(restored, gt) if gt_mean else restored.astype(np.float64)
    return float(np.mean([ssim_plane(a[i], gt[i]) for i in range(3)]))


def psnr(restored, gt, gt_mean=False):
    """the GT-mean image enters as its fp32 cast; squared errors summed in fp64"""
    a = gt_mean_image(restored, gt).astype(np.float32) if gt_mean else restored
    d = a.astype(np.float64) - gt.astype(np.float64)
    return float(10.0 * np.log10(255.0 * 255.0 / (np.mean(d * d) + 1e-8)))


def quantize(rgb, h, w):
    """fp32 (3,H,W) numpy -> uint8 (3,h,w): clamp to [0, 1], x 255 in fp32, truncate, crop"""
    x = np.clip(rgb.astype(np.float32), 0, 1) * np.float32(255)
    return x.astype(np.uint8)[:, :h, :w]
