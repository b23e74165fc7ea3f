"""Restatement of the reference's training transform for one sample, through the library calls torchvision itself makes on
PIL images: RandomCrop -> Image.crop, RandomHorizontalFlip -> transpose(FLIP_LEFT_RIGHT), RandomVerticalFlip ->
transpose(FLIP_TOP_BOTTOM), ToTensor -> np.array, HWC -> CHW, .to(float32).div(255); then train.py:54-56, `im1 ** gamma`, for
the low image.  Written from those semantics (data/data.py:6-12); torchvision is not installed, so the restatement is
unpinned, but it adds no arithmetic of its own beyond the division.

Images are uint8 (h,w,3) numpy arrays."""
import numpy as np
import torch
from PIL import Image


def to_tensor(pil) -> torch.Tensor:
    a = np.array(pil)
    return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def transform(img_hwc: np.ndarray, y0, x0, hflip, vflip, size) -> torch.Tensor:
    """fp32 (3,S_h,S_w) on the CPU"""
    sh, sw = (size, size) if isinstance(size, int) else size
    im = Image.fromarray(img_hwc, "RGB").crop((x0, y0, x0 + sw, y0 + sh))
    if hflip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if vflip:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    return to_tensor(im)


def batch(lows, highs, gt_index, index, y0, x0, hflip, vflip, size, gamma=None):
    """(x, gt), fp32 (B,3,S_h,S_w) on the CPU; gamma None: no power"""
    xs, gs = [], []
    for k, i in enumerate(index):
        j = gt_index[i] if gt_index is not None else i
        xs.append(transform(lows[i], int(y0[k]), int(x0[k]), bool(hflip[k]), bool(vflip[k]), size))
        gs.append(transform(highs[j], int(y0[k]), int(x0[k]), bool(hflip[k]), bool(vflip[k]), size))
    x, gt = torch.stack(xs), torch.stack(gs)
    if gamma is not None:
        x = x ** gamma
    return x, gt


def random_images(seed, sizes):
    """uint8 (h,w,3) arrays from a seed"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in fp32 units in the last place between non-negative fp32 arrays"""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


def gamma_yardstick(gamma) -> np.ndarray:
    """(256,) fp32(pow(fp64(fp32(q) / 255), gamma)), libm's pow per level"""
    import math
    q = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.array([math.pow(float(v), float(gamma)) for v in q], dtype=np.float64).astype(np.float32)
