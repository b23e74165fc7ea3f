"""Image-quality evaluation on the device: the reference's eval.py (model -> clamped 8-bit output) and measure.py (PSNR,
SSIM, optionally after the "GT mean" rescale).  The scores are formed on the device from the quantized output; save_dir=
also writes the files eval.py writes (image_io's egress kernel and writer), which a PNG reader decodes to the scored values.

    from hvi_cidnet_amd import metrics as M
    q = M.to_uint8(rgb, size=(h, w))        # fp32 (B,3,Hp,Wp) -> uint8 (B,3,h,w): clamp, x255, truncate, crop
    r = M.resize_u8(q, (h2, w2))            # uint8 (B,3,h,w) -> uint8 (B,3,h2,w2): PIL's Image.resize, byte for byte
    p = M.psnr(q, gt_u8, gt_mean=False)     # (B,) float64 on the device, no host synchronisation
    k = M.gt_mean_scale(q, gt_u8)           # (B,) float64 on the device: the GT-mean scale every gt_mean=True uses
    s = M.ssim(q, gt_u8, gt_mean=False)     # (B,) float64 on the device
    res = M.evaluate(model, pairs, gamma=1.0, gated=False, alpha_s=1.3, gated2=False, alpha=1.0, batch_size=1, save_dir=None,
                     resize=False, lpips=None, ciede2000=False)
    prm = M.load_lpips_params(alexnet_path, heads_path)       # torchvision's AlexNet state dict + lpips' alex.pth (not shipped)
    d = M.lpips(q, gt_u8, prm, gt_mean=False)                 # (B,) float64 on the device: lpips.LPIPS(net='alex')
    f = M.lpips_features(q, prm)                              # the five fp32 taps; M.lpips_layers: the five layer terms (B,5)
    e = M.ciede2000(q, gt_u8, gt_mean=False)                  # (B,) float64 on the device: mean CIEDE2000 colour difference
    m = M.ciede2000_map(q, gt_u8)                             # (B,h,w) float64; M.ciede2000_lab(lab1, lab2): dE00 of Lab pairs
    pairs = M.folder_pairs(low_dir, high_dir)
    pairs = M.nested_folder_pairs(low_root, high_root, gt="name")      # LOL-Blur / SID: one sub-folder per scene
    per_folder, overall = M.group_means(res, pairs)

and, for the sets without ground truth (eval.py --unpaired + measure_niqe_bris.py), NIQE:

    prm = M.load_niqe_params(path)          # the reference's loss/niqe_pris_params.npz (not shipped: pass its path)
    f = M.niqe_features(q, prm)             # uint8 (B,3,h,w) -> (B, blocks, 36) float64 on the device
    s = M.niqe(q, prm)                      # (B,) float64 (the 36 x 36 tail runs on the host: one copy per batch)
    res = M.evaluate_unpaired(model, images, prm, alpha=1.0, gamma=1.0, batch_size=1, save_dir=None)
    images = M.folder_images(dir)

and LOE, the lightness order error of the enhanced image against the low input (the reference has none: opt-in):

    step, rows, cols = M.loe_grid(h, w, sample=50)
    num, m = M.loe_counts(low_u8, q, sample=50)     # exact int64 pair counts (B,) on the device, and the sample count
    v = M.loe(low_u8, q, sample=50)                 # (B,) float64 on the device: num / m (normalized=True: num / m^2)
    res = M.evaluate_unpaired(model, images, prm, loe=True)     # res.loe, res.per_image["loe"]

and the file round trip of the .jpg sets (eval.py saves such an output as a JPEG and the reference scores the decoded file):

    plan = M.jpeg_quant_plan(75)                    # host: the tables Pillow writes, the divisors, the exact-division constants
    r = M.jpeg_roundtrip_u8(q, quality=75)          # uint8 (B,3,h,w) -> what PIL's save(.., 'JPEG') + open() returns, byte for byte
    res = M.evaluate_unpaired(model, images, prm, file_roundtrip=True)      # .jpg / .jpeg names scored as their decoded files

and BRISQUE, the second number of measure_niqe_bris.py (imquality.brisque.score), all fp64 on the device:

    bp = M.load_brisque_params(model_path, range_path)    # libsvm text model + normalize.pickle / .npz (not shipped)
    f = M.brisque_features(q)                       # uint8 (B,3,h,w), h, w >= 16 -> (B,36) fp64 on the device
    s = M.brisque(q, bp)                            # (B,) fp64 on the device, no host synchronisation; M.brisque_score(f, bp)
    y = M.brisque_gray(q); y2 = M.brisque_half(y); m, mom = M.brisque_mscn(y); f18 = M.brisque_fit(mom)      # the stages
    res = M.evaluate_unpaired(model, images, prm, brisque=bp)       # res.brisque, res.per_image["brisque"]

The kernels are csrc/metrics.hip, csrc/lpips.hip, csrc/ciede2000.hip, csrc/resize.hip, csrc/niqe.hip, csrc/brisque.hip, csrc/loe.hip and csrc/jpeg.hip (C ABI: cidnet_metric_*); their semantics are documented in include/cidnet_hip.h.
Differences from the reference scripts, none of which changes a per-image value:
  * measure.py counts a low image without a ground truth in the divisor of its averages (it skips the image after
    `n += 1`); here such an image is skipped and reported (FolderPairs.skipped, EvalResult.skipped) and not counted;
  * eval.py leaves `trans.alpha` (and with it the model's state) as the last run set it; evaluate() restores every
    attribute it touches and the train / eval mode of every submodule;
  * a ground truth whose size differs from the output raises unless evaluate(resize=True) is asked for; then the quantized
    output is resized as measure.py:133-134 resizes it (resize_u8: Pillow >= 7's default filter, byte for byte);
  * PSNR sums its squared errors exactly (fp64) where measure.py averages in fp32: < 1e-4 dB apart;
  * LPIPS (lpips(), evaluate(lpips=)) needs torchvision's AlexNet weights and the lpips package's heads,
    which are not shipped: pass their paths (load_lpips_params); its layer distances are summed in fp64 from the fp32
    features where the lpips package stays in fp32;
  * CIEDE2000 (ciede2000(), evaluate(ciede2000=True)) has no counterpart in the reference: opt-in, the mean
    dE00 between the output and the ground truth with scikit-image's sRGB -> Lab constants, in fp64;
  * NIQE: the half-size image sums its 8 taps in fp64 and rounds once per pass where the reference sums them in fp32 (two
    fp32 ulps apart at most), and the block moments are summed in fp64 where the reference's are fp32 means; an image with
    fewer than two NaN-free blocks scores NaN (the reference raises from inside the SVD); BRISQUE, the script's second
    number, is opt-in (brisque(), evaluate_unpaired(brisque=)): its model and range files are the user's own,
    passed by path, and its stages are pinned to scipy / scikit-learn, not to the imquality package itself; and by
    default the score is that of the quantized output itself, while for a .jpg input eval.py's output file is a JPEG and the
    reference scores what that file decodes to: evaluate_unpaired(file_roundtrip=True) scores exactly that.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import warnings
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from ._lib import lib
from .inference import pad_to_multiple

_NO_CPU = ("hvi-cidnet_amd ops run only on a ROCm device (got a CPU tensor); there is no CPU fallback -- use the oracle "
           "under oracle/ for CPU checks")
# measure.py:98-125: the ground truth of `name` is `name` itself in the GT directory, else the same stem with these extensions
GT_EXTENSIONS = (".jpg", ".JPG", ".jpeg", ".JPEG", ".png", ".PNG")
_IMAGE_EXTENSIONS = {".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp"}


def _on_device(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _batched(t, what):
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] != 3:
        raise RuntimeError(f"{what}: expected (B,3,H,W) or (3,H,W), got {tuple(t.shape)}")
    return t.contiguous()


def to_uint8(rgb: torch.Tensor, size=None) -> torch.Tensor:
    """fp32 (B,3,Hp,Wp) (or (3,Hp,Wp)) on the device -> uint8 (B,3,h,w): the top-left (h, w) = `size` crop (default the whole
    image) of trunc(clamp(x, 0, 1) * 255.0f), bit-equal to torch.clamp(x, 0, 1).mul(255).byte() (eval.py:69-73 and
    ToPILImage).  NaN becomes 0."""
    _on_device(rgb)
    if rgb.dtype != torch.float32:
        raise RuntimeError(f"to_uint8: expected fp32 (got {rgb.dtype})")
    squeeze = rgb.dim() == 3
    x = _batched(rgb, "to_uint8")
    B, _, Hp, Wp = x.shape
    h, w = (Hp, Wp) if size is None else (int(size[0]), int(size[1]))
    if not (0 < h <= Hp and 0 < w <= Wp):
        raise RuntimeError(f"to_uint8: crop {(h, w)} outside the {(Hp, Wp)} image")
    q = torch.empty((B, 3, h, w), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_to_uint8", ops._p(x), ops._p(q), B, Hp, Wp, h, w, ops._stream())
    return q[0] if squeeze else q


# ---- PIL's 8-bit bicubic resize (measure.py:133-134) ----------------------------------------------------------------------
_RESIZE_BITS = 22                                                  # Pillow's PRECISION_BITS for 8-bit images
_resize_plans = {}                                                 # (n_in, n_out) -> (bounds, coeffs)
_resize_plans_dev = {}                                             # (device index, n_in, n_out) -> (bounds, coeffs, ksize) there


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_plan(n_in: int, n_out: int):
    """Pillow's coefficient tables for one axis of an 8-bit bicubic resize over the whole axis (Resample.c: precompute_coeffs
    + normalize_coeffs_8bpc, restated; every operation in IEEE double, in Pillow's order) -> (bounds int32 (n_out, 2): first
    tap, tap count; coeffs int32 (n_out, ksize): the normalised weights scaled by 2^22 and rounded half away from zero, rows
    padded with zeros).  Cached per (n_in, n_out); the arrays are read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"resize_plan: sizes must be positive (got {n_in} -> {n_out})")
    key = (n_in, n_out)
    if key in _resize_plans:
        return _resize_plans[key]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coeffs = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                 # int(): C's truncation
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * (1 << _RESIZE_BITS) + (-0.5 if v < 0 else 0.5))
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    _resize_plans[key] = (bounds, coeffs)
    return bounds, coeffs


def _resize_plan_on(device, n_in, n_out):
    """uploaded once per process, device and (n_in, n_out)"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), n_in, n_out)
    if key not in _resize_plans_dev:
        bounds, coeffs = resize_plan(n_in, n_out)
        _resize_plans_dev[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coeffs.copy()).to(device),
                                  coeffs.shape[1])
    return _resize_plans_dev[key]


def resize_u8(q: torch.Tensor, size) -> torch.Tensor:
    """uint8 (B,3,H,W) (or (3,H,W)) on the device -> uint8 (B,3,h,w), (h, w) = `size`: what PIL.Image.resize((w, h)) of
    Pillow >= 7 returns for each 8-bit RGB image, byte for byte -- the default filter (antialiased bicubic, a = -0.5) over the
    whole image with reducing_gap=None, in Pillow's fixed-point arithmetic: the horizontal pass first, rounded to uint8, then
    the vertical one; an axis that keeps its size is not touched (measure.py:133-134).  `size` equal to the input's returns
    the input itself.  (Pillow < 7 defaulted to nearest-neighbour: not reproduced, nor any other filter.)"""
    _on_device(q)
    if q.dtype != torch.uint8:
        raise RuntimeError(f"resize_u8 takes uint8 images (got {q.dtype}); see to_uint8")
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"resize_u8: size {(h, w)} must be positive")
    if q.dim() in (3, 4) and tuple(q.shape[-2:]) == (h, w) and q.shape[-3] == 3:
        return q
    squeeze = q.dim() == 3
    x = _batched(q, "resize_u8")
    B, _, H, W = x.shape
    L = lib()
    out = torch.empty((B, 3, h, w), dtype=torch.uint8, device=x.device)
    n_tmp = L.raw("cidnet_metric_resize_ws_bytes")(B, H, W, h, w)
    tmp = torch.empty(n_tmp, dtype=torch.uint8, device=x.device) if n_tmp else None
    bx, cx, kx = _resize_plan_on(x.device, W, w) if W != w else (None, None, 0)
    by, cy, ky = _resize_plan_on(x.device, H, h) if H != h else (None, None, 0)
    with torch.cuda.device(x.device):
        L.call("cidnet_metric_resize_u8", ops._p(x), ops._p(out), ops._p(tmp), ops._p(bx), ops._p(cx), kx, ops._p(by), ops._p(cy),
               ky, B, H, W, h, w, ops._stream())
    return out[0] if squeeze else out


def _u8_pair(who, restored, gt):
    """the input checks of the paired metrics -> the two images as contiguous (B,3,h,w)"""
    _on_device(restored, gt)
    if restored.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise RuntimeError(f"{who} take uint8 images (got {restored.dtype}, {gt.dtype}); see to_uint8")
    a, g = _batched(restored, "restored"), _batched(gt, "gt")
    if a.shape != g.shape or a.device != g.device:
        raise RuntimeError(f"{who}: restored {tuple(a.shape)} and gt {tuple(g.shape)} differ")
    return a, g


def _checked_scale(who, scale, B, device):
    """a caller's GT-mean scale -> (B,) float64, contiguous, on `device`"""
    if scale.dtype != torch.float64 or tuple(scale.shape) != (B,):
        raise RuntimeError(f"{who}: scale must be ({B},) float64 (got {tuple(scale.shape)} {scale.dtype})")
    _on_device(scale)
    if scale.device != device:
        raise RuntimeError(f"{who}: scale is on {scale.device}, the images on {device}")
    return scale.contiguous()


def _gt_mean_scale(a, g):
    """gt_mean_scale() of a checked (B,3,h,w) pair.  The caller has made the device current."""
    B, _, h, w = a.shape
    n = lib().raw("cidnet_metric_gt_mean_scale_ws_floats")(B, h, w)
    ws = torch.empty(n, dtype=torch.float32, device=a.device)
    s = torch.empty(B, dtype=torch.float64, device=a.device)
    lib().call("cidnet_metric_gt_mean_scale", ops._p(a), ops._p(g), ops._p(s), ops._p(ws), n, B, h, w, ops._stream())
    return s


def gt_mean_scale(restored_u8: torch.Tensor, gt_u8: torch.Tensor) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) pairs on the device -> (B,) float64 on the device, no host synchronisation: the "GT mean"
    scale s = mean(gray(gt)) / mean(gray(restored)) of measure.py:138-141, gray the BT.601 fixed-point rule, summed exactly.
    Every paired metric's gt_mean=True rescales `restored` to clip(restored * s, 0, 255) with this number; psnr_ssim(scale=)
    and lpips_features(scale=) take it as it is.  An image whose gray mean is 0 gives inf or NaN.  Any h, w >= 1."""
    a, g = _u8_pair("gt_mean_scale", restored_u8, gt_u8)
    with torch.cuda.device(a.device):
        return _gt_mean_scale(a, g)


def psnr_ssim(restored: torch.Tensor, gt: torch.Tensor, gt_mean: bool = False, want_psnr: bool = True,
              want_ssim: bool = True, scale=None):
    """uint8 (B,3,h,w) pairs on the device -> (psnr, ssim), each (B,) float64 on the device (None where not wanted), from one
    pass over the images.  gt_mean: rescale `restored` by gt_mean_scale(restored, gt) first (measure.py:138-141), on the
    device.  scale: a (B,) float64 tensor on the images' device is used as that scale as it is, and implies gt_mean.  SSIM
    needs h, w >= 11."""
    a, g = _u8_pair("psnr / ssim", restored, gt)
    B, _, h, w = a.shape
    if want_ssim and (h < 11 or w < 11):
        raise RuntimeError(f"ssim needs images of at least 11 x 11 pixels (got {h} x {w}): the 11 x 11 window's valid region "
                           "would be empty")
    if scale is not None:
        scale = _checked_scale("psnr_ssim", scale, B, a.device)
    n = lib().raw("cidnet_metric_ws_floats")(B, h, w)
    ws = torch.empty(n, dtype=torch.float32, device=a.device)
    p = torch.empty(B, dtype=torch.float64, device=a.device) if want_psnr else None
    s = torch.empty(B, dtype=torch.float64, device=a.device) if want_ssim else None
    with torch.cuda.device(a.device):
        if scale is None and gt_mean:
            scale = _gt_mean_scale(a, g)
        lib().call("cidnet_metric_psnr_ssim", ops._p(a), ops._p(g), ops._p(scale), ops._p(p), ops._p(s), ops._p(ws), n,
                   B, h, w, ops._stream())
    return p, s


def psnr(restored: torch.Tensor, gt: torch.Tensor, gt_mean: bool = False) -> torch.Tensor:
    """(B,) float64: 10 log10(255^2 / (mean((restored - gt)^2) + 1e-8)) per image (measure.py:66-71)"""
    return psnr_ssim(restored, gt, gt_mean, want_ssim=False)[0]


def ssim(restored: torch.Tensor, gt: torch.Tensor, gt_mean: bool = False) -> torch.Tensor:
    """(B,) float64: mean over the three colour planes of the mean SSIM map (measure.py:23-64)"""
    return psnr_ssim(restored, gt, gt_mean, want_psnr=False)[1]


# ---- ground truth / input conversion (host side: what PIL, numpy or ToTensor() hand over) ---------------------------------
def _to_array(img):
    if isinstance(img, (torch.Tensor, np.ndarray)):
        return img
    if hasattr(img, "convert"):                                  # a PIL image
        return np.array(img.convert("RGB"))
    return np.asarray(img)


def _gt_u8(gt, device) -> torch.Tensor:
    """-> uint8 (3,h,w) on `device`.  uint8 input: HWC (PIL / numpy) or CHW; float input: a ToTensor() image (CHW in [0, 1]),
    converted with round(x * 255), which is exact for such tensors."""
    gt = _to_array(gt)
    t = torch.from_numpy(np.ascontiguousarray(gt)) if isinstance(gt, np.ndarray) else gt
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3:
        raise ValueError(f"ground truth: expected a 3-dimensional image, got {tuple(t.shape)}")
    if t.dtype == torch.uint8:
        hwc = t.shape[-1] == 3 and (t.shape[0] != 3 or isinstance(gt, np.ndarray))
        t = t.permute(2, 0, 1) if hwc else t
        if t.shape[0] != 3:
            raise ValueError(f"ground truth: expected 3 colour channels, got {tuple(t.shape)}")
        return t.to(device).contiguous()
    if not t.is_floating_point() or t.shape[0] != 3:
        raise ValueError(f"ground truth: expected uint8 HWC / CHW or a float CHW ToTensor() image, got {t.dtype} "
                         f"{tuple(t.shape)}")
    return torch.round(t.to(device, torch.float32) * 255).clamp_(0, 255).to(torch.uint8).contiguous()


def _image_f32(img, device) -> torch.Tensor:
    """-> fp32 (3,h,w) on `device`: a float CHW image (or (1,3,h,w)) as it is; a uint8 image (HWC array / PIL image, or a CHW
    tensor) as ToTensor() converts it, x / 255 by a true division (dividing by a host scalar on the device would multiply by
    fl(1/255): one ulp off for some levels, which the gamma power carries into the output)"""
    a = _to_array(img)
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if t.dtype == torch.uint8 and t.dim() == 3 and t.shape[-1] == 3 and (t.shape[0] != 3 or isinstance(a, np.ndarray)):
        t = t.permute(2, 0, 1)
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f"input image: expected (3,h,w) or (h,w,3), got {tuple(t.shape)}")
    if t.dtype == torch.uint8:
        return t.to(device).float() / torch.full((), 255.0, dtype=torch.float32, device=device)
    return t.to(device, torch.float32)


# ---- evaluate ---------------------------------------------------------------------------------------------------------
@dataclass
class EvalResult:
    """Means over the evaluated images (in input order, divided by their number) and the per-image values"""
    alpha: float
    psnr: float
    ssim: float
    psnr_gt_mean: float
    ssim_gt_mean: float
    per_image: dict = field(default_factory=dict)     # "psnr" / "ssim" / "psnr_gt_mean" / "ssim_gt_mean" -> list, input order
    names: list = field(default_factory=list)
    skipped: list = field(default_factory=list)       # low images without a ground truth (folder_pairs)
    resized: list = field(default_factory=list)       # indices of the pairs whose output was resized to the ground truth's size
    ensemble: int = 1                                 # the number of views each output was averaged over (evaluate(ensemble=))
    lpips: float = float("nan")                       # evaluate(lpips=): the means of per_image["lpips"] / ["lpips_gt_mean"]
    lpips_gt_mean: float = float("nan")
    ciede2000: float = float("nan")                   # evaluate(ciede2000=True): the means of per_image["ciede2000"] / [.._gt_mean]
    ciede2000_gt_mean: float = float("nan")


_KEYS = ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")
_LPIPS_KEYS = ("lpips", "lpips_gt_mean")


def _model_device(model):
    for p in model.parameters():
        return p.device
    raise RuntimeError("evaluate: the model has no parameters")


@contextlib.contextmanager
def _eval_state(model, trans_attrs):
    """The model as an evaluation runs it -- eval mode, the given model.trans attributes set -- and afterwards as it was found:
    trans.gated / alpha_s / gated2 / alpha, the snapshot behind trans.this_k and the train / eval mode of every submodule.
    Shared by _evaluate() and image_io (enhance_u8, enhance_folder).  Yields model.trans."""
    trans = model.trans
    saved_attrs = {k: getattr(trans, k) for k in ("gated", "alpha_s", "gated2", "alpha")}
    saved_k = {k: trans.__dict__[k] for k in ("_this_k_host", "_this_k_dev") if k in trans.__dict__}
    saved_modes = [(m, m.training) for m in model.modules()]
    try:
        model.eval()
        for k, v in trans_attrs.items():
            setattr(trans, k, v)
        yield trans
    finally:
        for k, v in saved_attrs.items():
            setattr(trans, k, v)
        trans.__dict__.update(saved_k)
        for m, mode in saved_modes:
            m.training = mode


def _plan(sizes, rank, world, batch_size):
    """The index arithmetic of an evaluation, free of tensors.  `sizes`: (padded shape, crop size) of this rank's images --
    images rank, rank + world, ... of the input, in that order --, consumed one at a time.  Yields (lo, hi, runs) per batch:
    the batch is this rank's images lo .. hi - 1, consecutive ones of equal padded shape and at most batch_size of them (it
    is yielded once the image after it has been seen); runs lists (j, k, rows): the batch's samples j .. k - 1 share a crop
    size, and `rows` selects their positions in the input -- this rank's images are every world-th one, so consecutive
    samples are a strided slice."""
    lo, shape, crops = 0, None, []

    def batch():
        runs, j = [], 0
        while j < len(crops):
            k = j + 1
            while k < len(crops) and crops[k] == crops[j]:
                k += 1
            i0 = rank + (lo + j) * world
            runs.append((j, k, slice(i0, i0 + (k - j - 1) * world + 1, world)))
            j = k
        return lo, lo + len(crops), runs
    for padded, crop in sizes:
        if crops and (len(crops) == batch_size or padded != shape):
            yield batch()
            lo, crops = lo + len(crops), []
        shape = padded
        crops.append(crop)
    if crops:
        yield batch()


@torch.no_grad()
def _evaluate(who, noun, model, items, load, trans_attrs, score, keys, result, alpha, gamma, batch_size, process_group,
              save_dir=None, run_key=None, ensemble=1, png="pillow", jpeg="pillow"):
    """The evaluation loop of evaluate() and evaluate_unpaired(), `who` / `noun` naming them in errors.  load(i, item, device)
    -> (input fp32 (3,h,w), what score needs of the image); trans_attrs: the model.trans attributes set for the run; score(q
    uint8 (B,3,h,w), [load's second values]) -> one (B,) fp64 device tensor per key; result(alpha=, per_image=, names=,
    <key>=mean ...) builds the result for one alpha.  save_dir: every scored image is also written there (image_io's egress
    kernel and writer), under items.names[i] or "<i as 5 digits>.png" (a name may hold sub-folders: they are created).
    run_key(load's second value): what, beside the crop size, the samples of one score() call must share.
    ensemble: 1, or 2 / 4 / 8 -- the model runs on the views of the padded input, once per view group, and the merged fp32
    result (image_io.ensemble_views / ensemble_merge) stands where the model's output stood.
    png: "pillow", or "device" -- save_dir's .png files carry a stream encoded on the device (image_io._Writer).
    jpeg: "pillow", or "device" -- save_dir's .jpg / .jpeg files are encoded on the device, byte-equal to Pillow's."""
    from . import image_io                                       # image_io imports this module
    na, nb = image_io._check_ensemble(ensemble)
    png = image_io._check_png(png)
    jpeg = image_io._check_jpeg(jpeg)
    device = _model_device(model)
    if not device.type == "cuda":
        raise RuntimeError(_NO_CPU)
    sweep = isinstance(alpha, (list, tuple))
    alphas = [float(a) for a in alpha] if sweep else [float(alpha)]
    if not alphas:
        raise ValueError(f"{who}: empty alpha sweep")
    if sweep and save_dir is not None:
        raise ValueError(f"{who}: save_dir with an alpha sweep -- the files of which alpha? Evaluate one alpha per directory")
    n = len(items)
    if n == 0:
        raise ValueError(f"{who}: no {noun}")
    world, rank = 1, 0
    if process_group is not None or (dist.is_available() and dist.is_initialized()):
        world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
    use_trunk = sweep and hasattr(model, "trunk")
    # rows: images in input order; columns: keys.  This rank fills the rows of its images, zeros elsewhere.
    res = torch.zeros((len(alphas), n, len(keys)), dtype=torch.float64, device=device)
    loaded = []                # this rank's images not yet scored: (padded input, (h, w), load's second); _plan looks one ahead
    writer = None
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        file_names = getattr(items, "names", None)
        with torch.cuda.device(device):
            writer = image_io._Writer(device, threads=8, depth=2, png=png, jpeg=jpeg)

    def sizes():
        for i in range(rank, n, world):
            x, aux = load(i, items[i], device)
            xp, hw = pad_to_multiple(x.unsqueeze(0), 8)
            loaded.append((xp, hw, aux))
            yield xp.shape, (hw if run_key is None else (hw, run_key(aux)))
    try:
        with _eval_state(model, trans_attrs) as trans, torch.cuda.device(device):
            for lo, hi, runs in _plan(sizes(), rank, world, max(1, int(batch_size))):
                batch = loaded[:hi - lo]
                del loaded[:hi - lo]
                x = torch.cat([b[0] for b in batch]) if len(batch) > 1 else batch[0][0]
                xg = x ** gamma
                if ensemble != 1:                                # one input per view group: views 0 .. na - 1, views 4 .. 4 + nb - 1
                    groups = [image_io.ensemble_views(xg, 0, na)] + ([image_io.ensemble_views(xg, 4, nb)] if nb else [])
                    trunks = [model.trunk(g) for g in groups] if use_trunk else None
                trunk = model.trunk(xg) if use_trunk and ensemble == 1 else None
                for ai, a in enumerate(alphas):
                    trans.alpha = a
                    if ensemble != 1:                            # the trunk once per group, PHVIT per alpha and group, one merge
                        outs = [trans.PHVIT_residual(*t) for t in trunks] if use_trunk else [image_io._first(model(g)) for g in groups]
                        out = image_io.ensemble_merge(outs[0], outs[1] if nb else None, na)
                    elif trunk is not None:
                        out = trans.PHVIT_residual(*trunk)
                    else:
                        out = model(xg)
                        if isinstance(out, tuple):               # CIDNet_TNSM: (rgb, noise map or None)
                            out = out[0]
                    for j, k, rows in runs:                      # runs of equal crop size share one launch
                        q = to_uint8(out[j:k], batch[j][1])
                        into = res[ai, rows]
                        for col, v in enumerate(score(q, [b[2] for b in batch[j:k]])):
                            into[:, col].copy_(v)
                        if writer is not None:
                            ids = range(rows.start, rows.stop, rows.step)
                            paths = [os.path.join(save_dir, str(file_names[i]) if file_names is not None else f"{i:05d}.png")
                                     for i in ids]
                            for d in {os.path.dirname(p) for p in paths}:
                                os.makedirs(d, exist_ok=True)
                            writer.put(image_io.egress(out[j:k], batch[j][1]), paths)
            if writer is not None:
                writer.close()
                writer = None
            if world > 1:
                dist.all_reduce(res, op=dist.ReduceOp.SUM, group=process_group)
            host = res.cpu().numpy()
    finally:
        if writer is not None:
            writer.abort()
    names = list(getattr(items, "names", range(n)))
    out = []
    for ai, a in enumerate(alphas):
        per = {k: [float(v) for v in host[ai, :, j]] for j, k in enumerate(keys)}
        means = {}
        for k, vals in per.items():                               # running sum in input order, / n (measure.py:146-150)
            acc = 0.0
            for v in vals:
                acc += v
            means[k] = acc / n
        out.append(result(alpha=a, per_image=per, names=names, **means))
    return out if sweep else out[0]


def evaluate(model, pairs, gamma: float = 1.0, gated: bool = False, alpha_s: float = 1.3, gated2: bool = False,
             alpha=1.0, batch_size: int = 1, process_group=None, save_dir=None, resize: bool = False, ensemble: int = 1,
             png: str = "pillow", jpeg: str = "pillow", lpips=None, ciede2000: bool = False):
    """eval.py + measure.py on the device.  `pairs`: a sequence of (low, gt) -- low a (3,h,w) float image in [0, 1] (or a
    uint8 HWC image, converted as ToTensor() does), gt uint8 HWC / CHW or a float ToTensor() image of the same size
    (folder_pairs() yields these).  Each input is reflect-padded to a multiple of 8, run through model(pow(x, gamma)) in eval
    mode under no_grad with trans.gated / alpha_s / gated2 / alpha set (a tuple result -- CIDNet_TNSM -- gives its [0]),
    clamped, cropped and quantized to uint8, and measured against its ground truth without and with the GT-mean rescale.

    alpha: a number, or a sequence of numbers (an alpha sweep): the result is then a list with one EvalResult per value, and
    the model's trunk runs once per batch -- only PHVIT, the quantization and the metrics run per value.
    batch_size > 1 batches consecutive images of equal padded size.
    Data-parallel: with torch.distributed initialised (or `process_group` given), rank r evaluates images i % world == r and
    the per-image values are gathered back into image order with one SUM all-reduce, so every rank returns the same result
    (with batch_size=1 bit-identical to a single process).
    save_dir: each scored image is also written to save_dir/<name> (pairs.names[i] where the pairs have names, else
    "<i as 5 digits>.png") by PIL in the format the name's extension gives -- the files eval.py writes and measure.py reads;
    each rank writes its own images.  ValueError together with an alpha sweep.  None: nothing is written.
    png: "pillow" -- every file is encoded by PIL.  "device" -- a name ending in .png gets a file whose IDAT stream was encoded
    on the device (image_io.png_zlib_u8: filters and Huffman coding, no LZ77): the same pixels in another, valid file; other
    extensions keep PIL.  The scores are untouched.  Any other value is a ValueError before anything runs.
    jpeg: "pillow" -- as above.  "device" -- a name ending in .jpg or .jpeg (any case) gets the file Pillow would write at
    quality 75, byte for byte, encoded on the device (image_io.jpeg_scan_u8).  The scores are untouched.
    resize: False -- a ground truth whose size differs from its input's is a ValueError.  True -- such a pair is scored as
    measure.py:133-134 scores it: the quantized output is resized to the ground truth's size (resize_u8: Pillow >= 7's default
    bicubic, byte for byte; per alpha of a sweep) and GT mean, PSNR and SSIM are taken from the resized image; the pairs'
    indices are reported in EvalResult.resized.  save_dir still receives the un-resized output, as eval.py writes it.  A
    ground truth smaller than 11 x 11 raises as ssim() does.
    ensemble: 2, 4 or 8 -- geometric self-ensemble as image_io.enhance_u8(ensemble=) runs it: the model on the views of the
    padded input, once per view group (with a sweep: the trunk once per group, PHVIT once per value and group), and the merged
    fp32 result is what is quantized, saved and resized.  1: no view is built.  Any other value is a ValueError.
    lpips: None -- PSNR and SSIM only, nothing else runs.  An LpipsParams, or (alexnet path, heads path) -- every pair is also
    scored with lpips() without and with the GT-mean rescale, from the image PSNR and SSIM are taken from (the resized one
    under resize=True, the merged one under ensemble=, per value of a sweep): EvalResult.lpips / .lpips_gt_mean and
    per_image["lpips"] / ["lpips_gt_mean"], gathered like the other keys.  A batch's ground truths go through the extractor
    once, for both variants and every alpha; an image under 31 x 31 raises as lpips() does.
    ciede2000: False -- nothing of it runs and the result is what it was without the keyword.  True -- every pair is also scored
    with ciede2000() (the mean CIEDE2000 colour difference; the reference has none) without and with the GT-mean
    rescale, from the image PSNR and SSIM are taken from: EvalResult.ciede2000 / .ciede2000_gt_mean and per_image["ciede2000"] /
    ["ciede2000_gt_mean"], after the LPIPS keys, gathered like the other keys.
    The model's attributes and the train / eval mode of every submodule are restored afterwards."""
    lp = None if lpips is None else _lpips_params(lpips)
    gt_taps = [None, None]                          # the last batch's ground truths and their taps: shared by a sweep's values

    def lpips_cols(q, g, s, gts):
        if gt_taps[0] is None or len(gt_taps[0]) != len(gts) or any(a is not b for a, b in zip(gt_taps[0], gts)):
            gt_taps[:] = [list(gts), None]
        plain, gtm, gt_taps[1] = _lpips_both(q, g, lp, s, gt_taps[1])
        return plain, gtm

    def cols(q, g, gts):                            # every column of one scored batch, in key order; the GT-mean scale once
        plain = psnr_ssim(q, g)
        s = gt_mean_scale(q, g)
        return (*plain, *psnr_ssim(q, g, scale=s), *(lpips_cols(q, g, s, gts) if lp else ()),
                *(_ciede_both(q, g, s) if ciede2000 else ()))

    def load(i, pair, device):
        x, g = _image_f32(pair[0], device), _gt_u8(pair[1], device)
        if tuple(g.shape) != tuple(x.shape) and not resize:
            raise ValueError(f"evaluate: image {i}: ground truth {tuple(g.shape[1:])} and input {tuple(x.shape[1:])} "
                             "differ in size (resize=True scores the output resized to the ground truth's size, as "
                             "measure.py does)")
        return x, g

    def score(q, gts):
        g = torch.stack(gts) if len(gts) > 1 else gts[0].unsqueeze(0)
        if not resize:
            return cols(q, g, gts)
        # the samples of a run share the ground truth's size (run_key); the flag column travels with the values, so that
        # every rank of a sharded evaluation reports the same indices
        flag = torch.full((q.shape[0],), float(q.shape[-2:] != g.shape[-2:]), dtype=torch.float64, device=q.device)
        q = resize_u8(q, g.shape[-2:])
        return (*cols(q, g, gts), flag)
    skipped = list(getattr(pairs, "skipped", []))

    def result(per_image, **kw):
        flags = per_image.pop("resized", [])
        kw.pop("resized", None)
        return EvalResult(skipped=skipped, per_image=per_image, resized=[i for i, f in enumerate(flags) if f],
                          ensemble=int(ensemble), **kw)
    return _evaluate("evaluate", "image pairs", model, pairs, load,
                     dict(gated=bool(gated), alpha_s=float(alpha_s), gated2=bool(gated2)), score,
                     _KEYS + (_LPIPS_KEYS if lp else ()) + (_CIEDE_KEYS if ciede2000 else ()) + (("resized",) if resize else ()),
                     result, alpha, gamma, batch_size,
                     process_group, save_dir,
                     run_key=(lambda g: tuple(g.shape[-2:])) if resize else None, ensemble=ensemble, png=png, jpeg=jpeg)


# ---- folder pairing (the one piece of host / disk code) ------------------------------------------------------------
def _read_rgb(path) -> np.ndarray:
    """uint8 (h,w,3)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


class FolderPairs:
    """Sequence of (low, gt) pairs read from disk on access: low = the low-light image as ToTensor() gives it (fp32 (3,h,w) in
    [0, 1]), gt = the ground truth as uint8 (h,w,3); both through PIL's .convert('RGB').  names: the low images' file names;
    skipped: low images without a ground truth; paths: (low path, gt path) per pair."""

    def __init__(self, paths, names, skipped):
        self.paths, self.names, self.skipped = paths, names, skipped

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        lp, gp = self.paths[i]
        return torch.from_numpy(_read_rgb(lp)).permute(2, 0, 1).float().div(255), _read_rgb(gp)


def folder_pairs(low_dir: str, high_dir: str) -> FolderPairs:
    """Pairs every image file of low_dir (sorted by name) with its ground truth in high_dir, as measure.py:88-131 does: the
    same file name, else the same stem with .jpg / .JPG / .jpeg / .JPEG / .png / .PNG, in that order.  A low image without
    one is skipped and reported (a warning and FolderPairs.skipped); unlike measure.py it does not count in any average."""
    names = sorted(f for f in os.listdir(low_dir)
                   if os.path.isfile(os.path.join(low_dir, f)) and os.path.splitext(f)[1].lower() in _IMAGE_EXTENSIONS)
    paths, kept, skipped = [], [], []
    for name in names:
        stem = os.path.splitext(name)[0]
        for cand in (name, *(stem + e for e in GT_EXTENSIONS)):
            gp = os.path.join(high_dir, cand)
            if os.path.isfile(gp):
                paths.append((os.path.join(low_dir, name), gp))
                kept.append(name)
                break
        else:
            skipped.append(name)
    if skipped:
        warnings.warn(f"folder_pairs: no ground truth in {high_dir} for {len(skipped)} image(s): {', '.join(skipped)}")
    return FolderPairs(paths, kept, skipped)


def _image_files(directory):
    return sorted(f for f in os.listdir(directory)
                  if os.path.isfile(os.path.join(directory, f)) and os.path.splitext(f)[1].lower() in _IMAGE_EXTENSIONS)


def nested_folder_pairs(low_root: str, high_root: str, gt: str = "name") -> FolderPairs:
    """The sets kept as one sub-folder per scene (measure_SID_blur.py): every sub-folder of low_root, in sorted order, and
    in it every image file, sorted by name.  gt="name": the ground truth is the same file name in high_root/<sub>/ (LOL-Blur,
    measure_SID_blur.py:89).  gt="first": every image of a sub-folder is paired with the first image file of
    high_root/<sub>/ (SID, measure_SID_blur.py:85-87) -- the first of sorted(): the reference takes os.listdir's order, which
    is not defined, and SID's label folders hold one file.  names are "<sub>/<file>" (evaluate(save_dir=) creates the
    sub-folders); groups holds one (sub, [indices]) entry per sub-folder that has pairs; an image without a ground truth,
    its whole sub-folder where high_root lacks it, is skipped and reported (a warning and .skipped) and counts in no average.
    measure_SID_blur.py's PSNR omits the + 1e-8 of measure.py's; scoring keeps measure.py's (psnr())."""
    if gt not in ("name", "first"):
        raise ValueError(f"nested_folder_pairs: gt must be 'name' or 'first' (got {gt!r})")
    paths, names, skipped, groups = [], [], [], []
    for sub in sorted(d for d in os.listdir(low_root) if os.path.isdir(os.path.join(low_root, d))):
        low_dir, high_dir = os.path.join(low_root, sub), os.path.join(high_root, sub)
        labels = _image_files(high_dir) if os.path.isdir(high_dir) else []
        members = []
        for f in _image_files(low_dir):
            label = (labels[0] if labels else None) if gt == "first" else (f if f in labels else None)
            if label is None:
                skipped.append(f"{sub}/{f}")
                continue
            members.append(len(paths))
            paths.append((os.path.join(low_dir, f), os.path.join(high_dir, label)))
            names.append(f"{sub}/{f}")
        if members:
            groups.append((sub, members))
    if skipped:
        warnings.warn(f"nested_folder_pairs: no ground truth under {high_root} for {len(skipped)} image(s): {', '.join(skipped)}")
    pairs = FolderPairs(paths, names, skipped)
    pairs.groups = groups
    return pairs


def group_means(result: EvalResult, pairs):
    """-> ({sub: {"n": images, "psnr": mean, "ssim": ..., "psnr_gt_mean": ..., "ssim_gt_mean": ...}}, overall): the means of
    each sub-folder of pairs.groups (nested_folder_pairs) over its images, and `overall`, the same keys over all of them --
    the sum over every image divided by their number, which is what measure_SID_blur.py prints."""
    per, total, n_all = {}, {k: 0.0 for k in _KEYS}, 0
    for sub, members in pairs.groups:
        sums = {k: 0.0 for k in _KEYS}
        for k in _KEYS:
            for i in members:
                sums[k] += result.per_image[k][i]
            total[k] += sums[k]
        n_all += len(members)
        per[sub] = {"n": len(members), **{k: sums[k] / len(members) for k in _KEYS}}
    if n_all == 0:
        raise ValueError("group_means: no images")
    return per, {"n": n_all, **{k: total[k] / n_all for k in _KEYS}}


# ---- NIQE (measure_niqe_bris.py -> loss/niqe_utils.py) -----------------------------------------------------------------
NIQE_BLOCK = 96
# data/util.py: is_image_file -- a case-sensitive suffix test
UNPAIRED_EXTENSIONS = (".png", ".jpg", ".bmp", ".JPG", ".jpeg")
_NIQE_NO_PARAMS = ("NIQE needs the pristine-model parameters (mu_pris_param, cov_pris_param, gaussian_window): pass a NiqeParams "
                   "or the path of the reference's loss/niqe_pris_params.npz (load_niqe_params); they are data of the reference "
                   "and are not shipped with this package")


@dataclass
class NiqeParams:
    """The pristine multivariate-Gaussian model and the MSCN window of the reference's niqe_pris_params.npz"""
    mu_pris_param: np.ndarray                           # (1, 36) fp64
    cov_pris_param: np.ndarray                          # (36, 36) fp64
    gaussian_window: np.ndarray                         # (7, 7) fp64
    _dev: dict = field(default_factory=dict, repr=False, compare=False)      # device index -> the window as a device tensor

    def window_on(self, device):
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(np.ascontiguousarray(self.gaussian_window, dtype=np.float64).ravel()).to(device)
        return self._dev[key]


def load_niqe_params(path) -> NiqeParams:
    """Reads mu_pris_param (1,36), cov_pris_param (36,36) and gaussian_window (7,7) from an .npz with the reference's keys"""
    if path is None:
        raise ValueError(_NIQE_NO_PARAMS)
    with np.load(path) as z:
        missing = [k for k in ("mu_pris_param", "cov_pris_param", "gaussian_window") if k not in z.files]
        if missing:
            raise ValueError(f"load_niqe_params: {path} lacks {', '.join(missing)}")
        mu, cov, win = (np.array(z[k], dtype=np.float64) for k in ("mu_pris_param", "cov_pris_param", "gaussian_window"))
    if mu.size != 36 or cov.shape != (36, 36) or win.shape != (7, 7):
        raise ValueError(f"load_niqe_params: unexpected shapes {mu.shape}, {cov.shape}, {win.shape} in {path}")
    if not np.array_equal(win, win[::-1, ::-1]):
        raise ValueError("load_niqe_params: the window is not point-symmetric (the kernels correlate, the reference convolves)")
    return NiqeParams(mu.reshape(1, 36), cov, win)


def _niqe_params(params) -> NiqeParams:
    if isinstance(params, NiqeParams):
        return params
    if params is None:
        raise ValueError(_NIQE_NO_PARAMS)
    return load_niqe_params(params)


NIQE_GRID = 9801
_niqe_tables_host = None
_niqe_tables_dev = {}


def niqe_tables() -> np.ndarray:
    """(4, 9801) fp64 over alpha = np.arange(0.2, 10.001, 0.001): r_gam = gamma(2/a)^2 / (gamma(1/a) gamma(3/a)),
    sqrt(gamma(1/a) / gamma(3/a)), gamma(2/a) / gamma(1/a), alpha -- what estimate_aggd_param / compute_feature evaluate with
    scipy's gamma, here with math.gamma (2.2e-15 relative apart)"""
    global _niqe_tables_host
    if _niqe_tables_host is None:
        a = np.arange(0.2, 10.001, 0.001)
        assert a.size == NIQE_GRID
        rec = 1.0 / a
        g1 = np.array([math.gamma(v) for v in rec])
        g2 = np.array([math.gamma(v) for v in rec * 2])
        g3 = np.array([math.gamma(v) for v in rec * 3])
        b13 = np.sqrt(np.array([math.gamma(1 / v) / math.gamma(3 / v) for v in a]))
        m21 = np.array([math.gamma(2 / v) / math.gamma(1 / v) for v in a])
        _niqe_tables_host = np.ascontiguousarray(np.stack([g2 * g2 / (g1 * g3), b13, m21, a]))
    return _niqe_tables_host


def _niqe_tables_on(device):
    """uploaded once per process and device"""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _niqe_tables_dev:
        _niqe_tables_dev[key] = torch.from_numpy(niqe_tables()).to(device)
    return _niqe_tables_dev[key]


def _niqe_input(images, what):
    _on_device(images)
    if images.dtype != torch.uint8:
        raise RuntimeError(f"{what} takes uint8 images (got {images.dtype}); see to_uint8")
    x = _batched(images, what)
    h, w = x.shape[-2:]
    if h < NIQE_BLOCK or w < NIQE_BLOCK:
        raise ValueError(f"{what}: images of at least {NIQE_BLOCK} x {NIQE_BLOCK} pixels are needed (got {h} x {w}): NIQE is "
                         "measured on whole 96 x 96 blocks")
    return x


def niqe_luma(images: torch.Tensor, crop: bool = True) -> torch.Tensor:
    """uint8 (B,3,h,w) -> uint8 (B,hc,wc): the Y plane the reference's NIQE works on (to_y_channel on an RGB array: the
    BT.601 weights in B, G, R order, rounded half to even), cropped to whole blocks (crop=False: the whole image).  A stage
    of niqe_features, for tests."""
    x = _niqe_input(images, "niqe_luma")
    B, _, h, w = x.shape
    hc, wc = (h // NIQE_BLOCK * NIQE_BLOCK, w // NIQE_BLOCK * NIQE_BLOCK) if crop else (h, w)
    y = torch.empty((B, hc, wc), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_niqe_luma", ops._p(x), ops._p(y), B, h, w, hc, wc, ops._stream())
    return y


def _plane(img, what):
    _on_device(img)
    if img.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"{what}: expected a uint8 or fp32 plane (got {img.dtype})")
    if img.dim() == 2:
        img = img.unsqueeze(0)
    if img.dim() != 3:
        raise RuntimeError(f"{what}: expected (B,h,w) or (h,w), got {tuple(img.shape)}")
    return img.contiguous()


def niqe_half(img: torch.Tensor) -> torch.Tensor:
    """(B,h,w) uint8 or fp32 plane in 0..255, h and w even -> fp32 (B,h/2,w/2): imresize(img / 255, 0.5) * 255 (MATLAB-style
    antialiased bicubic).  A stage of niqe_features, for tests."""
    x = _plane(img, "niqe_half")
    B, h, w = x.shape
    if h % 2 or w % 2 or h < 4 or w < 4:
        raise ValueError(f"niqe_half: even sizes of at least 4 are needed (got {h} x {w})")
    rows = torch.empty((B, h // 2, w), dtype=torch.float32, device=x.device)
    out = torch.empty((B, h // 2, w // 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_niqe_half", ops._p(x), int(x.dtype == torch.float32), ops._p(rows), ops._p(out), B, h, w,
                   ops._stream())
    return out


def niqe_mscn(img: torch.Tensor, params, block: int = NIQE_BLOCK):
    """(B,h,w) uint8 or fp32 plane (h, w multiples of block = 96 or 48) -> (mscn fp32 (B,h,w), moments fp64 (B,blocks,5,6)):
    the locally normalised image and, per block and per map (the block; the block times itself rolled by (0,1), (1,0), (1,1),
    (1,-1)), the six sums of the asymmetric-Gaussian fit.  A stage of niqe_features, for tests."""
    prm = _niqe_params(params)
    x = _plane(img, "niqe_mscn")
    B, h, w = x.shape
    if block not in (96, 48) or h % block or w % block or h == 0 or w == 0:
        raise ValueError(f"niqe_mscn: block {block} (96 or 48) must divide the {h} x {w} plane")
    nblk = (h // block) * (w // block)
    m = torch.empty((B, h, w), dtype=torch.float32, device=x.device)
    mom = torch.empty((B, nblk, 5, 6), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_niqe_moments", ops._p(x), int(x.dtype == torch.float32), ops._p(prm.window_on(x.device)), block,
                   ops._p(m), ops._p(mom), B, h, w, ops._stream())
    return m, mom


def niqe_fit(moments: torch.Tensor, block: int = NIQE_BLOCK) -> torch.Tensor:
    """moments fp64 (..., 5, 6) of blocks of block x block pixels -> the 18 features (..., 18) fp64.  A stage of
    niqe_features, for tests."""
    _on_device(moments)
    if moments.dtype != torch.float64 or moments.dim() < 2 or tuple(moments.shape[-2:]) != (5, 6):
        raise RuntimeError(f"niqe_fit: expected fp64 (...,5,6) moments, got {moments.dtype} {tuple(moments.shape)}")
    mom = moments.contiguous()
    n = mom.numel() // 30
    feat = torch.empty(tuple(mom.shape[:-2]) + (18,), dtype=torch.float64, device=mom.device)
    with torch.cuda.device(mom.device):
        lib().call("cidnet_metric_niqe_fit", ops._p(mom), ops._p(_niqe_tables_on(mom.device)), int(block), ops._p(feat), 18, n,
                   ops._stream())
    return feat


def niqe_features(images: torch.Tensor, params) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) on the device -> (B, blocks, 36) float64 on the device: per 96 x 96 block of the
    top-left (h // 96 * 96, w // 96 * 96) crop, in the reference's block order (for w: for h), the 18 features at full size
    and the 18 at half size (niqe_utils.py: niqe()).  A row holds NaN where a fit has an empty tail or no variance.
    params: a NiqeParams or the path of the reference's niqe_pris_params.npz."""
    prm = _niqe_params(params)
    x = _niqe_input(images, "niqe_features")
    B, _, h, w = x.shape
    nblk = (h // NIQE_BLOCK) * (w // NIQE_BLOCK)
    n = lib().raw("cidnet_metric_niqe_ws_floats")(B, h, w)
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    feat = torch.empty((B, nblk, 36), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_niqe_features", ops._p(x), ops._p(prm.window_on(x.device)), ops._p(_niqe_tables_on(x.device)),
                   ops._p(feat), ops._p(ws), n, B, h, w, ops._stream())
    return feat


def niqe_score(features, params) -> np.ndarray:
    """(B, blocks, 36) features (a device or host tensor, or an array) -> (B,) fp64 numpy: nanmean over the blocks, covariance
    of the NaN-free rows, sqrt(d pinv((cov_pris + cov) / 2) d^T) (niqe_utils.py: the tail of niqe()), in numpy fp64 on the
    host.  Fewer than two NaN-free blocks: NaN (the reference raises from inside the SVD there)."""
    prm = _niqe_params(params)
    f = features.detach().cpu().numpy() if isinstance(features, torch.Tensor) else np.asarray(features, dtype=np.float64)
    if f.ndim == 2:
        f = f[None]
    out = np.full(f.shape[0], np.nan)
    for b, fb in enumerate(f):
        ok = ~np.isnan(fb).any(axis=1)
        if ok.sum() < 2:
            continue
        with np.errstate(all="ignore"):
            mu = np.nanmean(fb, axis=0)
        cov = np.cov(fb[ok], rowvar=False)
        d = prm.mu_pris_param - mu
        out[b] = np.sqrt((d @ np.linalg.pinv((prm.cov_pris_param + cov) / 2) @ d.T).item())
    return out


def niqe(images: torch.Tensor, params) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) on the device -> (B,) float64 on the device: calculate_niqe(image) of the reference with
    its defaults (Y of the RGB array as the reference forms it, no border crop).  The features come from the device
    kernels; the 36 x 36 tail runs on the host after one device-to-host copy of the batch's features."""
    feat = niqe_features(images, params)
    return torch.from_numpy(niqe_score(feat, params)).to(feat.device)


# ---- LOE (Wang et al. 2013; no counterpart in the reference) -------------------------------------------------------------
def loe_grid(h: int, w: int, sample=50):
    """The sampling grid of LOE, pure host code -> (step, rows, cols): step = max(1, min(h, w) // sample) (1 when sample is
    None: every pixel), rows = h // step, cols = w // step; sample (i, j) is source pixel (i * step, j * step)."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"loe_grid: sizes must be positive (got {h} x {w})")
    if sample is None:
        step = 1
    else:
        if int(sample) < 1:
            raise ValueError(f"loe_grid: sample must be positive or None (got {sample})")
        step = max(1, min(h, w) // int(sample))
    return step, h // step, w // step


def _loe_input(low, out):
    if not (isinstance(low, torch.Tensor) and isinstance(out, torch.Tensor)):
        raise ValueError("loe: expected two tensors")
    _on_device(low, out)
    if low.dtype != torch.uint8 or out.dtype != torch.uint8:
        raise ValueError(f"loe takes uint8 images (got {low.dtype}, {out.dtype}); see to_uint8")
    for t, what in ((low, "low"), (out, "out")):
        if t.dim() not in (3, 4) or t.shape[-3] != 3:
            raise ValueError(f"loe: {what}: expected (B,3,h,w) or (3,h,w), got {tuple(t.shape)}")
    a, b = _batched(low, "low"), _batched(out, "out")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"loe: low {tuple(a.shape)} and out {tuple(b.shape)} differ")
    return a, b


def _loe_launch(low, out, sample):
    a, b = _loe_input(low, out)
    B, _, h, w = a.shape
    step, rows, cols = loe_grid(h, w, sample)
    L = lib()
    n = L.raw("cidnet_metric_loe_ws_bytes")(B)
    ws = torch.empty(n, dtype=torch.uint8, device=a.device)
    num = torch.empty(B, dtype=torch.int64, device=a.device)
    val = torch.empty(B, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        L.call("cidnet_metric_loe_u8", ops._p(a), ops._p(b), B, h, w, step, ops._p(num), ops._p(val), ops._p(ws), n, ops._stream())
    return num, val, rows * cols


def loe_counts(low_u8: torch.Tensor, out_u8: torch.Tensor, sample=50):
    """uint8 (B,3,h,w) (or (3,h,w)) pairs on the device -> (num int64 (B,) on the device, m): over the m = rows * cols samples
    of loe_grid(h, w, sample), with L = max(R, G, B) of the low image and Le of the enhanced one, num counts the ordered pairs
    (x, y), y = x included, whose order differs: (L(x) >= L(y)) != (Le(x) >= Le(y)).  Exact; no host synchronisation."""
    num, _, m = _loe_launch(low_u8, out_u8, sample)
    return num, m


def loe(low_u8: torch.Tensor, out_u8: torch.Tensor, sample=50, normalized: bool = False) -> torch.Tensor:
    """(B,) float64 on the device: num / m, the classic lightness order error (0 .. m), or num / m^2 (normalized=True, 0 .. 1);
    see loe_counts.  Numbers compare only under the same sampler: sample=50 strides to about 50 samples on the short side,
    sample=None takes every pixel."""
    num, val, m = _loe_launch(low_u8, out_u8, sample)
    if not normalized:
        return val
    # a true division: dividing by a host scalar on the device would multiply by fl(1 / m^2), one ulp off for some counts
    return num.to(torch.float64) / torch.full((), float(m * m), dtype=torch.float64, device=num.device)


# ---- JPEG file round trip (eval.py saves a .jpg input's output as a JPEG; measure_niqe_bris.py scores the decoded file) --------
# Annex K.1 / K.2 of the JPEG standard, in natural (row-major) order: the tables libjpeg's jpeg_set_quality scales
_JPEG_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                  14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                    47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
JPEG_EXTENSIONS = (".jpg", ".jpeg")                                # lower-cased: the names PIL saves as JPEG
_jpeg_plans = {}                                                   # quality -> JpegQuantPlan
_jpeg_plans_dev = {}                                               # (device index, quality) -> the int32 (2,2,64) table there


@dataclass(frozen=True)
class JpegQuantPlan:
    """What quantising at one quality needs (jpeg_quant_plan); the arrays are read-only.  A coefficient v of libjpeg's scaled
    forward DCT becomes sign(v) ((|v| + (d >> 1)) // d) t with d = 8 t; the kernel forms the quotient as the high 32 bits of
    (|v| + (d >> 1)) * magic, magic = ceil(2^32 / d): exact for every numerator below 2^16 (n d < 2^32)."""
    quality: int
    luma: np.ndarray                                               # int32 (8,8), 1..255
    chroma: np.ndarray                                             # int32 (8,8)
    divisors: np.ndarray                                           # int32 (2,8,8): 8 t, luma then chroma
    magic: np.ndarray                                              # int64 (2,8,8): ceil(2^32 / (8 t)), at most 2^29
    shift: int = 32

    def device_table(self) -> np.ndarray:
        """int32 (2,2,64), what cidnet_metric_jpeg_roundtrip_u8 reads: per component the table, then the constants"""
        t = np.stack([self.luma, self.chroma]).reshape(2, 64)
        return np.ascontiguousarray(np.stack([t, self.magic.reshape(2, 64)], axis=1).astype(np.int32))


def _jpeg_magic(divisor: int) -> int:
    """ceil(2^32 / divisor): floor(n / divisor) is the high word of n * it whenever n * divisor < 2^32"""
    return -((-1 << 32) // int(divisor))


def jpeg_quant_plan(quality: int = 75) -> JpegQuantPlan:
    """The baseline quantisation tables Pillow writes at `quality` (1..100) with its defaults -- Annex K scaled by s = 5000 //
    q below 50, else 200 - 2 q: t = clamp((std s + 50) // 100, 1, 255) -- with the divisors 8 t and the exact-division
    constants of the kernel.  Pure host code; cached per quality."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg_quant_plan: quality must be an integer in 1..100 (got {quality!r})")
    q = int(quality)
    if q not in _jpeg_plans:
        s = 5000 // q if q < 50 else 200 - 2 * q
        tabs = [np.clip((np.array(std, dtype=np.int64) * s + 50) // 100, 1, 255).reshape(8, 8) for std in
                (_JPEG_STD_LUMA, _JPEG_STD_CHROMA)]
        div = np.stack(tabs) * 8
        arrays = (tabs[0].astype(np.int32), tabs[1].astype(np.int32), div.astype(np.int32),
                  np.array([_jpeg_magic(d) for d in div.reshape(-1)], dtype=np.int64).reshape(2, 8, 8))
        for a in arrays:
            a.setflags(write=False)
        _jpeg_plans[q] = JpegQuantPlan(q, *arrays)
    return _jpeg_plans[q]


def _jpeg_table_on(device, quality):
    """uploaded once per process, device and quality"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(quality))
    if key not in _jpeg_plans_dev:
        _jpeg_plans_dev[key] = torch.from_numpy(jpeg_quant_plan(quality).device_table()).to(device)
    return _jpeg_plans_dev[key]


def jpeg_roundtrip_u8(q: torch.Tensor, quality: int = 75) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) on the device -> uint8 of the same form: per image what PIL's Image.open() returns for the
    file Image.save(f, 'JPEG', quality=quality) writes of it (4:2:0, baseline tables: Pillow's defaults, as eval.py saves a
    .jpg), byte for byte and without the file: the lossy stages of libjpeg in its own fixed-point arithmetic (csrc/jpeg.hip,
    DESIGN.md 6.10).  A non-contiguous view is read as its values.  w < 5, h < 1 or a quality outside 1..100: ValueError."""
    if not isinstance(q, torch.Tensor):
        raise RuntimeError("jpeg_roundtrip_u8: expected a tensor")
    _on_device(q)
    if q.dtype != torch.uint8:
        raise RuntimeError(f"jpeg_roundtrip_u8 takes uint8 images (got {q.dtype}); see to_uint8")
    plan = jpeg_quant_plan(quality)
    squeeze = q.dim() == 3
    x = _batched(q, "jpeg_roundtrip_u8")
    B, _, h, w = x.shape
    if h < 1 or w < 5 or B < 1:
        raise ValueError(f"jpeg_roundtrip_u8: images of at least 1 x 5 pixels are needed (got {B} of {h} x {w}): libjpeg's "
                         "decoder reads padded columns of narrower ones")
    L = lib()
    n = L.raw("cidnet_metric_jpeg_ws_bytes")(B, h, w)
    ws = torch.empty(n, dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        L.call("cidnet_metric_jpeg_roundtrip_u8", ops._p(x), ops._p(out), ops._p(ws), n, ops._p(_jpeg_table_on(x.device, plan.quality)),
               B, h, w, ops._stream())
    return out[0] if squeeze else out


@dataclass
class UnpairedResult:
    """Mean NIQE -- and mean LOE and mean BRISQUE, where evaluate_unpaired(loe=True) / (brisque=params) asked for them, else
    NaN -- over the evaluated images (running sum in input order, divided by their number) and the per-image values"""
    alpha: float
    niqe: float
    per_image: dict = field(default_factory=dict)     # "niqe" (and "loe", "brisque") -> list, input order
    names: list = field(default_factory=list)
    ensemble: int = 1                                 # the number of views each output was averaged over
    loe: float = math.nan                             # mean lightness order error against the inputs as supplied
    brisque: float = math.nan                         # mean BRISQUE score of the outputs


def evaluate_unpaired(model, images, params, alpha=1.0, gamma: float = 1.0, batch_size: int = 1, process_group=None,
                      save_dir=None, ensemble: int = 1, loe: bool = False, loe_sample=50, file_roundtrip: bool = False,
                      jpeg_quality: int = 75, png: str = "pillow", jpeg: str = "pillow", brisque=None):
    """eval.py --unpaired + measure_niqe_bris.py on the device.  `images`: a sequence of (3,h,w) float images in [0, 1] (or
    uint8 HWC images, converted as ToTensor() does; folder_images() yields these), each at least 96 x 96.  Each is reflect-
    padded to a multiple of 8, run through model(pow(x, gamma)) in eval mode under no_grad with trans.gated2 = True and
    trans.alpha = alpha (a tuple result -- CIDNet_TNSM -- gives its [0]), clamped, cropped, quantized to uint8 and scored
    with NIQE.  params: a NiqeParams or the path of the reference's niqe_pris_params.npz.

    alpha: a number, or a sequence (a sweep): the result is then a list with one UnpairedResult per value and the model's
    trunk runs once per batch, as in evaluate().  batch_size > 1 batches consecutive images of equal padded size.
    Data-parallel as evaluate(): rank r scores images i % world == r, one SUM all-reduce gathers the values.
    save_dir: as evaluate() -- the enhanced images are also written there, under images.names[i] or "<i as 5 digits>.png".
    png: as evaluate() -- "device" writes save_dir's .png files from a stream encoded on the device; the scores are untouched.
    jpeg: as evaluate() -- "device" writes save_dir's .jpg / .jpeg files from the device, byte-equal to Pillow's at quality 75.
    ensemble: as evaluate() -- 2, 4 or 8 views of the padded input, the merged result scored.
    loe: True -- each output is also scored with LOE (loe(), sampler loe_sample) against its input as supplied: to_uint8 of the
    fp32 input before the reflect pad and before ** gamma.  UnpairedResult.loe is the mean, per_image["loe"] the values; NIQE is
    untouched.  False: nothing of it runs, UnpairedResult.loe is NaN.  The reference has no LOE.
    file_roundtrip: True -- an image whose name (images.names[i]) ends, lower-cased, in .jpg or .jpeg is scored as
    measure_niqe_bris.py scores it: eval.py saves its output under the input's name, so PIL writes a JPEG of quality
    jpeg_quality (75, PIL's default) and the score is that of the decoded file.  The quantized, cropped output goes through
    jpeg_roundtrip_u8 (the file's lossy stages on the device, byte-equal to PIL's save + open) and the result is what NIQE --
    and LOE, when asked for -- sees.  Other names and unnamed images are untouched, each image of a batch by its own name;
    per_image["file_roundtrip"] holds one bool per image.  save_dir still receives the un-round-tripped output: its .jpg,
    decoded again, is exactly what was scored.  False: nothing of it runs and the result is what it was without the keyword.
    brisque: a BrisqueParams or the (libsvm model, range file) pair of paths -- each output is also scored with BRISQUE
    (brisque(), measure_niqe_bris.py's second number) on the same bytes NIQE sees, after the file round trip where that applies.
    UnpairedResult.brisque is the mean, per_image["brisque"] the values, after "niqe" and "loe".  None: nothing of it runs,
    UnpairedResult.brisque is NaN and the result is what it was without the keyword.
    The model's attributes and the train / eval mode of every submodule are restored afterwards.
    Without file_roundtrip=True
    the score is the quantized output's, not that of a lossy file decoded again (.jpg names: DICM, NPE, VV)."""
    prm = _niqe_params(params)
    bprm = _brisque_params(brisque) if brisque is not None else None
    names = getattr(images, "names", None)
    if file_roundtrip:
        jpeg_quant_plan(jpeg_quality)                            # a bad quality raises before anything runs
    lossy = [bool(file_roundtrip) and names is not None and os.path.splitext(str(names[i]))[1].lower() in JPEG_EXTENSIONS
             for i in range(len(images))]

    def load(i, img, device):
        x = _image_f32(img, device)
        if x.shape[1] < NIQE_BLOCK or x.shape[2] < NIQE_BLOCK:
            raise ValueError(f"evaluate_unpaired: image {i} is {x.shape[1]} x {x.shape[2]}; NIQE needs at least "
                             f"{NIQE_BLOCK} x {NIQE_BLOCK} pixels")
        return x, ((to_uint8(x) if loe else None), lossy[i])

    def score(q, aux):
        flagged = [k for k, a in enumerate(aux) if a[1]]
        if len(flagged) == len(aux):
            q = jpeg_roundtrip_u8(q, jpeg_quality)
        elif flagged:                                            # a batch of mixed names: each image its own treatment
            q = q.clone()
            q[flagged] = jpeg_roundtrip_u8(q[flagged], jpeg_quality)
        out = [niqe(q, prm)]
        if loe:
            low = torch.stack([a[0] for a in aux]) if len(aux) > 1 else aux[0][0].unsqueeze(0)
            out.append(_loe_launch(low, q, loe_sample)[1])       # loe(): the keyword shadows its name in here
        if bprm is not None:
            out.append(brisque_score(brisque_features(q), bprm))  # brisque(): shadowed likewise
        return tuple(out)

    def result(per_image, **kw):
        if file_roundtrip:
            per_image["file_roundtrip"] = list(lossy)
        return UnpairedResult(per_image=per_image, ensemble=int(ensemble), **kw)
    return _evaluate("evaluate_unpaired", "images", model, images, load, dict(gated2=True), score,
                     ("niqe",) + (("loe",) if loe else ()) + (("brisque",) if bprm is not None else ()), result, alpha,
                     gamma, batch_size, process_group, save_dir, ensemble=ensemble, png=png, jpeg=jpeg)


class FolderImages:
    """Sequence of images read from disk on access, each as ToTensor() gives it (fp32 (3,h,w) in [0, 1]) through PIL's
    .convert('RGB').  names: the file names; paths: their paths."""

    def __init__(self, paths, names):
        self.paths, self.names = paths, names

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        return torch.from_numpy(_read_rgb(self.paths[i])).permute(2, 0, 1).float().div(255)


def folder_images(directory: str) -> FolderImages:
    """Every image file of `directory`, sorted by path, chosen as the reference's unpaired loader chooses them (data/util.py:
    is_image_file: the name ends in .png, .jpg, .bmp, .JPG or .jpeg, case-sensitively); loaded lazily."""
    names = sorted(f for f in os.listdir(directory)
                   if f.endswith(UNPAIRED_EXTENSIONS) and os.path.isfile(os.path.join(directory, f)))
    return FolderImages([os.path.join(directory, f) for f in names], names)


# ---- LPIPS, AlexNet variant (measure.py:78,145-153 -> lpips.LPIPS(net='alex')) ------------------------------------------
LPIPS_MIN = 31
# (index in torchvision's AlexNet `features`, out channels, in channels, kernel, stride, padding, pooled first)
LPIPS_LAYERS = ((0, 64, 3, 11, 4, 2, False), (3, 192, 64, 5, 1, 2, True), (6, 384, 192, 3, 1, 1, True),
                (8, 256, 384, 3, 1, 1, False), (10, 256, 256, 3, 1, 1, False))
_LPIPS_NO_PARAMS = ("LPIPS needs torchvision's AlexNet weights and the lpips package's alex.pth heads: pass an LpipsParams or "
                    "the pair of paths (load_lpips_params); neither file is shipped with this package")


@dataclass(frozen=True)
class LpipsParams:
    """The frozen parameters of lpips.LPIPS(net='alex'): per tap the convolution's weight (M,C,k,k) and bias (M), fp32 host
    tensors in torchvision's shapes, and the 1x1 head as a (C_l,) fp32 tensor.  on(device) uploads them once per device;
    dgrad_on(device) forms, once per device, the weights as the training loss's data gradients read them."""
    weights: tuple
    biases: tuple
    heads: tuple
    _dev: dict = field(default_factory=dict, repr=False, compare=False)      # device index -> (weights, biases, heads) there
    _dgrad: dict = field(default_factory=dict, repr=False, compare=False)    # device index -> the five data-gradient weights

    def __post_init__(self):
        for name, got, want in _lpips_shapes(self.weights, self.biases, self.heads):
            if got != want:
                raise ValueError(f"LpipsParams: {name} has shape {got}, expected {want}")

    def on(self, device):
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            self._dev[key] = tuple(tuple(t.to(device, torch.float32).contiguous() for t in ts)
                                   for ts in (self.weights, self.biases, self.heads))
        return self._dev[key]

    def dgrad_on(self, device):
        """-> per layer the device weights in cidnet_lpips_dgrad_weights' form (flipped and transposed for the stride-1 layers,
        phase-ordered for the first); the weights are frozen, so this happens once, outside any step"""
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dgrad:
            out = []
            with torch.cuda.device(device):
                for w, (_, m, c, k, stride, _, _) in zip(self.on(device)[0], LPIPS_LAYERS):
                    wt = torch.empty(lib().raw("cidnet_lpips_dgrad_weights_floats")(m, c, k, stride), dtype=torch.float32, device=w.device)
                    lib().call("cidnet_lpips_dgrad_weights", ops._p(w), ops._p(wt), m, c, k, stride, ops._stream())
                    out.append(wt)
            self._dgrad[key] = tuple(out)
        return self._dgrad[key]

    @staticmethod
    def random(seed: int = 19) -> "LpipsParams":
        """Deterministic stand-ins for tests and benchmarks: convolutions He-uniform with bound sqrt(6 / (k k C_in)), biases
        uniform in +-0.05, heads uniform in [0, 2 / C).  These are NOT the trained metric: scores computed with them mean
        nothing outside tests -- the real parameters come from load_lpips_params."""
        gen = torch.Generator().manual_seed(int(seed))
        ws, bs, hs = [], [], []
        for _, m, c, k, _, _, _ in LPIPS_LAYERS:
            bound = (6.0 / (k * k * c)) ** 0.5
            ws.append((torch.rand((m, c, k, k), generator=gen) * 2 - 1) * bound)
            bs.append((torch.rand(m, generator=gen) * 2 - 1) * 0.05)
        for _, m, *_ in LPIPS_LAYERS:
            hs.append(torch.rand(m, generator=gen) * (2.0 / m))
        return LpipsParams(tuple(ws), tuple(bs), tuple(hs))


def _lpips_shapes(weights, biases, heads):
    if not (len(weights) == len(biases) == len(heads) == 5):
        raise ValueError("LpipsParams: five weights, five biases and five heads are needed")
    for l, (i, m, c, k, _, _, _) in enumerate(LPIPS_LAYERS):
        yield f"weight {l}", tuple(weights[l].shape), (m, c, k, k)
        yield f"bias {l}", tuple(biases[l].shape), (m,)
        yield f"head {l}", tuple(heads[l].shape), (m,)


def load_lpips_params(alexnet_path, heads_path) -> LpipsParams:
    """Reads the two public files: torchvision's AlexNet state dict (keys features.{0,3,6,8,10}.{weight,bias}; the bare
    {i}.weight form of a `features` state dict is accepted too) and the lpips package's weights/v0.1/alex.pth (keys
    lin{0..4}.model.1.weight, (1,C,1,1)).  A missing key or a wrong shape is a ValueError that names it."""
    if alexnet_path is None or heads_path is None:
        raise ValueError(_LPIPS_NO_PARAMS)
    sd = torch.load(alexnet_path, map_location="cpu", weights_only=True)
    hd = torch.load(heads_path, map_location="cpu", weights_only=True)

    def get(d, path, keys, shape):
        for k in keys:
            if k in d:
                t = d[k]
                if tuple(t.shape) != shape:
                    raise ValueError(f"load_lpips_params: {k} in {path} has shape {tuple(t.shape)}, expected {shape}")
                return t.detach().to(torch.float32).clone()
        raise ValueError(f"load_lpips_params: {path} lacks {keys[0]}")
    ws, bs, hs = [], [], []
    for l, (i, m, c, k, _, _, _) in enumerate(LPIPS_LAYERS):
        ws.append(get(sd, alexnet_path, (f"features.{i}.weight", f"{i}.weight"), (m, c, k, k)))
        bs.append(get(sd, alexnet_path, (f"features.{i}.bias", f"{i}.bias"), (m,)))
        hs.append(get(hd, heads_path, (f"lin{l}.model.1.weight",), (1, m, 1, 1)).reshape(m))
    return LpipsParams(tuple(ws), tuple(bs), tuple(hs))


def _lpips_params(params) -> LpipsParams:
    if isinstance(params, LpipsParams):
        return params
    if isinstance(params, (tuple, list)) and len(params) == 2:
        return load_lpips_params(*params)
    raise ValueError(_LPIPS_NO_PARAMS)


def lpips_feature_sizes(h: int, w: int):
    """Host only -> the five (height, width) of the taps of an h x w image.  ValueError under 31 x 31: at 31 the first
    convolution gives 7 and the pools 3 and then 1; anything smaller leaves a pool without a window."""
    h, w = int(h), int(w)
    if h < LPIPS_MIN or w < LPIPS_MIN:
        raise ValueError(f"lpips needs images of at least {LPIPS_MIN} x {LPIPS_MIN} pixels (got {h} x {w}): a smaller one "
                         "leaves AlexNet's second pool without a window")
    out = (ctypes.c_int * 10)()
    lib().call("cidnet_lpips_feature_sizes", h, w, out)
    return [(out[2 * l], out[2 * l + 1]) for l in range(5)]


def _lpips_input(q, what):
    _on_device(q)
    if q.dtype != torch.uint8:
        raise RuntimeError(f"{what} takes uint8 images (got {q.dtype}); see to_uint8")
    x = _batched(q, what)
    lpips_feature_sizes(*x.shape[-2:])
    return x


def _lpips_extract(parts, prm):
    """parts: [(uint8 (B_i,3,h,w), scale (B_i,) fp64 or None), ...] of one size -> the five fp32 taps of their concatenation,
    one batch through the extractor.  The caller has made the device current."""
    dev = parts[0][0].device
    h, w = parts[0][0].shape[-2:]
    N = sum(q.shape[0] for q, _ in parts)
    L = lib()
    x = torch.empty((N, 3, h, w), dtype=torch.float32, device=dev)
    i = 0
    for q, s in parts:
        L.call("cidnet_metric_lpips_ingest", ops._p(q), ops._p(s), ops._p(x[i:]), q.shape[0], h, w, ops._stream())
        i += q.shape[0]
    weights, biases, _ = prm.on(dev)
    return ops.lpips_taps(x, weights, biases, LPIPS_LAYERS)


def _lpips_distance(f0, f1, prm, h, w, want_layers=True, want_score=True):
    """f0, f1: the five taps of B images each (contiguous, a batch slice of _lpips_extract's result will do) of h x w images
    -> (layers (B,5) fp64, score (B,) fp64)"""
    dev = f0[0].device
    B = f0[0].shape[0]
    L = lib()
    n = L.raw("cidnet_metric_lpips_ws_floats")(B, h, w)
    ws = torch.empty(n, dtype=torch.float32, device=dev)
    heads = prm.on(dev)[2]
    for l in range(5):
        _, C, fh, fw = f0[l].shape
        L.call("cidnet_metric_lpips_layer", ops._p(f0[l]), ops._p(f1[l]), ops._p(heads[l]), ops._p(ws), n, l, B, C, fh, fw, h, w,
               ops._stream())
    layers = torch.empty((B, 5), dtype=torch.float64, device=dev) if want_layers else None
    score = torch.empty(B, dtype=torch.float64, device=dev) if want_score else None
    L.call("cidnet_metric_lpips_finish", ops._p(ws), n, ops._p(layers), ops._p(score), B, h, w, ops._stream())
    return layers, score


def lpips_features(q_u8: torch.Tensor, params, scale=None):
    """uint8 (B,3,h,w) (or (3,h,w)) on the device -> the five fp32 taps [(B,64,.,.), (B,192,.,.), (B,384,.,.), (B,256,.,.),
    (B,256,.,.)] of AlexNet on x = u / 127.5 - 1 behind lpips' scaling layer (include/cidnet_hip.h: LPIPS, steps 1-2).
    scale: None, or (B,) fp64 on the device -- the image enters as the float clip(u * scale, 0, 255) (GT mean).
    params: an LpipsParams or (alexnet path, heads path).  h, w >= 31."""
    prm = _lpips_params(params)
    x = _lpips_input(q_u8, "lpips_features")
    if scale is not None:
        scale = _checked_scale("lpips_features", scale, x.shape[0], x.device)
    with torch.cuda.device(x.device):
        return _lpips_extract([(x, scale)], prm)


def _lpips_pair(restored, gt, what):
    a, g = _lpips_input(restored, what), _lpips_input(gt, what)
    if a.shape != g.shape or a.device != g.device:
        raise RuntimeError(f"{what}: restored {tuple(a.shape)} and gt {tuple(g.shape)} differ")
    return a, g


def _lpips_run(restored, gt, params, gt_mean, what, want_layers, want_score):
    prm = _lpips_params(params)
    a, g = _lpips_pair(restored, gt, what)
    B, _, h, w = a.shape
    with torch.cuda.device(a.device):
        f = _lpips_extract([(a, _gt_mean_scale(a, g) if gt_mean else None), (g, None)], prm)
        return _lpips_distance([t[:B] for t in f], [t[B:] for t in f], prm, h, w, want_layers, want_score)


def lpips_layers(restored_u8: torch.Tensor, gt_u8: torch.Tensor, params, gt_mean: bool = False) -> torch.Tensor:
    """uint8 (B,3,h,w) pairs on the device -> (B,5) float64 on the device: the five layer terms d_l whose sum is lpips()"""
    return _lpips_run(restored_u8, gt_u8, params, gt_mean, "lpips_layers", True, False)[0]


def lpips(restored_u8: torch.Tensor, gt_u8: torch.Tensor, params, gt_mean: bool = False) -> torch.Tensor:
    """uint8 (B,3,h,w) pairs on the device -> (B,) float64 on the device, no host synchronisation: lpips.LPIPS(net='alex')
    (version 0.1, lpips=True, spatial=False, eval mode) of each pair as measure.py:145-153 calls it.  gt_mean: `restored`
    enters as the float clip(restored * s, 0, 255), s = mean(gray(gt)) / mean(gray(restored)) (measure.py:138-146).
    Identical images score exactly 0; a result is bit-identical from call to call and independent of the rest of the batch.
    params: an LpipsParams or (alexnet path, heads path).  h, w >= 31."""
    return _lpips_run(restored_u8, gt_u8, params, gt_mean, "lpips", False, True)[1]


def _lpips_both(q, g, prm, scale, gt_feats=None):
    """evaluate()'s LPIPS columns: (lpips, lpips_gt_mean, the ground truth's taps); scale = gt_mean_scale(q, g).  The restored
    and the rescaled images go through the extractor as one batch; the ground truth's taps are computed unless handed in (an
    alpha sweep reuses them)."""
    B, _, h, w = q.shape
    lpips_feature_sizes(h, w)
    if gt_feats is None:
        gt_feats = _lpips_extract([(g, None)], prm)
    f = _lpips_extract([(q, None), (q, scale)], prm)
    plain = _lpips_distance([t[:B] for t in f], gt_feats, prm, h, w, False, True)[1]
    gtm = _lpips_distance([t[B:] for t in f], gt_feats, prm, h, w, False, True)[1]
    return plain, gtm, gt_feats


# ---- CIEDE2000 (no counterpart in the reference) -----------------------------------------------------------
_CIEDE_KEYS = ("ciede2000", "ciede2000_gt_mean")
_ciede_tables_host = None
_ciede_tables_dev = {}


def ciede2000_tables() -> np.ndarray:
    """(256,) fp64, host only: the linear value of every 8-bit sRGB level, v = level / 255, v > 0.04045 ? ((v + 0.055) /
    1.055)^2.4 : v / 12.92 -- what the kernel reads where scikit-image's rgb2lab would call pow.  Read-only, cached."""
    global _ciede_tables_host
    if _ciede_tables_host is None:
        v = np.arange(256, dtype=np.float64) / 255.0
        t = np.where(v > 0.04045, np.power((v + 0.055) / 1.055, 2.4), v / 12.92)
        t.setflags(write=False)
        _ciede_tables_host = t
    return _ciede_tables_host


def _ciede_tables_on(device):
    """uploaded once per process and device"""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _ciede_tables_dev:
        _ciede_tables_dev[key] = torch.from_numpy(ciede2000_tables().copy()).to(device)
    return _ciede_tables_dev[key]


def ciede2000_lab(lab1: torch.Tensor, lab2: torch.Tensor) -> torch.Tensor:
    """fp64 (n,3) tensors of (L, a, b) on the device -> (n,) fp64 on the device: dE00 of each pair, lab1 as colour 1, by the
    formulation of Sharma, Wu and Dalal (2005) with kL = kC = kH = 1 (include/cidnet_hip.h: CIEDE2000) -- the core of
    ciede2000(), exposed so that it can be held against published Lab data."""
    _on_device(lab1, lab2)
    for t in (lab1, lab2):
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3:
            raise RuntimeError(f"ciede2000_lab: expected fp64 (n,3) Lab values, got {t.dtype} {tuple(t.shape)}")
    if lab1.shape != lab2.shape or lab1.device != lab2.device:
        raise RuntimeError(f"ciede2000_lab: lab1 {tuple(lab1.shape)} and lab2 {tuple(lab2.shape)} differ")
    a, b = lab1.contiguous(), lab2.contiguous()
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    if a.shape[0]:
        with torch.cuda.device(a.device):
            lib().call("cidnet_metric_ciede2000_lab", ops._p(a), ops._p(b), ops._p(out), a.shape[0], ops._stream())
    return out


def _ciede_launch(a, g, scale, want_map, want_mean):
    """a, g: checked (B,3,h,w) uint8 pairs; scale: None or (B,) fp64 on the device -> (map or None, mean or None).  The caller
    has made the device current."""
    B, _, h, w = a.shape
    L = lib()
    n = L.raw("cidnet_metric_ciede2000_ws_bytes")(B, h, w)
    ws = torch.empty(n, dtype=torch.uint8, device=a.device) if want_mean else None
    dmap = torch.empty((B, h, w), dtype=torch.float64, device=a.device) if want_map else None
    mean = torch.empty(B, dtype=torch.float64, device=a.device) if want_mean else None
    L.call("cidnet_metric_ciede2000_u8", ops._p(a), ops._p(g), ops._p(scale), ops._p(_ciede_tables_on(a.device)), ops._p(dmap),
           ops._p(mean), ops._p(ws), n, B, h, w, ops._stream())
    return dmap, mean


def _ciede_run(restored, gt, gt_mean, want_map, want_mean):
    a, g = _u8_pair("ciede2000 / ciede2000_map", restored, gt)
    with torch.cuda.device(a.device):
        return _ciede_launch(a, g, _gt_mean_scale(a, g) if gt_mean else None, want_map, want_mean)


def ciede2000_map(restored_u8: torch.Tensor, gt_u8: torch.Tensor, gt_mean: bool = False) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) pairs on the device -> (B,h,w) fp64 on the device: dE00 of every pixel, see ciede2000()"""
    return _ciede_run(restored_u8, gt_u8, gt_mean, True, False)[0]


def ciede2000(restored_u8: torch.Tensor, gt_u8: torch.Tensor, gt_mean: bool = False) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) pairs on the device -> (B,) fp64 on the device, no host synchronisation: the mean over the
    pixels of the CIEDE2000 difference between `restored` (colour 1) and `gt` (colour 2), each converted sRGB -> Lab with
    scikit-image's constants (D65 / 2 degree white) -- what deltaE_ciede2000(rgb2lab(a), rgb2lab(b)).mean() states, all in fp64
    (the definition: include/cidnet_hip.h, CIEDE2000).  gt_mean: `restored` enters as the real number clip(restored * s, 0,
    255), s = mean(gray(gt)) / mean(gray(restored)) as gt_mean_scale() forms it, not re-quantized (measure.py:138-141);
    an image whose gray mean is 0 gives whatever IEEE arithmetic makes of the infinite or NaN ratio.
    Identical images score exactly 0; a fixed-order reduction: bit-identical from call to call and independent of the rest of
    the batch (not bit-equal to ciede2000_map(...).mean(), which sums in another order).  Any h, w >= 1."""
    return _ciede_run(restored_u8, gt_u8, gt_mean, False, True)[1]


def _ciede_both(q, g, scale):
    """evaluate()'s CIEDE2000 columns of a checked batch: (plain, GT mean); scale = gt_mean_scale(q, g)"""
    return _ciede_launch(q, g, None, False, True)[1], _ciede_launch(q, g, scale, False, True)[1]


# ---- BRISQUE (measure_niqe_bris.py:26 -> imquality.brisque.score; csrc/brisque.hip) ---------------------------
BRISQUE_MIN = 16
BRISQUE_FEATURES = 36
_BRISQUE_NO_PARAMS = ("BRISQUE needs the trained support-vector model and the feature ranges: pass a BrisqueParams or the pair of "
                      "paths (libsvm text model, normalize.pickle or an .npz with min_ / max_; load_brisque_params); neither file "
                      "is shipped with this package")


@dataclass
class BrisqueParams:
    """The epsilon-SVR of BRISQUE (RBF kernel) and the feature ranges it was trained under: sv (n,36), coef (n,), rho, gamma,
    fmin (36,), fmax (36,), fp64 host arrays.  on(device) uploads them once per device."""
    sv: np.ndarray
    coef: np.ndarray
    rho: float
    gamma: float
    fmin: np.ndarray
    fmax: np.ndarray
    _dev: dict = field(default_factory=dict, repr=False, compare=False)      # device index -> (sv, coef, fmin, fmax, rho_gamma)

    def __post_init__(self):
        self.sv = np.ascontiguousarray(self.sv, dtype=np.float64)
        self.coef = np.ascontiguousarray(self.coef, dtype=np.float64).reshape(-1)
        self.fmin = np.ascontiguousarray(self.fmin, dtype=np.float64).reshape(-1)
        self.fmax = np.ascontiguousarray(self.fmax, dtype=np.float64).reshape(-1)
        self.rho, self.gamma = float(self.rho), float(self.gamma)
        n = self.coef.size
        if n < 1 or self.sv.shape != (n, BRISQUE_FEATURES) or self.fmin.size != BRISQUE_FEATURES or self.fmax.size != BRISQUE_FEATURES:
            raise ValueError(f"BrisqueParams: expected sv (n,36), coef (n,), fmin (36,), fmax (36,); got {self.sv.shape}, "
                             f"{self.coef.shape}, {self.fmin.shape}, {self.fmax.shape}")

    def on(self, device):
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            rg = np.array([self.rho, self.gamma], dtype=np.float64)
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.sv, self.coef, self.fmin, self.fmax, rg))
        return self._dev[key]

    @classmethod
    def random(cls, seed: int = 0, n_sv: int = 64) -> "BrisqueParams":
        """Stand-ins for tests only: scores from them mean nothing.  The ranges bracket what the features of noisy images take,
        and rho keeps the score away from a cancellation to zero."""
        rng = np.random.default_rng(seed)
        fmin = -rng.uniform(0.1, 1.0, BRISQUE_FEATURES)
        fmax = fmin + rng.uniform(2.0, 6.0, BRISQUE_FEATURES)
        return cls(rng.uniform(-1.0, 1.0, (int(n_sv), BRISQUE_FEATURES)), rng.normal(0.0, 1.0, int(n_sv)),
                   -(3.0 + rng.uniform()), 0.05, fmin, fmax)


def _brisque_model(path):
    """the libsvm text model of an epsilon-SVR with an RBF kernel -> (sv (n,36), coef (n,), rho, gamma)"""
    with open(path) as f:
        lines = [l.strip() for l in f.read().splitlines() if l.strip()]
    head, at = {}, None
    for i, l in enumerate(lines):
        if l == "SV":
            at = i + 1
            break
        parts = l.split()
        # nr_class is written by libsvm for every model type (2 for a regression) and carries nothing here
        if parts[0] not in ("svm_type", "kernel_type", "gamma", "total_sv", "rho", "nr_class") or len(parts) != 2:
            raise ValueError(f"load_brisque_params: {path}: unexpected header line {l!r} (an epsilon_svr / rbf libsvm text model "
                             "has svm_type, kernel_type, gamma, nr_class, total_sv, rho, then SV)")
        head[parts[0]] = parts[1]
    if at is None:
        raise ValueError(f"load_brisque_params: {path}: no SV line (not a libsvm text model, or a truncated one)")
    missing = [k for k in ("svm_type", "kernel_type", "gamma", "total_sv", "rho") if k not in head]
    if missing:
        raise ValueError(f"load_brisque_params: {path}: the header lacks {', '.join(missing)}")
    if head["svm_type"] != "epsilon_svr" or head["kernel_type"] != "rbf":
        raise ValueError(f"load_brisque_params: {path}: svm_type {head['svm_type']} / kernel_type {head['kernel_type']}; only "
                         "epsilon_svr with an rbf kernel is BRISQUE's model")
    try:
        n, gamma, rho = int(head["total_sv"]), float(head["gamma"]), float(head["rho"])
    except ValueError:
        raise ValueError(f"load_brisque_params: {path}: gamma, total_sv or rho is not a number") from None
    body = lines[at:]
    if n < 1 or len(body) != n:
        raise ValueError(f"load_brisque_params: {path}: total_sv says {n} support vectors, the file holds {len(body)}")
    sv, coef = np.zeros((n, BRISQUE_FEATURES)), np.zeros(n)
    for i, l in enumerate(body):
        parts = l.split()
        try:
            coef[i] = float(parts[0])
            for p in parts[1:]:
                k, v = p.split(":")
                k = int(k)
                if not 1 <= k <= BRISQUE_FEATURES:
                    raise IndexError(k)
                sv[i, k - 1] = float(v)                          # an index that is absent stays 0
        except IndexError as e:
            raise ValueError(f"load_brisque_params: {path}: support vector {i} has feature index {e.args[0]}; BRISQUE has "
                             f"{BRISQUE_FEATURES} features, numbered from 1") from None
        except ValueError:
            raise ValueError(f"load_brisque_params: {path}: support vector {i} is not `coef index:value ...`: {l[:60]!r}") from None
    return sv, coef, rho, gamma


def _brisque_range(path):
    """min_ / max_ of the 36 features from imquality's normalize.pickle (a mapping, or an object with these attributes) or an
    .npz with these keys"""
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            missing = [k for k in ("min_", "max_") if k not in z.files]
            if missing:
                raise ValueError(f"load_brisque_params: {path} lacks {', '.join(missing)}")
            lo, hi = np.array(z["min_"], dtype=np.float64), np.array(z["max_"], dtype=np.float64)
    else:
        import pickle
        with open(path, "rb") as f:
            obj = pickle.load(f)
        try:
            lo, hi = (obj["min_"], obj["max_"]) if isinstance(obj, dict) else (obj.min_, obj.max_)
        except (KeyError, AttributeError):
            raise ValueError(f"load_brisque_params: {path} holds neither min_ nor max_") from None
        lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    if lo.size != BRISQUE_FEATURES or hi.size != BRISQUE_FEATURES:
        raise ValueError(f"load_brisque_params: {path}: min_ {lo.shape} and max_ {hi.shape} are not 36 values each")
    return lo.reshape(-1), hi.reshape(-1)


def load_brisque_params(model_path, range_path) -> BrisqueParams:
    """model_path: the libsvm text model of imquality's BRISQUE (svm_type epsilon_svr, kernel_type rbf, gamma, total_sv, rho, SV,
    then `coef index:value ...` lines with 1-based indices, an absent index being 0).  range_path: its normalize.pickle (min_,
    max_) or an .npz with those keys.  Neither file is shipped: both are the user's own.  Anything else raises ValueError."""
    if model_path is None or range_path is None:
        raise ValueError(_BRISQUE_NO_PARAMS)
    sv, coef, rho, gamma = _brisque_model(model_path)
    lo, hi = _brisque_range(range_path)
    return BrisqueParams(sv, coef, rho, gamma, lo, hi)


def _brisque_params(params) -> BrisqueParams:
    if isinstance(params, BrisqueParams):
        return params
    if isinstance(params, (tuple, list)) and len(params) == 2:
        return load_brisque_params(*params)
    raise ValueError(_BRISQUE_NO_PARAMS)


def brisque_plan(h: int, w: int) -> dict:
    """cidnet_metric_brisque_plan (host only): tile side, tile rows / columns at both scales, the half size, the tile
    kernel's LDS bytes and the workspace floats per image"""
    buf = (ctypes.c_int * 9)()
    lib().call("cidnet_metric_brisque_plan", int(h), int(w), buf, 9)
    return dict(zip(("tile", "tiles_y", "tiles_x", "h2", "w2", "tiles_y2", "tiles_x2", "lds", "ws_floats"), buf))


def _brisque_input(q, what):
    if not isinstance(q, torch.Tensor):
        raise RuntimeError(f"{what}: expected a tensor")
    _on_device(q)
    if q.dtype != torch.uint8:
        raise RuntimeError(f"{what} takes uint8 images (got {q.dtype}); see to_uint8")
    x = _batched(q, what)
    h, w = x.shape[-2:]
    if h < BRISQUE_MIN or w < BRISQUE_MIN:
        raise ValueError(f"{what}: images of at least {BRISQUE_MIN} x {BRISQUE_MIN} pixels are needed (got {h} x {w})")
    return x


def _brisque_plane(y, what, least):
    if not isinstance(y, torch.Tensor):
        raise RuntimeError(f"{what}: expected a tensor")
    _on_device(y)
    if y.dtype != torch.float64:
        raise RuntimeError(f"{what}: expected an fp64 plane (got {y.dtype})")
    if y.dim() == 2:
        y = y.unsqueeze(0)
    if y.dim() != 3:
        raise RuntimeError(f"{what}: expected (B,h,w) or (h,w), got {tuple(y.shape)}")
    if y.shape[1] < least or y.shape[2] < least:
        raise ValueError(f"{what}: planes of at least {least} x {least} are needed (got {y.shape[1]} x {y.shape[2]})")
    return y.contiguous()


def brisque_gray(q: torch.Tensor) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) on the device -> fp64 (B,h,w): (0.2125 R + 0.7154 G + 0.0721 B) / 255, skimage's rgb2gray of
    a uint8 image.  A stage of brisque_features."""
    x = _brisque_input(q, "brisque_gray")
    B, _, h, w = x.shape
    y = torch.empty((B, h, w), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_brisque_gray", ops._p(x), ops._p(y), B, h, w, ops._stream())
    return y


def brisque_half(y: torch.Tensor) -> torch.Tensor:
    """fp64 (B,h,w) (or (h,w)) -> fp64 (B, round(h/2), round(w/2)) (half to even): skimage.transform.rescale(y, 1/2) with its
    defaults, restated as scipy's gaussian_filter(sigma 0.5, mirror) and zoom(order 1, grid mode).  The stage of
    brisque_features that is least certain to match imquality's, and the one to replace if it does not."""
    x = _brisque_plane(y, "brisque_half", BRISQUE_MIN)
    B, h, w = x.shape
    p = brisque_plan(h, w)
    tmp = torch.empty((2, B, h, w), dtype=torch.float64, device=x.device)
    out = torch.empty((B, p["h2"], p["w2"]), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_brisque_half", ops._p(x), ops._p(tmp), ops._p(out), B, h, w, ops._stream())
    return out


def brisque_mscn(y: torch.Tensor):
    """fp64 gray plane (B,h,w) (or (h,w)), or uint8 images (B,3,h,w) whose gray value is formed on the way -> (mscn fp64 (B,h,w),
    moments fp64 (B,tiles,5,6)): the locally normalised image (7 x 7 Gaussian of sigma 7/6, zero fill) and, per 32 x 32 tile
    in row-major order and per map (M, and M times its right, lower, lower-right and lower-left neighbour, where that exists),
    the count and sum of squares of the negatives, the same of the elements >= 0, sum |v| and sum v^2.  A stage of
    brisque_features."""
    rgb = isinstance(y, torch.Tensor) and y.dtype == torch.uint8
    x = _brisque_input(y, "brisque_mscn") if rgb else _brisque_plane(y, "brisque_mscn", BRISQUE_MIN // 2)
    B, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    tiles = -(-h // 32) * -(-w // 32)
    m = torch.empty((B, h, w), dtype=torch.float64, device=x.device)
    mom = torch.empty((B, tiles, 5, 6), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_brisque_moments", ops._p(x), int(not rgb), ops._p(m), ops._p(mom), B, h, w, ops._stream())
    return m, mom


def brisque_fit(moments: torch.Tensor) -> torch.Tensor:
    """moments fp64 (B,tiles,5,6) -> the 18 features of one scale (B,18) fp64: the tiles' sums added in a fixed order and the
    asymmetric generalised Gaussian fitted to each map, its shape the root of the moment ratio in [0.05, 100].  A map with an
    empty side or no variance gives NaN.  A stage of brisque_features."""
    _on_device(moments)
    if moments.dtype != torch.float64 or moments.dim() != 4 or tuple(moments.shape[-2:]) != (5, 6) or moments.shape[1] < 1:
        raise RuntimeError(f"brisque_fit: expected fp64 (B,tiles,5,6) moments, got {moments.dtype} {tuple(moments.shape)}")
    mom = moments.contiguous()
    B, tiles = mom.shape[:2]
    feat = torch.empty((B, 18), dtype=torch.float64, device=mom.device)
    with torch.cuda.device(mom.device):
        lib().call("cidnet_metric_brisque_fit", ops._p(mom), tiles, ops._p(feat), 18, B, ops._stream())
    return feat


def brisque_features(q: torch.Tensor) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) on the device, h, w >= 16 -> (B,36) fp64 on the device: the 18 features of the gray image and
    the 18 of its half-size version, per scale [alpha, variance] of M and [alpha, mean, left variance, right variance] of H, V,
    D1, D2 (include/cidnet_hip.h: BRISQUE).  NaN where a fit has an empty side or no variance -- an exactly flat image."""
    x = _brisque_input(q, "brisque_features")
    B, _, h, w = x.shape
    n = lib().raw("cidnet_metric_brisque_ws_floats")(B, h, w)
    if n <= 0:
        raise ValueError(f"brisque_features: {B} images of {h} x {w} are outside the kernels' limits (h w <= 2^26, B <= 65535)")
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    feat = torch.empty((B, BRISQUE_FEATURES), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_metric_brisque_features", ops._p(x), ops._p(feat), ops._p(ws), n, B, h, w, ops._stream())
    return feat


def brisque_score(features: torch.Tensor, params) -> torch.Tensor:
    """(B,36) fp64 features on the device -> (B,) fp64 on the device: the features scaled to [-1, 1] by the model's ranges, then
    libsvm's epsilon-SVR decision sum_i coef_i exp(-gamma |sv_i - z|^2) - rho over the support vectors in file order.
    params: a BrisqueParams or the (model, range) pair of paths.  NaN features give NaN."""
    prm = _brisque_params(params)
    if not isinstance(features, torch.Tensor):
        raise RuntimeError("brisque_score: expected a tensor")
    _on_device(features)
    if features.dtype != torch.float64 or features.dim() != 2 or features.shape[1] != BRISQUE_FEATURES or features.shape[0] < 1:
        raise RuntimeError(f"brisque_score: expected fp64 (B,36) features, got {features.dtype} {tuple(features.shape)}")
    f = features.contiguous()
    sv, coef, fmin, fmax, rg = prm.on(f.device)
    out = torch.empty(f.shape[0], dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        lib().call("cidnet_metric_brisque_svr", ops._p(f), ops._p(sv), ops._p(coef), ops._p(fmin), ops._p(fmax), ops._p(rg),
                   coef.shape[0], ops._p(out), f.shape[0], ops._stream())
    return out


def brisque(q_u8: torch.Tensor, params) -> torch.Tensor:
    """uint8 (B,3,h,w) (or (3,h,w)) on the device -> (B,) fp64 on the device, no host synchronisation: the BRISQUE score of each
    image as imquality.brisque.score states it (measure_niqe_bris.py:26), restated stage by stage from that package's
    description and pinned to scipy / scikit-learn, not to imquality itself.  params: a BrisqueParams or the
    (libsvm model, range file) pair of paths -- the user's own files.  An exactly flat image scores NaN; in a partly flat one the
    side of zero its rounding noise falls on follows the summation order, here as on the host."""
    prm = _brisque_params(params)
    return brisque_score(brisque_features(q_u8), prm)
