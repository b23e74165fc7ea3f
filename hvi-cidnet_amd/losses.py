"""Training losses on device ("next" rows f1 and f4 of SURVEY section 8): drop-ins for the reference's `L1Loss` and `SSIM`
(loss/losses.py:10-38, 166-190), `EdgeLoss` (:41-65) and `PerceptualLoss` (:68-161 over loss/vgg_arch.py:133-239) with
the same constructor arguments.  `CIDNetLoss` is the reference's training objective (train.py:61-65).  The pretrained
VGG19 weights cannot be fetched here (torchvision / network absent): `VGGFeatureExtractor` starts from build-owned
deterministic random weights and loads a torchvision `vgg19` state_dict when one is supplied."""
from collections import OrderedDict

import torch
import torch.nn as nn

from . import metrics, ops


class L1Loss(nn.Module):
    """mean(|pred - target|) * loss_weight (reduction='mean', the only mode train.py uses)."""

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"Unsupported reduction mode: {reduction}. hvi-cidnet_amd builds 'mean' (train.py:189)")
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("element-wise loss weights are not used by the reference's training loop")
        loss = ops.L1LossFn.apply(pred, target)
        return loss if self.loss_weight == 1.0 else loss * self.loss_weight


class SSIM(nn.Module):
    """(1 - mean SSIM map) * weight with the reference's 11x11 Gaussian window (sigma 1.5, zero padding)."""

    def __init__(self, window_size=11, size_average=True, weight=1.0):
        super().__init__()
        if window_size != 11 or not size_average:
            raise NotImplementedError("hvi-cidnet_amd builds the SSIM loss as train.py constructs it: window 11, size_average=True")
        self.window_size = window_size
        self.size_average = size_average
        self.weight = weight

    def forward(self, img1, img2):
        return ops.SSIMLossFn.apply(img1, img2, float(self.weight))


class EdgeLoss(nn.Module):
    """Laplacian-pyramid edge loss: mse(laplacian(x), laplacian(y)) * loss_weight (5x5 blur, replicate padding)."""

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        self.weight = loss_weight

    def forward(self, x, y):
        return ops.EdgeLossFn.apply(x, y, float(self.weight))


class VGGFeatureExtractor(nn.Module):
    """Parameter container with the reference's layout (loss/vgg_arch.py:133-239): `vgg_net.<convN_M>.weight / .bias`
    for the VGG19 prefix that reaches the deepest requested layer, buffers `mean` / `std`, everything frozen.
    torchvision's pretrained weights are not available offline; `load_torchvision_state_dict` takes a `vgg19().state_dict()`
    (keys `features.<i>.weight`) when the user has one."""

    def __init__(self, layer_name_list, vgg_type="vgg19", use_input_norm=True, range_norm=False, requires_grad=False,
                 remove_pooling=False, pooling_stride=2, seed=19):
        super().__init__()
        if vgg_type != "vgg19" or requires_grad or remove_pooling or pooling_stride != 2:
            raise NotImplementedError("hvi-cidnet_amd builds the extractor as train.py:192 constructs it: frozen vgg19, MaxPool2d(2, 2)")
        self.layer_name_list = list(layer_name_list)
        self.use_input_norm = use_input_norm
        self.range_norm = range_norm
        self.plan = ops.vgg_plan(self.layer_name_list)
        gen = torch.Generator().manual_seed(seed)          # identical on every rank, independent of the global RNG
        mods = OrderedDict()
        n_pool = 0
        for layer in self.plan:
            if layer == "pool":
                n_pool += 1
                mods[f"pool{n_pool}"] = nn.MaxPool2d(kernel_size=2, stride=2)
                continue
            name, ci, co = layer
            conv = nn.Conv2d(ci, co, kernel_size=3, padding=1)
            with torch.no_grad():                           # He-uniform, the scale real VGG activations live at
                bound = (6.0 / (9 * ci)) ** 0.5
                conv.weight.copy_((torch.rand(conv.weight.shape, generator=gen) * 2 - 1) * bound)
                conv.bias.copy_((torch.rand(co, generator=gen) * 2 - 1) * 0.05)
            mods[name] = conv
            mods[name.replace("conv", "relu")] = nn.ReLU(inplace=True)
        last = self.plan[-1][0].replace("conv", "relu")     # the reference cuts the stack at the deepest requested layer
        mods.pop(last)
        self.vgg_net = nn.Sequential(mods)
        for p in self.parameters():
            p.requires_grad = False
        if use_input_norm:
            self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def conv_params(self):
        out = []
        for layer in self.plan:
            if layer != "pool":
                conv = getattr(self.vgg_net, layer[0])
                out += [conv.weight, conv.bias]
        return out

    def load_torchvision_state_dict(self, sd):
        """sd: torchvision.models.vgg19().state_dict() (or its `features.` part)"""
        idx, mapped = 0, {}
        for layer in ops.VGG19_LAYERS:
            if layer == "pool":
                idx += 1
                continue
            mapped[layer[0]] = idx
            idx += 2                                        # conv, relu
        with torch.no_grad():
            for layer in self.plan:
                if layer == "pool":
                    continue
                conv = getattr(self.vgg_net, layer[0])
                i = mapped[layer[0]]
                conv.weight.copy_(sd.get(f"features.{i}.weight", sd.get(f"{i}.weight")))
                conv.bias.copy_(sd.get(f"features.{i}.bias", sd.get(f"{i}.bias")))


class PerceptualLoss(nn.Module):
    """Reference: PerceptualLoss, loss/losses.py:68-161, as train.py:192 builds it: layer_weights over 'convN_M' features
    (before the ReLU), criterion 'mse', no style term.  forward returns (percep_loss, None) like the reference."""

    def __init__(self, layer_weights, vgg_type="vgg19", use_input_norm=True, range_norm=True, perceptual_weight=1.0,
                 style_weight=0., criterion="l1"):
        super().__init__()
        if style_weight > 0:
            raise NotImplementedError("the style (Gram) term is never enabled by the reference's training loop (style_weight=0)")
        if criterion != "mse":
            raise NotImplementedError("hvi-cidnet_amd builds the criterion train.py:192 uses: 'mse'")
        self.perceptual_weight = perceptual_weight
        self.style_weight = style_weight
        self.layer_weights = dict(layer_weights)
        self.criterion_type = criterion
        self.vgg = VGGFeatureExtractor(list(layer_weights.keys()), vgg_type=vgg_type, use_input_norm=use_input_norm,
                                       range_norm=range_norm)

    def forward(self, x, gt):
        if not self.perceptual_weight > 0:
            return None, None
        names = list(self.layer_weights.keys())
        loss = ops.PerceptualLossFn.apply(x, gt.detach(), names, [float(self.layer_weights[k]) for k in names],
                                          float(self.perceptual_weight), self.vgg.range_norm, self.vgg.use_input_norm,
                                          *self.vgg.conv_params())
        return loss, None


class LPIPSLoss(nn.Module):
    """loss_weight * mean over the batch of lpips.LPIPS(net='alex')(x, gt, normalize=True): the AlexNet LPIPS that
    metrics.lpips reports, as a training term (include/cidnet_hip.h, "LPIPS training loss").  x, gt: fp32
    (B,3,h,w) on the device in [0, 1] (nothing is clamped), h, w >= 31; gt is detached, as PerceptualLoss detaches it, and the
    extractor is frozen, so the only gradient is d/dx.  forward returns a 0-dim fp32 tensor.
    params: a metrics.LpipsParams, or the (alexnet path, heads path) pair metrics.load_lpips_params reads; nothing is shipped.
    The parameters reach a device, and their data-gradient forms are made there, by prepare(device) -- which .to(device) /
    .cuda() call, and which CIDNetLoss calls with the model's device when it is built -- or else on the first call on that
    device.  Prepare before capturing a step: a captured step then holds no host-to-device copy and no host synchronisation.
    The term computes in fp32 under set_precision("bf16") and set_storage_dtype too: its kernels have no other form."""

    def __init__(self, params, loss_weight=1.0):
        super().__init__()
        self.params = metrics._lpips_params(params)
        self.loss_weight = float(loss_weight)

    def prepare(self, device):
        """upload the frozen parameters to `device` and form their data-gradient copies there (once per device)"""
        device = torch.device(device)
        if device.type != "cuda":
            return self
        with torch.cuda.device(device):
            self.params.on(device)
            self.params.dgrad_on(device)
        return self

    def _apply(self, fn, *args, **kwargs):
        # .to(device) / .cuda(): the module has no tensors of its own, so ask fn where it sends one
        moved = fn(torch.empty(0))
        if moved.is_cuda:
            self.prepare(moved.device)
        return super()._apply(fn, *args, **kwargs)

    def forward(self, x, gt):
        if x.dim() != 4 or x.shape[1] != 3 or gt.shape != x.shape:
            raise RuntimeError("LPIPSLoss expects two (B,3,H,W) images of the same shape")
        metrics.lpips_feature_sizes(*x.shape[-2:])              # ValueError under 31 x 31, before anything runs
        ops._check(x, gt)
        need = ops.needs_grad(x)
        self.prepare(x.device)                                  # a dictionary hit after the first time
        with torch.cuda.device(x.device):
            return ops.LpipsLossFn.apply(x, gt.detach(), self.params, self.loss_weight, metrics.LPIPS_LAYERS, need)


class FFTLoss(nn.Module):
    """loss_weight * F.l1_loss(view_as_real(rfft2(pred, norm=norm)), view_as_real(rfft2(target, norm=norm))): the L1 distance of
    the half spectra that MIMO-UNet / DeepRFT add to a restoration objective (include/cidnet_hip.h, "frequency-domain training
    loss").  pred, target: fp32 (B,C,H,W) on the device, any H, W from 1 to 2048; differentiable in both.
    norm: "backward" (unnormalised, torch's default) or "ortho".  forward returns a 0-dim fp32 tensor.  The term computes in
    fp32 under set_precision("bf16") and set_storage_dtype too: its kernels have no other form."""

    def __init__(self, loss_weight=1.0, norm="backward"):
        super().__init__()
        if norm not in ops.FFT_NORMS:
            raise ValueError(f"FFTLoss: norm must be 'backward' or 'ortho' (got {norm!r})")
        if not (0.0 <= float(loss_weight) < float("inf")):
            raise ValueError(f"FFTLoss: loss_weight must be finite and not negative (got {loss_weight!r})")
        self.loss_weight = float(loss_weight)
        self.norm = norm

    def forward(self, pred, target):
        if pred.dim() != 4 or target.shape != pred.shape:
            raise RuntimeError("FFTLoss expects two (B,C,H,W) tensors of the same shape")
        ops._check(pred, target)
        return ops.FFTLossFn.apply(pred, target, self.loss_weight, self.norm)


class CIDNetLoss(nn.Module):
    """loss_rgb + HVI_weight * loss_hvi with loss_* = L1 + SSIM + Edge + P_weight * Perceptual (train.py:61-65);
    defaults are data/options.py:56-59 (P_weight 1e-2 there; 0 here leaves the VGG term out, the round-1 objective).
    `model` supplies HVIT for the HVI-space terms, exactly as train.py calls `model.HVIT` on the output and on the ground
    truth.  The perceptual term is built as train.py:192 does: conv1_2 / conv2_2 / conv3_4 / conv4_4, 'mse'.
    lpips_weight > 0 (not in the reference; the default 0 builds nothing and leaves the objective as it is) adds
    lpips_weight * LPIPSLoss(lpips_params)(output_rgb, gt_rgb) to loss_rgb only -- LPIPS of an HVI map means nothing;
    lpips_params as LPIPSLoss takes them, and their absence is an error.  The term stays fp32 in the bf16 mode.
    fft_weight > 0 (not in the reference either; the default 0 builds nothing) adds FFTLoss(fft_weight, fft_norm) to loss_*:
    a signal-level term like L1 / SSIM / Edge, so it counts in RGB and, scaled by HVI_weight, in HVI space."""

    def __init__(self, model, L1_weight=1.0, D_weight=0.5, E_weight=50.0, HVI_weight=1.0, P_weight=0.0, tnsm_weight=0.0,
                 lpips_weight=0.0, lpips_params=None, fft_weight=0.0, fft_norm="backward"):
        super().__init__()
        if fft_weight < 0:
            raise ValueError(f"CIDNetLoss: fft_weight must not be negative (got {fft_weight!r})")
        self.fft = FFTLoss(loss_weight=fft_weight, norm=fft_norm) if fft_weight > 0 else None
        if lpips_weight > 0 and lpips_params is None:
            raise ValueError(metrics._LPIPS_NO_PARAMS)
        self.lpips = LPIPSLoss(lpips_params, loss_weight=lpips_weight) if lpips_weight > 0 else None
        if self.lpips is not None:
            p = next(iter(model.parameters()), None) if hasattr(model, "parameters") else None
            if p is not None:
                self.lpips.prepare(p.device)
        self.tnsm_weight = tnsm_weight
        self.l1 = L1Loss(loss_weight=L1_weight)
        self.ssim = SSIM(weight=D_weight)
        self.edge = EdgeLoss(loss_weight=E_weight)
        self.hvi_weight = HVI_weight
        self.p_weight = P_weight
        self.perceptual = PerceptualLoss({"conv1_2": 1, "conv2_2": 1, "conv3_4": 1, "conv4_4": 1}, perceptual_weight=1.0,
                                         criterion="mse") if P_weight > 0 else None
        self._hvit = model.HVIT

    def _terms(self, a, b):
        t = self.l1(a, b) + self.ssim(a, b) + self.edge(a, b)
        if self.perceptual is not None:
            t = t + self.p_weight * self.perceptual(a, b)[0]
        if self.fft is not None:
            t = t + self.fft(a, b)
        return t

    # dp.DataParallelTrainer passes the step's input as `im1=` to a loss function with this attribute
    wants_input = True

    def forward(self, output_rgb, gt_rgb, noise_map=None, im1=None):
        """`output_rgb`: the model's result -- a tensor, or CIDNet_TNSM's train-mode pair (rgb, fused noise map), which is
        unpacked here.  `noise_map`, `im1`: that second result and the RAW low-light image -- train_tnsm.py:69 uses im1 as
        loaded, before the optional `im1 ** gamma` the network is fed with (:55) -- with tnsm_weight > 0 they add
        train_tnsm.py:68-72's  tnsm_weight * (noise_consistency_loss + noise_smoothing_loss).  A positive tnsm_weight without
        a noise map raises: the reference's default is tnsm_weight = 1 (options.py:61) and silently training without the
        terms would be a different objective."""
        if isinstance(output_rgb, (tuple, list)):
            output_rgb, model_noise = output_rgb[0], output_rgb[1]
            noise_map = model_noise if noise_map is None else noise_map
        if self.tnsm_weight > 0 and noise_map is None:
            raise ValueError("CIDNetLoss(tnsm_weight > 0) needs the fused noise map: pass CIDNet_TNSM's train-mode result (rgb, noise) "
                             "or noise_map=...; a model in eval mode returns (rgb, None)")
        loss_hvi = self._terms(self._hvit(output_rgb), self._hvit(gt_rgb))
        loss_rgb = self._terms(output_rgb, gt_rgb)
        if self.lpips is not None:
            loss_rgb = loss_rgb + self.lpips(output_rgb, gt_rgb)
        loss = loss_rgb + self.hvi_weight * loss_hvi
        if self.tnsm_weight > 0:
            if im1 is None:
                raise ValueError("CIDNetLoss: the TNSM noise terms need the network input im1 (train_tnsm.py:69)")
            loss = loss + tnsm_noise_loss(noise_map, output_rgb, im1, self.tnsm_weight)
        return loss


def tnsm_noise_loss(noise_map, output_rgb, im1, weight=1.0):
    """weight * (noise_consistency_loss + noise_smoothing_loss), train_tnsm.py:68-72 (options.py:61: tnsm_weight = 1)"""
    return ops.TNSMNoiseLossFn.apply(noise_map, output_rgb, im1.detach(), float(weight))
