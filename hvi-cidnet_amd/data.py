"""Training batches on the device: the stage of the reference's train.py in front of the step -- data/data.py's transform1
(RandomCrop, RandomHorizontalFlip, RandomVerticalFlip, ToTensor), the DataLoader / DistributedSampler around it and
`im1 ** gamma` (train.py:54-56) -- from a training set that is decoded once and kept on the device as uint8.

    from hvi_cidnet_amd import ResidentPairs, TrainBatches
    pairs = ResidentPairs.from_folders(low_dir, high_dir, device)          # or ResidentPairs(lows, highs, device, gt_index)
    batches = TrainBatches(pairs, batch_size=8, crop=256, seed=0, gamma=(60, 120))
    for e in range(epochs):
        for x, gt in batches.epoch(e):                                      # one cidnet:: kernel launch per batch
            trainer.step(x, gt)

A batch is one launch of csrc/augment.hip (C ABI: cidnet_augment_crop_flip, semantics in include/cidnet_hip.h): both fp32
tensors, crop + flips + / 255 + gamma power, straight from the uint8 arena.  The power is a 256-entry table per batch, built
here in fp64 and rounded once (gamma_table); the division is a correctly rounded fp32 division, as ToTensor's .div(255).
Everything random is drawn on the host by epoch_plan(), a pure function of (seed, epoch, rank, world): an epoch's plan rows
and gamma tables go to the device in ONE copy, and the loop over the batches never synchronises with the host.

Every plan row is range-checked on the host where it is made (epoch_plan by construction, crop_flip explicitly); the kernel
cannot check a device-resident plan and trusts it.

Differences from the reference, none of which changes the distribution of a batch:
  * own stream of random numbers: the reference seeds python's `random`, numpy and torch per sample and lets torchvision
    draw; torchvision's draw order is not reproduced.  Same distribution (crop origin uniform over the legal origins, each
    flip with probability 1/2, gamma = randint(start, end) / 100 with both ends included), own stream;
  * files are paired by metrics.folder_pairs' rule with names sorted, where data/LOLdataset.py indexes os.listdir() order;
  * an epoch has the set's real length, where the reference's dataset classes hard-code 485 / 685 / 900;
  * low image and ground truth share crop origin and flips by construction (the reference reseeds between its two
    transform calls to get exactly that);
  * with several ranks the permutation is padded by wrapping to world * ceil(N / world), as DistributedSampler does.

The sets kept as one sub-folder per scene (data/SICE_blur_SID.py: LOLBlurDatasetFromFolder, SIDDatasetFromFolder,
SICEDatasetFromFolder) train from the same arena:

    pairs = ResidentPairs.from_scene_folders(low_root, high_root, device, gt="label")      # "name" LOL-Blur, "first" SID
    batches = TrainBatches(pairs, batch_size=8, crop=256, gamma=(60, 120), sampling="scene")

scene_pairs() pairs the files (a scene's label is decoded and stored once), scene_epoch_plan() draws every sample in the
reference's two stages -- a scene uniformly, then one of its images uniformly, independently and with replacement -- and
returns an ordinary EpochPlan, so the rows and the launch are the ones above.  An epoch has `samples` draws, by default the
number of low images in the scenes, where the reference hard-codes 10200 / 2099 / 4803; every rank draws the same list and
takes every world-th entry.

TrainBatches(raw=True) yields (x, gt, raw): raw is the low image WITHOUT the power, which train_tnsm.py:55,68 keeps for the
noise-consistency term of its loss while the network is fed `im1 ** gamma` (dp.DataParallelTrainer.step(x, gt, raw_input=raw);
fit.run_epoch passes it on).  With gamma on the three tensors come from one launch of cidnet_augment_crop_flip_raw, which
reads the low image once; with gamma off raw IS x.
"""
from __future__ import annotations

import concurrent.futures as cf
import ctypes
import math
import os
import warnings
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from . import metrics, ops
from ._lib import lib

_NO_CPU = metrics._NO_CPU
PLAN_WORDS = 8                    # int64 words per plan row (include/cidnet_hip.h)
ARENA_ALIGN = 16                  # every image starts on a 16-byte boundary of the arena
_TABLE_WORDS = 256 * 4 // 8       # a 256-entry fp32 table, in int64 words of the upload buffer


def _name(names, i):
    return f"'{names[i]}'" if names is not None else f"#{i}"


# ---- the arena (pure host code) ----------------------------------------------------------------------------------------
@dataclass
class ArenaLayout:
    """Where every image of the set lives in the uint8 arena: planar (3,h,w) at a byte offset"""
    low_offsets: list             # byte offset of low image i
    high_offsets: list            # byte offset of ground truth k (each stored once)
    gt_index: list                # ground truth of low image i
    sizes: list                   # (h, w) of low image i (= the size of its ground truth)
    total_bytes: int

    def gt_offset(self, i):
        return self.high_offsets[self.gt_index[i]]


def arena_layout(low_sizes, high_sizes, gt_index=None, max_bytes=None, names=None) -> ArenaLayout:
    """Lay out a set: low_sizes / high_sizes are (h, w) per image; gt_index[i] names the ground truth of low image i (default:
    the i-th).  Low images first, then the ground truths, each 3 h w bytes at a multiple of 16.  Raises ValueError for a pair
    whose sizes differ and for a set larger than max_bytes (sizes in the message)."""
    low_sizes = [(int(h), int(w)) for h, w in low_sizes]
    high_sizes = [(int(h), int(w)) for h, w in high_sizes]
    if gt_index is None:
        if len(low_sizes) != len(high_sizes):
            raise ValueError(f"{len(low_sizes)} low images but {len(high_sizes)} ground truths (pass gt_index to share them)")
        gt_index = list(range(len(low_sizes)))
    gt_index = [int(k) for k in gt_index]
    if len(gt_index) != len(low_sizes):
        raise ValueError(f"gt_index has {len(gt_index)} entries for {len(low_sizes)} low images")
    if not low_sizes:
        raise ValueError("empty set")
    for i, k in enumerate(gt_index):
        if not 0 <= k < len(high_sizes):
            raise ValueError(f"gt_index[{i}] = {k} outside the {len(high_sizes)} ground truths")
        if low_sizes[i] != high_sizes[k]:
            raise ValueError(f"pair {_name(names, i)}: low image is {low_sizes[i][0]} x {low_sizes[i][1]}, its ground truth "
                             f"(#{k}) is {high_sizes[k][0]} x {high_sizes[k][1]}")
    for what, sizes in (("low image", low_sizes), ("ground truth", high_sizes)):
        for i, (h, w) in enumerate(sizes):
            if h <= 0 or w <= 0:
                raise ValueError(f"{what} #{i} has size {h} x {w}")
    off, offsets = 0, []
    for h, w in low_sizes + high_sizes:
        offsets.append(off)
        off += -(-3 * h * w // ARENA_ALIGN) * ARENA_ALIGN
    if max_bytes is not None and off > max_bytes:
        raise ValueError(f"the set needs {off} bytes on the device ({len(low_sizes)} low images, {len(high_sizes)} ground "
                         f"truths), more than max_bytes = {int(max_bytes)}")
    n = len(low_sizes)
    return ArenaLayout(offsets[:n], offsets[n:], gt_index, low_sizes, off)


def _chw_u8(img) -> torch.Tensor:
    """-> contiguous uint8 (3,h,w) CPU tensor.  numpy arrays and PIL images are HWC, tensors CHW (HWC when only that fits)"""
    if hasattr(img, "convert"):
        img = np.array(img.convert("RGB"))
    hwc = isinstance(img, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(img)) if hwc else img
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError(f"expected a uint8 (h,w,3) array or (3,h,w) tensor, got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    if t.is_cuda:
        t = t.cpu()
    if hwc or (t.shape[0] != 3 and t.shape[-1] == 3):
        t = t.permute(2, 0, 1)
    if t.shape[0] != 3:
        raise ValueError(f"expected 3 colour channels, got {tuple(t.shape)}")
    return t.contiguous()


def check_groups(groups, count) -> list:
    """-> [(sub, [int indices])]: the scenes of a set of `count` low images, validated (ValueError): every index in range, no
    scene empty, every low image in at most one scene.  A low image in no scene is legal and is never drawn."""
    out, owner = [], {}
    for entry in groups:
        sub, members = entry
        members = [int(i) for i in members]
        if not members:
            raise ValueError(f"groups: scene '{sub}' is empty")
        for i in members:
            if not 0 <= i < count:
                raise ValueError(f"groups: scene '{sub}' names image {i}, outside the {count} low images of the set")
            if i in owner:
                raise ValueError(f"groups: image {i} is listed twice (scene '{owner[i]}' and scene '{sub}')")
            owner[i] = sub
        out.append((sub, members))
    if not out:
        raise ValueError("groups: no scene")
    return out


def scene_pairs(low_root: str, high_root: str, gt: str = "name") -> metrics.FolderPairs:
    """The training sets kept as one sub-folder per scene (data/SICE_blur_SID.py) -> metrics.FolderPairs with names
    "<sub>/<file>" and .groups = [(sub, [indices])], one entry per sub-folder that has pairs.  gt="name" (LOL-Blur: the same
    file name in high_root/<sub>/) and gt="first" (SID: the first image file of high_root/<sub>/) are
    metrics.nested_folder_pairs; gt="label" (SICE) pairs every image of low_root/<sub>/ with the file high_root/<sub><ext>,
    <ext> the first of metrics.GT_EXTENSIONS that exists.  A scene without a label is skipped and reported as
    nested_folder_pairs reports its skips (a warning and .skipped)."""
    if gt in ("name", "first"):
        return metrics.nested_folder_pairs(low_root, high_root, gt=gt)
    if gt != "label":
        raise ValueError(f"scene_pairs: gt must be 'name', 'first' or 'label' (got {gt!r})")
    paths, names, skipped, groups = [], [], [], []
    for sub in sorted(d for d in os.listdir(low_root) if os.path.isdir(os.path.join(low_root, d))):
        low_dir = os.path.join(low_root, sub)
        label = next((p for p in (os.path.join(high_root, sub + e) for e in metrics.GT_EXTENSIONS) if os.path.isfile(p)), None)
        members = []
        for f in metrics._image_files(low_dir):
            if label is None:
                skipped.append(f"{sub}/{f}")
                continue
            members.append(len(paths))
            paths.append((os.path.join(low_dir, f), label))
            names.append(f"{sub}/{f}")
        if members:
            groups.append((sub, members))
    if skipped:
        warnings.warn(f"scene_pairs: no ground truth under {high_root} for {len(skipped)} image(s): {', '.join(skipped)}")
    pairs = metrics.FolderPairs(paths, names, skipped)
    pairs.groups = groups
    return pairs


class ResidentPairs:
    """A paired training set on the device: one uint8 arena holding every image as planar (3,h,w), plus the host-side table
    of offsets and sizes (`layout`).  lows / highs: uint8 images, (h,w,3) arrays / PIL images or (3,h,w) tensors, of any
    sizes; gt_index[i] names the ground truth of low image i, so a label shared by many exposures is stored once.
    max_bytes: refuse a larger set (default: a quarter of the device's memory).  groups: None, or the scenes of the set as
    [(sub, [indices of its low images])] (what TrainBatches(sampling="scene") draws from): indices in range, no scene empty,
    a low image in at most one scene, else ValueError."""

    def __init__(self, lows, highs, device, gt_index=None, max_bytes=None, names=None, groups=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        lows = [_chw_u8(a) for a in lows]
        highs = [_chw_u8(a) for a in highs]
        if max_bytes is None:
            max_bytes = torch.cuda.get_device_properties(device).total_memory // 4
        self.names = list(names) if names is not None else None
        self.groups = check_groups(groups, len(lows)) if groups is not None else None
        self.layout = arena_layout([t.shape[1:] for t in lows], [t.shape[1:] for t in highs], gt_index, max_bytes, self.names)
        self.device = device
        self.skipped = []
        self.arena = torch.empty(self.layout.total_bytes, dtype=torch.uint8, device=device)
        for t, off in zip(lows + highs, self.layout.low_offsets + self.layout.high_offsets):
            self.arena[off:off + t.numel()].copy_(t.reshape(-1))            # host-to-device copies: no kernel

    @classmethod
    def from_folders(cls, low_dir, high_dir, device, max_bytes=None, threads=16):
        """Pair the image files of low_dir with their ground truths in high_dir by metrics.folder_pairs' rule (names sorted),
        decode each file once through PIL's .convert('RGB') on at most 16 threads, and keep the set on `device`.  A ground
        truth named by several low images is stored once.  `skipped`: low images without a ground truth."""
        if torch.device(device).type != "cuda":
            raise RuntimeError(_NO_CPU)
        fp = metrics.folder_pairs(low_dir, high_dir)
        if len(fp) == 0:
            raise ValueError(f"no image of {low_dir} has a ground truth in {high_dir}")
        return cls._from_pairs(fp, device, max_bytes, threads)

    @classmethod
    def from_scene_folders(cls, low_root, high_root, device, gt="name", max_bytes=None, threads=16):
        """The sets kept as one sub-folder per scene, paired by scene_pairs(low_root, high_root, gt) and decoded as
        from_folders does; a ground truth shared by a scene (gt="first", gt="label") is decoded and stored once.  names are
        "<sub>/<file>", `groups` the scenes (TrainBatches(sampling="scene")), `skipped` the low images without a ground
        truth.  A low image whose size differs from its label's raises (arena_layout)."""
        if torch.device(device).type != "cuda":
            raise RuntimeError(_NO_CPU)
        fp = scene_pairs(low_root, high_root, gt)
        if len(fp) == 0:
            raise ValueError(f"no image under {low_root} has a ground truth under {high_root} (gt={gt!r})")
        return cls._from_pairs(fp, device, max_bytes, threads, groups=fp.groups)

    @classmethod
    def _from_pairs(cls, fp, device, max_bytes, threads, groups=None):
        high_paths, slot, gt_index = [], {}, []
        for _, gp in fp.paths:
            if gp not in slot:
                slot[gp] = len(high_paths)
                high_paths.append(gp)
            gt_index.append(slot[gp])
        with cf.ThreadPoolExecutor(max_workers=max(1, min(16, int(threads), os.cpu_count() or 1))) as ex:
            images = list(ex.map(metrics._read_rgb, [lp for lp, _ in fp.paths] + high_paths))
        n = len(fp.paths)
        self = cls(images[:n], images[n:], device, gt_index=gt_index, max_bytes=max_bytes, names=fp.names, groups=groups)
        self.skipped = list(fp.skipped)
        return self

    def __len__(self):
        return len(self.layout.sizes)

    @property
    def sizes(self):
        return self.layout.sizes

    def low(self, i) -> torch.Tensor:
        """uint8 (3,h,w) view of low image i in the arena"""
        h, w = self.layout.sizes[i]
        off = self.layout.low_offsets[i]
        return self.arena[off:off + 3 * h * w].view(3, h, w)

    def high(self, i) -> torch.Tensor:
        """uint8 (3,h,w) view of the ground truth of low image i"""
        h, w = self.layout.sizes[i]
        off = self.layout.gt_offset(i)
        return self.arena[off:off + 3 * h * w].view(3, h, w)


# ---- the plan (pure host code) -----------------------------------------------------------------------------------------
def _crop_hw(crop):
    sh, sw = (crop, crop) if isinstance(crop, int) else (int(crop[0]), int(crop[1]))
    if sh <= 0 or sw <= 0:
        raise ValueError(f"crop {crop!r}: sizes must be positive")
    return sh, sw


@dataclass
class EpochPlan:
    """One rank's epoch: a row per sample in the order drawn, and the batches that cut them"""
    crop: tuple                   # (S_h, S_w)
    index: torch.Tensor           # (n,) int64: low image of each sample
    y0: torch.Tensor              # (n,) int64
    x0: torch.Tensor              # (n,) int64
    hflip: torch.Tensor           # (n,) bool
    vflip: torch.Tensor           # (n,) bool
    batches: list                 # (lo, hi) sample ranges, one per step
    gammas: list                  # one float per step, or None (gamma off)

    def __len__(self):
        return len(self.batches)


def _epoch_seed(seed, epoch):
    """(seed, epoch) mixed into one generator seed (splitmix64's finaliser): the CPU generator keeps only the low 32 bits of
    what it is given, so both have to reach them"""
    m = (1 << 64) - 1
    z = ((int(seed) & 0xFFFFFFFF) << 32 | (int(epoch) & 0xFFFFFFFF)) + 0x9E3779B97F4A7C15 & m
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & m
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & m
    return (z ^ (z >> 31)) & 0x7FFFFFFFFFFFFFFF


def epoch_plan(sizes, crop, batch_size, seed=0, epoch=0, rank=0, world=1, shuffle=True, drop_last=False, gamma=None,
               names=None) -> EpochPlan:
    """Everything random of one rank's epoch, drawn on the host from a torch.Generator seeded with (seed, epoch).  sizes:
    (h, w) per image.  The permutation and the per-sample draws are the same on every rank; the permutation is padded by
    wrapping to world * ceil(N / world) and rank r takes positions r, r + world, ..., so every rank runs the same number of
    steps with the same shapes.  y0 is uniform on [0, h - S_h], x0 on [0, w - S_w], each flip has probability 1/2; gamma =
    (start, end) draws randint(start, end) / 100 per batch and rank, both ends included.  drop_last drops a short last batch.
    An image smaller than the crop raises ValueError."""
    sh, sw = _crop_hw(crop)
    sizes = [(int(h), int(w)) for h, w in sizes]
    n, world, rank, batch_size = len(sizes), int(world), int(rank), int(batch_size)
    if n == 0:
        raise ValueError("epoch_plan: empty set")
    if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f"epoch_plan: batch_size {batch_size}, rank {rank}, world {world}")
    for i, (h, w) in enumerate(sizes):
        if h < sh or w < sw:
            raise ValueError(f"image {_name(names, i)} is {h} x {w}, smaller than the {sh} x {sw} crop")
    g = torch.Generator(device="cpu")
    g.manual_seed(_epoch_seed(seed, epoch))
    perm = torch.randperm(n, generator=g) if shuffle else torch.arange(n)
    per_rank = -(-n // world)
    total = per_rank * world
    padded = perm.repeat(-(-total // n))[:total]
    return _rest_of_plan(g, padded, sizes, sh, sw, per_rank, rank, world, batch_size, drop_last, gamma)


def _rest_of_plan(g, padded, sizes, sh, sw, per_rank, rank, world, batch_size, drop_last, gamma) -> EpochPlan:
    """what follows the index list `padded` (world * per_rank samples, the same on every rank) in the generator's stream: crop
    origins, flips, per-batch gammas; then rank's share"""
    total = per_rank * world
    hw = torch.tensor(sizes, dtype=torch.int64)[padded]
    u = torch.rand((2, total), dtype=torch.float64, generator=g)
    span_y, span_x = hw[:, 0] - sh, hw[:, 1] - sw
    y0 = torch.minimum((u[0] * (span_y + 1).double()).floor().long(), span_y)
    x0 = torch.minimum((u[1] * (span_x + 1).double()).floor().long(), span_x)
    flips = torch.randint(0, 2, (2, total), generator=g).bool()
    mine = slice(rank, total, world)
    n_steps = per_rank // batch_size if drop_last else -(-per_rank // batch_size)
    batches = [(k * batch_size, min((k + 1) * batch_size, per_rank)) for k in range(n_steps)]
    gammas = None
    if gamma is not None:
        start, end = int(gamma[0]), int(gamma[1])
        if not 0 < start <= end:
            raise ValueError(f"gamma range {gamma!r}: expected 0 < start <= end (hundredths)")
        steps_all = -(-per_rank // batch_size)                   # drawn for every step, so drop_last does not shift the stream
        draws = torch.randint(start, end + 1, (steps_all, world), generator=g)
        gammas = [int(draws[k, rank]) / 100 for k in range(n_steps)]
    last = batches[-1][1] if batches else 0
    return EpochPlan((sh, sw), padded[mine][:last].clone(), y0[mine][:last].clone(), x0[mine][:last].clone(),
                     flips[0][mine][:last].clone(), flips[1][mine][:last].clone(), batches, gammas)


def scene_epoch_plan(groups, sizes, crop, batch_size, samples=None, seed=0, epoch=0, rank=0, world=1, drop_last=False,
                     gamma=None, names=None) -> EpochPlan:
    """One rank's epoch of a scene-folder set, drawn as data/SICE_blur_SID.py draws a sample: a scene uniformly over the
    scenes, then one of its images uniformly, independently and with replacement.  groups: [(sub, [indices])]
    (ResidentPairs.groups, scene_pairs().groups); sizes: (h, w) of every low image of the set.  samples: draws per epoch over
    all ranks, default the number of low images in the scenes; world * ceil(samples / world) are drawn from one
    torch.Generator seeded with (seed, epoch), the same list on every rank, and rank r takes positions r, r + world, ..., so
    every rank runs the same number of steps with the same shapes.  Crop origins, flips, per-batch gammas, drop_last and the
    error for an image smaller than the crop are epoch_plan's.  A pure function of its arguments."""
    sh, sw = _crop_hw(crop)
    sizes = [(int(h), int(w)) for h, w in sizes]
    world, rank, batch_size = int(world), int(rank), int(batch_size)
    groups = check_groups(groups, len(sizes))
    if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f"scene_epoch_plan: batch_size {batch_size}, rank {rank}, world {world}")
    samples = sum(len(m) for _, m in groups) if samples is None else int(samples)
    if samples <= 0:
        raise ValueError(f"scene_epoch_plan: samples must be positive (got {samples})")
    for _, members in groups:
        for i in members:
            if sizes[i][0] < sh or sizes[i][1] < sw:
                raise ValueError(f"image {_name(names, i)} is {sizes[i][0]} x {sizes[i][1]}, smaller than the {sh} x {sw} crop")
    g = torch.Generator(device="cpu")
    g.manual_seed(_epoch_seed(seed, epoch))
    per_rank = -(-samples // world)
    total = per_rank * world
    count = torch.tensor([len(m) for _, m in groups], dtype=torch.int64)
    start = torch.cumsum(count, 0) - count                       # where each scene's members begin in `flat`
    flat = torch.tensor([i for _, m in groups for i in m], dtype=torch.int64)
    scene = torch.randint(0, len(groups), (total,), generator=g)
    k = count[scene]
    member = torch.minimum((torch.rand(total, dtype=torch.float64, generator=g) * k.double()).floor().long(), k - 1)
    padded = flat[start[scene] + member]
    return _rest_of_plan(g, padded, sizes, sh, sw, per_rank, rank, world, batch_size, drop_last, gamma)


def gamma_table(gamma: float) -> np.ndarray:
    """(256,) fp32: pow(q / 255, gamma) for the 256 levels -- the quotient a correctly rounded fp32 division (ToTensor), the
    power in fp64, rounded to fp32 once.  gamma == 1 gives the quotients themselves, bit for bit."""
    gamma = float(gamma)
    if not gamma > 0 or not math.isfinite(gamma):
        raise ValueError(f"gamma must be positive and finite (got {gamma})")
    q = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.power(q.astype(np.float64), gamma).astype(np.float32)


def plan_rows(layout: ArenaLayout, index, y0, x0, hflip, vflip, crop) -> torch.Tensor:
    """(n, 8) int64 CPU tensor: the kernel's plan rows for these samples, every one range-checked here (ValueError)"""
    sh, sw = _crop_hw(crop)
    cols = [torch.as_tensor(v).reshape(-1).to(torch.int64).cpu() for v in (index, y0, x0, hflip, vflip)]
    n = cols[0].numel()
    if n == 0 or any(c.numel() != n for c in cols):
        raise ValueError(f"plan rows: {[c.numel() for c in cols]} values for index, y0, x0, hflip, vflip")
    idx, y0, x0, hf, vf = cols
    count = len(layout.sizes)
    bad = ((idx < 0) | (idx >= count)).nonzero()
    if bad.numel():
        raise ValueError(f"sample {int(bad[0])}: index {int(idx[bad[0]])} outside the {count} images of the set")
    hw = torch.tensor(layout.sizes, dtype=torch.int64)[idx]
    bad = ((y0 < 0) | (x0 < 0) | (y0 + sh > hw[:, 0]) | (x0 + sw > hw[:, 1])).nonzero()
    if bad.numel():
        k = int(bad[0])
        raise ValueError(f"sample {k}: the {sh} x {sw} window at (y0, x0) = ({int(y0[k])}, {int(x0[k])}) leaves image "
                         f"{int(idx[k])} ({int(hw[k, 0])} x {int(hw[k, 1])})")
    if ((hf != 0) & (hf != 1)).any() or ((vf != 0) & (vf != 1)).any():
        raise ValueError("flips must be 0 / 1")
    rows = torch.zeros((n, PLAN_WORDS), dtype=torch.int64)
    rows[:, 0] = torch.tensor(layout.low_offsets, dtype=torch.int64)[idx]
    rows[:, 1] = torch.tensor([layout.gt_offset(i) for i in range(count)], dtype=torch.int64)[idx]
    rows[:, 2:4] = hw
    rows[:, 4], rows[:, 5] = y0, x0
    rows[:, 6] = hf + 2 * vf
    return rows


def _pack(rows: torch.Tensor, tables) -> torch.Tensor:
    """plan rows and gamma tables in one int64 CPU buffer (one copy to the device): rows first, then 128 words per table"""
    n = rows.shape[0] * PLAN_WORDS
    buf = torch.empty(n + len(tables) * _TABLE_WORDS, dtype=torch.int64)
    buf[:n] = rows.reshape(-1)
    if tables:
        buf[n:].view(torch.float32).copy_(torch.from_numpy(np.stack(tables)).reshape(-1))
    return buf


def _launch(pairs, buf_ptr, row, table_word, b, sh, sw, raw=False):
    """one batch: samples row .. row + b - 1 of the uploaded plan at buf_ptr; table_word: word offset of its table or None.
    raw: the launch that also writes the un-powered low image -> (x, gt, raw)"""
    x = torch.empty((b, 3, sh, sw), dtype=torch.float32, device=pairs.device)
    gt = torch.empty((b, 3, sh, sw), dtype=torch.float32, device=pairs.device)
    plan = ctypes.c_void_p(buf_ptr + 8 * PLAN_WORDS * row)
    table = ctypes.c_void_p(buf_ptr + 8 * table_word) if table_word is not None else None
    if raw:
        r = torch.empty((b, 3, sh, sw), dtype=torch.float32, device=pairs.device)
        lib().call("cidnet_augment_crop_flip_raw", ops._p(pairs.arena), plan, table, ops._p(x), ops._p(r), ops._p(gt), b, sh, sw,
                   ops._stream())
        return x, gt, r
    lib().call("cidnet_augment_crop_flip", ops._p(pairs.arena), plan, table, ops._p(x), ops._p(gt), b, sh, sw, ops._stream())
    return x, gt


def _check_pairs(pairs):
    if not isinstance(pairs, ResidentPairs):
        raise TypeError(f"expected a ResidentPairs, got {type(pairs).__name__}")
    if not pairs.arena.is_cuda:
        raise RuntimeError(_NO_CPU)


def crop_flip(pairs: ResidentPairs, index, y0, x0, hflip, vflip, size, gamma: float = 1.0, raw: bool = False):
    """The batch kernel with explicit rows: sample k is the size = S | (S_h, S_w) window of pair index[k] at (y0[k], x0[k]),
    mirrored where hflip[k] / vflip[k] -> (x, gt), fp32 (B,3,S_h,S_w); x = (low / 255) ** gamma, gt = high / 255.  The rows
    (lists or CPU tensors) are checked on the host before anything is launched: ValueError for a window outside its image, an
    index out of range or gamma <= 0.  raw=True -> (x, gt, raw), raw = low / 255 without the power, all three from one launch
    of cidnet_augment_crop_flip_raw (at gamma 1 without a table: x and raw are then the same values in two tensors)."""
    _check_pairs(pairs)
    sh, sw = _crop_hw(size)
    rows = plan_rows(pairs.layout, index, y0, x0, hflip, vflip, (sh, sw))
    if not float(gamma) > 0:
        raise ValueError(f"gamma must be positive (got {gamma})")
    tables = [gamma_table(gamma)] if float(gamma) != 1.0 else []
    b = rows.shape[0]
    if 3 * b > 65535:
        raise ValueError(f"at most 21845 samples per launch (got {b})")
    with torch.cuda.device(pairs.device):
        buf = _pack(rows, tables).to(pairs.device)
        return _launch(pairs, buf.data_ptr(), 0, b * PLAN_WORDS if tables else None, b, sh, sw, raw=bool(raw))


class TrainBatches:
    """The training loop's source of (x, gt): len() steps per epoch; epoch(e) draws the epoch's plan on the host
    (epoch_plan), uploads it with one host-to-device copy and yields one batch per step, each from one kernel launch on the
    current stream into freshly allocated tensors (several steps may be in flight, so buffers are not recycled here).
    gamma: None, or (start, end) in hundredths as the reference's --start_gamma / --end_gamma.  With a process group (or an
    initialised default group) every rank takes its share of the same permutation.
    sampling: "permutation" (epoch_plan), or "scene" for a set with pairs.groups (scene_epoch_plan: a scene, then one of its
    images, with replacement; `shuffle` has no meaning there); samples: draws per epoch of "scene" sampling over all ranks
    (default: the number of low images in the scenes).  raw=True yields (x, gt, raw), raw being the low image without the
    gamma power (train_tnsm.py:55,68): one launch of cidnet_augment_crop_flip_raw per batch with gamma on; with gamma off the
    plain launch and raw is x itself, the same tensor."""

    def __init__(self, pairs, batch_size, crop, seed=0, gamma=None, shuffle=True, drop_last=False, process_group=None,
                 sampling="permutation", samples=None, raw=False):
        _check_pairs(pairs)
        if sampling not in ("permutation", "scene"):
            raise ValueError(f"sampling must be 'permutation' or 'scene' (got {sampling!r})")
        if sampling == "scene" and not getattr(pairs, "groups", None):
            raise ValueError("sampling='scene' needs a set with scenes: ResidentPairs.from_scene_folders or ResidentPairs(groups=)")
        if sampling == "permutation" and samples is not None:
            raise ValueError("samples= belongs to sampling='scene': a permutation has the set's length")
        self.sampling, self.samples, self.raw = sampling, None if samples is None else int(samples), bool(raw)
        self.pairs, self.batch_size, self.crop, self.seed = pairs, int(batch_size), _crop_hw(crop), int(seed)
        self.gamma, self.shuffle, self.drop_last = gamma, bool(shuffle), bool(drop_last)
        self.world, self.rank = 1, 0
        if process_group is not None or (dist.is_available() and dist.is_initialized()):
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        if 3 * self.batch_size > 65535:
            raise ValueError(f"at most 21845 samples per batch (got {batch_size})")
        self._steps = len(self.plan(0))

    def __len__(self):
        return self._steps

    def plan(self, epoch) -> EpochPlan:
        if self.sampling == "scene":
            return scene_epoch_plan(self.pairs.groups, self.pairs.sizes, self.crop, self.batch_size, samples=self.samples,
                                    seed=self.seed, epoch=epoch, rank=self.rank, world=self.world, drop_last=self.drop_last,
                                    gamma=self.gamma, names=self.pairs.names)
        return epoch_plan(self.pairs.sizes, self.crop, self.batch_size, seed=self.seed, epoch=epoch, rank=self.rank,
                          world=self.world, shuffle=self.shuffle, drop_last=self.drop_last, gamma=self.gamma,
                          names=self.pairs.names)

    def epoch(self, epoch):
        """generator of (x, gt) -- (x, gt, raw) with raw=True --, one per step of epoch `epoch`"""
        p = self.plan(epoch)
        if not p.batches:
            return
        rows = plan_rows(self.pairs.layout, p.index, p.y0, p.x0, p.hflip, p.vflip, p.crop)
        tables = [gamma_table(g) for g in p.gammas] if p.gammas is not None else []
        words = rows.shape[0] * PLAN_WORDS
        sh, sw = p.crop
        with torch.cuda.device(self.pairs.device):
            buf = _pack(rows, tables).to(self.pairs.device)      # the epoch's only host-to-device copy
        ptr = buf.data_ptr()
        for k, (lo, hi) in enumerate(p.batches):
            with torch.cuda.device(self.pairs.device):
                batch = _launch(self.pairs, ptr, lo, words + k * _TABLE_WORDS if tables else None, hi - lo, sh, sw,
                                raw=self.raw and bool(tables))
            yield (batch[0], batch[1], batch[0]) if self.raw and not tables else batch
