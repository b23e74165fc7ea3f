"""Image files in and out: what the reference's eval.py, eval_SID_blur.py, demo.py and app.py do around the model -- PIL image
-> ToTensor -> reflect pad to a multiple of 8 -> ** gamma -> model -> clamp -> crop -> ToPILImage -> save under the input's
file name -- with the image crossing the host link as 3 bytes per pixel in both directions and the model the only thing
between two launches of this package's own kernels.

    from hvi_cidnet_amd import ingest, egress, enhance_u8, enhance_folder
    x, (h, w) = ingest(img_u8, gamma=1.0)          # uint8 (B,h,w,3) on the device -> fp32 (B,3,Hp,Wp), Hp, Wp multiples of 8
    q = egress(model(x), (h, w))                   # fp32 (B,3,Hp,Wp) -> uint8 (B,h,w,3) on the device
    q = enhance_u8(model, img_u8, gamma=1.0, gated=False, alpha_s=1.3, gated2=False, alpha=1.0)
    report = enhance_folder(model, in_dir, out_dir, batch_size=8, threads=16)

Large images, opt-in (tile=None, the default everywhere, is the path above, untouched):
    plan = tile_plan(h, w, tile=1024, overlap=32)  # pure host code: overlapping windows of one shape over the padded image
    x = ingest_tiles(img_u8, plan, gamma=1.0)      # uint8 (h,w,3) on the device -> fp32 (n,3,th,tw), cut from the bytes
    q = egress_tiles(y, plan)                      # fp32 (n,3,th,tw) -> uint8 (h,w,3): blended by the plan's weights
    q = enhance_u8(model, img_u8, tile=1024, overlap=32, tile_batch=8)
    report = enhance_folder(model, in_dir, out_dir, tile=1024)
The contract of the tiled mode is "the model applied to each window, blended by the plan's weights".  CIDNet's channel attention
is global (the gram matrix and the q / k norms run over all pixels of a sample), so a tiled result is NOT the whole-image
result and nothing is claimed about their distance; the reference has no such mode.

Geometric self-ensemble, opt-in (ensemble=1, the default everywhere, is the path above, untouched, with no new launch):
    v = ensemble_views(x, first=0, count=4)        # fp32 (B,C,H,W) -> (B*4,C,H,W): views 0..3 (flips); first=4: (B*4,C,W,H)
    y = ensemble_merge(ya, yb, na=4)               # the results mapped back, summed in view order, / (na + nb)
    q = enhance_u8(model, img_u8, ensemble=8)      # 2: views {0,1}; 4: {0..3}; 8: all; the model runs once per view group
    report = enhance_folder(model, in_dir, out_dir, ensemble=8)
The contract is "the model applied to each view, mapped back, summed in a fixed order, divided by the count" (DESIGN.md 6.8);
the reference has no such mode.  Not combined with tile=.

The kernels are csrc/imageio.hip (C ABI: cidnet_image_ingest / cidnet_image_egress and their _tiles forms) and
csrc/ensemble.hip (cidnet_ensemble_views / cidnet_ensemble_merge), semantics in include/cidnet_hip.h.

PNG files from the device, opt-in (png="pillow", the default everywhere, is the path above, untouched, with no new launch):
    p = png_plan(h, w, segment_bytes=32768)        # host: rows per segment, segments, workspace bytes, slot capacity (a bound)
    streams, sizes = png_zlib_u8(q)                # uint8 (B,h,w,3) -> the zlib stream of each image's IDAT chunk, on the device
    data = png_file(h, w, stream_bytes)            # host: signature, IHDR, IDAT, IEND and the CRC-32s around one stream
    files = png_encode_u8(q)                       # the two together: a list of bytes (synchronises)
    report = enhance_folder(model, in_dir, out_dir, png="device")
The stream is "adaptive row filters, one dynamic-Huffman deflate block per segment of rows, literals only" (DESIGN.md 6.12,
csrc/png.hip): the files decode to exactly the pixels Pillow's would and are smaller than Pillow's on photographs; flat
synthetic content compresses badly (no LZ77: one bit per byte at the least).

JPEG files from the device, opt-in (jpeg="pillow", the default everywhere, is the path above, untouched, with no new launch):
    p = jpeg_encode_plan(h, w)                     # host: MCU grid, luma blocks, dummy blocks, workspace bytes, slot capacity
    streams, sizes = jpeg_scan_u8(q, quality=75)   # uint8 (B,h,w,3) -> each image's entropy-coded scan, on the device
    data = jpeg_file(h, w, 75, scan_bytes)         # host: the 623 bytes of framing, the scan, EOI
    files = jpeg_encode_u8(q, quality=75)          # the two together: a list of bytes (synchronises)
    report = enhance_folder(model, in_dir, out_dir, jpeg="device")
The file is Pillow's own -- Image.fromarray(a).save(f, 'JPEG', quality=q) at its defaults -- byte for byte (DESIGN.md 6.13,
csrc/jpegenc.hip): baseline, 4:2:0, the Annex K tables, one scan without restart markers.

enhance_folder is a pipeline; who owns what, and when:
  * decode workers (min(threads, 16)) read one file each through PIL's .convert('RGB') and write its bytes into a pinned
    per-image staging buffer that the main thread handed them; a buffer still too small is grown by the main thread;
  * the main thread is the only one that talks to the device.  Per batch: one non-blocking copy of 3 h w bytes per image on
    the upload stream, an event, the three stages of enhance_u8 on the current stream, an event, one non-blocking copy of the
    uint8 result into a pinned output buffer on the download stream, an event.  The two copy streams carry pinned copies
    and nothing else (concurrency rule);
  * encode workers wait for the download's event -- in the worker, never in the main thread -- and save through PIL;
  * at most `depth` batches are past the decode stage at any time.  A batch's staging buffers, device input and pinned output
    go back to the pool when every encode future of that batch has completed (which implies that its upload, its kernels
    and its download have); the main thread waits for futures only and never synchronises the device.
"""
from __future__ import annotations

import collections
import concurrent.futures as cf
import functools
import ctypes
import os
import struct
import threading
import time
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist

from . import metrics, ops
from ._lib import lib
from .data import gamma_table

_NO_CPU = metrics._NO_CPU
_tables = {}                      # (device index, gamma) -> the 256-entry table on the device


def padded_size(h, w, multiple=8):
    """(Hp, Wp) of inference.pad_to_multiple: ((h + f) // f) * f where h % f != 0, else h"""
    f = int(multiple)
    if f <= 0:
        raise ValueError(f"multiple must be positive (got {multiple})")
    return (((h + f) // f) * f if h % f else h), (((w + f) // f) * f if w % f else w)


def _check_reflect(h, w, Hp, Wp):
    if Hp - h > h - 1 or Wp - w > w - 1:
        raise ValueError(f"a {h} x {w} image cannot be reflect-padded to {Hp} x {Wp}: the pad must be smaller than the side")


def _table_on(device, gamma):
    gamma = float(gamma)
    if not gamma > 0:
        raise ValueError(f"gamma must be positive (got {gamma})")
    if gamma == 1.0:
        return None
    key = (device.index if device.index is not None else torch.cuda.current_device(), gamma)
    if key not in _tables:
        if len(_tables) >= 64:
            _tables.clear()
        _tables[key] = torch.from_numpy(gamma_table(gamma)).to(device)
    return _tables[key]


def _images_u8(images, what):
    """-> (B,h,w,3) uint8 whose images are dense (a batch stride >= 3 h w is kept: no copy)"""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise RuntimeError(f"{what}: expected a uint8 tensor, got {getattr(images, 'dtype', type(images).__name__)}")
    if not images.is_cuda:
        raise RuntimeError(_NO_CPU)
    t = images.unsqueeze(0) if images.dim() == 3 else images
    if t.dim() != 4 or t.shape[-1] != 3 or 0 in t.shape:
        raise RuntimeError(f"{what}: expected (B,h,w,3) or (h,w,3), got {tuple(images.shape)}")
    B, h, w, _ = t.shape
    dense = t.stride()[1:] == (3 * w, 3, 1) and (B == 1 or t.stride(0) >= 3 * h * w)
    return t if dense else t.contiguous()


def _ingest(t, table, multiple=8):
    B, h, w, _ = t.shape
    Hp, Wp = padded_size(h, w, multiple)
    _check_reflect(h, w, Hp, Wp)
    x = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        lib().call("cidnet_image_ingest", ops._p(t), t.stride(0) if B > 1 else 3 * h * w, ops._p(table), ops._p(x), B, h, w, Hp,
                   Wp, ops._stream())
    return x, (h, w)


def ingest(images_u8: torch.Tensor, gamma: float = 1.0, multiple: int = 8):
    """uint8 (B,h,w,3) (or (h,w,3)) on the device, as PIL / numpy hold an image -> (x, (h, w)): x fp32 (B,3,Hp,Wp) =
    pow(ToTensor(image), gamma), reflect-padded at the bottom and right to multiples of `multiple` (pad_to_multiple's
    arithmetic), from one kernel launch.  gamma != 1 goes through data.gamma_table (fp64 power, rounded once).  ValueError for
    gamma <= 0 and for an image too small to be reflected (pad >= side), before anything is launched."""
    if isinstance(images_u8, torch.Tensor) and not images_u8.is_cuda:
        raise RuntimeError(_NO_CPU)
    t = _images_u8(images_u8, "ingest")
    _check_reflect(t.shape[1], t.shape[2], *padded_size(t.shape[1], t.shape[2], multiple))
    return _ingest(t, _table_on(t.device, gamma), multiple)


def egress(out: torch.Tensor, size=None) -> torch.Tensor:
    """fp32 (B,3,Hp,Wp) (or (3,Hp,Wp)) on the device -> uint8 (B,h,w,3) on the device: the top-left (h, w) = `size` crop (default
    the whole image) of trunc(clamp(x, 0, 1) * 255.0f), interleaved as PIL takes it -- value for value metrics.to_uint8
    (eval.py:69-73 and ToPILImage).  NaN becomes 0."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
        raise RuntimeError(f"egress: expected an fp32 tensor (got {getattr(out, 'dtype', type(out).__name__)})")
    if not out.is_cuda:
        raise RuntimeError(_NO_CPU)
    x = metrics._batched(out, "egress")
    B, _, Hp, Wp = x.shape
    h, w = (Hp, Wp) if size is None else (int(size[0]), int(size[1]))
    if not (0 < h <= Hp and 0 < w <= Wp):
        raise RuntimeError(f"egress: crop {(h, w)} outside the {(Hp, Wp)} image")
    q = torch.empty((B, h, w, 3), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_image_egress", ops._p(x), ops._p(q), 3 * h * w, B, Hp, Wp, h, w, ops._stream())
    return q


# ---- self-ensemble: the dihedral views of the input, the model on each, the inverse-mapped results averaged -----------------
_ENSEMBLE = {1: (1, 0), 2: (2, 0), 4: (4, 0), 8: (4, 4)}         # ensemble -> (na, nb): views 0 .. na - 1 and 4 .. 4 + nb - 1


def _check_ensemble(ensemble, tile=None):
    """-> (na, nb), or ValueError: ensemble is 1, 2, 4 or 8 (an int), and only 1 goes with tile="""
    if isinstance(ensemble, bool) or not isinstance(ensemble, (int, np.integer)) or int(ensemble) not in _ENSEMBLE:
        raise ValueError(f"ensemble must be 1, 2, 4 or 8 (got {ensemble!r})")
    if int(ensemble) != 1 and tile is not None:
        raise ValueError(f"ensemble={ensemble} with tile=: the self-ensemble runs on whole images only")
    return _ENSEMBLE[int(ensemble)]


def _planes(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected an fp32 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
    if not t.is_cuda:
        raise RuntimeError(_NO_CPU)
    if t.dim() != 4 or 0 in t.shape:
        raise RuntimeError(f"{what}: expected (B,C,H,W), got {tuple(t.shape)}")
    return t.contiguous()


def ensemble_views(x: torch.Tensor, first: int, count: int) -> torch.Tensor:
    """fp32 (B,C,H,W) on the device -> (B * count, C, Ho, Wo): views first .. first + count - 1 of every image, image b's view
    first + v at index b * count + v.  View k in 0..7: if k & 1 reverse the columns, then if k & 2 reverse the rows, then if
    k & 4 transpose -- torch's flip(-1), flip(-2), transpose(-1, -2), bit for bit, from one launch.  The range lies wholly in
    0..3 ((Ho, Wo) = (H, W)) or wholly in 4..7 ((W, H)); anything else is a ValueError."""
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    x = _planes(x, "ensemble_views")
    first, count = int(first), int(count)
    if count < 1 or first < 0 or first + count > 8 or (first < 4) != (first + count <= 4):
        raise ValueError(f"ensemble_views: views {first} .. {first + count - 1} must lie inside 0..3 or inside 4..7")
    B, C, H, W = x.shape
    y = torch.empty((B * count, C, W, H) if first >= 4 else (B * count, C, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        lib().call("cidnet_ensemble_views", ops._p(x), ops._p(y), B, C, H, W, first, count, ops._stream())
    return y


def ensemble_merge(ya: torch.Tensor, yb: torch.Tensor = None, na: int = 4) -> torch.Tensor:
    """ya fp32 (B * na, C, H, W): views 0 .. na - 1 of B images as ensemble_views lays them out (or the model's results for
    them), na = 1..4 views per image; yb (B * nb, C, W, H): views 4 .. 4 + nb - 1, nb = 1..4 (taken from yb's batch), or None
    -> (B,C,H,W): per element acc = the view-0 value, then acc += every further view's value at the inverse-mapped position
    (the transpose undone first, then the flips), view number ascending (ya before yb), each one fp32 addition, then acc /
    (na + nb), a correctly rounded fp32 division.  No clamp: NaN and infinity propagate.  One launch."""
    for t in (ya, yb):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError(_NO_CPU)
    ya = _planes(ya, "ensemble_merge")
    na = int(na)
    if not 1 <= na <= 4 or ya.shape[0] % na:
        raise ValueError(f"ensemble_merge: na = {na} must be 1..4 and divide ya's batch of {ya.shape[0]}")
    B, (_, C, H, W), nb = ya.shape[0] // na, ya.shape, 0
    if yb is not None:
        yb = _planes(yb, "ensemble_merge")
        nb = yb.shape[0] // B
        if tuple(yb.shape) != (B * nb, C, W, H) or not 1 <= nb <= 4 or yb.device != ya.device:
            raise ValueError(f"ensemble_merge: yb {tuple(yb.shape)} does not hold 1..4 transposed views of each of the {B} images "
                             f"of ya {tuple(ya.shape)}")
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=ya.device)
    with torch.cuda.device(ya.device):
        lib().call("cidnet_ensemble_merge", ops._p(ya), na, ops._p(yb), nb, ops._p(out), B, C, H, W, ops._stream())
    return out


def _first(out):
    return out[0] if isinstance(out, tuple) else out             # CIDNet_TNSM: (rgb, noise map or None)


def _ensemble(fn, x, na, nb):
    """fn (the model, or a stage of it) on the views of x, one call per group, merged: always two calls when nb > 0, square
    image or not, so that an image's result does not depend on whether it happens to be square"""
    ya = _first(fn(ensemble_views(x, 0, na)))
    yb = _first(fn(ensemble_views(x, 4, nb))) if nb else None
    return ensemble_merge(ya, yb, na)


def _run(model, t, table, ensemble=(1, 0)):
    """ingest -> model -> egress of a checked (B,h,w,3) batch; the caller holds the model's state (metrics._eval_state).
    ensemble = (na, nb) other than (1, 0): ingest -> views -> model per group -> merge -> egress"""
    x, hw = _ingest(t, table)
    if ensemble != (1, 0):
        return egress(_ensemble(model, x, *ensemble), hw)
    out = model(x)
    if isinstance(out, tuple):                                   # CIDNet_TNSM: (rgb, noise map or None)
        out = out[0]
    return egress(out, hw)


# ---- tiles: the plan (pure host code), window ingest, blended egress ----------------------------------------------------------
@dataclass(eq=False)
class TilePlan:
    """Overlapping windows of one shape over the reflect-padded image (tile_plan).  size (h, w); padded (Hp, Wp); tile (th, tw);
    ys, xs: the window origins per axis, ascending; origins: (n, 2) int32 (y, x), row-major over ys x xs; wy (len(ys), th) and
    wx (len(xs), tw): fp32 blending weights per axis, strictly positive -- tile (ky, kx) weighs its pixel (i, j) with
    wy[ky, i] * wx[kx, j].  The arrays are read-only; the device copies are made once per device and kept with the plan."""
    size: tuple
    padded: tuple
    tile: tuple
    ys: tuple
    xs: tuple
    origins: np.ndarray
    wy: np.ndarray
    wx: np.ndarray
    _on: dict = field(default_factory=dict, repr=False)          # device index -> (origins, ys, xs, wy, wx) on that device

    def __len__(self):
        return len(self.ys) * len(self.xs)


def _axis_origins(P, t, overlap):
    """0, S, 2S, ... (S = t - overlap) while a tile fits, then one tile flush with the edge unless it repeats the last"""
    if t == P:
        return (0,)
    S = t - overlap
    o = list(range(0, P - t + 1, S))
    if o[-1] != P - t:
        o.append(P - t)
    return tuple(o)


def _axis_weights(o, t):
    """a_k(i) = min(1, (i + 1) / (l_k + 1), (t - i) / (r_k + 1)), l_k / r_k the overlap of tile k with tile k - 1 / k + 1 (0 at
    the ends): fp64, rounded once to fp32"""
    i = np.arange(t, dtype=np.float64)
    rows = []
    for k, y in enumerate(o):
        l = max(0, o[k - 1] + t - y) if k > 0 else 0
        r = max(0, y + t - o[k + 1]) if k + 1 < len(o) else 0
        rows.append(np.minimum(1.0, np.minimum((i + 1) / (l + 1), (t - i) / (r + 1))))
    a = np.stack(rows).astype(np.float32)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=64)
def _tile_plan(h, w, Th, Tw, overlap, multiple):
    if h <= 0 or w <= 0:
        raise ValueError(f"tile_plan: the image must be positive (got {(h, w)})")
    Hp, Wp = padded_size(h, w, multiple)
    _check_reflect(h, w, Hp, Wp)
    th, tw = min(Th, Hp), min(Tw, Wp)
    if (th < Hp or tw < Wp) and 2 * overlap > min(th, tw):
        raise ValueError(f"tile_plan: overlap {overlap} is more than half of the {(th, tw)} tile")
    ys, xs = _axis_origins(Hp, th, overlap), _axis_origins(Wp, tw, overlap)
    origins = np.array([(y, x) for y in ys for x in xs], dtype=np.int32).reshape(-1, 2)
    origins.flags.writeable = False
    return TilePlan((h, w), (Hp, Wp), (th, tw), ys, xs, origins, _axis_weights(ys, th), _axis_weights(xs, tw))


def _check_tile(tile, overlap, multiple=8):
    """what can be said of tile / overlap / multiple without an image -> (Th, Tw, overlap, multiple) as ints, or ValueError"""
    pair = tuple(tile) if isinstance(tile, (tuple, list)) else (tile, tile)
    if len(pair) != 2:
        raise ValueError(f"tile_plan: tile must be T or (Th, Tw) (got {tile!r})")
    Th, Tw, overlap, multiple = (_whole(v) for v in (*pair, overlap, multiple))
    if multiple <= 0:
        raise ValueError(f"multiple must be positive (got {multiple})")
    if Th <= 0 or Tw <= 0:
        raise ValueError(f"tile_plan: the tile must be positive (got {(Th, Tw)})")
    if Th % multiple or Tw % multiple:
        raise ValueError(f"tile_plan: the tile {(Th, Tw)} must be a multiple of {multiple}")
    if overlap < 0:
        raise ValueError(f"tile_plan: overlap must not be negative (got {overlap})")
    return Th, Tw, overlap, multiple


def _whole(v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer)) or v != v or v in (float("inf"), float("-inf")) \
            or int(v) != v:
        raise ValueError(f"tile_plan: sizes must be integers (got {v!r})")
    return int(v)


def tile_plan(h, w, tile, overlap=32, multiple=8) -> TilePlan:
    """The windows of a (h, w) image for the tiled mode.  (Hp, Wp) = padded_size(h, w, multiple); tile = T or (Th, Tw), multiples
    of `multiple`; (th, tw) = (min(Th, Hp), min(Tw, Wp)), so an image no larger than the tile is ONE tile of the padded image's
    own shape.  Per axis the origins are 0, S, 2S, ... with S = t - overlap while a tile fits, then one last tile flush with
    the edge (dropped when it repeats the previous one): every window lies inside the padded image, every pixel is covered, by
    at most three tiles per axis.  ValueError for a non-positive size, a tile that is no multiple, an image that cannot be
    reflected (pad >= side), a negative overlap, and 2 * overlap > min(th, tw) when there is more than one tile.  Plans are
    cached (the last 64), and with them their device copies: one buffer of 4 (2 n + ny + nx + ny th + nx tw) bytes each."""
    Th, Tw, overlap, multiple = _check_tile(tile, overlap, multiple)
    return _tile_plan(_whole(h), _whole(w), Th, Tw, overlap, multiple)


def _plan_on(plan, device):
    """the plan's origins (n,2), ys, xs (int32) and wy, wx (fp32) on the device.  Uploaded once per plan and device: one packed
    pinned buffer, one non-blocking copy on the current stream (nothing waits for the work already queued there); a later
    caller's stream waits for that copy's event."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in plan._on:
        parts = (plan.origins.reshape(-1), np.asarray(plan.ys, dtype=np.int32), np.asarray(plan.xs, dtype=np.int32),
                 plan.wy.reshape(-1).view(np.int32), plan.wx.reshape(-1).view(np.int32))
        host = torch.empty(sum(a.size for a in parts), dtype=torch.int32, pin_memory=True)
        np.concatenate(parts, out=host.numpy())
        with torch.cuda.device(key):
            buf = host.to(torch.device("cuda", key), non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
        o, ys, xs, wy, wx = torch.split(buf, [a.size for a in parts])
        tensors = (o.view(-1, 2), ys, xs, wy.view(torch.float32).view(len(plan.ys), -1), wx.view(torch.float32).view(len(plan.xs), -1))
        plan._on[key] = (tensors, copied, host)                  # host: alive until the copy has run
    tensors, copied, _ = plan._on[key]
    torch.cuda.current_stream(key).wait_event(copied)
    return tensors


def _ingest_tiles(img, table, plan, lo=0, hi=None):
    """tiles [lo, hi) of a checked dense (h,w,3) image -> (hi - lo,3,th,tw)"""
    hi = len(plan) if hi is None else hi
    h, w = plan.size
    th, tw = plan.tile
    x = torch.empty((hi - lo, 3, th, tw), dtype=torch.float32, device=img.device)
    origins = _plan_on(plan, img.device)[0][lo:hi]
    with torch.cuda.device(img.device):
        lib().call("cidnet_image_ingest_tiles", ops._p(img), h, w, ops._p(table), ops._p(origins), ops._p(x), hi - lo, th, tw,
                   ops._stream())
    return x


def _one_image(image_u8, plan, what):
    t = _images_u8(image_u8, what)
    if t.shape[0] != 1 or tuple(t.shape[1:3]) != tuple(plan.size):
        raise RuntimeError(f"{what}: the plan is for one {plan.size} image, got {tuple(image_u8.shape)}")
    return t[0]


def ingest_tiles(image_u8: torch.Tensor, plan: TilePlan, gamma: float = 1.0) -> torch.Tensor:
    """uint8 (h,w,3) (or (1,h,w,3)) on the device -> fp32 (n,3,th,tw): window t is ingest(image)[..., y:y+th, x:x+tw] at the
    plan's origin t, cut straight from the bytes in one launch (the padded fp32 image never exists)."""
    if isinstance(image_u8, torch.Tensor) and not image_u8.is_cuda:
        raise RuntimeError(_NO_CPU)
    img = _one_image(image_u8, plan, "ingest_tiles")
    return _ingest_tiles(img, _table_on(img.device, gamma), plan)


def egress_tiles(tiles: torch.Tensor, plan: TilePlan) -> torch.Tensor:
    """fp32 (n,3,th,tw) on the device, tile t at the plan's origin t -> uint8 (h,w,3) on the device: per pixel the weighted
    mean, by the plan's wy * wx, of clamp(v, 0, 1) over the tiles that cover it (fp32, ascending tile order), the clamped value
    itself where one tile covers it, then trunc(* 255.0f), interleaved.  NaN becomes 0.  A plan of one tile gives
    egress(tiles[0], (h, w))."""
    if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.float32:
        raise RuntimeError(f"egress_tiles: expected an fp32 tensor (got {getattr(tiles, 'dtype', type(tiles).__name__)})")
    if not tiles.is_cuda:
        raise RuntimeError(_NO_CPU)
    if tuple(tiles.shape) != (len(plan), 3, *plan.tile):
        raise RuntimeError(f"egress_tiles: expected {(len(plan), 3, *plan.tile)} for this plan, got {tuple(tiles.shape)}")
    tiles = tiles.contiguous()
    h, w = plan.size
    _, ys, xs, wy, wx = _plan_on(plan, tiles.device)
    q = torch.empty((h, w, 3), dtype=torch.uint8, device=tiles.device)
    with torch.cuda.device(tiles.device):
        lib().call("cidnet_image_egress_tiles", ops._p(tiles), ops._p(ys), len(plan.ys), ops._p(xs), len(plan.xs), ops._p(wy),
                   ops._p(wx), ops._p(q), h, w, *plan.tile, ops._stream())
    return q


def _run_tiled(model, img, table, plan, tile_batch):
    """window ingest -> the model over the tiles in chunks of tile_batch -> blended egress of a checked (h,w,3) image; the
    caller holds the model's state.  Every chunk has the same shape, except possibly the last."""
    n = len(plan)
    out = torch.empty((n, 3, *plan.tile), dtype=torch.float32, device=img.device)
    for lo in range(0, n, tile_batch):
        hi = min(n, lo + tile_batch)
        y = model(_ingest_tiles(img, table, plan, lo, hi))
        out[lo:hi] = y[0] if isinstance(y, tuple) else y
    return egress_tiles(out, plan)


def _tile_batch(tile_batch):
    if int(tile_batch) <= 0:
        raise ValueError(f"tile_batch must be positive (got {tile_batch})")
    return int(tile_batch)


def _trans_attrs(gated, alpha_s, gated2, alpha):
    return dict(gated=bool(gated), alpha_s=float(alpha_s), gated2=bool(gated2), alpha=float(alpha))


@torch.no_grad()
def enhance_u8(model, images_u8: torch.Tensor, gamma: float = 1.0, gated: bool = False, alpha_s: float = 1.3,
               gated2: bool = False, alpha: float = 1.0, tile=None, overlap: int = 32, tile_batch: int = 8,
               ensemble: int = 1) -> torch.Tensor:
    """uint8 (B,h,w,3) (or (h,w,3)) on the device -> the enhanced images, uint8 (B,h,w,3) on the device: ingest, the model in
    eval mode under no_grad with trans.gated / alpha_s / gated2 / alpha set (a tuple result -- CIDNet_TNSM -- gives its [0]),
    egress.  The model's attributes and the train / eval mode of every submodule are restored afterwards.
    tile = T or (Th, Tw): each image runs as tile_plan(h, w, tile, overlap) -> window ingest -> the model over the tiles in
    chunks of tile_batch -> blended egress; NOT the whole-image result (module docstring).  tile=None: the whole image.
    ensemble = 2, 4 or 8: geometric self-ensemble over views {0, 1}, {0..3} or {0..7} (ensemble_views) -- ingest, the views,
    the model once per view group (0..3, then 4..7) on a batch of B * views, ensemble_merge, egress.  1: no view is built.
    ValueError for any other value, and for ensemble != 1 together with tile=, before anything is launched."""
    views = _check_ensemble(ensemble, tile)
    if isinstance(images_u8, torch.Tensor) and not images_u8.is_cuda:
        raise RuntimeError(_NO_CPU)
    t = _images_u8(images_u8, "enhance_u8")
    _check_reflect(t.shape[1], t.shape[2], *padded_size(t.shape[1], t.shape[2]))
    table = _table_on(t.device, gamma)
    if tile is not None:
        plan, tile_batch = tile_plan(t.shape[1], t.shape[2], tile, overlap), _tile_batch(tile_batch)
        with metrics._eval_state(model, _trans_attrs(gated, alpha_s, gated2, alpha)), torch.cuda.device(t.device):
            return torch.stack([_run_tiled(model, img, table, plan, tile_batch) for img in t])
    with metrics._eval_state(model, _trans_attrs(gated, alpha_s, gated2, alpha)), torch.cuda.device(t.device):
        return _run(model, t, table, views)


# ---- PNG files: the IDAT stream from the device, the framing on the host ------------------------------------------------------
PNG_FILTERS = ("none", "sub", "up", "avg", "paeth", "adaptive")  # the position is the C ABI's filter code
_PNG_MODES = ("pillow", "device")


@dataclass(frozen=True)
class PngPlan:
    """cidnet_png_plan for one image size: rows per segment (the contract's R, not clipped to h), segments, whether the last
    one is short, whether a single row exceeds segment_bytes, workspace bytes per image, and capacity: a proven bound on one
    stream's size, the size of an output slot"""
    rows: int
    segments: int
    last_short: bool
    row_exceeds: bool
    ws_bytes: int
    capacity: int


def _check_png(png):
    if png not in _PNG_MODES:
        raise ValueError(f"png must be 'pillow' or 'device' (got {png!r})")
    return png


def _png_args(filter, segment_bytes):
    if filter not in PNG_FILTERS:
        raise ValueError(f"png: filter must be one of {PNG_FILTERS} (got {filter!r})")
    if isinstance(segment_bytes, bool) or not isinstance(segment_bytes, (int, np.integer)) or not 1 <= int(segment_bytes) < 2 ** 31:
        raise ValueError(f"png: segment_bytes must be an integer in 1 .. 2^31 - 1 (got {segment_bytes!r})")
    return PNG_FILTERS.index(filter), int(segment_bytes)


@functools.lru_cache(maxsize=256)
def _png_plan(h, w, segment_bytes):
    out = (ctypes.c_long * 6)()
    rc = lib().raw("cidnet_png_plan")(h, w, segment_bytes, out, 6)
    if rc != 0:
        raise ValueError(f"png_plan: a {h} x {w} image in segments of {segment_bytes} bytes is refused: "
                         + ("sizes must be positive" if rc == -1 else "a segment (or one row) of more than 2^22 bytes"))
    return PngPlan(int(out[0]), int(out[1]), bool(out[2]), bool(out[3]), int(out[4]), int(out[5]))


def png_plan(h, w, segment_bytes: int = 32768) -> PngPlan:
    """What png_zlib_u8 will do with (h, w) images: the library's own plan (host code, nothing is launched).  ValueError for a
    non-positive size and for a segment -- or a single row -- of more than 2^22 bytes."""
    return _png_plan(_whole(h), _whole(w), _png_args("adaptive", segment_bytes)[1])


def _png_zlib(t, code, segment_bytes):
    """checked (B,h,w,3) -> (buf, streams, sizes): one flat uint8 buffer holding sizes (int64 (B,), padded to 16 bytes) and
    then the B slots, and the two views into it -- one buffer so that one copy brings both to the host"""
    B, h, w, _ = t.shape
    plan = _png_plan(h, w, segment_bytes)
    head = (8 * B + 15) // 16 * 16
    buf = torch.empty(head + B * plan.capacity, dtype=torch.uint8, device=t.device)
    sizes, streams = buf[:8 * B].view(torch.int64), buf[head:].view(B, plan.capacity)
    ws = torch.empty(B * plan.ws_bytes, dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        lib().call("cidnet_png_encode_u8", ops._p(t), t.stride(0) if B > 1 else 3 * h * w, ops._p(streams), plan.capacity,
                   ops._p(sizes), ops._p(ws), ws.numel(), B, h, w, code, segment_bytes, ops._stream())
    return buf, streams, sizes


def png_zlib_u8(q: torch.Tensor, filter: str = "adaptive", segment_bytes: int = 32768):
    """uint8 (B,h,w,3) (or (h,w,3)) on the device, as egress writes it -> (streams uint8 (B, capacity), sizes int64 (B,)), both
    on the device, no synchronisation: streams[b, :sizes[b]] is the complete zlib stream of image b's IDAT chunk (png_file
    frames it), the rest of the slot is zero; capacity = png_plan(h, w, segment_bytes).capacity.  filter: "adaptive" (per row
    the type with the smallest sum of |signed filtered byte|, ties to the lowest) or one of "none", "sub", "up", "avg", "paeth"
    for every row.  segment_bytes: a deflate block takes max(1, segment_bytes // (1 + 3 w)) rows.  The bytes are those of
    tests/png_ref.py, identical from call to call and independent of the rest of the batch."""
    code, segment_bytes = _png_args(filter, segment_bytes)
    if isinstance(q, torch.Tensor) and not q.is_cuda:
        raise RuntimeError(_NO_CPU)
    t = _images_u8(q, "png_zlib_u8")
    _, streams, sizes = _png_zlib(t, code, segment_bytes)
    return streams, sizes


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def png_file(h, w, stream_bytes) -> bytes:
    """The PNG file around one zlib stream (host): signature, IHDR (8-bit, colour type 2, no interlace), one IDAT, IEND"""
    h, w = _whole(h), _whole(w)
    if not (0 < h < 2 ** 31 and 0 < w < 2 ** 31):
        raise ValueError(f"png_file: the image must be positive (got {(h, w)})")
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _png_chunk(b"IDAT", bytes(stream_bytes)) + _png_chunk(b"IEND", b""))


def png_encode_u8(q: torch.Tensor, filter: str = "adaptive", segment_bytes: int = 32768) -> list:
    """uint8 (B,h,w,3) (or (h,w,3)) on the device -> the B PNG files as bytes: png_zlib_u8, one download, png_file.  The
    convenience form: it synchronises."""
    streams, sizes = png_zlib_u8(q, filter, segment_bytes)
    h, w = (q.shape[-3], q.shape[-2])
    host, n = streams.cpu().numpy(), sizes.cpu().tolist()
    return [png_file(h, w, host[b, :n[b]].tobytes()) for b in range(len(n))]


# ---- JPEG files: the entropy-coded scan from the device, the framing on the host ------------------------------------------------
_JPEG_MODES = ("pillow", "device")
_JPEG_NAMES = (".jpg", ".jpeg")                                  # lower-cased: the names PIL saves as JPEG
# ITU T.81 Annex K.3 - K.6 as a DHT segment carries them: class / id, the number of codes of each length 1..16, the symbols
_JPEG_DC = bytes(range(12))
_JPEG_DHT = (
    (0x00, bytes.fromhex("00010501010101010100000000000000"), _JPEG_DC),
    (0x10, bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
        "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
        "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, bytes.fromhex("00030101010101010101010000000000"), _JPEG_DC),
    (0x11, bytes.fromhex("00020102040403040705040400010277"), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
        "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                47, 55, 62, 63)
JPEG_HEADER_BYTES = 623


@dataclass(frozen=True)
class JpegEncodePlan:
    """cidnet_jpeg_encode_plan for one image size: the MCU grid, the luma blocks libjpeg transforms (ceil(w/8) x ceil(h/8)),
    the dummy blocks of the edge MCUs beyond them, workspace bytes per image, capacity: a proven bound on one scan's size, the
    size of an output slot, and groups: the number of partial sums of the bit-offset scan (16 MCUs each)"""
    mcu_cols: int
    mcu_rows: int
    block_cols: int
    block_rows: int
    dummies: int
    ws_bytes: int
    capacity: int
    groups: int
    workgroups: int


def _check_jpeg(jpeg):
    if jpeg not in _JPEG_MODES:
        raise ValueError(f"jpeg must be 'pillow' or 'device' (got {jpeg!r})")
    return jpeg


@functools.lru_cache(maxsize=256)
def _jpeg_encode_plan(h, w):
    out = (ctypes.c_long * 9)()
    rc = lib().raw("cidnet_jpeg_encode_plan")(h, w, out, 9)
    if rc != 0:
        raise ValueError(f"jpeg_encode_plan: a {h} x {w} image is refused: "
                         + ("sizes must be positive" if rc == -1 else "a side above 65500 or more than 2^22 MCUs"))
    return JpegEncodePlan(*(int(v) for v in out))


def jpeg_encode_plan(h, w) -> JpegEncodePlan:
    """What jpeg_scan_u8 will do with (h, w) images: the library's own plan (host code, nothing is launched).  ValueError for a
    non-positive size, a side above 65500 (no such file exists) and more than 2^22 MCUs."""
    return _jpeg_encode_plan(_whole(h), _whole(w))


def _jpeg_scan(t, quality):
    """checked (B,h,w,3) -> (buf, streams, sizes): one flat uint8 buffer holding sizes (int64 (B,), padded to 16 bytes) and
    then the B slots, and the two views into it"""
    B, h, w, _ = t.shape
    plan = _jpeg_encode_plan(h, w)
    qplan = metrics.jpeg_quant_plan(quality)
    head = (8 * B + 15) // 16 * 16
    buf = torch.empty(head + B * plan.capacity, dtype=torch.uint8, device=t.device)
    sizes, streams = buf[:8 * B].view(torch.int64), buf[head:].view(B, plan.capacity)
    ws = torch.empty(B * plan.ws_bytes, dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        lib().call("cidnet_jpeg_encode_u8", ops._p(t), t.stride(0) if B > 1 else 3 * h * w, ops._p(streams), plan.capacity,
                   ops._p(sizes), ops._p(ws), ws.numel(), ops._p(metrics._jpeg_table_on(t.device, qplan.quality)), B, h, w,
                   ops._stream())
    return buf, streams, sizes


def jpeg_scan_u8(q: torch.Tensor, quality: int = 75):
    """uint8 (B,h,w,3) (or (h,w,3)) on the device, as egress writes it -> (streams uint8 (B, capacity), sizes int64 (B,)), both
    on the device, no synchronisation: streams[b, :sizes[b]] is the entropy-coded scan of the JPEG file Pillow writes of image
    b at `quality` with its defaults (jpeg_file frames it), the rest of the slot is zero; capacity =
    jpeg_encode_plan(h, w).capacity.  The bytes are Pillow's, identical from call to call and independent of the rest of the
    batch.  ValueError for a quality outside 1..100 and for a size the plan refuses."""
    metrics.jpeg_quant_plan(quality)
    if isinstance(q, torch.Tensor) and not q.is_cuda:
        raise RuntimeError(_NO_CPU)
    t = _images_u8(q, "jpeg_scan_u8")
    _, streams, sizes = _jpeg_scan(t, quality)
    return streams, sizes


def _jpeg_segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


@functools.lru_cache(maxsize=64)
def _jpeg_header(h, w, quality):
    plan = metrics.jpeg_quant_plan(quality)
    out = b"\xff\xd8" + _jpeg_segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, t in enumerate((plan.luma, plan.chroma)):
        flat = t.reshape(64)
        out += _jpeg_segment(0xDB, bytes([i]) + bytes(int(flat[n]) for n in _JPEG_ZIGZAG))
    out += _jpeg_segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, counts, symbols in _JPEG_DHT:
        out += _jpeg_segment(0xC4, bytes([tc_th]) + counts + symbols)
    out += _jpeg_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == JPEG_HEADER_BYTES
    return out


def jpeg_file(h, w, quality, scan_bytes) -> bytes:
    """The JPEG file around one entropy-coded scan (host): SOI, APP0 (JFIF 1.01, density 1 x 1), the two quantisation tables
    of jpeg_quant_plan(quality) in zigzag order, SOF0 (8 bits, three components, 2x2 / 1x1 / 1x1), the four Annex K Huffman
    tables, SOS -- 623 bytes that depend on h, w and quality alone -- then the scan and EOI"""
    h, w = _whole(h), _whole(w)
    if not (0 < h <= 65500 and 0 < w <= 65500):
        raise ValueError(f"jpeg_file: sides must lie in 1..65500 (got {(h, w)})")
    return _jpeg_header(h, w, metrics.jpeg_quant_plan(quality).quality) + bytes(scan_bytes) + b"\xff\xd9"


def jpeg_encode_u8(q: torch.Tensor, quality: int = 75) -> list:
    """uint8 (B,h,w,3) (or (h,w,3)) on the device -> the B JPEG files as bytes, each what Image.fromarray(a).save(f, 'JPEG',
    quality=quality) writes: jpeg_scan_u8, one download, jpeg_file.  The convenience form: it synchronises."""
    streams, sizes = jpeg_scan_u8(q, quality)
    h, w = (q.shape[-3], q.shape[-2])
    n = sizes.cpu().tolist()
    host = streams[:, :max(n)].cpu().numpy()
    return [jpeg_file(h, w, quality, host[b, :n[b]].tobytes()) for b in range(len(n))]


# ---- the batching plan (pure host code) -------------------------------------------------------------------------------
def shard(n, rank=0, world=1):
    """input positions of rank's images: i % world == rank, in input order"""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world}")
    return range(rank, n, world)


def plan_batches(sizes, rank=0, world=1, batch_size=1):
    """The batches of enhance_folder for one rank.  sizes: (h, w) of this rank's images -- input positions shard(n, rank,
    world) -- in that order, consumed one at a time (a batch is yielded once the image after it has been seen).  Yields the
    input positions of each batch: consecutive images of equal size, at most batch_size of them (metrics._plan's index
    arithmetic with the image size standing for both the padded shape and the crop)."""
    for _, _, runs in metrics._plan((((int(h), int(w)),) * 2 for h, w in sizes), rank, world, max(1, int(batch_size))):
        yield [i for _, _, rows in runs for i in range(rows.start, rows.stop, rows.step)]


# ---- the writer: device uint8 -> pinned -> files, `depth` batches deep ------------------------------------------------------
class _Writer:
    """put(q, paths): q uint8 (B,h,w,3) on the device, complete on the current stream when put() is called -> one
    non-blocking copy into a pinned buffer on the download stream and one encode task per image, which waits for that copy's
    event in its worker and saves through PIL.  At most `depth` batches are in flight: put() first retires the oldest one
    (waits for its futures; the time goes to `waited`) when they are.  on_done() of a batch runs when it is retired.  The
    first exception of a worker surfaces from retire() / put() / close() with the file's name.
    png="device": a batch with a path ending in .png (any case) is also encoded by png_zlib_u8 on the current stream right
    behind q; the download stream copies the sizes and the capacity-strided slots in ONE further non-blocking copy into a pinned
    buffer of their own, and the worker of such a path frames stream[:size] with png_file and writes it.  Paths of other
    extensions keep PIL; q itself is downloaded only when one of them is in the batch.
    jpeg="device": a batch with a path ending in .jpg or .jpeg (any case) is also encoded by jpeg_scan_u8 at quality 75 on the
    current stream right behind q.  A slot's proven capacity is about three times the raw image and a real scan a small
    fraction of it, so the download stream copies the sizes and a PREFIX of each slot -- jpeg_prefix * 3 h w bytes, rounded up
    to 4 KiB, the capacity at most; one non-blocking pinned copy per image, the first carrying the sizes -- and a worker whose
    image reports size > prefix fetches the remainder itself with a second copy on the download stream and waits for it (the
    device buffer lives until retire()).  The files do not depend on jpeg_prefix; second_copies counts such images, downloaded
    the bytes all copies brought to the host.  Both keywords combine in one batch."""

    def __init__(self, device, threads=8, depth=2, png="pillow", jpeg="pillow", jpeg_prefix=0.25):
        self.png = _check_png(png)
        self.jpeg = _check_jpeg(jpeg)
        if not 0 < float(jpeg_prefix) <= 8:
            raise ValueError(f"jpeg_prefix must lie in (0, 8] (got {jpeg_prefix!r})")
        self.jpeg_prefix = float(jpeg_prefix)
        self.host_jpeg = [None] * max(1, int(depth))             # pinned: sizes and slot prefixes of a batch's JPEG scans
        self.second_copies = 0
        self.downloaded = 0
        self.lock = threading.Lock()
        self.host_png = [None] * max(1, int(depth))              # pinned: sizes and slots of a batch's PNG streams
        self.device, self.depth = device, max(1, int(depth))
        self.pool = cf.ThreadPoolExecutor(max_workers=max(1, min(int(threads), 16)), thread_name_prefix="cidnet-encode")
        self.down = torch.cuda.Stream(device)
        self.host = [None] * self.depth                          # pinned output buffers
        self.inflight = collections.deque()                      # (futures, on_done, q kept alive)
        self.count = 0
        self.waited = 0.0
        self.stop = threading.Event()

    def _save(self, event, host, k, h, w, path):
        if self.stop.is_set():
            return
        try:
            from PIL import Image
            event.synchronize()
            n = 3 * h * w
            Image.fromarray(host[k * n:(k + 1) * n].view(h, w, 3).numpy()).save(path)
        except Exception as e:
            raise RuntimeError(f"image_io: {os.path.basename(path)}: could not be written: {e}") from e

    def _save_png(self, event, host, head, capacity, k, h, w, path):
        if self.stop.is_set():
            return
        try:
            event.synchronize()
            size = int(host[8 * k:8 * k + 8].view(torch.int64)[0])
            if not 0 < size <= capacity:
                raise RuntimeError(f"the encoder reported {size} bytes for a slot of {capacity}")
            o = head + k * capacity
            data = png_file(h, w, host[o:o + size].numpy().tobytes())
            with open(path, "wb") as f:
                f.write(data)
        except Exception as e:
            raise RuntimeError(f"image_io: {os.path.basename(path)}: could not be written: {e}") from e

    def _save_jpeg(self, event, host, buf, head, capacity, prefix, k, h, w, path):
        if self.stop.is_set():
            return
        try:
            event.synchronize()
            size = int(host[8 * k:8 * k + 8].view(torch.int64)[0])
            if not 0 < size <= capacity:
                raise RuntimeError(f"the encoder reported {size} bytes for a slot of {capacity}")
            o = head + k * prefix
            scan = host[o:o + min(size, prefix)].numpy().tobytes()
            if size > prefix:                                    # the rest of this slot: a copy of its own, waited for here
                rest = torch.empty(size - prefix, dtype=torch.uint8, pin_memory=True)
                d = head + k * capacity
                with torch.cuda.device(self.device), torch.cuda.stream(self.down):
                    rest.copy_(buf[d + prefix:d + size], non_blocking=True)
                    fetched = torch.cuda.Event()
                    fetched.record()
                fetched.synchronize()
                scan += rest.numpy().tobytes()
                with self.lock:
                    self.second_copies += 1
                    self.downloaded += size - prefix
            data = jpeg_file(h, w, 75, scan)
            with open(path, "wb") as f:
                f.write(data)
        except Exception as e:
            raise RuntimeError(f"image_io: {os.path.basename(path)}: could not be written: {e}") from e

    def _kind(self, path):
        name = str(path).lower()
        if self.png == "device" and name.endswith(".png"):
            return "png"
        if self.jpeg == "device" and name.endswith(_JPEG_NAMES):
            return "jpeg"
        return None

    def retire(self):
        """wait for the oldest batch in flight; False when there is none"""
        if not self.inflight:
            return False
        futures, on_done, _ = self.inflight.popleft()
        t0 = time.perf_counter()
        try:
            for f in futures:
                f.result()
        finally:
            self.waited += time.perf_counter() - t0
        if on_done is not None:
            on_done()
        return True

    def put(self, q, paths, on_done=None):
        while len(self.inflight) >= self.depth:
            self.retire()
        B, h, w, _ = q.shape
        slot = self.count % self.depth
        self.count += 1
        n = q.numel()
        kinds = [self._kind(p) for p in paths]
        buf = jbuf = None
        if "png" in kinds:                                       # the whole batch: its other images' slots are not used
            buf, streams, _ = _png_zlib(_images_u8(q, "image_io"), PNG_FILTERS.index("adaptive"), 32768)
            head, capacity = buf.numel() - streams.numel(), streams.shape[1]
            if self.host_png[slot] is None or self.host_png[slot].numel() < buf.numel():
                self.host_png[slot] = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
            host_png = self.host_png[slot]
        if "jpeg" in kinds:
            jbuf, jstreams, _ = _jpeg_scan(_images_u8(q, "image_io"), 75)
            jhead, jcap = jbuf.numel() - jstreams.numel(), jstreams.shape[1]
            prefix = min(jcap, -(-int(self.jpeg_prefix * 3 * h * w) // 4096) * 4096)
            if self.host_jpeg[slot] is None or self.host_jpeg[slot].numel() < jhead + B * prefix:
                self.host_jpeg[slot] = torch.empty(jhead + B * prefix, dtype=torch.uint8, pin_memory=True)
            host_jpeg = self.host_jpeg[slot]
        pillow = None in kinds
        if pillow and (self.host[slot] is None or self.host[slot].numel() < n):
            self.host[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        host = self.host[slot]
        ready = torch.cuda.Event()
        ready.record()                                           # q (and its streams) are complete here on the current stream
        self.down.wait_event(ready)
        got = 0
        with torch.cuda.stream(self.down):
            if pillow:
                host[:n].view(B, h, w, 3).copy_(q, non_blocking=True)
                got += n
            if buf is not None:
                host_png[:buf.numel()].copy_(buf, non_blocking=True)
                got += buf.numel()
            if jbuf is not None:                                 # the sizes travel with the first prefix
                host_jpeg[:jhead + prefix].copy_(jbuf[:jhead + prefix], non_blocking=True)
                for k in range(1, B):
                    if kinds[k] == "jpeg":
                        host_jpeg[jhead + k * prefix:jhead + (k + 1) * prefix].copy_(
                            jbuf[jhead + k * jcap:jhead + k * jcap + prefix], non_blocking=True)
                got += jhead + prefix * (1 + sum(kd == "jpeg" for kd in kinds[1:]))
        q.record_stream(self.down)
        for t in (buf, jbuf):
            if t is not None:
                t.record_stream(self.down)
        done = torch.cuda.Event()
        done.record(self.down)
        with self.lock:
            self.downloaded += got
        futures = []
        for k, (p, kind) in enumerate(zip(paths, kinds)):
            if kind == "png":
                futures.append(self.pool.submit(self._save_png, done, host_png, head, capacity, k, h, w, p))
            elif kind == "jpeg":
                futures.append(self.pool.submit(self._save_jpeg, done, host_jpeg, jbuf, jhead, jcap, prefix, k, h, w, p))
            else:
                futures.append(self.pool.submit(self._save, done, host, k, h, w, p))
        self.inflight.append((futures, on_done, (q, buf, jbuf)))

    def close(self):
        try:
            while self.retire():
                pass
        finally:
            self.abort()

    def abort(self):
        """stop: queued tasks return at once, running ones finish; nothing is left running"""
        self.stop.set()
        self.pool.shutdown(wait=True, cancel_futures=True)
        self.inflight.clear()


# ---- enhance a folder -------------------------------------------------------------------------------------------------
@dataclass
class EnhanceReport:
    """What one rank's enhance_folder did: names / sizes (h, w) of its images in input order, batches (the input positions of
    each launch), seconds: {"wall": the call, "wait_for_slot": of it, the main thread waiting for a batch in flight to
    finish so that its buffers come free}, tiles: with tile=, the number of tiles of each image (empty otherwise), ensemble:
    the number of views each image was averaged over (1: none were built), png: who encoded the .png files ("pillow" or
    "device"), jpeg: who encoded the .jpg / .jpeg files (likewise); with jpeg="device", jpeg_second_copies: the images whose
    scan was longer than the downloaded prefix, and downloaded: the bytes the writer's copies brought to the host"""
    names: list = field(default_factory=list)
    sizes: list = field(default_factory=list)
    batches: list = field(default_factory=list)
    seconds: dict = field(default_factory=dict)
    tiles: list = field(default_factory=list)
    ensemble: int = 1
    png: str = "pillow"
    jpeg: str = "pillow"
    jpeg_second_copies: int = 0
    downloaded: int = 0


class _Stage:
    """a pinned per-image staging buffer; grown by the main thread only"""
    __slots__ = ("buf",)

    def __init__(self):
        self.buf = None


def _decode(stop, path, name, stage):
    """worker: -> (h, w, None) with the bytes in the stage, or (h, w, array) when the stage is too small for them"""
    if stop.is_set():
        return None
    try:
        a = metrics._read_rgb(path)
        h, w, _ = a.shape
        if stage.buf is None or stage.buf.numel() < a.size:
            return h, w, a
        stage.buf[:a.size].view(h, w, 3).numpy()[...] = a
        return h, w, None
    except Exception as e:
        raise RuntimeError(f"enhance_folder: {name}: could not be read: {e}") from e


@torch.no_grad()
def enhance_folder(model, in_dir, out_dir, gamma: float = 1.0, gated: bool = False, alpha_s: float = 1.3, gated2: bool = False,
                   alpha: float = 1.0, batch_size: int = 1, threads: int = 8, depth: int = 2, process_group=None, tile=None,
                   overlap: int = 32, tile_batch: int = 8, ensemble: int = 1, png: str = "pillow", jpeg: str = "pillow",
                   jpeg_prefix: float = 0.25) -> EnhanceReport:
    """eval.py / demo.py for a folder: every image file of in_dir (metrics.folder_images: its files and order) is enhanced as
    enhance_u8 does and saved to out_dir/<same file name> by PIL in the format its extension names (the reference's
    output_img.save(output_folder + name[0])); out_dir is created.  Decoding, the device and encoding overlap (module
    docstring): `threads` decode and as many encode workers (16 at most), `depth` batches in flight, consecutive images of
    equal size sharing a batch of up to batch_size.  depth=1, threads=1 is the serial order; the files do not depend on any of
    the three.  With a process group (or an initialised default group) rank r takes images i % world == r; no collective runs
    and each rank reports its own images.  The first error of a worker stops the pipeline and is raised naming the file.
    The model's attributes and modes are restored afterwards.
    tile = T or (Th, Tw): every image is tiled on its own as enhance_u8(tile=, overlap=, tile_batch=) does, one image per
    launch group (batch_size is ignored); the pipeline around it is the same.  report.tiles holds each image's tile count.
    ensemble = 2, 4 or 8: every batch is self-ensembled as enhance_u8(ensemble=) does (the model sees batches of batch_size *
    views); ValueError for another value or together with tile=, before a worker starts.
    png: "pillow" -- every file is encoded by PIL.  "device" -- an output whose name ends in .png (any case) is encoded on the
    device (png_zlib_u8 behind egress: adaptive filters, Huffman coding, no LZ77) and only framed and written by its worker:
    the same pixels in another, valid PNG file, independent of batch_size, threads and depth; other extensions keep PIL.
    report.png says which.  ValueError for another value, before a worker starts.
    jpeg: "pillow" -- as above.  "device" -- an output whose name ends in .jpg or .jpeg (any case) is encoded on the device at
    quality 75 (jpeg_scan_u8 behind egress) and only framed and written by its worker: the file is Pillow's own, byte for byte,
    independent of batch_size, threads, depth and jpeg_prefix (the fraction of 3 h w bytes of each scan downloaded up front;
    _Writer).  report.jpeg says which.  ValueError for another value, before a worker starts."""
    views = _check_ensemble(ensemble, tile)
    png = _check_png(png)
    jpeg = _check_jpeg(jpeg)
    t_start = time.perf_counter()
    device = metrics._model_device(model)
    if device.type != "cuda":
        raise RuntimeError(_NO_CPU)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    files = in_dir if isinstance(in_dir, metrics.FolderImages) else metrics.folder_images(in_dir)
    world, rank = 1, 0
    if process_group is not None or (dist.is_available() and dist.is_initialized()):
        world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
    batch_size, depth = max(1, int(batch_size)), max(1, int(depth))
    if tile is not None:                                         # a bad tile / overlap / tile_batch raises before a worker starts
        _check_tile(tile, overlap)
        batch_size, tile_batch = 1, _tile_batch(tile_batch)
    workers = max(1, min(int(threads), 16))
    mine = list(shard(len(files), rank, world))
    report = EnhanceReport(names=[files.names[i] for i in mine], ensemble=int(ensemble), png=png, jpeg=jpeg)
    os.makedirs(out_dir, exist_ok=True)
    if not mine:
        report.seconds = {"wall": time.perf_counter() - t_start, "wait_for_slot": 0.0}
        return report

    stop = threading.Event()
    decoders = cf.ThreadPoolExecutor(max_workers=workers, thread_name_prefix="cidnet-decode")
    writer = _Writer(device, workers, depth, png=png, jpeg=jpeg, jpeg_prefix=jpeg_prefix)
    # depth batches in flight + the batch being formed + the image _plan looks ahead
    free = [_Stage() for _ in range((depth + 1) * batch_size + 1)]
    pending = collections.deque()                                # decodes submitted, not yet consumed: (position, stage, future)
    loaded = []                                                  # consumed, not yet launched: (stage, h, w)
    dev_in = [None] * depth
    todo = iter(mine)

    def submit():
        while free:
            i = next(todo, None)
            if i is None:
                return
            stage = free.pop()
            pending.append((i, stage, decoders.submit(_decode, stop, files.paths[i], files.names[i], stage)))

    def sizes():
        for _ in mine:
            submit()
            while not pending:                                   # every stage is held by a batch in flight: wait for the oldest
                if not writer.retire():
                    raise AssertionError("enhance_folder: no staging buffer free and no batch in flight")
                submit()
            _, stage, fut = pending.popleft()
            h, w, a = fut.result()
            if a is not None:                                    # the stage was too small: grow it here, in the main thread
                stage.buf = torch.empty(a.size, dtype=torch.uint8, pin_memory=True)
                stage.buf.view(h, w, 3).numpy()[...] = a
            loaded.append((stage, h, w))
            report.sizes.append((h, w))
            yield h, w

    try:
        with torch.cuda.device(device), metrics._eval_state(model, _trans_attrs(gated, alpha_s, gated2, alpha)):
            table = _table_on(device, gamma)
            up = torch.cuda.Stream(device)
            for n_batch, positions in enumerate(plan_batches(sizes(), rank, world, batch_size)):
                B = len(positions)
                batch, loaded[:B] = loaded[:B], []
                _, h, w = batch[0]
                try:
                    _check_reflect(h, w, *padded_size(h, w))
                    plan = tile_plan(h, w, tile, overlap) if tile is not None else None
                except ValueError as e:
                    raise ValueError(f"enhance_folder: {files.names[positions[0]]}: {e}") from None
                while len(writer.inflight) >= depth:             # the device input of this slot belongs to a batch in flight
                    writer.retire()
                n, slot = 3 * h * w, n_batch % depth
                if dev_in[slot] is None or dev_in[slot].numel() < B * n:
                    dev_in[slot] = torch.empty(B * n, dtype=torch.uint8, device=device)
                    up.wait_stream(torch.cuda.current_stream())  # fresh memory of the compute stream's pool
                t = dev_in[slot][:B * n].view(B, h, w, 3)
                with torch.cuda.stream(up):
                    for k, (stage, _, _) in enumerate(batch):
                        t[k].copy_(stage.buf[:n].view(h, w, 3), non_blocking=True)
                uploaded = torch.cuda.Event()
                uploaded.record(up)
                torch.cuda.current_stream().wait_event(uploaded)
                if plan is None:
                    q = _run(model, t, table, views)
                else:
                    q = _run_tiled(model, t[0], table, plan, tile_batch).unsqueeze(0)
                    report.tiles.append(len(plan))
                stages = [b[0] for b in batch]
                writer.put(q, [os.path.join(out_dir, files.names[i]) for i in positions], on_done=lambda s=stages: free.extend(s))
                report.batches.append(positions)
            writer.close()
    except BaseException:
        stop.set()
        writer.abort()
        raise
    finally:
        stop.set()
        decoders.shutdown(wait=True, cancel_futures=True)
    report.seconds = {"wall": time.perf_counter() - t_start, "wait_for_slot": writer.waited}
    report.jpeg_second_copies, report.downloaded = writer.second_copies, writer.downloaded
    return report
