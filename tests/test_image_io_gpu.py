"""GPU: the image ingest / egress kernels alone (csrc/imageio.hip through hvi_cidnet_amd.image_io and the raw C ABI), no model.
Everything compares exactly.

ingest: interleaved uint8 (h,w,3) -> planar fp32, reflect-padded, through the / 255 quotients or a gamma table, against
F.pad(T[img]) built from torch ops here; the source has a batch stride of 3 h w + 5 and an odd base address.
egress: planar fp32 -> interleaved uint8 against metrics.to_uint8 (the project's existing kernel) and metrics_ref.quantize, into
a sentinel-filled buffer (stride 3 h w + 5, odd base) of which no byte outside the images may change."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
# (8,8): no pad; (9,13): pads 7 and 3 (the deepest reflection a side of 9 allows), tail of 1; (10,23): tail of 3; (33,50): tail
# of 2, several blocks; (16,24): no pad, width a multiple of 4; (5,9): pad of 3 on a side of 5
SHAPES = [(8, 8), (9, 13), (10, 23), (33, 50), (16, 24), (5, 9)]
SENTINEL = 0xA5
CIDNET_ERR_SHAPE = -2


def _images(B, h, w, seed):
    """(B,h,w,3) uint8 on the CPU: random bytes, image 0 holding all 256 levels (as far as it has room)"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=g)
    flat = img[0].reshape(-1)
    n = min(256, flat.numel())
    where = torch.randperm(flat.numel(), generator=g)[:n]
    flat[where] = torch.arange(256, dtype=torch.int64)[:n].to(torch.uint8)
    return img


def _strided(img, dev, slack=5):
    """the images in a sentinel-filled device buffer at an odd base address with a batch stride of 3 h w + slack
    -> (buffer, the (B,h,w,3) view)"""
    B, h, w, _ = img.shape
    bs = 3 * h * w + slack
    buf = torch.full((1 + B * bs + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    view = buf[1:1 + B * bs].view(B, bs)[:, :3 * h * w].view(B, h, w, 3)
    assert view.data_ptr() % 2 == 1 and (B == 1 or view.stride(0) == bs)
    view.copy_(img.to(dev))
    return buf, view


def _ingest_ref(img_dev, table, Hp, Wp):
    B, h, w, _ = img_dev.shape
    return F.pad(table[img_dev.long()].permute(0, 3, 1, 2), (0, Wp - w, 0, Hp - h), "reflect").contiguous()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_ingest_is_the_padded_table_lookup(dev, hw, B):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import image_io as IO
    h, w = hw
    img = _images(B, h, w, seed=h * 100 + w + B)
    buf, view = _strided(img, dev)
    Hp, Wp = IO.padded_size(h, w)
    assert (Hp, Wp) == tuple(P.pad_to_multiple(torch.zeros(1, 3, h, w))[0].shape[-2:])
    quot = torch.arange(256, dtype=torch.float32).div(255).to(dev)                  # ToTensor's division, per level
    for gamma, table in ((1.0, quot), (1.4, torch.from_numpy(P.gamma_table(1.4)).to(dev))):
        x, size = P.ingest(view, gamma=gamma)
        assert size == (h, w) and x.shape == (B, 3, Hp, Wp) and x.dtype == torch.float32
        assert torch.equal(x, _ingest_ref(view, table, Hp, Wp)), (hw, B, gamma)
    # gamma 1 is ToTensor + F.pad, bit for bit
    ref = F.pad(img.permute(0, 3, 1, 2).float().div(255), (0, Wp - w, 0, Hp - h), "reflect").to(dev)
    assert torch.equal(P.ingest(view)[0], ref)
    assert torch.equal(P.ingest(img.to(dev))[0], ref)                                # the dense layout
    assert bool((buf[0] == SENTINEL) & (buf[1 + B * (3 * h * w + 5):] == SENTINEL).all())            # the source is only read


def _egress_input(B, Hp, Wp, seed, dev):
    """uniform in [-0.2, 1.2] with NaN, +-0, 1.0 and every q / 255 with its two fp32 neighbours planted"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, Hp, Wp), generator=g) * 1.4 - 0.2
    q = (torch.arange(256, dtype=torch.float32) / 255).numpy()
    levels = np.stack([q, np.nextafter(q, np.float32(2)), np.nextafter(q, np.float32(-1))], axis=1).reshape(-1)
    special = np.concatenate([np.array([np.nan, 0.0, -0.0, 1.0], dtype=np.float32), levels[::-1]]).astype(np.float32)
    flat = x.reshape(-1)
    n = min(special.size, flat.numel())                          # the smallest shapes have room for the upper levels only
    where = torch.randperm(flat.numel(), generator=g)[:n]
    flat[where] = torch.from_numpy(special)[:n]
    return x.to(dev)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_egress_is_to_uint8_interleaved_and_writes_nothing_else(dev, hw, B):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, image_io as IO, ops
    h, w = hw
    Hp, Wp = IO.padded_size(h, w)
    x = _egress_input(B, Hp, Wp, seed=h * 100 + w + B, dev=dev)
    ref = P.metrics.to_uint8(x, (h, w)).permute(0, 2, 3, 1).contiguous()             # the existing kernel
    # the restatement casts with numpy, which leaves the cast of a NaN undefined: the contract's NaN -> 0 is stated here
    host = np.stack([R.quantize(np.nan_to_num(xb, nan=0.0), h, w) for xb in x.cpu().numpy()]).transpose(0, 2, 3, 1)
    assert np.array_equal(ref.cpu().numpy(), host)
    q = P.egress(x, (h, w))
    assert q.shape == (B, h, w, 3) and q.dtype == torch.uint8
    assert torch.equal(q, ref), (hw, B)
    # through the raw ABI into a sentinel-filled buffer: batch stride 3 h w + 5, odd base
    bs = 3 * h * w + 5
    buf = torch.full((1 + B * bs + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    dst = buf[1:]
    assert dst.data_ptr() % 2 == 1
    _lib.lib().call("cidnet_image_egress", ops._p(x), ops._p(dst), bs, B, Hp, Wp, h, w, ops._stream())
    rows = buf[1:1 + B * bs].view(B, bs)
    assert torch.equal(rows[:, :3 * h * w].reshape(B, h, w, 3), ref)
    assert bool((rows[:, 3 * h * w:] == SENTINEL).all()), "slack between the images written"
    assert bool(buf[0] == SENTINEL) and bool((buf[1 + B * bs:] == SENTINEL).all()), "bytes outside the images written"
    # the whole padded image, no crop
    assert torch.equal(P.egress(x), P.metrics.to_uint8(x).permute(0, 2, 3, 1))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_round_trip_is_the_identity(dev, hw, B):
    import hvi_cidnet_amd as P
    h, w = hw
    img = _images(B, h, w, seed=7 * h + w).to(dev)
    x, size = P.ingest(img)
    assert torch.equal(P.egress(x, size), img)
    assert torch.equal(P.egress(P.ingest(img[0])[0], size), img[:1])                 # (h,w,3) in, a batch of one out


def test_rejections(dev):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, ops
    raw = _lib.lib().raw("cidnet_image_ingest")
    src = torch.zeros((16, 16, 3), dtype=torch.uint8, device=dev)
    x = torch.zeros((3, 32, 32), dtype=torch.float32, device=dev)
    st = ops._stream()
    assert raw(ops._p(src), 3 * 2 * 8, None, ops._p(x), 1, 2, 8, 8, 8, st) == CIDNET_ERR_SHAPE      # (h, Hp) = (2, 8)
    assert raw(ops._p(src), 3 * 8 * 2, None, ops._p(x), 1, 8, 2, 8, 8, st) == CIDNET_ERR_SHAPE      # the same for the width
    assert raw(ops._p(src), 3 * 9 * 8, None, ops._p(x), 1, 9, 8, 8, 8, st) == CIDNET_ERR_SHAPE      # Hp < h
    assert raw(ops._p(src), 3 * 8 * 9, None, ops._p(x), 1, 8, 9, 8, 8, st) == CIDNET_ERR_SHAPE      # Wp < w
    assert raw(ops._p(src), 3 * 8 * 8 - 1, None, ops._p(x), 1, 8, 8, 8, 8, st) == CIDNET_ERR_SHAPE  # stride below an image
    assert raw(ops._p(src), 3 * 8 * 8, None, ops._p(x), 1, 8, 8, 8, 8, st) == 0
    assert _lib.lib().raw("cidnet_image_egress")(ops._p(x), ops._p(src), 3 * 9 * 8, 1, 8, 8, 9, 8, st) == CIDNET_ERR_SHAPE
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="reflect"):
        P.ingest(torch.zeros((2, 8, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="gamma"):
        P.ingest(torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev), gamma=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.ingest(torch.zeros((8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.egress(torch.zeros((1, 3, 8, 8)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.enhance_u8(None, torch.zeros((8, 8, 3), dtype=torch.uint8))
