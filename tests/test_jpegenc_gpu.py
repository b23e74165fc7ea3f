"""GPU: the JPEG encoder on the device (csrc/jpegenc.hip through image_io.jpeg_scan_u8 and jpeg_file) against PILLOW'S FILE,
byte for byte, on every case of the contract (tests/jpegenc_ref.py: cases); batches against each image alone, repeated calls,
an odd source address, guard bytes around the slots and sizes, and every refusal with nothing written.  Pillow's files are
computed once per module and shared."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpegenc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
_ref = {}


def _want(kind, h, w, q=75):
    """-> (the image as interleaved (h,w,3), Pillow's file), shared between the tests"""
    key = (kind, h, w, q)
    if key not in _ref:
        img = R.case_image(kind, h, w, q)
        hwc = np.ascontiguousarray(img.transpose(1, 2, 0))
        hwc.setflags(write=False)
        _ref[key] = (hwc, R.pil_file(img, q))
    return _ref[key]


def _encode(dev, imgs, q=75):
    """a list of equal-sized images as ONE batch -> the files as bytes, with the shape checks"""
    from hvi_cidnet_amd import image_io as IO
    t = torch.from_numpy(np.stack(imgs)).to(dev)
    streams, sizes = IO.jpeg_scan_u8(t, q)
    h, w = t.shape[1:3]
    cap = IO.jpeg_encode_plan(h, w).capacity
    assert streams.dtype == torch.uint8 and tuple(streams.shape) == (len(imgs), cap) and streams.is_cuda
    assert sizes.dtype == torch.int64 and tuple(sizes.shape) == (len(imgs),) and sizes.is_cuda
    host, n = streams.cpu().numpy(), sizes.cpu().tolist()
    for b in range(len(imgs)):
        assert 0 < n[b] <= cap and not host[b, n[b]:].any(), (b, n[b], cap)      # the rest of a slot is zero
    return [IO.jpeg_file(h, w, q, host[b, :n[b]].tobytes()) for b in range(len(imgs))]


def _same(got, want, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        k = min(len(a), len(b))
        bad = np.flatnonzero(a[:k] != b[:k])
        print(what, "sizes", len(got), len(want), "first differing bytes", bad[:6].tolist())
    assert got == want, (what, len(got), len(want))


def _check_plan(h, w):
    from hvi_cidnet_amd import image_io as IO
    p, r = IO.jpeg_encode_plan(h, w), R.plan(h, w)
    assert (p.mcu_cols, p.mcu_rows, p.block_cols, p.block_rows, p.dummies, p.capacity, p.groups) == \
        (r["mcu_cols"], r["mcu_rows"], r["block_cols"], r["block_rows"], r["dummies"], r["capacity"], r["groups"]), (h, w, p)
    return p


# what each size is there for: (MCU columns, MCU rows, dummy blocks)
PLANS = {(1, 5): (1, 1, 3), (7, 9): (1, 1, 2), (8, 8): (1, 1, 3), (16, 16): (1, 1, 0), (18, 34): (3, 2, 9), (24, 24): (2, 2, 7),
         (31, 33): (3, 2, 4), (40, 56): (4, 3, 13), (50, 70): (5, 4, 17), (35, 277): (18, 3, 41), (97, 131): (9, 7, 31)}


@pytest.mark.parametrize("h,w", R.SIZES)
def test_files_equal_pillows(dev, h, w):
    p = _check_plan(h, w)
    assert (p.mcu_cols, p.mcu_rows, p.dummies) == PLANS[(h, w)], p
    if (h, w) == (35, 277):
        assert p.workgroups == 9 and p.mcu_rows == 3 and p.groups == 4        # several workgroups per row, three MCU rows
    if (h, w) == (97, 131):
        assert p.groups >= 3                                                   # the scan of the bit counts has partial sums
    want = [_want(kind, h, w) for kind in R.KINDS]
    got = _encode(dev, [x[0] for x in want])
    for kind, g, (_, data) in zip(R.KINDS, got, want):
        _same(g, data, (kind, h, w))


@pytest.mark.parametrize("q", (1, 50, 100))
def test_qualities(dev, q):
    _check_plan(50, 70)
    img, data = _want("random", 50, 70, q)
    _same(_encode(dev, [img], q)[0], data, q)


@pytest.mark.parametrize("h,w", R.TINY)
def test_tiny_images(dev, h, w):
    p = _check_plan(h, w)
    assert p.mcu_cols == p.mcu_rows == 1 and p.dummies == 3
    img, data = _want("random", h, w)
    _same(_encode(dev, [img])[0], data, (h, w))


@pytest.mark.parametrize("kind,h,w", (("checker_pixels", 16, 16), ("checker_blocks", 16, 32)))
def test_largest_categories(dev, kind, h, w):
    _check_plan(h, w)
    img, data = _want(kind, h, w, 100)
    _same(_encode(dev, [img], 100)[0], data, kind)


def test_batch_equals_each_alone_and_calls_repeat(dev):
    h, w = 40, 56
    imgs = [_want(kind, h, w)[0] for kind in ("ramp", "random", "saturated")]
    together = _encode(dev, imgs)
    assert len(set(together)) == 3
    for img, t in zip(imgs, together):
        _same(_encode(dev, [img])[0], t, "alone")
    for _ in range(3):
        assert _encode(dev, imgs) == together


def test_single_image_input_and_convenience_form(dev):
    from hvi_cidnet_amd import image_io as IO
    h, w = 31, 33
    img, data = _want("ramp", h, w)
    streams, sizes = IO.jpeg_scan_u8(torch.from_numpy(np.array(img)).to(dev))
    assert tuple(streams.shape) == (1, IO.jpeg_encode_plan(h, w).capacity) and tuple(sizes.shape) == (1,)
    _same(IO.jpeg_file(h, w, 75, streams[0, :int(sizes[0])].cpu().numpy().tobytes()), data, "(h,w,3)")
    assert IO.jpeg_encode_u8(torch.from_numpy(np.array(img)).to(dev)) == [data]


def test_odd_address_and_batch_stride(dev):
    """the source at an odd address with a batch stride above 3 h w: no copy is made (image_io._images_u8) and the bytes hold"""
    from hvi_cidnet_amd import image_io as IO
    h, w = 18, 34
    imgs = [_want(kind, h, w) for kind in ("ramp", "random")]
    n = 3 * h * w
    flat = torch.zeros(1 + 2 * (n + 5), dtype=torch.uint8, device=dev)
    q = torch.as_strided(flat, (2, h, w, 3), (n + 5, 3 * w, 3, 1), 1)
    for b in range(2):
        q[b] = torch.from_numpy(np.array(imgs[b][0])).to(dev)
    assert q.data_ptr() % 2 == 1 and IO._images_u8(q, "test").data_ptr() == q.data_ptr()
    streams, sizes = IO.jpeg_scan_u8(q)
    for b in range(2):
        _same(IO.jpeg_file(h, w, 75, streams[b, :int(sizes[b])].cpu().numpy().tobytes()), imgs[b][1], b)


def test_nothing_outside_the_slots_is_written(dev):
    """the C entry point with guard bytes before, between and behind the slots and around sizes"""
    from hvi_cidnet_amd import _lib, metrics as M, ops, image_io as IO
    h, w, B = 40, 56, 3
    p = IO.jpeg_encode_plan(h, w)
    imgs = [_want(kind, h, w) for kind in ("ramp", "random", "constant")]
    q = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
    stride = p.capacity + 64
    out = torch.full((16 + B * stride,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.full((B + 2,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(B * p.ws_bytes, dtype=torch.uint8, device=dev)
    _lib.lib().call("cidnet_jpeg_encode_u8", ops._p(q), 3 * h * w, out.data_ptr() + 16, stride, sizes.data_ptr() + 8, ops._p(ws),
                    ws.numel(), ops._p(M._jpeg_table_on(q.device, 75)), B, h, w, ops._stream())
    torch.cuda.synchronize()
    host, n = out.cpu().numpy(), sizes.cpu().tolist()
    assert n[0] == -7 and n[-1] == -7
    assert (host[:16] == 0xA5).all()
    for b in range(B):
        slot = host[16 + b * stride:16 + (b + 1) * stride]
        _same(IO.jpeg_file(h, w, 75, slot[:n[1 + b]].tobytes()), imgs[b][1], b)
        assert (slot[p.capacity:] == 0xA5).all() and not slot[n[1 + b]:p.capacity].any()


def test_refusals(dev):
    from hvi_cidnet_amd import _lib, metrics as M, ops, image_io as IO
    h, w = 7, 9
    p = IO.jpeg_encode_plan(h, w)
    q = torch.zeros((1, h, w, 3), dtype=torch.uint8, device=dev)
    out = torch.full((p.capacity,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(p.ws_bytes, dtype=torch.uint8, device=dev)
    good = dict(src=ops._p(q), ss=3 * h * w, dst=ops._p(out), ds=p.capacity, sizes=ops._p(sizes), ws=ops._p(ws), wsb=ws.numel(),
                qtab=ops._p(M._jpeg_table_on(q.device, 75)), B=1, h=h, w=w)

    def call(**kw):
        a = {**good, **kw}
        return _lib.lib().raw("cidnet_jpeg_encode_u8")(a["src"], a["ss"], a["dst"], a["ds"], a["sizes"], a["ws"], a["wsb"],
                                                       a["qtab"], a["B"], a["h"], a["w"], ops._stream())
    for bad in (dict(src=None), dict(dst=None), dict(sizes=None), dict(ws=None), dict(qtab=None), dict(h=0), dict(w=0), dict(B=0),
                dict(ds=p.capacity - 4), dict(ds=p.capacity + 1), dict(dst=out.data_ptr() + 1), dict(ws=ws.data_ptr() + 4),
                dict(sizes=sizes.data_ptr() + 4), dict(qtab=M._jpeg_table_on(q.device, 75).data_ptr() + 2),
                dict(ss=3 * h * w - 1)):
        assert call(**bad) == -1, bad
    assert call(wsb=ws.numel() - 1) == -3
    assert call(h=65501) == -2 and call(w=65501) == -2 and call(B=65536) == -2
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and sizes.item() == -7            # refused before any launch
    with pytest.raises(RuntimeError, match="CPU"):
        IO.jpeg_scan_u8(torch.zeros((2, 2, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        IO.jpeg_scan_u8(q, 0)
    with pytest.raises(RuntimeError):
        IO.jpeg_scan_u8(q.float())
