"""GPU: the PNG encoder on the device (csrc/png.hip through image_io.png_zlib_u8) against the numpy restatement of the stream
contract (tests/png_ref.py): the streams and their sizes are equal byte for byte, no tolerance; zlib and Pillow decode the
device's own files to the exact pixels.  The restatement's streams are computed once per module and shared."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
_ref = {}


def _want(kind, h, w, mode, seg):
    """-> (image, the restatement's stream, its filtered bytes), shared between the tests"""
    key = (kind, h, w, mode, seg)
    if key not in _ref:
        img = R.fibonacci_image() if kind == "fibonacci" else R.image(kind, h, w, 1000 * h + w)
        img.setflags(write=False)
        info = {}
        _ref[key] = (img, R.zlib_stream(img, mode, seg, info), info["filtered"])
    return _ref[key]


def _encode(dev, imgs, mode, seg):
    """a list of equal-sized images as ONE batch -> the streams as bytes, with the shape checks"""
    from hvi_cidnet_amd import image_io as IO
    q = torch.from_numpy(np.stack(imgs)).to(dev)
    streams, sizes = IO.png_zlib_u8(q, mode, seg)
    cap = IO.png_plan(q.shape[1], q.shape[2], seg).capacity
    assert streams.dtype == torch.uint8 and tuple(streams.shape) == (len(imgs), cap) and streams.is_cuda
    assert sizes.dtype == torch.int64 and tuple(sizes.shape) == (len(imgs),) and sizes.is_cuda
    host, n = streams.cpu().numpy(), sizes.cpu().tolist()
    for b in range(len(imgs)):
        assert 0 < n[b] <= cap and not host[b, n[b]:].any(), (b, n[b], cap)      # the rest of a slot is zero
    return [host[b, :n[b]].tobytes() for b in range(len(imgs))]


def _same(got, want, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        k = min(len(a), len(b))
        bad = np.flatnonzero(a[:k] != b[:k])
        print(what, "sizes", len(got), len(want), "first differing bytes", bad[:6].tolist())
    assert got == want, (what, len(got), len(want))


# the plan each case is there for at segments of 512 bytes: (rows per segment, segments, last short, a row exceeds the segment)
PLANS_512 = {(1, 1): (128, 1, 0, 0), (1, 5): (32, 1, 0, 0), (2, 3): (51, 1, 0, 0), (7, 9): (18, 1, 0, 0), (33, 47): (3, 11, 0, 0),
             (40, 56): (3, 14, 1, 0), (17, 300): (1, 17, 0, 1), (64, 96): (1, 64, 0, 0)}


@pytest.mark.parametrize("h,w", R.SIZES)
def test_streams_equal_the_restatement(dev, h, w):
    from hvi_cidnet_amd import image_io as IO
    from PIL import Image
    p = IO.png_plan(h, w, 512)
    assert (p.rows, p.segments, int(p.last_short), int(p.row_exceeds)) == PLANS_512[(h, w)], p
    p = IO.png_plan(h, w, 32768)
    assert p.segments == 1 and p.rows == 32768 // (1 + 3 * w) and not p.row_exceeds, p
    for seg in R.SEGMENTS:
        for mode in R.MODES:
            want = [_want(kind, h, w, mode, seg) for kind in R.KINDS]
            got = _encode(dev, [x[0] for x in want], mode, seg)
            for kind, g, (img, stream, filtered) in zip(R.KINDS, got, want):
                _same(g, stream, (kind, h, w, mode, seg))
                assert zlib.decompress(g) == filtered
                im = Image.open(io.BytesIO(IO.png_file(h, w, g)))
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), img), (kind, h, w, mode, seg)


def test_the_limiter_runs_on_the_device(dev):
    img, stream, filtered = _want("fibonacci", 48, 47, "none", 32768)
    freq = np.bincount(np.frombuffer(filtered, np.uint8), minlength=257)
    freq[256] = 1
    assert max(R.tree_depths({s: int(c) for s, c in enumerate(freq) if c}).values()) > 15
    got = _encode(dev, [img], "none", 32768)[0]
    _same(got, stream, "fibonacci")
    assert zlib.decompress(got) == filtered


def test_larger_image_many_chunks_per_segment(dev):
    """97 x 131: segments of 83 rows, 32702 bytes -- sixteen 2048-byte passes of the packer per block, the last one partial"""
    from hvi_cidnet_amd import image_io as IO
    h, w = 97, 131
    p = IO.png_plan(h, w)
    assert (p.rows, p.segments, p.last_short) == (83, 2, True), p
    for kind in ("grain", "constant"):
        img, stream, filtered = _want(kind, h, w, "adaptive", 32768)
        _same(_encode(dev, [img], "adaptive", 32768)[0], stream, (kind, h, w))


def test_batch_equals_each_alone_and_calls_repeat(dev):
    h, w = 40, 56
    imgs = [_want(kind, h, w, "adaptive", 512)[0] for kind in ("grain", "random", "saturated")]
    together = _encode(dev, imgs, "adaptive", 512)
    assert len(set(together)) == 3
    for img, t in zip(imgs, together):
        _same(_encode(dev, [img], "adaptive", 512)[0], t, "alone")
    for _ in range(3):
        assert _encode(dev, imgs, "adaptive", 512) == together


def test_single_image_input_and_convenience_form(dev):
    from hvi_cidnet_amd import image_io as IO
    h, w = 33, 47
    img, stream, _ = _want("grain", h, w, "adaptive", 32768)
    streams, sizes = IO.png_zlib_u8(torch.from_numpy(np.array(img)).to(dev))
    assert tuple(streams.shape) == (1, IO.png_plan(h, w).capacity) and tuple(sizes.shape) == (1,)
    _same(streams[0, :int(sizes[0])].cpu().numpy().tobytes(), stream, "(h,w,3)")
    files = IO.png_encode_u8(torch.from_numpy(np.array(img)).to(dev))
    assert files == [R.png_file(h, w, stream)]


def test_odd_address_and_batch_stride(dev):
    """the source at an odd address with a batch stride above 3 h w: no copy is made (image_io._images_u8) and the bytes hold"""
    from hvi_cidnet_amd import image_io as IO
    h, w = 7, 9
    imgs = [_want(kind, h, w, "paeth", 32768) for kind in ("grain", "random")]
    n = 3 * h * w
    flat = torch.zeros(1 + 2 * (n + 5), dtype=torch.uint8, device=dev)
    q = torch.as_strided(flat, (2, h, w, 3), (n + 5, 3 * w, 3, 1), 1)
    for b in range(2):
        q[b] = torch.from_numpy(np.array(imgs[b][0])).to(dev)
    assert q.data_ptr() % 2 == 1 and IO._images_u8(q, "test").data_ptr() == q.data_ptr()
    streams, sizes = IO.png_zlib_u8(q, "paeth")
    for b in range(2):
        _same(streams[b, :int(sizes[b])].cpu().numpy().tobytes(), imgs[b][1], b)


def test_nothing_outside_the_slots_is_written(dev):
    """the C entry point with guard bytes before, between and behind the slots and around sizes"""
    from hvi_cidnet_amd import _lib, ops, image_io as IO
    h, w, B, seg = 40, 56, 3, 512
    p = IO.png_plan(h, w, seg)
    imgs = [_want(kind, h, w, "adaptive", seg) for kind in ("grain", "random", "constant")]
    q = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
    stride = p.capacity + 64
    out = torch.full((16 + B * stride,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.full((B + 2,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(B * p.ws_bytes, dtype=torch.uint8, device=dev)
    _lib.lib().call("cidnet_png_encode_u8", ops._p(q), 3 * h * w, out.data_ptr() + 16, stride, sizes.data_ptr() + 8, ops._p(ws),
                    ws.numel(), B, h, w, 5, seg, ops._stream())
    torch.cuda.synchronize()
    host, n = out.cpu().numpy(), sizes.cpu().tolist()
    assert n[0] == -7 and n[-1] == -7
    assert (host[:16] == 0xA5).all()
    for b in range(B):
        slot = host[16 + b * stride:16 + (b + 1) * stride]
        _same(slot[:n[1 + b]].tobytes(), imgs[b][1], b)
        assert (slot[p.capacity:] == 0xA5).all() and not slot[n[1 + b]:p.capacity].any()


def test_refusals(dev):
    from hvi_cidnet_amd import _lib, ops, image_io as IO
    h, w = 7, 9
    p = IO.png_plan(h, w)
    q = torch.zeros((1, h, w, 3), dtype=torch.uint8, device=dev)
    out = torch.full((p.capacity,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(p.ws_bytes, dtype=torch.uint8, device=dev)
    good = dict(src=ops._p(q), ss=3 * h * w, dst=ops._p(out), ds=p.capacity, sizes=ops._p(sizes), ws=ops._p(ws), wsb=ws.numel(),
                B=1, h=h, w=w, filter=5, seg=32768)

    def call(**kw):
        a = {**good, **kw}
        return _lib.lib().raw("cidnet_png_encode_u8")(a["src"], a["ss"], a["dst"], a["ds"], a["sizes"], a["ws"], a["wsb"], a["B"],
                                                      a["h"], a["w"], a["filter"], a["seg"], ops._stream())
    for bad in (dict(src=None), dict(dst=None), dict(sizes=None), dict(ws=None), dict(h=0), dict(w=0), dict(B=0),
                dict(ds=p.capacity - 4), dict(filter=6), dict(filter=-1), dict(seg=0), dict(ss=3 * h * w - 1)):
        assert call(**bad) == -1, bad
    assert call(wsb=ws.numel() - 1) == -3
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and sizes.item() == -7            # refused before any launch
    with pytest.raises(RuntimeError, match="CPU"):
        IO.png_zlib_u8(torch.zeros((2, 2, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        IO.png_zlib_u8(q, "best")
    with pytest.raises(ValueError):
        IO.png_zlib_u8(q, "adaptive", 0)
    with pytest.raises(RuntimeError):
        IO.png_zlib_u8(q.float())
