"""GPU: the JPEG file round trip on the device (csrc/jpeg.hip through metrics.jpeg_roundtrip_u8) against Pillow itself: what
Image.open() returns for the file Image.save(buf, 'JPEG', quality=q) writes (tests/jpeg_ref.py: pil_roundtrip).  Integer
arithmetic on both sides: every comparison is byte equality, no tolerance.  Pillow's answers are computed once per module."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
_pil = {}


def _case(kind, h, w, quality=75):
    """-> (image, Pillow's round trip), uint8 (3,h,w), both read-only and shared between the tests"""
    key = (kind, h, w, quality)
    if key not in _pil:
        img = R.image(kind, h, w, 1000 * h + w)
        want = R.pil_roundtrip(img, quality)
        img.setflags(write=False)
        want.setflags(write=False)
        _pil[key] = (img, want)
    return _pil[key]


def _plan(h, w):
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_int * 9)()
    assert _lib.lib().raw("cidnet_metric_jpeg_plan")(h, w, buf, 9) == 0
    return dict(zip(("mcu_cols", "mcu_rows", "partial_right", "partial_bottom", "ch", "cw", "tiles_x", "blocks", "ws"), buf))


def _run(dev, img, quality=75):
    from hvi_cidnet_amd import metrics as M
    out = M.jpeg_roundtrip_u8(torch.from_numpy(np.array(img)).to(dev), quality)
    assert out.dtype == torch.uint8 and out.shape == img.shape and out.device.type == "cuda"
    return out.cpu().numpy()


def _same(got, want, what):
    bad = np.argwhere(got != want)
    print(what, "differing bytes:", len(bad))
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist())


# the path each case is there for: (partial right, partial bottom, MCU columns, MCU rows)
PATHS = {(1, 5): (1, 1, 1, 1), (7, 9): (1, 1, 1, 1), (8, 8): (1, 1, 1, 1), (15, 17): (1, 1, 2, 1), (16, 16): (0, 0, 1, 1),
         (18, 34): (1, 1, 3, 2), (24, 24): (1, 1, 2, 2), (31, 33): (1, 1, 3, 2), (40, 56): (1, 1, 4, 3), (50, 70): (1, 1, 5, 4),
         (64, 96): (0, 0, 6, 4), (97, 131): (1, 1, 9, 7)}


@pytest.mark.parametrize("h,w", R.CASES)
def test_equals_pillow_byte_for_byte(dev, h, w):
    p = _plan(h, w)
    assert (p["partial_right"], p["partial_bottom"], p["mcu_cols"], p["mcu_rows"]) == PATHS[(h, w)], p
    if (h, w) in ((18, 34), (24, 24), (40, 56), (50, 70)):                 # even height, partial bottom MCU: the padding rule
        assert h % 2 == 0 and p["partial_bottom"] == 1 and 8 * p["mcu_rows"] > p["ch"]
    for kind in R.KINDS:
        img, want = _case(kind, h, w)
        _same(_run(dev, img), want, (kind, h, w))


def test_wide_image_spans_workgroups(dev):
    h, w = R.WIDE
    p = _plan(h, w)
    assert p["tiles_x"] == 3 and p["mcu_rows"] == 3 and p["blocks"] == 9 and p["mcu_cols"] < 8 * p["tiles_x"], p
    for kind in R.KINDS:
        img, want = _case(kind, h, w)
        _same(_run(dev, img), want, (kind, h, w))


@pytest.mark.parametrize("quality", [1, 100])
def test_other_qualities(dev, quality):
    for kind in R.KINDS:
        img, want = _case(kind, 50, 70, quality)
        _same(_run(dev, img, quality), want, (kind, quality))


def test_batch_of_distinct_images_and_repeated_calls(dev):
    """B = 3: the batch and plane strides of src, dst and the workspace; two calls agree bit for bit; an image's bytes are the
    same alone and inside the batch"""
    from hvi_cidnet_amd import metrics as M
    h, w = 50, 70
    cases = [_case(kind, h, w) for kind in ("random", "ramp", "saturated")]
    batch = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
    a = M.jpeg_roundtrip_u8(batch)
    b = M.jpeg_roundtrip_u8(batch)
    assert a.shape == (3, 3, h, w) and torch.equal(a, b)
    assert torch.equal(batch, torch.from_numpy(np.stack([c[0] for c in cases])).to(dev))       # the input is left alone
    for i, (img, want) in enumerate(cases):
        _same(a[i].cpu().numpy(), want, ("batch", i))
        assert torch.equal(M.jpeg_roundtrip_u8(batch[i:i + 1])[0], a[i])


def test_forms_views_and_alignment(dev):
    from hvi_cidnet_amd import _lib, metrics as M
    h, w = 31, 33
    img, want = _case("random", h, w)
    t = torch.from_numpy(np.array(img)).to(dev)
    one = M.jpeg_roundtrip_u8(t)                                           # (3,h,w) in, (3,h,w) out
    assert one.shape == (3, h, w)
    _same(one.cpu().numpy(), want, "3-dimensional")
    # a flipped view is read as its values: Pillow on the flipped array
    flipped = torch.flip(t, dims=(2,))
    view = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 2, 0))).to(dev).permute(2, 0, 1)
    assert not view.is_contiguous()
    _same(M.jpeg_roundtrip_u8(view).cpu().numpy(), want, "channel-last view")
    _same(M.jpeg_roundtrip_u8(flipped).cpu().numpy(), R.pil_roundtrip(img[:, :, ::-1], 75), "flipped")
    big = torch.zeros((3, h + 4, w + 6), dtype=torch.uint8, device=dev)
    big[:, 1:1 + h, 3:3 + w] = t
    assert not big[:, 1:1 + h, 3:3 + w].is_contiguous()
    _same(M.jpeg_roundtrip_u8(big[:, 1:1 + h, 3:3 + w]).cpu().numpy(), want, "window view")
    # the C entry point on odd byte addresses; w = 56 is a multiple of 4, so an aligned dst takes the dword stores (above, in
    # test_equals_pillow_byte_for_byte) and this one must not
    h, w = 40, 56
    img, want = _case("random", h, w)
    n = 3 * h * w
    L = _lib.lib()
    src = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    dst = torch.full((n + 16,), 77, dtype=torch.uint8, device=dev)
    src[3:3 + n] = torch.from_numpy(np.array(img)).to(dev).reshape(-1)
    nws = L.raw("cidnet_metric_jpeg_ws_bytes")(1, h, w)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    qtab = torch.from_numpy(M.jpeg_quant_plan(75).device_table()).to(dev)
    with torch.cuda.device(dev):
        L.call("cidnet_metric_jpeg_roundtrip_u8", src.data_ptr() + 3, dst.data_ptr() + 5, ws.data_ptr(), nws, qtab.data_ptr(), 1, h,
               w, torch.cuda.current_stream().cuda_stream)
    got = dst.cpu().numpy()
    _same(got[5:5 + n].reshape(3, h, w), want, "odd addresses")
    assert (got[:5] == 77).all() and (got[5 + n:] == 77).all()            # not one byte outside the image


def test_errors(dev):
    from hvi_cidnet_amd import metrics as M
    ok = torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.jpeg_roundtrip_u8(ok.cpu())
    with pytest.raises(RuntimeError, match="uint8"):
        M.jpeg_roundtrip_u8(ok.float())
    with pytest.raises(RuntimeError):
        M.jpeg_roundtrip_u8(torch.zeros((1, 4, 8, 8), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        M.jpeg_roundtrip_u8(torch.zeros((1, 3, 8, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        M.jpeg_roundtrip_u8(torch.zeros((1, 3, 0, 8), dtype=torch.uint8, device=dev))
    for q in (0, 101, 75.5):
        with pytest.raises(ValueError):
            M.jpeg_roundtrip_u8(ok, q)
    assert M.jpeg_roundtrip_u8(ok).shape == ok.shape
