"""GPU: metrics.resize_u8 (csrc/resize.hip) equals PIL.Image.resize byte for byte -- no tolerance: for 8-bit images Pillow's
resampler is integer arithmetic over the tables metrics.resize_plan restates (tests/test_resize_cpu.py pins those)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _planar(imgs, dev):
    """uint8 (h,w,3) arrays -> uint8 (B,3,h,w) on the device"""
    return torch.from_numpy(np.stack([i.transpose(2, 0, 1) for i in imgs])).to(dev)


def _assert_equal(got, refs):
    got = got.cpu().numpy()
    assert got.shape == (len(refs), 3) + refs[0].shape[:2] and got.dtype == np.uint8
    for b, ref in enumerate(refs):
        bad = got[b] != ref.transpose(2, 0, 1)
        assert not bad.any(), (b, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("src,dst", R.CASES + [R.WIDE])
def test_equals_pil(dev, src, dst):
    """every shape with B = 1, on random bytes, on 0 / 255 (both ends of the clamp) and on a clipped normal; the cases with
    one axis unchanged would differ if the skipped pass still rounded"""
    from hvi_cidnet_amd import metrics as M
    for kind in R.KINDS:
        img = R.image(kind, *src)
        _assert_equal(M.resize_u8(_planar([img], dev), dst), [R.pil_resize(img, dst)])


@pytest.mark.parametrize("src,dst", [R.CASES[0], R.CASES[7]])
def test_batch_of_distinct_images(dev, src, dst):
    """B = 3 with a different image per sample: the batch and plane strides of both passes and of tmp"""
    from hvi_cidnet_amd import metrics as M
    imgs = [R.image(kind, *src, seed=3) for kind in R.KINDS]
    _assert_equal(M.resize_u8(_planar(imgs, dev), dst), [R.pil_resize(i, dst) for i in imgs])


def test_forms_and_errors(dev):
    from hvi_cidnet_amd import metrics as M
    img = R.image("random", 24, 40)
    q = _planar([img], dev)
    assert M.resize_u8(q, (24, 40)) is q and M.resize_u8(q[0], (24, 40)).data_ptr() == q.data_ptr()
    one = M.resize_u8(q[0], (17, 29))                          # (3,H,W) in, (3,h,w) out
    assert tuple(one.shape) == (3, 17, 29)
    _assert_equal(one.unsqueeze(0), [R.pil_resize(img, (17, 29))])
    flipped = q.flip(-1)                                       # a non-contiguous view is read as its values
    _assert_equal(M.resize_u8(flipped, (17, 29)), [R.pil_resize(np.ascontiguousarray(img[:, ::-1]), (17, 29))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.resize_u8(q.cpu(), (17, 29))
    with pytest.raises(RuntimeError, match="uint8"):
        M.resize_u8(q.float(), (17, 29))
    with pytest.raises(RuntimeError, match="expected"):
        M.resize_u8(q[:, :2], (17, 29))
    with pytest.raises(ValueError):
        M.resize_u8(q, (0, 29))
