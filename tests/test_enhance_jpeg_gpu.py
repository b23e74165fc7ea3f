"""GPU: .jpg / .jpeg outputs encoded on the device (jpeg="device") through enhance_folder, evaluate(save_dir=) and
evaluate_unpaired(save_dir=) with the reduced-width model: every file is BYTE-IDENTICAL to the default run's (Pillow's own),
whatever batch size / threads / depth / prefix, other extensions keep their bytes, png="device" combines with it, an image
whose scan exceeds the downloaded prefix takes the second copy and still comes out identical, the default makes no call of
the new entry point, and with file_roundtrip=True the saved device .jpg decodes to exactly what was scored.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegenc_ref as R  # noqa: E402
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402
from test_evaluate_gpu import _pairs  # noqa: E402
from test_evaluate_roundtrip_gpu import PARAMS, _bits, _sig, _images as _named_images, _read as _decode  # noqa: E402
from test_enhance_png_gpu import _count_calls, _read  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["a0.jpg", "a1.JPG", "a2.jpeg", "a3.png", "b0.bmp", "b1.jpg", "b2.png"]     # sorted; a*: 36 x 52, b*: 33 x 50
SIZES = [(36, 52)] * 4 + [(33, 50)] * 3
CFG = dict(gamma=1.4, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)
ENTRY = "cidnet_jpeg_encode_u8"


def _pillow_jpeg(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG")
    return buf.getvalue()


def _is_jpeg(name):
    return name.lower().endswith((".jpg", ".jpeg"))


def test_enhance_folder_jpeg_device(dev, tmp_path):
    _in_child(_case_folder, str(tmp_path))


def _case_folder(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, metrics as M
    from PIL import Image
    dev = torch.device("cuda:0")
    m = _model()
    rng = np.random.default_rng(31)
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    for n, (h, w) in zip(NAMES, SIZES):                                      # lossless inputs under lossy names
        Image.fromarray(rng.integers(0, 160, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(src, n), format="PNG")
    files = M.FolderImages([os.path.join(src, n) for n in NAMES], list(NAMES))
    with pytest.raises(ValueError, match="jpeg"):
        P.enhance_folder(m, files, os.path.join(tmp, "bad"), jpeg="gpu")
    assert not os.path.exists(os.path.join(tmp, "bad"))                     # raised before the output directory was made
    out = {k: os.path.join(tmp, k) for k in ("pillow", "device", "serial", "both")}
    L, seen = _lib.lib(), {}
    orig = _count_calls(L, seen)
    try:
        rep_p = P.enhance_folder(m, files, out["pillow"], batch_size=4, threads=4, depth=2, **CFG)
        assert ENTRY not in seen and rep_p.jpeg == "pillow" and rep_p.jpeg_second_copies == 0      # the default: no new call
        rep_d = P.enhance_folder(m, files, out["device"], batch_size=4, threads=4, depth=2, jpeg="device", **CFG)
        assert seen[ENTRY] == len(rep_d.batches) == 2 and rep_d.jpeg == "device" and "cidnet_png_encode_u8" not in seen
        rep_b = P.enhance_folder(m, files, out["both"], batch_size=4, threads=4, depth=2, jpeg="device", png="device", **CFG)
        assert seen[ENTRY] == 4 and seen["cidnet_png_encode_u8"] == 2 and (rep_b.jpeg, rep_b.png) == ("device", "device")
    finally:
        L.call = orig
    assert rep_d.batches == rep_p.batches == rep_b.batches == [[0, 1, 2, 3], [4, 5, 6]]
    rep_s = P.enhance_folder(m, files, out["serial"], batch_size=1, threads=1, depth=1, jpeg="device", **CFG)
    assert rep_s.batches == [[i] for i in range(len(NAMES))]
    for k in out:
        assert sorted(os.listdir(out[k])) == sorted(NAMES)
    for n, (h, w) in zip(NAMES, SIZES):
        a, b, c, d = (_read(os.path.join(out[k], n)) for k in ("pillow", "device", "serial", "both"))
        assert a == b == c, n                      # the device's file IS Pillow's; depth / threads / batch size do not show
        if _is_jpeg(n):
            q = P.enhance_u8(m, torch.from_numpy(M._read_rgb(os.path.join(src, n))).to(dev), **CFG)
            assert a == _pillow_jpeg(q[0].cpu().numpy()) == d, n              # what Pillow itself writes of the enhanced image
            assert P.jpeg_encode_u8(q) == [a], n
            with Image.open(io.BytesIO(b)) as im:
                assert im.format == "JPEG" and im.size == (w, h)
        elif n.endswith(".png"):                                             # png="device" took these, as without jpeg=
            assert d != a and np.array_equal(M._read_rgb(os.path.join(out["both"], n)), M._read_rgb(os.path.join(out["pillow"], n))), n
        else:
            assert d == a, n
    assert m.training


def test_second_copy_when_the_scan_exceeds_the_prefix(dev, tmp_path):
    _in_child(_case_second_copy, str(tmp_path))


def _case_second_copy(tmp):
    """_Writer itself: noise (a scan of about 0.2 x raw at quality 75, so the default 0.25 would hold it) beside a flat image,
    with a prefix of 0.1 x raw rounded up to 4 KiB"""
    from hvi_cidnet_amd import image_io as IO
    dev = torch.device("cuda:0")
    h, w = 96, 128
    noise, flat = R.case_image("random", h, w), R.case_image("constant", h, w)
    prefix = 4096                                                            # 0.1 * 3 h w = 3686, rounded up to 4 KiB
    sizes = [len(R.scan(x, 75)[0]) for x in (noise, flat)]
    print("scan bytes (noise, flat):", sizes, "raw:", 3 * h * w, "prefix:", prefix)
    assert sizes[0] > prefix > sizes[1]                                       # the premise, on the CPU restatement
    q = torch.from_numpy(np.stack([x.transpose(1, 2, 0) for x in (noise, flat)])).to(dev)
    want = [R.pil_file(x, 75) for x in (noise, flat)]
    for frac, second in ((0.1, 1), (8.0, 0)):                                 # a prefix as large as the slot never needs one
        paths = [os.path.join(tmp, f"{frac}_{k}.jpg") for k in range(2)]
        with torch.cuda.device(dev):
            wr = IO._Writer(dev, threads=2, depth=1, jpeg="device", jpeg_prefix=frac)
            wr.put(q, paths)
            wr.close()
        assert wr.second_copies == second, (frac, wr.second_copies)
        assert [_read(p) for p in paths] == want, frac
        cap = IO.jpeg_encode_plan(h, w).capacity
        head = 16
        assert wr.downloaded == (head + 2 * prefix + sizes[0] - prefix if second else head + 2 * cap), (frac, wr.downloaded)


def test_evaluate_jpeg_device(dev, tmp_path):
    _in_child(_case_evaluate, str(tmp_path))


class _Named(list):
    pass


def _case_evaluate(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib
    m = _model()
    pairs = _Named(_pairs()[0])
    pairs.names = [f"{i:02d}" + (".jpg", ".png", ".JPEG")[i % 3] for i in range(len(pairs))]
    cfg = dict(gamma=1.2, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)
    with pytest.raises(ValueError, match="jpeg"):
        P.evaluate(m, pairs, save_dir=os.path.join(tmp, "bad"), jpeg="turbo", **cfg)
    assert not os.path.exists(os.path.join(tmp, "bad"))
    L, seen = _lib.lib(), {}
    orig = _count_calls(L, seen)
    try:
        plain = P.evaluate(m, pairs, batch_size=4, save_dir=os.path.join(tmp, "pillow"), **cfg)
        assert ENTRY not in seen
        device = P.evaluate(m, pairs, batch_size=4, save_dir=os.path.join(tmp, "device"), jpeg="device", **cfg)
        assert seen[ENTRY] >= 1
    finally:
        L.call = orig
    assert device == plain                                                   # the scores do not know about the files
    assert sorted(os.listdir(os.path.join(tmp, "device"))) == sorted(os.listdir(os.path.join(tmp, "pillow"))) == sorted(pairs.names)
    for n in pairs.names:
        assert _read(os.path.join(tmp, "device", n)) == _read(os.path.join(tmp, "pillow", n)), n


def test_evaluate_unpaired_jpeg_device_and_file_roundtrip(dev, tmp_path):
    _in_child(_case_unpaired, str(tmp_path))


def _case_unpaired(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib
    M = P.metrics
    m = _model()
    images = _named_images()                                                 # a.jpg, b.png, c.JPG; a and b share a batch
    prm = P.load_niqe_params(PARAMS)
    cfg = dict(alpha=0.9, gamma=1.2, batch_size=2, file_roundtrip=True)
    with pytest.raises(ValueError, match="jpeg"):
        P.evaluate_unpaired(m, images, prm, save_dir=os.path.join(tmp, "bad"), jpeg=True)
    assert not os.path.exists(os.path.join(tmp, "bad"))
    L, seen = _lib.lib(), {}
    orig = _count_calls(L, seen)
    try:
        plain = P.evaluate_unpaired(m, images, prm, save_dir=os.path.join(tmp, "pillow"), **cfg)
        assert ENTRY not in seen
        device = P.evaluate_unpaired(m, images, prm, save_dir=os.path.join(tmp, "device"), jpeg="device", **cfg)
        assert seen[ENTRY] == 2                                              # a batch of .jpg + .png, then one .JPG
    finally:
        L.call = orig
    print("niqe, default:", plain.per_image["niqe"], "jpeg=device:", device.per_image["niqe"])
    assert _sig(device) == _sig(plain)                                       # bit patterns: a NaN score compares equal to itself
    assert plain.per_image["file_roundtrip"] == [True, False, True]
    for i, n in enumerate(images.names):
        assert _read(os.path.join(tmp, "device", n)) == _read(os.path.join(tmp, "pillow", n)), n
        if _is_jpeg(n):                                                      # Pillow's decode of the DEVICE's file is what was scored
            r = torch.from_numpy(_decode(os.path.join(tmp, "device", n))).permute(2, 0, 1).contiguous().cuda()
            assert _bits([M.niqe(r, prm).item()]) == _bits([device.per_image["niqe"][i]]), n
