"""GPU: .png outputs encoded on the device (png="device") through enhance_folder, evaluate(save_dir=) and
evaluate_unpaired(save_dir=) with the reduced-width model: the files decode to exactly the pixels of the default run's, they
are png_file(png_zlib_u8(enhance_u8(...))) byte for byte, other extensions keep their bytes, the files do not depend on batch
size / threads / depth, the default launches nothing new and still writes Pillow's own bytes, and a bad value raises before a
worker starts.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402
from test_evaluate_gpu import _pairs  # noqa: E402
from test_evaluate_unpaired_gpu import PARAMS, _images as _unpaired_images  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["a0.png", "a1.PNG", "a2.bmp", "a3.jpg", "b0.png", "b1.PNG", "b2.bmp"]     # sorted; a*: 36 x 52, b*: 33 x 50
SIZES = [(36, 52)] * 4 + [(33, 50)] * 3
CFG = dict(gamma=1.4, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _pillow_png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "PNG")
    return buf.getvalue()


def _count_calls(L, seen):
    orig = L.call

    def call(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return orig(name, *args)
    L.call = call
    return orig


def test_enhance_folder_png_device(dev, tmp_path):
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
    for n, (h, w) in zip(NAMES, SIZES):
        Image.fromarray(rng.integers(0, 160, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(src, n),
                                                                                   format="PNG" if n.endswith(".PNG") else None)
    files = M.FolderImages([os.path.join(src, n) for n in NAMES], list(NAMES))
    with pytest.raises(ValueError, match="png"):
        P.enhance_folder(m, files, os.path.join(tmp, "bad"), png="gpu")
    assert not os.path.exists(os.path.join(tmp, "bad"))                     # raised before the output directory was made
    out = {k: os.path.join(tmp, k) for k in ("pillow", "device", "serial")}
    L, seen = _lib.lib(), {}
    orig = _count_calls(L, seen)
    try:
        rep_p = P.enhance_folder(m, files, out["pillow"], batch_size=4, threads=4, depth=2, **CFG)
        assert "cidnet_png_encode_u8" not in seen and rep_p.png == "pillow"  # the default: no new launch
        rep_d = P.enhance_folder(m, files, out["device"], batch_size=4, threads=4, depth=2, png="device", **CFG)
        assert seen["cidnet_png_encode_u8"] == len(rep_d.batches) == 2 and rep_d.png == "device"
    finally:
        L.call = orig
    assert rep_d.batches == rep_p.batches == [[0, 1, 2, 3], [4, 5, 6]]
    rep_s = P.enhance_folder(m, files, out["serial"], batch_size=1, threads=1, depth=1, png="device", **CFG)
    assert rep_s.batches == [[i] for i in range(len(NAMES))]
    for k in out:
        assert sorted(os.listdir(out[k])) == sorted(NAMES)
    for n, (h, w) in zip(NAMES, SIZES):
        a, b, c = (_read(os.path.join(out[k], n)) for k in ("pillow", "device", "serial"))
        assert b == c, n                                                     # depth / threads / batch size do not show
        if not n.lower().endswith(".png"):
            assert a == b, n                                                 # other extensions keep the Pillow path
            continue
        q = P.enhance_u8(m, torch.from_numpy(M._read_rgb(os.path.join(src, n))).to(dev), **CFG)
        assert a == _pillow_png(q[0].cpu().numpy()), n                       # the default writes what Pillow itself writes
        with Image.open(io.BytesIO(b)) as im:
            assert im.mode == "RGB" and im.format == "PNG" and np.array_equal(np.asarray(im), q[0].cpu().numpy()), n
        assert np.array_equal(M._read_rgb(os.path.join(out["device"], n)), M._read_rgb(os.path.join(out["pillow"], n))), n
        streams, sizes = P.png_zlib_u8(q)
        assert b == P.png_file(h, w, streams[0, :int(sizes[0])].cpu().numpy().tobytes()), n
        assert a != b
    assert m.training


def test_evaluate_png_device(dev, tmp_path):
    _in_child(_case_evaluate, str(tmp_path))


def _case_evaluate(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, metrics as M
    m = _model()
    pairs, _ = _pairs()
    cfg = dict(gamma=1.2, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)
    with pytest.raises(ValueError, match="png"):
        P.evaluate(m, pairs, save_dir=os.path.join(tmp, "bad"), png="zlib", **cfg)
    assert not os.path.exists(os.path.join(tmp, "bad"))
    L, seen = _lib.lib(), {}
    orig = _count_calls(L, seen)
    try:
        plain = P.evaluate(m, pairs, batch_size=4, save_dir=os.path.join(tmp, "pillow"), **cfg)
        assert "cidnet_png_encode_u8" not in seen
        device = P.evaluate(m, pairs, batch_size=4, save_dir=os.path.join(tmp, "device"), png="device", **cfg)
        assert seen["cidnet_png_encode_u8"] >= 1
    finally:
        L.call = orig
    assert device == plain                                                   # the scores do not know about the files
    names = [f"{i:05d}.png" for i in range(len(pairs))]
    assert sorted(os.listdir(os.path.join(tmp, "device"))) == sorted(os.listdir(os.path.join(tmp, "pillow"))) == names
    for n in names:
        a = M._read_rgb(os.path.join(tmp, "pillow", n))
        assert np.array_equal(M._read_rgb(os.path.join(tmp, "device", n)), a), n
        assert _read(os.path.join(tmp, "pillow", n)) == _pillow_png(a), n    # the default: Pillow's own bytes
        assert _read(os.path.join(tmp, "device", n)) != _read(os.path.join(tmp, "pillow", n))


def test_evaluate_unpaired_png_device(dev, tmp_path):
    _in_child(_case_unpaired, str(tmp_path))


class _Named(list):
    pass


def _case_unpaired(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, metrics as M
    m = _model()
    images = _Named(_unpaired_images(sizes=[(192, 288), (192, 288), (197, 290)]))      # NIQE needs several 96 x 96 blocks
    images.names = ["x0.png", "x1.jpg", "sub/x2.png"]
    prm = P.load_niqe_params(PARAMS)
    with pytest.raises(ValueError, match="png"):
        P.evaluate_unpaired(m, images, prm, save_dir=os.path.join(tmp, "bad"), png=True)
    assert not os.path.exists(os.path.join(tmp, "bad"))
    L, seen = _lib.lib(), {}
    orig = _count_calls(L, seen)
    try:
        plain = P.evaluate_unpaired(m, images, prm, alpha=0.9, batch_size=2, save_dir=os.path.join(tmp, "pillow"))
        assert "cidnet_png_encode_u8" not in seen
        device = P.evaluate_unpaired(m, images, prm, alpha=0.9, batch_size=2, save_dir=os.path.join(tmp, "device"), png="device")
        assert seen["cidnet_png_encode_u8"] == 2                             # a batch of .png + .jpg, then one .png
    finally:
        L.call = orig
    print("niqe, default:", plain.per_image["niqe"], "png=device:", device.per_image["niqe"])
    assert all(np.isfinite(plain.per_image["niqe"]))
    assert device.per_image == plain.per_image and device.niqe == plain.niqe
    for n in images.names:
        a, b = _read(os.path.join(tmp, "pillow", n)), _read(os.path.join(tmp, "device", n))
        if n.endswith(".jpg"):
            assert a == b, n
        else:
            pix = M._read_rgb(os.path.join(tmp, "pillow", n))
            assert a == _pillow_png(pix) and a != b, n
            assert np.array_equal(M._read_rgb(os.path.join(tmp, "device", n)), pix), n
