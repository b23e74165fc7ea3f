"""GPU: metrics.evaluate_unpaired(file_roundtrip=True) -- an image named .jpg / .jpeg is scored as the file eval.py writes for
it decodes (metrics.jpeg_roundtrip_u8 of the quantized, cropped output), any other image as before; the saved .jpg, decoded
again by Pillow, is exactly what was scored.  NIQE values are compared bit for bit, NaN included: the same kernels on the
same bytes.  The three small images hold one 96 x 96 block each and so have no NIQE (fewer than two blocks: metrics.niqe_score
gives NaN); what reaches the scorer there is shown by LOE, by the launches and by the saved files, and the case of 192 x 200
images shows it in finite NIQE values.

Every case runs in a fresh spawned process, as in tests/test_evaluate_unpaired_gpu.py."""
import os
import struct
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402

pytestmark = pytest.mark.gpu
PARAMS = os.path.join(HERE, "golden", "niqe_pris_params.npz")
# a.jpg and b.png share a padded size, so batch_size=3 scores them in one call with different treatment; c.JPG is reflect-padded
SIZES = [(96, 104), (96, 104), (100, 96)]
NAMES = ["a.jpg", "b.png", "c.JPG"]
LOSSY = [True, False, True]
CFG = dict(alpha=0.9, gamma=1.2)


def _bits(values):
    return [struct.pack("<d", float(v)) for v in values]


def _sig(res):
    """a result with its floats as bit patterns, so that NaN compares equal to itself"""
    return (_bits([res.alpha, res.niqe, res.loe]), {k: (_bits(v) if k in ("niqe", "loe") else v) for k, v in res.per_image.items()},
            res.names, res.ensemble)


class _Named(list):
    """a list of images with the file names evaluate_unpaired reads (as metrics.folder_images carries them)"""

    def __init__(self, images, names):
        super().__init__(images)
        self.names = list(names)


def _images(names=NAMES, seed=11, sizes=SIZES):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([0.35 + 0.25 * np.sin(9 * xx + c) * np.cos(7 * yy - c) for c in range(3)])
        u8 = (np.clip(base + rng.normal(0, 0.06, (3, h, w)), 0.02, 0.9) * 255).astype(np.uint8)
        out.append(torch.from_numpy(u8).float().div(255))
    return _Named(out, names) if names is not None else out


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def _quantized_outputs(m, prm, sizes=SIZES):
    """the default run's quantized outputs, uint8 (3,h,w) on the device, read back from the lossless files it saves, and
    its result"""
    import hvi_cidnet_amd as P
    png = [f"{i}.png" for i in range(len(sizes))]
    with tempfile.TemporaryDirectory() as d:
        res = P.evaluate_unpaired(m, _images(png, sizes=sizes), prm, save_dir=d, **CFG)
        qs = [torch.from_numpy(_read(os.path.join(d, n))).permute(2, 0, 1).contiguous().cuda() for n in png]
    for q, v in zip(qs, res.per_image["niqe"]):                            # they are what that run scored
        assert _bits([P.metrics.niqe(q, prm).item()]) == _bits([v])
    return qs, res


def test_jpg_names_are_scored_as_their_decoded_files(dev):
    _in_child(_case_scores_and_files)


def _case_scores_and_files():
    import hvi_cidnet_amd as P
    M = P.metrics
    m = _model()
    prm = P.load_niqe_params(PARAMS)
    qs, base = _quantized_outputs(m, prm)
    with tempfile.TemporaryDirectory() as d:
        res = P.evaluate_unpaired(m, _images(), prm, file_roundtrip=True, save_dir=d, **CFG)
        saved = {n: _read(os.path.join(d, n)) for n in NAMES}
    assert res.per_image["file_roundtrip"] == LOSSY and res.names == NAMES
    assert _bits(res.per_image["niqe"][1:2]) == _bits(base.per_image["niqe"][1:2])      # b.png: bit-equal to the default run
    for i in (0, 2):
        r = M.jpeg_roundtrip_u8(qs[i])
        assert not torch.equal(r, qs[i])
        want = M.niqe(r, prm).item()
        print(NAMES[i], "niqe of the decoded file", res.per_image["niqe"][i], "of the output itself", base.per_image["niqe"][i])
        assert _bits([res.per_image["niqe"][i]]) == _bits([want])
        # save_dir received the un-round-tripped output: Pillow's own decode of that file is what was scored
        assert np.array_equal(saved[NAMES[i]], r.permute(1, 2, 0).cpu().numpy()), NAMES[i]
    assert np.array_equal(saved["b.png"], qs[1].permute(1, 2, 0).cpu().numpy())
    assert _bits([res.niqe]) == _bits([sum(res.per_image["niqe"]) / 3])
    assert m.training and not m.trans.gated2


def test_round_trip_moves_a_finite_niqe(dev):
    _in_child(_case_finite)


def _case_finite():
    """two images of four blocks each: NIQE is finite, and the .jpeg one's moves to that of its decoded file"""
    import hvi_cidnet_amd as P
    M = P.metrics
    m = _model()
    prm = P.load_niqe_params(PARAMS)
    sizes, names = [(192, 200), (192, 200)], ["x.jpeg", "y.bmp"]
    qs, base = _quantized_outputs(m, prm, sizes)
    res = P.evaluate_unpaired(m, _images(names, sizes=sizes), prm, batch_size=2, file_roundtrip=True, **CFG)
    got, plain = res.per_image["niqe"], base.per_image["niqe"]
    print("niqe with the round trip", got, "without", plain)
    assert np.isfinite(got).all() and np.isfinite(plain).all()
    assert res.per_image["file_roundtrip"] == [True, False]
    assert got[1] == plain[1] and got[0] != plain[0]
    assert got[0] == M.niqe(M.jpeg_roundtrip_u8(qs[0]), prm).item()
    assert res.niqe == (got[0] + got[1]) / 2


def test_batch_sizes_agree_on_mixed_names(dev):
    _in_child(_case_batch_sizes)


def _case_batch_sizes():
    import hvi_cidnet_amd as P
    m = _model()
    prm = P.load_niqe_params(PARAMS)
    r1 = P.evaluate_unpaired(m, _images(), prm, batch_size=1, file_roundtrip=True, loe=True, **CFG)
    r3 = P.evaluate_unpaired(m, _images(), prm, batch_size=3, file_roundtrip=True, loe=True, **CFG)
    assert _sig(r1) == _sig(r3) and r1.loe == r3.loe
    assert r1.per_image["file_roundtrip"] == LOSSY
    plain = P.evaluate_unpaired(m, _images(), prm, batch_size=3, loe=True, **CFG)
    print("loe with the round trip", r3.per_image["loe"], "without", plain.per_image["loe"])
    assert plain.per_image["loe"][1] == r3.per_image["loe"][1]
    assert plain.per_image["loe"][0] != r3.per_image["loe"][0] and plain.per_image["loe"][2] != r3.per_image["loe"][2]
    # LOE sees the round-tripped bytes too
    qs, _ = _quantized_outputs(m, prm)
    low = P.metrics.to_uint8(_images()[0].cuda())
    assert r1.per_image["loe"][0] == P.metrics.loe(low, P.metrics.jpeg_roundtrip_u8(qs[0])).item()


def test_default_is_unchanged_and_launches_nothing_new(dev):
    _in_child(_case_default)


def _case_default():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib
    m = _model()
    prm = P.load_niqe_params(PARAMS)
    L = _lib.lib()
    seen = {}
    orig = L.call

    def spy(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return orig(name, *args)
    L.call = spy
    try:
        omitted = P.evaluate_unpaired(m, _images(), prm, batch_size=3, **CFG)
        off = P.evaluate_unpaired(m, _images(), prm, batch_size=3, file_roundtrip=False, jpeg_quality=30, **CFG)
        assert "cidnet_metric_jpeg_roundtrip_u8" not in seen
        on = P.evaluate_unpaired(m, _images(), prm, batch_size=3, file_roundtrip=True, **CFG)
        assert seen["cidnet_metric_jpeg_roundtrip_u8"] == 2               # a.jpg out of its mixed batch, c.JPG
        unnamed = P.evaluate_unpaired(m, _images(None), prm, batch_size=3, file_roundtrip=True, **CFG)
        assert seen["cidnet_metric_jpeg_roundtrip_u8"] == 2               # unnamed images are untouched
        low = P.evaluate_unpaired(m, _images(), prm, batch_size=3, file_roundtrip=True, jpeg_quality=30, **CFG)
    finally:
        L.call = orig
    assert _sig(omitted) == _sig(off) and list(omitted.per_image) == ["niqe"]
    assert _bits(unnamed.per_image["niqe"]) == _bits(omitted.per_image["niqe"])
    assert unnamed.per_image["file_roundtrip"] == [False] * 3
    assert _bits(on.per_image["niqe"][1:2]) == _bits(omitted.per_image["niqe"][1:2])
    assert low.per_image["file_roundtrip"] == LOSSY
    sweep = P.evaluate_unpaired(m, _images(), prm, alpha=[0.9], gamma=1.2, batch_size=3, file_roundtrip=True)
    assert _sig(sweep[0]) == _sig(on)
    with pytest.raises(ValueError):
        P.evaluate_unpaired(m, _images(), prm, file_roundtrip=True, jpeg_quality=0)
