"""GPU: metrics.evaluate_unpaired(brisque=params) -- every output is also scored with BRISQUE on the bytes NIQE sees (after the
JPEG file round trip where file_roundtrip=True applies), per_image["brisque"] after "niqe" and "loe", the mean the running sum
in input order; brisque=None launches nothing new and returns what the call without the keyword returns.  Values are compared
bit for bit, NaN included: the same kernels on the same bytes (the three small images hold one 96 x 96 block each and so
have no NIQE).

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
# a.jpg and b.png share a padded size, so batch_size=3 scores them in one call; c.JPG is reflect-padded
SIZES = [(96, 104), (96, 104), (100, 96)]
NAMES = ["a.jpg", "b.png", "c.JPG"]
CFG = dict(alpha=0.9, gamma=1.2)


def _bits(values):
    return [struct.pack("<d", float(v)) for v in values]


def _sig(res):
    """a result with its floats as bit patterns, so that NaN compares equal to itself"""
    return (_bits([res.alpha, res.niqe, res.loe, res.brisque]),
            {k: (_bits(v) if k in ("niqe", "loe", "brisque") else v) for k, v in res.per_image.items()}, list(res.per_image),
            res.names, res.ensemble)


class _Named(list):
    def __init__(self, images, names):
        super().__init__(images)
        self.names = list(names)


def _images(names=NAMES, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in SIZES:
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([0.35 + 0.25 * np.sin(9 * xx + c) * np.cos(7 * yy - c) for c in range(3)])
        u8 = (np.clip(base + rng.normal(0, 0.06, (3, h, w)), 0.02, 0.9) * 255).astype(np.uint8)
        out.append(torch.from_numpy(u8).float().div(255))
    return _Named(out, names)


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def _quantized_outputs(m, prm):
    """the quantized outputs, uint8 (3,h,w) on the device, read back from the lossless files a default run saves"""
    import hvi_cidnet_amd as P
    png = [f"{i}.png" for i in range(len(SIZES))]
    with tempfile.TemporaryDirectory() as d:
        P.evaluate_unpaired(m, _images(png), prm, save_dir=d, **CFG)
        return [torch.from_numpy(_read(os.path.join(d, n))).permute(2, 0, 1).contiguous().cuda() for n in png]


def test_brisque_column_is_brisque_of_the_saved_outputs(dev):
    _in_child(_case_column)


def _case_column():
    import hvi_cidnet_amd as P
    M = P.metrics
    m = _model()
    prm = P.load_niqe_params(PARAMS)
    bp = M.BrisqueParams.random(3)
    qs = _quantized_outputs(m, prm)
    plain = P.evaluate_unpaired(m, _images(), prm, **CFG)
    res = P.evaluate_unpaired(m, _images(), prm, brisque=bp, **CFG)
    assert list(res.per_image) == ["niqe", "brisque"]
    want = [M.brisque(q, bp).item() for q in qs]
    print("brisque per image", res.per_image["brisque"], "of the saved outputs", want)
    assert np.isfinite(want).all() and len(set(want)) == 3
    assert _bits(res.per_image["brisque"]) == _bits(want)
    acc = 0.0
    for v in want:
        acc += v
    assert _bits([res.brisque]) == _bits([acc / 3])
    assert _bits(res.per_image["niqe"]) == _bits(plain.per_image["niqe"]) and _bits([res.niqe]) == _bits([plain.niqe])
    # key order niqe, loe, brisque; batches and an alpha sweep agree with the single run
    both = P.evaluate_unpaired(m, _images(), prm, brisque=bp, loe=True, batch_size=3, **CFG)
    assert list(both.per_image) == ["niqe", "loe", "brisque"]
    assert _bits(both.per_image["brisque"]) == _bits(want) and _bits([both.brisque]) == _bits([res.brisque])
    loe_only = P.evaluate_unpaired(m, _images(), prm, loe=True, batch_size=3, **CFG)
    assert _bits(both.per_image["loe"]) == _bits(loe_only.per_image["loe"])
    sweep = P.evaluate_unpaired(m, _images(), prm, alpha=[0.9], gamma=1.2, brisque=bp)
    assert _sig(sweep[0]) == _sig(res)
    assert m.training and not m.trans.gated2


def test_none_is_unchanged_and_launches_nothing_new(dev):
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
        omitted = P.evaluate_unpaired(m, _images(), prm, batch_size=3, loe=True, **CFG)
        off = P.evaluate_unpaired(m, _images(), prm, batch_size=3, loe=True, brisque=None, **CFG)
        assert not any("brisque" in k for k in seen), seen
        on = P.evaluate_unpaired(m, _images(), prm, batch_size=3, loe=True, brisque=P.metrics.BrisqueParams.random(3), **CFG)
        assert seen["cidnet_metric_brisque_features"] == 2 and seen["cidnet_metric_brisque_svr"] == 2      # two runs of equal size
    finally:
        L.call = orig
    assert _sig(omitted) == _sig(off) and list(omitted.per_image) == ["niqe", "loe"]
    assert np.isnan(omitted.brisque) and np.isnan(off.brisque) and np.isfinite(on.brisque)
    assert _bits(on.per_image["loe"]) == _bits(omitted.per_image["loe"])
    with pytest.raises(ValueError, match="BRISQUE needs"):
        P.evaluate_unpaired(m, _images(), prm, brisque="model-only.txt", **CFG)


def test_jpg_names_are_scored_after_the_round_trip(dev):
    _in_child(_case_roundtrip)


def _case_roundtrip():
    import hvi_cidnet_amd as P
    M = P.metrics
    m = _model()
    prm = P.load_niqe_params(PARAMS)
    bp = M.BrisqueParams.random(3)
    qs = _quantized_outputs(m, prm)
    plain = P.evaluate_unpaired(m, _images(), prm, brisque=bp, batch_size=3, **CFG)
    res = P.evaluate_unpaired(m, _images(), prm, brisque=bp, batch_size=3, file_roundtrip=True, **CFG)
    assert res.per_image["file_roundtrip"] == [True, False, True]
    assert list(res.per_image) == ["niqe", "brisque", "file_roundtrip"]
    got, before = res.per_image["brisque"], plain.per_image["brisque"]
    print("brisque with the round trip", got, "without", before)
    assert _bits(got[1:2]) == _bits(before[1:2])
    for i in (0, 2):
        r = M.jpeg_roundtrip_u8(qs[i])
        assert not torch.equal(r, qs[i])
        assert _bits([got[i]]) == _bits([M.brisque(r, bp).item()]) and got[i] != before[i]
    assert _bits([res.brisque]) == _bits([(got[0] + got[1] + got[2]) / 3])
