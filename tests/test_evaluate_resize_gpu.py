"""GPU: metrics.evaluate(resize=True) scores a pair whose ground truth has another size as measure.py scores it -- bit for
bit what psnr_ssim gives for the saved file read back, resized by PIL on the host and uploaded again.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402
from evaluate_harness import in_child as _in_child, model as _model, two_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
# (input, ground truth): two larger ground truths of one size (one launch resizes both at batch_size 4), one of the input's
# size, and a smaller one for the 17 x 29 input, which is reflect-padded to 24 x 32 and cropped
SIZES = [((24, 40), (33, 52)), ((24, 40), (33, 52)), ((24, 40), (24, 40)), ((17, 29), (13, 21))]
RESIZED = [0, 1, 3]
KEYS = ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")


def _pairs(seed=11):
    rng = np.random.default_rng(seed)
    pairs = []
    for (h, w), (gh, gw) in SIZES:
        low = torch.from_numpy(rng.random((3, h, w), dtype=np.float32) * 0.6 + 0.05)
        pairs.append((low, np.clip(rng.normal(140, 60, (gh, gw, 3)), 0, 255).astype(np.uint8)))
    return pairs


class _Named(list):
    names = None


def test_scores_equal_pil_resize_of_the_saved_files(dev, tmp_path):
    _in_child(_case_saved_files, str(tmp_path))


def _case_saved_files(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    from PIL import Image
    m = _model()
    pairs = _pairs()
    with pytest.raises(ValueError, match="differ in size"):                 # the default is what it was
        P.evaluate(m, pairs)
    res = P.evaluate(m, pairs, gamma=1.2, gated=True, resize=True, save_dir=tmp)
    assert res.resized == RESIZED and res.names == list(range(len(pairs)))
    for i, ((h, w), (gh, gw)) in enumerate(SIZES):
        with Image.open(os.path.join(tmp, f"{i:05d}.png")) as im:
            assert im.size == (w, h)                                         # the file is the un-resized output
            q = np.array(im.convert("RGB").resize((gw, gh)))
        q = torch.from_numpy(q).permute(2, 0, 1).contiguous().cuda()
        g = torch.from_numpy(pairs[i][1]).permute(2, 0, 1).contiguous().cuda()
        for gm, sfx in ((False, ""), (True, "_gt_mean")):
            p, s = M.psnr_ssim(q, g, gt_mean=gm)
            assert res.per_image["psnr" + sfx][i] == p.item(), (i, sfx)
            assert res.per_image["ssim" + sfx][i] == s.item(), (i, sfx)
    for k in KEYS:
        assert getattr(res, k) == sum(res.per_image[k]) / len(pairs)
    same = P.evaluate(m, [pairs[2]], gamma=1.2, gated=True)                 # a same-size pair: resize=True changes nothing
    assert same.resized == [] and all(same.per_image[k][0] == res.per_image[k][2] for k in KEYS)
    nested = _Named(pairs[:2])                                               # names as nested_folder_pairs gives them
    nested.names = ["0001/a.png", "0002/b.png"]
    sub = P.evaluate(m, nested, gamma=1.2, gated=True, resize=True, save_dir=os.path.join(tmp, "nested"), batch_size=2)
    assert sub.names == nested.names and all(sub.per_image[k] == res.per_image[k][:2] for k in KEYS)
    for name in nested.names:
        with Image.open(os.path.join(tmp, "nested", name)) as im:
            assert im.size == (40, 24)
    with pytest.raises(RuntimeError, match="11 x 11"):                       # as ssim() raises
        P.evaluate(m, [(pairs[0][0], np.zeros((10, 30, 3), np.uint8))], resize=True)


def test_batches_and_alpha_sweeps_agree(dev):
    _in_child(_case_batches_and_sweeps)


def _case_batches_and_sweeps():
    import hvi_cidnet_amd as P
    m = _model()
    pairs = _pairs()
    r1 = P.evaluate(m, pairs, gated=True, resize=True, batch_size=1)
    r4 = P.evaluate(m, pairs, gated=True, resize=True, batch_size=4)
    assert r1.resized == RESIZED
    assert r1 == r4                                                          # values, means and `resized`, bit for bit
    alphas = [0.9, 1.0]
    sweep = P.evaluate(m, pairs, gated2=True, alpha=alphas, resize=True, batch_size=4)
    single = [P.evaluate(m, pairs, gated2=True, alpha=a, resize=True, batch_size=4) for a in alphas]
    assert [r.alpha for r in sweep] == alphas and sweep == single
    assert sweep[0].per_image["psnr"] != sweep[1].per_image["psnr"]
    assert m.trans.alpha == 1.0 and m.training


@pytest.mark.timeout(600)
def test_two_ranks_report_the_same_resized_pairs(dev):
    """two ranks sharing the GPU over gloo: rank r resizes and measures pairs i % 2 == r, and both return exactly the
    single-process values -- `resized` included, which travels with them through the all-reduce"""
    got = two_ranks(_case_sharded)
    ref = _in_child(_case_sharded)
    assert ref[0] == RESIZED and got[0] == ref and got[1] == ref


def _case_sharded():
    import hvi_cidnet_amd as P
    r = P.evaluate(_model(), _pairs(), gated=True, resize=True, batch_size=1)
    return r.resized, r.psnr, r.ssim, r.psnr_gt_mean, r.ssim_gt_mean, r.per_image
