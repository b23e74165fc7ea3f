"""CPU checks of the evaluation metrics: the fp64 restatement the GPU tests compare against (tests/metrics_ref.py),
folder_pairs' file pairing, the refusal of CPU tensors, the input converter's shapes, and the index arithmetic of an
evaluation (batches, runs of equal crop size, the rows they fill) against the per-image loop."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as R  # noqa: E402


def test_gaussian_window_closed_form():
    g = R.gaussian_1d()
    raw = np.array([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)])
    assert np.allclose(g, raw / raw.sum(), rtol=0, atol=1e-16)
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1])
    w = R.gaussian_window()
    assert w.shape == (11, 11) and abs(w.sum() - 1.0) < 1e-14
    assert abs(w[5, 5] - g[5] ** 2) < 1e-18


def test_separable_filter_equals_the_2d_window():
    from scipy.signal import correlate2d
    x = np.random.default_rng(0).integers(0, 256, (23, 31)).astype(np.float64)
    d = np.abs(R.filter_valid(x) - correlate2d(x, R.gaussian_window(), mode="valid")).max()
    assert d < 1e-11


def test_gray_rule_on_hand_values():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [128, 64, 32]], dtype=np.uint8)
    img = px.T.reshape(3, 1, -1)
    assert R.gray(img).ravel().tolist() == [76, 150, 29, 255, 0, (4899 * 128 + 9617 * 64 + 1868 * 32 + 8192) >> 14]


def test_psnr_of_identical_images():
    a = np.random.default_rng(1).integers(0, 256, (3, 16, 20), dtype=np.uint8)
    expect = 10 * math.log10(65025 / 1e-8)
    assert R.psnr(a, a) == pytest.approx(expect, abs=1e-12)
    assert R.psnr(a, a, gt_mean=True) == pytest.approx(expect, abs=1e-12)
    assert abs(R.ssim(a, a) - 1.0) < 1e-14


def _png(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path)


def test_folder_pairs(tmp_path):
    import hvi_cidnet_amd as P
    low, high = tmp_path / "low", tmp_path / "high"
    low.mkdir()
    high.mkdir()
    rng = np.random.default_rng(2)
    imgs = {n: rng.integers(0, 256, (6, 5, 3), dtype=np.uint8) for n in ("b.png", "a.png", "c.bmp", "d.png", "e.png")}
    for n, im in imgs.items():
        _png(low / n, im)
    _png(high / "a.png", imgs["a.png"][::-1].copy())     # same name
    _png(high / "b.PNG", imgs["b.png"])                  # stem + .PNG, after .png (absent)
    _png(high / "c.png", imgs["c.bmp"])                  # stem + .jpg wins over stem + .png
    _png(high / "c.jpg", imgs["c.bmp"])
    _png(high / "e.JPEG", imgs["e.png"])                 # d has no ground truth
    (low / "notes.txt").write_text("not an image")
    with pytest.warns(UserWarning, match="d.png"):
        pairs = P.folder_pairs(str(low), str(high))
    assert pairs.names == ["a.png", "b.png", "c.bmp", "e.png"]
    assert pairs.skipped == ["d.png"]
    assert len(pairs) == 4
    assert [os.path.basename(g) for _, g in pairs.paths] == ["a.png", "b.PNG", "c.jpg", "e.JPEG"]
    lo, gt = pairs[0]
    assert lo.dtype == torch.float32 and tuple(lo.shape) == (3, 6, 5)
    assert torch.equal(lo, torch.from_numpy(imgs["a.png"]).permute(2, 0, 1).float().div(255))
    assert gt.dtype == np.uint8 and np.array_equal(gt, imgs["a.png"][::-1])


def test_metrics_refuse_cpu_tensors():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    q = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.to_uint8(torch.rand(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.psnr(q, q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.ssim(q, q, gt_mean=True)
    m = P.CIDNet(channels=[12, 12, 24, 48])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.evaluate(m, [(torch.rand(3, 16, 16), np.zeros((16, 16, 3), np.uint8))])
    assert m.training                                    # nothing was touched


def test_psnr_ssim_launcher_checks_on_the_host():
    import ctypes
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                       # never dereferenced: every call returns before a launch
    # tiles of 64 x 32: 10 x 13 per plane, two 8-byte words each, counted as floats; no scale slot, no gray partials
    assert L.raw("cidnet_metric_ws_floats")(2, 400, 600) == 2 * (2 * 3 * 10 * 13 * 2)
    assert L.raw("cidnet_metric_ws_floats")(0, 400, 600) == 0
    run = L.raw("cidnet_metric_psnr_ssim")
    assert run(None, p, None, p, p, p, 10 ** 9, 1, 16, 16, None) == -1          # a plain call (scale NULL) without `restored`
    assert run(p, p, None, None, None, p, 10 ** 9, 1, 16, 16, None) == -1       # neither result wanted
    assert run(p, p, None, p, p, p, 1, 1, 16, 16, None) == -3                   # plain, workspace too small
    assert run(p, p, p, p, p, p, 2 * (3 * 1 * 1 * 2) - 1, 1, 16, 16, None) == -3
    assert run(p, p, p, p, p, p, 10 ** 9, 1, 10, 16, None) == -2                # SSIM under 11 rows


def test_gt_mean_scale_arguments_are_checked():
    from hvi_cidnet_amd import metrics as M
    q = torch.zeros(2, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.gt_mean_scale(q, q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.psnr_ssim(q, q, scale=torch.ones(2, dtype=torch.float64))
    # the scale's own checks (the images' come first, and on this machine they are CPU tensors): dtype and length, then the device
    dev = torch.device("cpu")
    for bad in (torch.ones(2), torch.ones(3, dtype=torch.float64), torch.ones(2, 1, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=r"psnr_ssim: scale must be \(2,\) float64 \(got"):
            M._checked_scale("psnr_ssim", bad, 2, dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M._checked_scale("psnr_ssim", torch.ones(2, dtype=torch.float64), 2, dev)


def test_input_converter_accepts_and_refuses():
    """the one input converter on a CPU device: the shapes (the rounding of uint8 inputs needs the GPU: test_metrics_gpu.py)"""
    from hvi_cidnet_amd import metrics as M
    a = np.random.default_rng(4).integers(0, 256, (3, 5, 3), dtype=np.uint8)      # HWC although its first axis is 3 too
    want = torch.from_numpy(a).permute(2, 0, 1).float().div(255)
    chw8 = torch.from_numpy(a).permute(2, 0, 1).contiguous()
    for img in (a, chw8, chw8[None], want, want[None], want.double().numpy()):
        got = M._image_f32(img, "cpu")
        assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(M._image_f32(torch.zeros(7, 5, 3, dtype=torch.uint8), "cpu"), torch.zeros(3, 7, 5))
    for bad in (torch.rand(6, 5), torch.rand(4, 6, 5), torch.rand(2, 3, 6, 5), torch.rand(6, 5, 3), np.zeros((6, 5), np.uint8),
                np.zeros((6, 5, 4), np.uint8), np.zeros((1, 6, 5, 3), np.uint8), torch.zeros(1, 6, 5, dtype=torch.uint8),
                torch.zeros(2, 3, 6, 5, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"input image: expected \(3,h,w\) or \(h,w,3\), got"):
            M._image_f32(bad, "cpu")


# sizes (h, w) of the images; each pads to a multiple of 8.  The first list is tests/test_evaluate_gpu.py's SIZES.
PLAN_SIZES = [[(36, 52), (36, 52), (33, 50), (40, 56), (32, 48), (32, 48)],
              [(40, 56), (40, 56), (48, 56), (48, 56), (48, 56), (47, 56), (40, 56)],   # the padded shape changes inside a batch
              [(200, 296), (197, 290), (194, 295), (192, 288), (192, 288)],
              [(33, 50)] * 9, [(33, 50), (40, 56)]]                                        # the last is shorter than world = 3


@pytest.mark.parametrize("sizes", PLAN_SIZES)
@pytest.mark.parametrize("batch_size", [1, 2, 3, 8])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_evaluation_plan(sizes, batch_size, world):
    """metrics._plan against the per-image loop: which images a rank's batches and runs hold, and which rows they fill"""
    from hvi_cidnet_amd import metrics as M
    n = len(sizes)
    padded = [(1, 3, -(-h // 8) * 8, -(-w // 8) * 8) for h, w in sizes]
    seen = []
    for rank in range(world):
        mine = list(range(rank, n, world))
        batches = list(M._plan(((padded[i], sizes[i]) for i in mine), rank, world, batch_size))
        # the obvious loop: an image joins the current batch unless that is full or of another padded shape
        want, cur = [], []
        for i in mine:
            if cur and (len(cur) == batch_size or padded[cur[0]] != padded[i]):
                want.append(cur)
                cur = []
            cur.append(i)
        want += [cur] if cur else []
        assert [mine[lo:hi] for lo, hi, _ in batches] == want
        order = []
        for (lo, hi, runs), imgs in zip(batches, want):
            assert 1 <= len(imgs) <= batch_size and len({padded[i] for i in imgs}) == 1
            assert [j for j, _, _ in runs] + [len(imgs)] == [0] + [k for _, k, _ in runs]        # the runs tile the batch
            for j, k, rows in runs:
                assert len({sizes[i] for i in imgs[j:k]}) == 1
                assert k == len(imgs) or sizes[imgs[k]] != sizes[imgs[j]]                          # and are maximal
                assert list(range(n))[rows] == imgs[j:k]
                order += imgs[j:k]
        assert order == mine                                                                     # ascending within a rank
        seen += order
    assert sorted(seen) == list(range(n))                                                         # every image exactly once
