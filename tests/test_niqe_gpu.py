"""GPU: the NIQE kernels (csrc/niqe.hip through hvi_cidnet_amd.metrics) stage by stage against the numpy restatement
(tests/niqe_ref.py) and the values recorded from the reference (tests/golden/niqe*.npz).

Bars ("NIQE"; every figure is printed before it is asserted):
  * Y: bit-equal to the restatement on all 2^24 RGB triples and on every fixture;
  * scale-1 MSCN map and the MSCN map of the golden half-size image against the golden maps, and the half-size image
    against the restatement's: both sides round at the same points from fp64 sums, so at most 0.1 % of the pixels may
    differ at all; a differing half-size pixel by at most 2 fp32 ulps (one per pass); a differing MSCN value by at most
    MSCN_DIFF_BAR = 4 x the device-vs-golden maximum recorded on the MI355X -- no pixel differed there, so the bar is 0;
  * six-sum moments against the restatement's sums over the DEVICE's own MSCN map: 4e-12 relative (9216 non-negative fp64
    terms per side: n 2^-53 ~ 1e-12 each, two sides, a factor 2 to spare), the counts exactly;
  * fitted grid index equal to the restatement's wherever the restatement's decision margin exceeds 1e-6 (at most 1 % of
    the fits may be excluded);
  * score against the restatement: 10 x the change the restatement's score shows under a 1e-12 relative perturbation of
    its moments (niqe.npz: score_perturb, measured by tools/gen_niqe_golden.py); against the reference: the CPU bar.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref as R  # noqa: E402
from test_niqe_cpu import ALPHA_COLS, N_INPUTS, PARAMS, SCORE_BAR, load_input, meta, params  # noqa: E402

pytestmark = pytest.mark.gpu
MOMENT_TOL = 4e-12
MARGIN = 1e-6
MSCN_DIFF_BAR = 0.0              # 4 x the largest |device - golden| at a differing pixel on the MI355X: none differed
MAX_DIFFERING = 1e-3             # share of pixels that may differ at all
ULP_AT_256 = 2.0 ** -16


def M():
    from hvi_cidnet_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def prm():
    return M().load_niqe_params(PARAMS)


@pytest.fixture(scope="module")
def inputs():
    win = params()[2]
    out = []
    for i in range(N_INPUTS):
        g = load_input(i)
        out.append((g, R.stages(g["rgb"], win)))
    return out


def _dev_u8(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_luma_on_all_rgb_triples(dev):
    rgb = R.luma_all_triples()
    y = M().niqe_luma(_dev_u8(rgb[None], dev), crop=False)[0].cpu().numpy()
    want = R.luma(rgb)
    n = int((y != want).sum())
    print(f"luma: {n} of 2^24 triples differ from the restatement")
    assert y.shape == (4096, 4096) and n == 0


def test_luma_and_crop_on_the_fixtures(dev, inputs):
    for g, st in inputs:
        y = M().niqe_luma(_dev_u8(g["rgb"], dev).unsqueeze(0))[0].cpu().numpy()
        assert y.shape == g["y"].shape
        assert np.array_equal(y, st["y"]) and np.array_equal(y, g["y"])


def _compare_map(name, got, want, value_bar):
    diff = got != want
    share = diff.mean()
    worst = float(np.abs(got.astype(np.float64) - want)[diff].max()) if diff.any() else 0.0
    print(f"{name}: {int(diff.sum())} of {diff.size} pixels differ ({share * 100:.4f} %), max |diff| there {worst:.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert not np.isnan(got).any()
    assert share <= MAX_DIFFERING
    assert worst <= value_bar
    return worst


def test_mscn_scale1_against_the_reference(dev, inputs, prm):
    for i, (g, _) in enumerate(inputs):
        m, _ = M().niqe_mscn(_dev_u8(g["y"], dev), prm, block=96)
        _compare_map(f"input {i} MSCN scale 1", m[0].cpu().numpy(), g["mscn1"], MSCN_DIFF_BAR)


def test_mscn_of_the_golden_half_size_image_against_the_reference(dev, inputs, prm):
    for i, (g, _) in enumerate(inputs):
        m, _ = M().niqe_mscn(torch.from_numpy(g["half"]).to(dev), prm, block=48)
        _compare_map(f"input {i} MSCN of the golden half-size image", m[0].cpu().numpy(), g["mscn2"], MSCN_DIFF_BAR)


def test_mscn_takes_a_float_image_like_the_y_plane(dev, inputs, prm):
    g = inputs[3][0]
    y = _dev_u8(g["y"], dev)
    m8, mom8 = M().niqe_mscn(y, prm, block=96)
    mf, momf = M().niqe_mscn(y.float(), prm, block=96)
    assert torch.equal(m8, mf) and torch.equal(mom8, momf)


def test_half_size_image_against_the_restatement(dev, inputs):
    for i, (g, st) in enumerate(inputs):
        h = M().niqe_half(_dev_u8(g["y"], dev))[0].cpu().numpy()
        _compare_map(f"input {i} half-size image", h, st["half"], 2 * ULP_AT_256)
        hf = M().niqe_half(_dev_u8(g["y"], dev).float())[0].cpu().numpy()
        assert np.array_equal(h, hf)


def test_moments_against_the_restatement_on_the_devices_own_map(dev, inputs, prm):
    worst = 0.0
    for g, _ in inputs:
        for img, bs in ((_dev_u8(g["y"], dev), 96), (torch.from_numpy(g["half"]).to(dev), 48)):
            m, mom = M().niqe_mscn(img, prm, block=bs)
            mom = mom[0].cpu().numpy()
            want = R.block_moments(m[0].cpu().numpy(), bs)
            assert mom.shape == want.shape
            assert np.array_equal(mom[..., [0, 2]], want[..., [0, 2]])                  # the counts
            rel = np.abs(mom - want) / np.maximum(np.abs(want), 1e-300)
            rel[want == 0] = np.abs(mom)[want == 0]
            worst = max(worst, float(rel.max()))
    print(f"moments: max relative difference {worst:.3e} (bar {MOMENT_TOL:.0e})")
    assert worst <= MOMENT_TOL


def test_fitted_indices_against_the_restatement(dev, inputs, prm):
    grid0, step = 0.2, 0.001
    for i, (g, st) in enumerate(inputs):
        f = M().niqe_features(_dev_u8(g["rgb"], dev), prm)[0].cpu().numpy()
        assert f.shape == st["feat"].shape
        idx = np.rint((f[:, ALPHA_COLS] - grid0) / step).astype(np.int64)
        margin = R.decision_margin(st["rhn"])
        excluded = np.isfinite(margin) & (margin <= MARGIN)
        moved = (idx != st["idx"]) & ~excluded
        print(f"input {i}: {int(excluded.sum())} of {idx.size} fits inside the margin, {int(moved.sum())} others moved; "
              f"smallest margin {np.nanmin(margin):.3e}")
        assert excluded.sum() <= 0.01 * idx.size
        assert not moved.any()
        assert np.array_equal(f[:, ALPHA_COLS], R.alpha_grid()[idx])                    # the grid values themselves


def test_fit_stage_alone_equals_the_restatement_on_the_same_moments(dev, inputs):
    g, st = inputs[1]                                                                    # the input with a NaN row
    for mom, bs, cols in ((st["mom1"], 96, slice(0, 18)), (st["mom2"], 48, slice(18, 36))):
        f = M().niqe_fit(torch.from_numpy(mom).to(dev), block=bs).cpu().numpy()
        want = st["feat"][:, cols]
        assert np.array_equal(np.isnan(f), np.isnan(want))
        ok = ~np.isnan(want)
        d = np.abs(f[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
        print(f"fit stage, block {bs}: max relative feature difference {d.max():.3e}")
        assert d.max() <= 1e-13                  # the same ~20 correctly rounded fp64 operations on both sides: ~20 x 2^-53 = 2e-15


def test_scores(dev, inputs, prm):
    mu, cov, _ = params()
    bar = 10 * float(meta()["score_perturb"])
    for i, (g, st) in enumerate(inputs):
        s = float(M().niqe(_dev_u8(g["rgb"], dev), prm)[0])
        want = R.score(st["feat"], mu, cov)
        print(f"input {i}: device {s:.12f}, restatement {want:.12f} (|diff| {abs(s - want):.3e}, bar {bar:.3e}), "
              f"reference {float(g['score']):.9f} (|diff| {abs(s - float(g['score'])):.3e}, bar {SCORE_BAR:.3e})")
        assert np.isfinite(s)
        assert abs(s - want) <= bar
        assert abs(s - float(g["score"])) <= SCORE_BAR


def test_nan_rows(dev, inputs, prm):
    g, st = inputs[1]
    f = M().niqe_features(_dev_u8(g["rgb"], dev), prm)[0].cpu().numpy()
    rows = np.isnan(g["feat"]).any(axis=1)
    assert rows.sum() >= 1
    assert np.array_equal(np.isnan(f), np.isnan(g["feat"])) and np.array_equal(np.isnan(f), np.isnan(st["feat"]))
    assert f[0, 0] == R.alpha_grid()[0]                                     # an all-NaN distance row selects entry 0
    assert np.isfinite(float(M().niqe(_dev_u8(g["rgb"], dev), prm)[0]))


def test_batch_equals_single_calls_and_calls_repeat(dev, inputs, prm):
    imgs = [inputs[0][0]["rgb"], inputs[1][0]["rgb"], inputs[2][0]["rgb"][:, :384, :576]]
    batch = _dev_u8(np.stack(imgs), dev)
    fb = M().niqe_features(batch, prm)
    assert tuple(fb.shape) == (3, 24, 36)
    fb2 = M().niqe_features(batch, prm)
    assert torch.equal(torch.nan_to_num(fb, nan=-1.0), torch.nan_to_num(fb2, nan=-1.0))
    assert torch.equal(fb.view(torch.int64), fb2.view(torch.int64))
    for i, img in enumerate(imgs):
        f1 = M().niqe_features(_dev_u8(img, dev), prm)
        assert tuple(f1.shape) == (1, 24, 36)
        assert torch.equal(f1[0].view(torch.int64), fb[i].view(torch.int64)), i
    s = M().niqe(batch, prm)
    assert s.dtype == torch.float64 and s.is_cuda and tuple(s.shape) == (3,)
    assert float(s[0]) == float(M().niqe(_dev_u8(imgs[0], dev), prm)[0])


def test_small_images_and_wrong_types_are_refused(dev, prm):
    with pytest.raises(ValueError, match="96 x 96"):
        M().niqe(torch.zeros((1, 3, 95, 200), dtype=torch.uint8, device=dev), prm)
    with pytest.raises(ValueError, match="96 x 96"):
        M().niqe_features(torch.zeros((1, 3, 200, 64), dtype=torch.uint8, device=dev), prm)
    with pytest.raises(RuntimeError, match="uint8"):
        M().niqe(torch.zeros((1, 3, 96, 96), dtype=torch.float32, device=dev), prm)
    with pytest.raises(ValueError, match="niqe_pris_params.npz"):
        M().niqe(torch.zeros((1, 3, 96, 96), dtype=torch.uint8, device=dev), None)
    # a single flat block: no variance, one NaN row, fewer than two clean rows -> NaN, not an exception
    s = M().niqe(torch.full((1, 3, 96, 96), 77, dtype=torch.uint8, device=dev), prm)
    assert torch.isnan(s).all()
