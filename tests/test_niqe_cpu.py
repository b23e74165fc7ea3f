"""CPU checks of NIQE: the numpy restatement the GPU tests compare against (tests/niqe_ref.py) against values recorded from
the reference implementation (tests/golden/niqe*.npz, written by tools/gen_niqe_golden.py), and the host-side pieces of
hvi_cidnet_amd.metrics (parameter loading, the file list, the refusal of CPU tensors).

Bars ("NIQE"):
  * Y and the scale-1 MSCN map, and the MSCN map of the golden half-size image: bit-equal to the reference;
  * the restatement's own half-size image: within 4 fp32 ulps at 256 (6.1e-5) -- it sums its 8 taps in fp64, the
    reference in fp32; twice the 2 ulps measured;
  * every fitted alpha within one grid step, at most 1 % of an input's fits moved at all;
  * score: 3 x the largest |restatement - reference| measured on the committed fixtures (6.04e-6) = 1.82e-5.
"""
import glob
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import niqe_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
PARAMS = os.path.join(GOLDEN, "niqe_pris_params.npz")
SCORE_BAR = 3 * 6.04e-6                  # 3 x the largest difference measured on the committed fixtures (the generator prints it)
HALF_BAR = 4 * 2.0 ** -16                # 4 fp32 ulps at 256
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
N_INPUTS = 4


def load_input(i):
    out = {}
    for p in sorted(glob.glob(os.path.join(GOLDEN, f"niqe_img{i}.part*.npz"))):
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    assert out, f"no fixture niqe_img{i}"
    return out


def meta():
    with np.load(os.path.join(GOLDEN, "niqe.npz")) as z:
        return {k: z[k] for k in z.files}


def params():
    with np.load(PARAMS) as z:
        return z["mu_pris_param"], z["cov_pris_param"], z["gaussian_window"]


@pytest.fixture(scope="module")
def staged():
    win = params()[2]
    out = []
    for i in range(N_INPUTS):
        g = load_input(i)
        out.append((g, R.stages(g["rgb"], win)))
    return out


def test_fixture_set_is_what_the_tests_expect():
    m = meta()
    assert int(m["n_inputs"]) == N_INPUTS
    shapes = [load_input(i)["rgb"].shape for i in range(N_INPUTS)]
    assert shapes == [(3, 384, 576), (3, 384, 576), (3, 397, 603), (3, 192, 288)]
    assert float(m["score_ref_diff"].max()) * 3 <= SCORE_BAR * (1 + 1e-3)
    assert 0 < float(m["score_perturb"]) < 1e-9
    for p in glob.glob(os.path.join(GOLDEN, "niqe*.npz")):
        assert os.path.getsize(p) < (1 << 20), p


def test_luma_equals_the_reference_on_the_fixtures(staged):
    for g, st in staged:
        assert st["y"].dtype == np.uint8 and np.array_equal(st["y"], g["y"])
        assert st["y"].shape == (g["rgb"].shape[1] // 96 * 96, g["rgb"].shape[2] // 96 * 96)


def test_luma_hash_over_all_rgb_triples():
    y = R.luma(R.luma_all_triples())
    assert y.shape == (4096, 4096) and y.min() == 16 and y.max() == 235
    assert hashlib.sha256(y.tobytes()).hexdigest() == str(meta()["luma_sha256"])


def test_luma_is_the_bgr_rule_on_rgb_input():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
    y = R.luma(px.T.reshape(3, 1, -1)).ravel().tolist()
    assert y == [41, 145, 81, 235, 16]                      # pure red carries the BLUE weight 24.966: 16 + 24.966 = 40.97


def test_mscn_scale1_bit_equal(staged):
    for g, st in staged:
        assert st["mscn1"].dtype == np.float32
        assert np.array_equal(st["mscn1"], g["mscn1"])


def test_mscn_of_the_golden_half_size_image_bit_equal(staged):
    win = params()[2]
    for g, _ in staged:
        assert np.array_equal(R.mscn(g["half"], win), g["mscn2"])


def test_half_size_image_within_four_ulps(staged):
    worst = 0.0
    for g, st in staged:
        assert st["half"].shape == g["half"].shape == (g["y"].shape[0] // 2, g["y"].shape[1] // 2)
        worst = max(worst, float(np.abs(st["half"].astype(np.float64) - g["half"]).max()))
    print(f"half-size image: max |restatement - reference| = {worst:.3e} (bar {HALF_BAR:.3e})")
    assert worst <= HALF_BAR


def test_half_size_taps_are_the_antialiased_bicubic_kernel():
    """0.5 * cubic(0.5 * d) at the 8 distances of a half-size sample, normalised: the closed form the taps come from"""
    def cubic(x):
        x = abs(x)
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1 if x <= 1 else (-0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2 if x <= 2 else 0.0)
    wts = np.array([0.5 * cubic(0.5 * (k - 3.5)) for k in range(8)])
    assert np.array_equal(wts / wts.sum(), R.TAPS) and R.TAPS.sum() == 1.0


def test_fitted_alphas_within_one_grid_step(staged):
    for i, (g, st) in enumerate(staged):
        assert st["feat"].shape == g["feat"].shape
        d = np.abs(st["feat"][:, ALPHA_COLS] - g["feat"][:, ALPHA_COLS])
        moved = int((d > 1e-9).sum())
        print(f"input {i}: {moved} of {d.size} fits moved, max step {d.max():.4f}")
        assert d.max() <= 0.001 + 1e-12
        assert moved <= 0.01 * d.size


def test_nan_rows_equal_the_reference(staged):
    seen = 0
    for g, st in staged:
        a, b = np.isnan(st["feat"]), np.isnan(g["feat"])
        assert np.array_equal(a, b)
        seen += int(b.any(axis=1).sum())
    assert seen >= 1, "the fixture set must exercise a NaN row"
    g, st = staged[1]
    assert np.isnan(g["feat"][0]).any() and g["feat"][0, 0] == 0.2     # numpy's argmin over NaN distances: entry 0


def test_score_against_the_reference(staged):
    mu, cov, _ = params()
    for i, (g, st) in enumerate(staged):
        s = R.score(st["feat"], mu, cov)
        d = abs(s - float(g["score"]))
        print(f"input {i}: restatement {s:.9f}, reference {float(g['score']):.9f}, |diff| {d:.3e} (bar {SCORE_BAR:.3e})")
        assert np.isfinite(s) and d <= SCORE_BAR
        # the tail alone, on the reference's own features
        assert abs(R.score(g["feat"], mu, cov) - float(g["score"])) <= 1e-9


def test_score_needs_two_clean_rows():
    mu, cov, _ = params()
    f = np.full((3, 36), np.nan)
    f[0] = 1.0
    assert np.isnan(R.score(f, mu, cov))


def test_roll_wraps_inside_the_block():
    m = (np.arange(96 * 192, dtype=np.float32).reshape(96, 192) - 5000) / 1000
    mom = R.block_moments(m, 96)
    blk = m[:, 96:].astype(np.float64)
    v = (m[:, 96:] * np.roll(m[:, 96:], (0, 1), axis=(0, 1))).astype(np.float64)
    assert mom.shape == (2, 5, 6)
    assert mom[1, 0, 5] == (blk * blk).sum() and mom[1, 1, 4] == np.abs(v).sum()
    assert mom[1, 0, 0] + mom[1, 0, 2] <= 96 * 96


# ---- the product's host-side pieces --------------------------------------------------------------------------------
def test_load_niqe_params_round_trips_the_fixture(tmp_path):
    import hvi_cidnet_amd as P
    mu, cov, win = params()
    prm = P.load_niqe_params(PARAMS)
    assert isinstance(prm, P.NiqeParams)
    assert prm.mu_pris_param.shape == (1, 36) and np.array_equal(prm.mu_pris_param, mu.reshape(1, 36))
    assert np.array_equal(prm.cov_pris_param, cov) and np.array_equal(prm.gaussian_window, win)
    again = str(tmp_path / "p.npz")
    np.savez(again, mu_pris_param=prm.mu_pris_param, cov_pris_param=prm.cov_pris_param, gaussian_window=prm.gaussian_window)
    p2 = P.load_niqe_params(again)
    assert np.array_equal(p2.cov_pris_param, cov) and np.array_equal(p2.gaussian_window, win)
    np.savez(again, mu_pris_param=mu)
    with pytest.raises(ValueError, match="lacks"):
        P.load_niqe_params(again)


def test_niqe_without_parameters_is_a_clear_error():
    import hvi_cidnet_amd as P
    with pytest.raises(ValueError, match="niqe_pris_params.npz"):
        P.load_niqe_params(None)
    with pytest.raises(ValueError, match="niqe_pris_params.npz"):
        P.metrics.niqe_score(np.zeros((1, 6, 36)), None)


def test_niqe_refuses_cpu_tensors():
    import hvi_cidnet_amd as P
    prm = P.load_niqe_params(PARAMS)
    img = torch.zeros((1, 3, 96, 96), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.metrics.niqe(img, prm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.metrics.niqe_features(img, prm)


def test_product_tables_equal_the_restatement():
    import hvi_cidnet_amd as P
    t = P.metrics.niqe_tables()
    assert t.shape == (4, R.GRID_N) and t.dtype == np.float64
    for a, b in zip(t[:3], R.tables()):
        assert np.array_equal(a, b)
    assert np.array_equal(t[3], R.alpha_grid())
    assert abs(t[3][0] - 0.2) < 1e-15 and abs(t[3][-1] - 10.0) < 1e-12


def test_host_tail_equals_the_restatement(staged):
    import hvi_cidnet_amd as P
    prm = P.load_niqe_params(PARAMS)
    mu, cov, _ = params()
    feats = np.stack([staged[0][1]["feat"], staged[1][1]["feat"]])
    s = P.metrics.niqe_score(feats, prm)
    assert s.shape == (2,)
    assert s[0] == R.score(feats[0], mu, cov) and s[1] == R.score(feats[1], mu, cov)
    assert np.isnan(P.metrics.niqe_score(np.full((1, 4, 36), np.nan), prm)[0])


def test_folder_images_ordering(tmp_path):
    import hvi_cidnet_amd as P
    from PIL import Image
    rng = np.random.default_rng(0)
    for n in ["b.png", "a.jpg", "c.bmp", "d.JPG", "e.jpeg", "skip.PNG", "skip.tif"]:
        Image.fromarray(rng.integers(0, 256, (8, 10, 3), dtype=np.uint8)).save(str(tmp_path / n))
    (tmp_path / "notes.txt").write_text("x")
    (tmp_path / "dir.png").mkdir()
    fi = P.folder_images(str(tmp_path))
    assert fi.names == ["a.jpg", "b.png", "c.bmp", "d.JPG", "e.jpeg"] and len(fi) == 5
    with Image.open(str(tmp_path / "b.png")) as im:
        want = torch.from_numpy(np.array(im.convert("RGB"))).permute(2, 0, 1).float().div(255)
    got = fi[1]
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 8, 10) and torch.equal(got, want)
