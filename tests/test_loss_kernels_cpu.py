"""Host-side checks of tests/loss_kernels_ref.py, the fixtures and criteria of tests/test_loss_kernels_gpu.py: the SSIM content
criteria can be met by a correct fp32 implementation of the kernel's algorithm (its numpy restatement, with and without FMA), the
ill-conditioned cases really are ill-conditioned (the fp32 oracle itself misses the plain criterion there), and every fixture
reaches the path or the tie it is there for.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_kernels_ref as R  # noqa: E402

RESTATED_SHAPES = [(1, 1, 1, 1), (1, 1, 3, 4), (2, 3, 16, 65), (1, 4, 2, 9), (2, 3, 33, 129)]
CONTENT_CASES = [(k, s) for s in R.SSIM_CONTENT_SHAPES for k in R.SSIM_CONTENT]


def _err(got, ref):
    return abs(got - ref) if isinstance(ref, float) else (got - ref).abs().max().item()


@pytest.mark.parametrize("shape", RESTATED_SHAPES, ids=R.ids(RESTATED_SHAPES))
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
def test_restatement_meets_the_plain_criterion_on_white_noise(shape, fma):
    """the restatement is the kernel's algorithm: halo, taps and moments right, or it would miss these"""
    x, y, (l64, gx64, gy64) = R.ssim_geometry_ref(shape)
    loss, gx, gy = R.ssim_kernel_restated(x, y, fma=fma)
    assert abs(loss - l64) <= R.ssim_loss_bound()
    assert _err(gx, gx64) <= R.ssim_grad_bound(gx64) and _err(gy, gy64) <= R.ssim_grad_bound(gy64)


@pytest.mark.parametrize("kind,shape", CONTENT_CASES, ids=[f"{k}-{R.ids([s])[0]}" for k, s in CONTENT_CASES])
def test_ssim_content_criteria_are_satisfiable(kind, shape):
    x, y, (l64, gx64, gy64), (e_l, e_x, e_y) = R.ssim_content_ref(kind, shape)
    for fma in (True, False):
        loss, gx, gy = R.ssim_kernel_restated(x, y, fma=fma)
        el, ex, ey = abs(loss - l64), _err(gx, gx64), _err(gy, gy64)
        print(f"{kind} {shape} fma={int(fma)}: restated error / E32: loss {el:.2e} / {e_l:.2e}, d/dx {ex:.2e} / {e_x:.2e}, d/dy {ey:.2e} / {e_y:.2e}")
        assert el <= R.ssim_loss_bound(e_l), (el, e_l)
        assert ex <= R.ssim_grad_bound(gx64, e_x), (ex, e_x, gx64.abs().max().item())
        assert ey <= R.ssim_grad_bound(gy64, e_y), (ey, e_y, gy64.abs().max().item())


@pytest.mark.parametrize("kind", R.SSIM_ILL_CONDITIONED)
def test_fp32_oracle_misses_the_plain_criterion(kind):
    """the flat-patch and constant-pair cases measure what they claim: the fp32 CPU evaluation of the reference itself is
    outside 2e-6 (loss) or 1e-4 * max|ref| + 1e-10 (a gradient) at one of the two shapes at least"""
    worst = 0.0
    for shape in R.SSIM_CONTENT_SHAPES:
        _, _, (l64, gx64, gy64), (e_l, e_x, e_y) = R.ssim_content_ref(kind, shape)
        worst = max(worst, e_l / R.ssim_loss_bound(), e_x / R.ssim_grad_bound(gx64), e_y / R.ssim_grad_bound(gy64))
    print(f"{kind}: E32 / plain criterion = {worst:.2f}")
    assert worst > 1.0, worst


@pytest.mark.parametrize("kind", ["const_07_07", "identical"])
def test_identical_images_have_zero_gradient(kind):
    for shape in R.SSIM_CONTENT_SHAPES:
        x, y, (l64, gx64, gy64), _ = R.ssim_content_ref(kind, shape)
        assert torch.equal(x, y) and abs(l64) <= 1e-15
        assert gx64.abs().max().item() <= 1e-12 and gy64.abs().max().item() <= 1e-12


def test_ssim_content_fixtures():
    for shape in R.SSIM_CONTENT_SHAPES:
        b, c, h, w = shape
        x, y = R.ssim_content_pair("flat_one", shape)
        assert bool((x[..., h // 4:h - h // 4, w // 4:w - w // 4] == 1).all()) and x.min().item() < 0.5
        x, y = R.ssim_content_pair("uint8", shape)
        assert torch.equal(torch.round(x * 255) / 255, x) and torch.equal(torch.round(y * 255) / 255, y)
        x, y = R.ssim_content_pair("signed", shape)
        assert x.min().item() < -0.9 and y.min().item() < -0.5
        x, y = R.ssim_content_pair("ramp", shape)
        assert 0.1 <= x.min().item() and x.max().item() <= 0.9 and 0 < (x - y).abs().max().item() < 0.12


def test_ssim_geometry_covers_the_tile_edges():
    assert R.ssim_blocks((8, 4, 33, 129)) == 288 > 256
    hw = {(h, w) for _, _, h, w in R.SSIM_GEOMETRY}
    assert {(15, 64), (16, 65), (17, 128), (33, 129), (1, 1)} <= hw
    for h, w in R.SSIM_HW:
        assert (1, 1, h, w) in R.SSIM_GEOMETRY and (2, 3, h, w) in R.SSIM_GEOMETRY


def test_grid_wraps():
    """each large size is past its kernel's grid: threads * elements per thread of the capped grid"""
    n = 3 * 593 * 591
    assert n == 1051389 and n % 4 == 1 and n // 4 > 1024 * 256               # l1, mse
    assert R.MSE_N[-1] == n and R.NORM_HW[-1] * 3 == n > 4096 * 256          # vgg_normalize at B = 1
    assert 3 * 419 * 421 == 529197 > 2048 * 256                              # edge
    b, c, h, w = R.POOL_SHAPES[-1]
    assert b * c * (h // 2) * (w // 2) > 8192 * 256 and h % 2 and w % 2      # maxpool fwd (bwd has more cells)
    assert (257 * 257 + 3) // 4 > 64 * 256 and (257 * 257) % 4 == 1          # bias_relu
    assert R.RELU_BWD_N[-1] // 4 > 4096 * 256 - 1 and R.RELU_BWD_N[-1] % 4 == 3
    assert R.SCALE_N[-1] // 4 >= 4096 * 256
    assert 3 * 3 * ((R.HVI_HW[-1] + 3) // 4) > 8192 * 256 and R.HVI_HW[-1] % 4 == 1
    assert all(b * h * w > 1024 * 256 for b, _, h, w in R.TNSM_WRAP_SHAPES)
    assert len(R.HVI_COMBOS) == 7


def test_l1_fixture_has_ties():
    x, y = R.l1_pair(1023, True)
    _, g = R.l1_ref(x, y)
    assert 0.03 < (g == 0).float().mean().item() < 0.1
    assert set(g.unique().tolist()) == {0.0, (torch.ones(()) / 1023).item(), -(torch.ones(()) / 1023).item()}


def test_edge_constant_difference_is_exact():
    for shape in R.EDGE_CONST_SHAPES:
        x, y = R.edge_const_pair(shape)
        assert torch.equal(x - y, torch.full(shape, 0.25)) and y.unique().numel() > 8


@pytest.mark.parametrize("kind", R.POOL_KINDS)
def test_pool_fixtures_tie(kind):
    x = R.pool_input(kind, (2, 3, 6, 8))
    win = x.unfold(2, 2, 2).unfold(3, 2, 2).reshape(2, 3, 3, 4, 4)
    tied = (win == win.max(-1, keepdim=True).values).sum(-1) > 1
    all_zero = (win == 0).all(-1)
    if kind == "noise":
        assert not bool(tied.any())
    if kind == "relu":
        assert bool(all_zero.any()) and 0.3 < (x == 0).float().mean().item() < 0.7
    if kind == "dup":
        assert tied.float().mean().item() > 0.3
    # the reference routes to the first maximum in scan order
    gy = torch.ones(2, 3, 3, 4)
    _, gx = R.pool_ref(x, gy)
    first = (win == win.max(-1, keepdim=True).values).float().argmax(-1)
    got = gx.unfold(2, 2, 2).unfold(3, 2, 2).reshape(2, 3, 3, 4, 4).argmax(-1)
    assert torch.equal(first, got)


@pytest.mark.parametrize("shape", R.TNSM_TIE_SHAPES + R.TNSM_WRAP_SHAPES, ids=R.ids(R.TNSM_TIE_SHAPES + R.TNSM_WRAP_SHAPES))
def test_tnsm_masks(shape):
    quantised = shape in R.TNSM_TIE_SHAPES
    nm, out, im = R.tnsm_inputs(shape, quantised)
    strict_n, strict_o, near_n, near_o = R.tnsm_masks(nm, out, im)
    assert bool((near_n | ~strict_n).all()) and bool((near_o | ~strict_o).all())       # near keeps everything strict keeps
    if quantised:
        assert strict_n.double().mean().item() >= R.TNSM_MASK_KEEPS and strict_o.double().mean().item() >= R.TNSM_MASK_KEEPS
        assert int((~strict_n).sum()) > 0 and int((~strict_o).sum()) > 0, "no tie in the fixture"
        assert torch.equal(torch.round(nm * R.TNSM_LEVELS) / R.TNSM_LEVELS, nm)
    else:
        assert bool(near_n.all()) and bool(near_o.all())


def test_hvi_grad_sum_reference():
    g = R.gen(3)
    ga, gc, gi = torch.randn(2, 3, 5, generator=g), torch.randn(2, 3, 5, generator=g), torch.randn(2, 1, 5, generator=g)
    full = R.hvi_grad_sum_ref(ga, gc, gi, 2, 5)
    assert torch.equal(full[:, :2], (ga + gc)[:, :2]) and torch.equal(full[:, 2], (ga + gc)[:, 2] + gi[:, 0])
    only_i = R.hvi_grad_sum_ref(None, None, gi, 2, 5)
    assert bool((only_i[:, :2] == 0).all()) and torch.equal(only_i[:, 2], gi[:, 0])


@pytest.mark.parametrize("shape", list(R.PERCEPTUAL_SEEDS), ids=R.ids(list(R.PERCEPTUAL_SEEDS)))
def test_perceptual_fixture_is_off_the_kinks(shape):
    """the seed pair of each shape is the first whose ReLU pre-activations and pooling gaps all stay KINK_MARGIN times the fp32
    CPU evaluation's own error away from their kink; the frozen VGG weights are built from a fixed seed on the host"""
    import hvi_cidnet_amd as P
    convs = R.perceptual_convs(P.PerceptualLoss(R.PERCEPTUAL_LAYER_WEIGHTS, perceptual_weight=1.5, criterion="mse"))
    chosen = R.PERCEPTUAL_SEEDS[shape]
    assert chosen[0] >= 151 and (chosen[0] - 151) % 2 == 0 and chosen[1] == chosen[0] + 1
    for k in range((chosen[0] - 151) // 2 + 1):
        seeds = (151 + 2 * k, 152 + 2 * k)
        m = R.kink_margin(R.perceptual_pair(shape, seeds)[0], convs)
        print(f"{shape} seeds {seeds}: kink margin {m:.2f}")
        assert (m >= R.KINK_MARGIN) == (seeds == chosen), (seeds, m)
