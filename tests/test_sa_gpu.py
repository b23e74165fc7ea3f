"""csrc/sa.hip against fp64: SpatialAttention of the MSSA variant, out = x * sigmoid(conv7x7([mean_c x, max_c x])), through
cidnet_sa_fwd and cidnet_sa_bwd (six kernels), compared with a plain torch fp64 CPU evaluation (mean, first arg-max and
gather, conv2d with padding 3, sigmoid; autograd supplies gx and gw; nothing of the project is on the reference side).

Every output and the workspace are allocated NaN-filled (amax: -1), must be finite after the call, and a second call into
fresh buffers must be bit-identical.  fp32 criterion: max|out - ref| <= 2e-5 * max|ref| + 1e-6 per output tensor
(test_ops_gpu.close); amax exactly equal.  gw is 98 sums over all samples and pixels: x has mean 0.5 and the upstream
gradient comes from [0.25, 1.25), and every case asserts max|gw| >= 0.05 * max_i sum|terms_i| in fp64 before it compares.

  (B, C, H, W)       what it reaches
  1x1x1x1            one lane of one pixel; 97 of the 98 taps clipped; C = 1 (mean == max, arg-max 0)
  2x3x3x3            HW = 9: n = 1 tail; every tap window clipped on all four sides
  1x12x6x5           H and W below 7: no pixel has a full window in either direction; HW % 4 = 2
  1x7x7x9            H = 7: only the middle row sees all seven rows; HW % 4 = 3
  2x12x5x15          the 50x75 level in small (HW % 4 = 3), interior columns with full-width windows; also SpatialAttentionFn
  1x36x9x14          HW = 126, % 4 = 2; interior pixels with the full 7x7 window
  3x9x3x43           HW = 129, % 4 = 1, three samples
  1x144x5x15         the widest channel count
  2x9x5x15 quantised x = randint(0, 4) / 3: ties between channels at nearly every pixel, the first channel must win
  2x2x257x256        B*H*W = 131 584 > 512 * 256: sa_bwd_stats_kernel's capped grid walks a second iteration (512 partial rows,
                     the first two blocks with two pixels per thread); gw sums 131 584 terms per tap
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ops_gpu import close  # noqa: E402
from test_tnsm_gpu import F32, I32, NAN, _gen, _half, _ids, _ops, _pos, _randn, noncancelling, twice  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 3, 3, 3), (1, 12, 6, 5), (1, 7, 7, 9), (2, 12, 5, 15), (1, 36, 9, 14), (3, 9, 3, 43), (1, 144, 5, 15)]
QUANTISED = (2, 9, 5, 15)
STATS_LOOP = (2, 2, 257, 256)
STAT_GRID = 512 * 256                          # pixels one pass of sa_bwd_stats_kernel's capped grid covers


def ref_sa(x, w, g=None):
    """x (B, C, H, W), w (1, 2, 7, 7), fp64.  torch documents argmax as the first occurrence."""
    x, w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    i = x.argmax(1, keepdim=True)
    stats = torch.cat([x.mean(1, keepdim=True), x.gather(1, i)], 1)
    logit = F.conv2d(stats, w, padding=3)
    att = torch.sigmoid(logit)
    out = x * att
    r = dict(stats=stats.detach(), amax=i[:, 0], att=att.detach(), out=out.detach())
    if g is not None:
        r["gx"], r["gw"], gl = torch.autograd.grad(out, (x, w, logit), g)
        r["gw_abs_terms"] = torch.nn.grad.conv2d_weight(stats.detach().abs(), w.shape, gl.abs(), padding=3)
    return r


def test_reference_ties_as_torch_max():
    """the arg-max / gather form gives the gradient of torch.max(x, dim=1), which the reference model calls, on quantised
    inputs (ties between channels everywhere)"""
    t, _ = sa_case(QUANTISED, True)
    x, w, g = (t[k].double() for k in ("x", "w", "g"))
    assert (x.flatten(2).transpose(1, 2).reshape(-1, x.shape[1]).sort(-1).values.diff().eq(0).any(-1)).double().mean() > 0.5
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    stats = torch.cat([xr.mean(1, keepdim=True), torch.max(xr, dim=1, keepdim=True)[0]], 1)
    gx, gw = torch.autograd.grad(xr * torch.sigmoid(F.conv2d(stats, wr, padding=3)), (xr, wr), g)
    r = ref_sa(x, w, g)
    assert torch.equal(gx, r["gx"]) and torch.equal(gw, r["gw"])


def test_table_reaches_what_it_claims():
    B, C, H, W = STATS_LOOP
    assert B * H * W > STAT_GRID and B * H * W <= 2 * STAT_GRID
    assert {s[2] * s[3] % 4 for s in SHAPES} == {1, 2, 3}
    assert any(s[2] < 7 and s[3] < 7 for s in SHAPES) and any(s[2] >= 7 and s[3] >= 7 for s in SHAPES)
    assert _ops()._raw("cidnet_sa_bwd_ws_floats", B, H, W) == 3 * B * H * W + 512 * 98
    for shape in SHAPES + [QUANTISED]:                 # the fixture condition of gw, on the host
        sa_case(shape, shape == QUANTISED)


@functools.lru_cache(maxsize=None)
def sa_case(shape, quantised=False):
    B, C, H, W = shape
    g = _gen(21, *shape, quantised)
    x = torch.randint(0, 4, shape, generator=g).float() / 3 if quantised else _half(g, *shape)
    t = dict(x=x, w=0.1 * _randn(g, 1, 2, 7, 7), g=_pos(g, *shape))
    r = ref_sa(*(t[k].double() for k in ("x", "w", "g")))
    noncancelling(r["gw"], r["gw_abs_terms"], f"sa gw {shape}")
    return t, r


def k_sa_fwd(x, w, stats, amax, att, out):
    ops = _ops()
    ops.lib().call("cidnet_sa_fwd", ops._p(x), ops._p(w), ops._p(stats), ops._p(amax), ops._p(att), ops._p(out), *x.shape, ops._stream())


def k_sa_bwd(x, w, stats, amax, att, g, gx, gw):
    ops = _ops()
    B, C, H, W = x.shape
    n = ops._raw("cidnet_sa_bwd_ws_floats", B, H, W)
    ws = torch.full((n,), NAN, device=x.device)
    ops.lib().call("cidnet_sa_bwd", ops._p(x), ops._p(w), ops._p(stats), ops._p(amax), ops._p(att), ops._p(g), ops._p(gx), ops._p(gw),
                   ops._p(ws), n, B, C, H, W, ops._stream())


def run_sa(dev, shape, quantised=False):
    B, C, H, W = shape
    t, r = sa_case(shape, quantised)
    d = {k: v.to(dev) for k, v in t.items()}
    stats, amax, att, out = twice(dev, lambda *o: k_sa_fwd(d["x"], d["w"], *o), ((B, 2, H, W), F32), ((B, H, W), I32),
                                  ((B, 1, H, W), F32), (shape, F32))
    close(stats, r["stats"], what="mean / max")
    assert torch.equal(amax.cpu().long(), r["amax"]), "arg-max channel is not the first occurrence"
    close(att, r["att"], what="att")
    close(out, r["out"], what="out")
    sr, ar, tr = r["stats"].float().to(dev), r["amax"].int().to(dev), r["att"].float().to(dev)
    gx, gw = twice(dev, lambda a, b: k_sa_bwd(d["x"], d["w"], sr, ar, tr, d["g"], a, b), (shape, F32), ((1, 2, 7, 7), F32))
    close(gx, r["gx"], what="gx")
    close(gw, r["gw"], what="gw")


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_spatial_attention(dev, shape):
    run_sa(dev, shape)


@gpu
def test_spatial_attention_channel_ties(dev):
    _, r = sa_case(QUANTISED, True)
    assert r["amax"].unique().numel() > 3
    run_sa(dev, QUANTISED, True)


@gpu
def test_spatial_attention_stats_grid_second_iteration(dev):
    B, C, H, W = STATS_LOOP
    assert B * H * W > STAT_GRID
    run_sa(dev, STATS_LOOP)


@gpu
def test_spatial_attention_fn(dev):
    """SpatialAttentionFn: output, gx and gw through autograd"""
    shape = (2, 12, 5, 15)
    t, r = sa_case(shape)
    runs = []
    for _ in range(2):
        x, w = (t[k].to(dev).requires_grad_(True) for k in ("x", "w"))
        out = _ops().SpatialAttentionFn.apply(x, w)
        runs.append([out.detach()] + list(torch.autograd.grad(out, (x, w), t["g"].to(dev))))
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    for o, k in zip(runs[0], ("out", "gx", "gw")):
        close(o, r[k], what=k)
