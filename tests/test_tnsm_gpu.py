"""csrc/tnsm.hip and the two row-sum kernels of csrc/attn.hip against fp64: every TNSM kernel that is elementwise, a stencil or
a fixed-order sum (no attention kernel, no whole block or model), each compared with a plain torch fp64 CPU evaluation of the
same formula (autograd supplies the gradients; nothing of the project is on the reference side), at the pixel counts, channel
counts and sizes where its 4-pixel lanes, its 32-quad chunks, its 256-thread blocks or its capped grid take another path.

Every output is allocated NaN-filled (int32: -1), must be finite after the call, and a second call into fresh buffers must be
bit-identical (all reductions here are fixed-order).  fp32 criterion: max|out - ref| <= 2e-5 * max|ref| + 1e-6 per output
tensor (test_ops_gpu.close); integer outputs (amax) exactly equal.  Outputs that are sums (gv, gws, the pooled avg, the
weight-gradient partials, sum_rows) get inputs whose terms do not cancel: upstream gradients come from [0.25, 1.25) and the
summed factor has mean 0.5, and each such fixture asserts max|ref| >= 0.05 * max_i sum|terms_i| in fp64 before it compares
(`noncancelling`; test_fixture_sums_do_not_cancel does the same on the CPU).  An output or input that is a channel slice of a
wider tensor sits in the full tensor: outputs between sentinel channels that must come back bit-unchanged, inputs between
NaN channels that would poison the result if read.

Pixel counts (H x W -> HW, quads nq = ceil(HW / 4), chunks = ceil(nq / 32)) and the edge each is there for:

  HxW     HW   nq  chunks  4-pixel lanes                  modulate_bwd / blend_bwd chunks        256-thread blocks (pool, bwd_v)
  1x1      1    1    1     one lane, n = 1                31 dead quads                          255 threads without a pixel
  1x3      3    1    1     n = 3                          "                                      "
  2x2      4    1    1     one exact lane                 "                                      "
  1x5      5    2    1     exact lane + n = 1             30 dead quads                          "
  3x7     21    6    1     n = 1 after 5 exact            26 dead quads                          "
  5x15    75   19    1     n = 3 (the 50x75 level, small) 13 dead quads                          181 threads without a pixel
  9x14   126   32    1     n = 2                          exactly 32 quads, the last of 2 pixels
  8x16   128   32    1     exact                          exactly 32 quads
  3x43   129   33    2     n = 1                          2nd chunk: one live quad of one pixel
  15x17  255   64    2     n = 3                          two full chunks                        thread 255 without a pixel
  16x16  256   64    2     exact                          two full chunks                        one pixel per thread
  1x257  257   65    3     n = 1                          3rd chunk: one live quad of one pixel  thread 0 takes a second pixel
  25x37  925  232    8     n = 1                          8 chunks, 8 live quads in the last     4 pixels in threads 0..156, else 3

Kernels and cases:

  ew_kernel<0..3> (cidnet_elementwise)    n in 1, 2, 3, 4, 5, 7, 1023, 1024, 1025 (its own tail: lane n / 4 holds n & 3 elements or
                                          nothing); inputs with exact zeros (leaky forward at u == 0, backward at y == 0); mode 0
                                          in place and mode 1 with y == a as NoiseMapFn calls them; n = 4 194 311: n / 4 + 1 lanes
                                          exceed the 4096 x 256 grid by two (grid-stride wrap)
  global_pool_kernel / _bwd_kernel        LANES + BLOCK pixel counts x (B, C) in (1, 1), (3, 7), (1, 12), C = 144 at 5x15; mixed-sign,
                                          all-negative and quantised (randint(0, 4) / 3: ties everywhere) planes; 2x300 zeros with
                                          ones at 255, 256, 310 (the lower index sits in the higher thread); backward wrap at
                                          1x3x349531 (1 048 593 elements)
  noise_global_fwd / _bwd_kernel          (C, R) in (12, 8), (36, 9), (144, 36), (7, 8), (1, 1) x B in 1, 3; a zero row of W1 (both
                                          pre-activations exactly 0: masks 0); partials summed over B by cidnet_sum_rows
  rowdot_sigmoid_kernel / _bwd_t / _bwd_v LANES + BLOCK x C in 1, 7, 12, 36, C = 144 at 5x15, B in 1, 3; forward wrap 1x1x4194311
  NoiseMapFn                              2x12x5x15, 1x36x9x14, 3x7x3x43 against the un-folded module, output and six gradients
  modulate_fwd / _bwd_kernel              all pixel counts x C in 1, 7, 8, 9, 12, 36 (C % 8 != 0: channel lanes leave the loop on
                                          different iterations; odd C: the two half waves of a wave do), C = 144 at 5x15, B in 1, 3;
                                          v and gv are the last third of (B, 3C, HW); gws through cidnet_sum_rows; C = 36 at 50x75
                                          (30 chunks): B = 2 -> 60 rows (sum_rows_kernel), B = 3 -> 90 rows (sum_rows_wide_kernel);
                                          forward wrap 1x129x32517 (1 048 770 lanes)
  blend_fwd / _bwd_kernel                 the same table, contiguous tensors; forward wrap 1x129x32517
  sum_rows_kernel / sum_rows_wide_kernel  n_red in 1, 63, 64 (narrow), 65, 95, 96, 97, 128, 129, 944 (wide: lanes of 2 .. 5 and of
                                          29 / 30 rows; an odd count ends on the remainder row) x n in 1, 7, 8, 9, 36, 257, 1300
                                          (the wide kernel's 8 outputs per block, the narrow one's 256)
  resize_fwd / _bwd_kernel                identity, the model's x8 / x4 / x2, non-integer up, down, 1 -> N, N -> 1; two maps (1 and 3
                                          channels) into channel offsets 0 and 1 of (B, 6, Ho, Wo), B in 1, 2; ResizeCatFn once;
                                          wrap at the exact ratio 2: forward 1024x1025 -> 2048x2050 (4 198 400 outputs), its
                                          adjoint, and the adjoint of 2048x2050 -> 1024x1025 (4 198 400 inputs gathered)

The resize cases keep every input dimension <= 40 and every output dimension <= 129 unless the ratio is exact: the kernel
computes the source index in fp32, and over that range its taps stay within 4.0e-6 of torch's fp64 weights and the adjoint's
candidate window misses no contributing output, so the 2e-5 criterion holds with margin for a correct kernel.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ops_gpu import close  # noqa: E402

gpu = pytest.mark.gpu          # the tests that only check the case tables and the fixtures on the host carry no mark

NAN = float("nan")
SENT = 12345.0                 # fills the channels next to an output slice
F32, I32 = torch.float32, torch.int32
EW_GRID = 4096 * 256           # lanes of a full grid of the kernels capped at 4096 blocks
RS_GRID = 16384 * 256          # the same for the resize kernels

LANES = [(1, 1), (1, 3), (2, 2), (1, 5), (3, 7), (5, 15), (25, 37)]
CHUNK = [(9, 14), (8, 16), (3, 43)]
BLOCK = [(15, 17), (16, 16), (1, 257)]
ALL_PIX = LANES + CHUNK + BLOCK
CHUNKS_OF = {1: 1, 3: 1, 4: 1, 5: 1, 21: 1, 75: 1, 126: 1, 128: 1, 129: 2, 255: 2, 256: 2, 257: 3, 925: 8}   # HW -> chunks
MOD_C = [1, 7, 8, 9, 12, 36]


def _ids(cases):
    return ["x".join(map(str, c)) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# common helpers
# ---------------------------------------------------------------------------------------------------------------------
def _fresh(dev, spec):
    if callable(spec):
        return spec()
    shape, dt = spec
    return torch.full(shape, -1 if dt == I32 else NAN, device=dev, dtype=dt)


def twice(dev, call, *specs):
    """run `call` on fresh outputs twice: a spec is (shape, dtype), allocated NaN-filled (int32: -1), or a function that
    builds the buffer.  Finite (int32: non-negative) everywhere, bit-identical between the runs."""
    runs = []
    for _ in range(2):
        bufs = [_fresh(dev, s) for s in specs]
        call(*bufs)
        runs.append(bufs)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        ok = (a >= 0).all() if a.dtype == I32 else torch.isfinite(a).all()
        assert bool(ok), "elements left unwritten or not finite"
        assert torch.equal(a, b), "two runs differ"
    return runs[0]


def sliced(dev, B, ctot, lo, hi, n):
    """(B, ctot, n): NaN in channels lo..hi-1 (the output slice), the sentinel in all others"""
    def make():
        t = torch.full((B, ctot, n), SENT, device=dev, dtype=F32)
        t[:, lo:hi] = NAN
        return t
    return make


def untouched(t, lo, hi):
    assert bool((t[:, :lo] == SENT).all()) and bool((t[:, hi:] == SENT).all()), "channels outside the slice were written"


def noncancelling(ref, abs_terms, what):
    """the fixture condition of a summed output: ref = sum of terms, abs_terms = sum of |terms|, elementwise, in fp64"""
    r, t = ref.abs().max().item(), abs_terms.max().item()
    assert r >= 0.05 * t, f"{what}: the fixture's sums cancel (max|ref| {r:.3e} < 0.05 * {t:.3e})"


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1009 + int(v)
    return torch.Generator().manual_seed(s)


def _randn(g, *s):
    return torch.randn(*s, generator=g)


def _pos(g, *s):
    """upstream gradients and other factors of sums: [0.25, 1.25)"""
    return 0.25 + torch.rand(*s, generator=g)


def _half(g, *s):
    """mixed-sign values of mean 0.5 (the summed factor of gv, gws, avg)"""
    return 0.5 + 0.5 * torch.randn(*s, generator=g)


def _ops():
    from hvi_cidnet_amd import ops
    return ops


def sum_rows(part, n_red, n, out):
    ops = _ops()
    ops.lib().call("cidnet_sum_rows", ops._p(part), n_red, n, ops._p(out), ops._stream())


def mod_ws_floats(B, C, HW):
    return _ops()._raw("cidnet_modulate_bwd_ws_floats", B, C, HW)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables, on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_reach_what_they_claim():
    """the docstring's arithmetic: quads and chunks per pixel count (the chunk count read back from the library's own
    workspace query), the 60 / 90 rows around the sum_rows switch, and every wrap inequality"""
    assert {h * w for h, w in ALL_PIX} == set(CHUNKS_OF) and len(ALL_PIX) == 13
    for H, W in ALL_PIX:
        HW = H * W
        nq = (HW + 3) // 4
        assert (nq + 31) // 32 == CHUNKS_OF[HW]
        for B, C in ((1, 1), (3, 9)):
            assert mod_ws_floats(B, C, HW) == B * CHUNKS_OF[HW] * C
    assert {(h * w) % 4 for h, w in ALL_PIX} == {0, 1, 2, 3}
    assert (126 + 3) // 4 == 32 and (129 + 3) // 4 == 33 and (257 + 3) // 4 == 65 and (925 + 3) // 4 == 232
    for B, rows in STRADDLE:
        assert mod_ws_floats(B, 36, 50 * 75) // 36 == rows
    assert [r for _, r in STRADDLE] == [60, 90] and 60 <= 64 < 90                 # cidnet_sum_rows switches at n_red > 64
    assert EW_WRAP // 4 + 1 > EW_GRID and EW_WRAP % 4 == 3
    B, C, HW = POOL_BWD_WRAP
    assert B * C * HW > EW_GRID
    B, C, HW = ROWDOT_WRAP
    assert C == 1 and B * ((HW + 3) // 4) > EW_GRID
    B, C, HW = MOD_WRAP
    assert B * C * ((HW + 3) // 4) > EW_GRID
    (hi, wi), (ho, wo) = RS_WRAP
    assert ho * wo > RS_GRID and ho == 2 * hi and wo == 2 * wi                   # forward up, and the adjoint of the down-scale
    assert {n for n in SUM_NRED if n <= 64} == {1, 63, 64}
    rows_per_lane = {n: {len(range(sl, n, 32)) for sl in range(32)} for n in SUM_NRED if n > 64}      # the wide kernel's lanes
    assert rows_per_lane == {65: {2, 3}, 95: {2, 3}, 96: {3}, 97: {3, 4}, 128: {4}, 129: {4, 5}, 944: {29, 30}}
    for hi_wi, ho_wo in RESIZE:
        for i, o in zip(hi_wi, ho_wo):
            assert (i <= 40 and o <= 129) or o % i == 0 or i % o == 0
    for C, R in NOISE_CR:
        assert R == (1 if C == 1 else max(8, C // 4))                            # (1, 1): the smallest launch, below the module's R >= 8


# ---------------------------------------------------------------------------------------------------------------------
# 1. cidnet_elementwise
# ---------------------------------------------------------------------------------------------------------------------
EW_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025)
EW_WRAP = 4_194_311


@functools.lru_cache(maxsize=None)
def ew_case(n):
    """u with exact zeros at every index = 1 mod 3 (n = 2, 5, 1025: the last element); fp64 leaky / sigmoid and their
    gradients for an upstream g through autograd.  The backward modes read the forward's fp32 output."""
    g = _gen(1, n)
    u = _randn(g, n)
    u[torch.arange(n) % 3 == 1] = 0.0
    up = _pos(g, n)
    u64 = u.double().requires_grad_(True)
    y0, y2 = F.leaky_relu(u64, 0.2), torch.sigmoid(u64)
    g1, = torch.autograd.grad(y0, u64, up.double())
    g3, = torch.autograd.grad(y2, u64, up.double())
    return dict(u=u, g=up, y0=y0.detach(), g1=g1, y2=y2.detach(), g3=g3)


def k_ew(mode, a, b, y):
    ops = _ops()
    ops.lib().call("cidnet_elementwise", mode, ops._p(a), ops._p(b), ops._p(y), a.numel(), ops._stream())


@gpu
@pytest.mark.parametrize("n", EW_N + (EW_WRAP,))
def test_elementwise(dev, n):
    """modes 0..3 out of place; mode 0 in place (y == a) and mode 1 with y == a and b given, bit-equal to out of place"""
    c = ew_case(n)
    u, g = c["u"].to(dev), c["g"].to(dev)
    y0f, y2f = c["y0"].float().to(dev), c["y2"].float().to(dev)
    spec = ((n,), F32)
    y0, = twice(dev, lambda o: k_ew(0, u, None, o), spec)
    close(y0, c["y0"], what="leaky fwd")
    assert bool((y0[u == 0] == 0).all())
    g1, = twice(dev, lambda o: k_ew(1, g, y0f, o), spec)
    close(g1, c["g1"], what="leaky bwd")
    y2, = twice(dev, lambda o: k_ew(2, u, None, o), spec)
    close(y2, c["y2"], what="sigmoid fwd")
    g3, = twice(dev, lambda o: k_ew(3, g, y2f, o), spec)
    close(g3, c["g3"], what="sigmoid bwd")
    i0, = twice(dev, lambda o: k_ew(0, o, None, o), lambda: u.clone())
    assert torch.equal(i0, y0), "mode 0 in place"
    i1, = twice(dev, lambda o: k_ew(1, o, y0f, o), lambda: g.clone())
    assert torch.equal(i1, g1), "mode 1 in place"


# ---------------------------------------------------------------------------------------------------------------------
# 2. cidnet_global_pool_fwd / bwd
# ---------------------------------------------------------------------------------------------------------------------
POOL_PIX = LANES + BLOCK
POOL_BC = [(1, 1), (3, 7), (1, 12)]
POOL_KINDS = ("mixed", "negative", "quantised")
POOL_BWD_WRAP = (1, 3, 349_531)


def ref_pool(x):
    """avg, max, first arg-max of each plane of x (B, C, H, W) -- torch documents argmax as the first occurrence"""
    f = x.flatten(2)
    i = f.argmax(-1)
    return f.mean(-1), f.gather(2, i[..., None])[..., 0], i


def ref_pool_bwd(x, gavg, gmx):
    x = x.detach().clone().requires_grad_(True)
    avg, mx, _ = ref_pool(x)
    gx, = torch.autograd.grad((avg * gavg).sum() + (mx * gmx).sum(), x)
    return gx


def hand_made_ties():
    x = torch.zeros(1, 1, 2, 300)
    x.view(-1)[[255, 256, 310]] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def pool_case(kind, B, C, H, W):
    g = _gen(2, POOL_KINDS.index(kind) if kind in POOL_KINDS else 9, B, C, H, W)
    if kind == "mixed":
        x = _half(g, B, C, H, W)
    elif kind == "negative":
        x = -_pos(g, B, C, H, W)
    elif kind == "quantised":
        x = torch.randint(0, 4, (B, C, H, W), generator=g).float() / 3
    else:
        x = hand_made_ties()
    gavg, gmx = _pos(g, B, C), _pos(g, B, C)
    x64 = x.double()
    avg, mx, i = ref_pool(x64)
    noncancelling(avg, x64.flatten(2).abs().mean(-1), f"pool avg {kind}")
    return dict(x=x, gavg=gavg, gmx=gmx, avg=avg, mx=mx, amax=i, gx=ref_pool_bwd(x64, gavg.double(), gmx.double()))


def k_pool_fwd(x, avg, mx, amax):
    ops = _ops()
    B, C, H, W = x.shape
    ops.lib().call("cidnet_global_pool_fwd", ops._p(x), ops._p(avg), ops._p(mx), ops._p(amax), B, C, H * W, ops._stream())


def k_pool_bwd(gavg, gmx, amax, gx):
    ops = _ops()
    B, C, H, W = gx.shape
    ops.lib().call("cidnet_global_pool_bwd", ops._p(gavg), ops._p(gmx), ops._p(amax), ops._p(gx), B, C, H * W, ops._stream())


def run_pool(dev, c):
    x = c["x"].to(dev)
    B, C = x.shape[:2]
    avg, mx, amax = twice(dev, lambda a, m, i: k_pool_fwd(x, a, m, i), ((B, C), F32), ((B, C), F32), ((B, C), I32))
    close(avg, c["avg"], what="avg")
    close(mx, c["mx"], what="max")
    assert torch.equal(amax.cpu().long(), c["amax"]), "arg-max is not the first occurrence"
    gavg, gmx, ai = c["gavg"].to(dev), c["gmx"].to(dev), c["amax"].int().to(dev)
    gx, = twice(dev, lambda o: k_pool_bwd(gavg, gmx, ai, o), (tuple(x.shape), F32))
    close(gx, c["gx"], what="pool bwd")


def test_pool_reference_ties_as_adaptive_max_pool():
    """the arg-max / gather form of the reference puts the gradient where autograd through F.adaptive_max_pool2d puts it,
    on the tie fixtures: the first occurrence (index 255 of the hand-made plane)"""
    fixtures = [hand_made_ties().double()] + [pool_case("quantised", 3, 7, H, W)["x"].double() for H, W in POOL_PIX]
    for x in fixtures:
        B, C = x.shape[:2]
        gmx = _pos(_gen(3), B, C).double()
        xr = x.clone().requires_grad_(True)
        gx, = torch.autograd.grad((F.adaptive_max_pool2d(xr, 1)[:, :, 0, 0] * gmx).sum(), xr)
        assert torch.equal(gx, ref_pool_bwd(x, torch.zeros_like(gmx), gmx))
    x = hand_made_ties().double()
    assert ref_pool(x)[2].item() == 255
    assert ref_pool_bwd(x, torch.zeros(1, 1, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64)).flatten().nonzero().flatten().tolist() == [255]


@gpu
@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("hw", POOL_PIX, ids=_ids(POOL_PIX))
def test_global_pool(dev, hw, kind):
    for B, C in POOL_BC:
        run_pool(dev, pool_case(kind, B, C, *hw))


@gpu
def test_global_pool_hand_made_ties_and_144_channels(dev):
    """ones at flat indices 255 (thread 255), 256 (thread 0) and 310 of a 600-pixel plane of zeros: arg-max 255; and the
    one C = 144 case"""
    c = pool_case("hand", 1, 1, 2, 300)
    assert c["amax"].item() == 255
    run_pool(dev, c)
    for kind in POOL_KINDS:
        run_pool(dev, pool_case(kind, 1, 144, 5, 15))


@gpu
def test_global_pool_bwd_wraps_the_grid(dev):
    B, C, HW = POOL_BWD_WRAP
    g = _gen(4)
    gavg, gmx = _pos(g, B, C), _pos(g, B, C)
    amax = torch.tensor([[0, HW - 1, 262_144]])
    ref = (gavg.double() / HW)[..., None].expand(B, C, HW).clone()
    ref.scatter_add_(2, amax[..., None], gmx.double()[..., None])
    d = [t.to(dev) for t in (gavg, gmx, amax.int())]
    gx, = twice(dev, lambda o: k_pool_bwd(*d, o), ((B, C, 1, HW), F32))
    close(gx[:, :, 0], ref, what="pool bwd wrap")


# ---------------------------------------------------------------------------------------------------------------------
# 3. cidnet_noise_global_fwd / bwd
# ---------------------------------------------------------------------------------------------------------------------
NOISE_CR = [(12, 8), (36, 9), (144, 36), (7, 8), (1, 1)]


def ref_noise_global(avg, mx, W1, W2, Wn, wf):
    """h = relu(W1 avg) + relu(W1 mx), gf = sigmoid(W2 h), vrow[k] = sum_c wf[c] gf[c] Wn[c][k]; rows are samples"""
    a, m = avg @ W1.t(), mx @ W1.t()
    h = F.relu(a) + F.relu(m)
    gf = torch.sigmoid(h @ W2.t())
    return dict(a=a, m=m, h=h, gf=gf, vrow=(wf * gf) @ Wn)


@functools.lru_cache(maxsize=None)
def noise_case(C, R, B, zero_row=False):
    g = _gen(5, C, R, B, zero_row)
    avg = _half(g, B, C)
    t = dict(avg=avg, mx=avg + torch.rand(B, C, generator=g), W1=_randn(g, R, C) / C ** 0.5, W2=_randn(g, C, R) / R ** 0.5,
             Wn=_randn(g, C, C) / C ** 0.5, wf=_randn(g, C), gv=_pos(g, B, C))
    if zero_row:
        t["W1"][0] = 0.0
    d = {k: v.double() for k, v in t.items()}
    r = {k: v.detach() for k, v in ref_noise_global(d["avg"], d["mx"], d["W1"], d["W2"], d["Wn"], d["wf"]).items()}
    names = ("W1", "W2", "Wn", "wf", "avg", "mx")
    per = {k: [] for k in names}                                       # per-sample gradients: the kernel's partials
    for b in range(B):
        leaf = {k: d[k].clone().requires_grad_(True) for k in names}
        vrow = ref_noise_global(leaf["avg"][b:b + 1], leaf["mx"][b:b + 1], leaf["W1"], leaf["W2"], leaf["Wn"], leaf["wf"])["vrow"]
        vrow.backward(d["gv"][b:b + 1])
        for k in names:
            per[k].append(leaf[k].grad)
    for k in ("W1", "W2", "Wn", "wf"):
        s = torch.stack(per[k])
        r["g" + k] = s.sum(0)
        noncancelling(r["g" + k], s.abs().sum(0), f"noise_global g{k} C={C} B={B}")
    r["gavg"], r["gmx"] = sum(per["avg"]), sum(per["mx"])              # sample b's gradient is non-zero in row b only
    r["hsum"] = torch.stack([r["h"], (r["a"] > 0).double(), (r["m"] > 0).double()], -1)
    return t, r


def k_noise_fwd(d, hsum, gf, vrow):
    ops = _ops()
    B, C = d["avg"].shape
    ops.lib().call("cidnet_noise_global_fwd", *(ops._p(d[k]) for k in ("avg", "mx", "W1", "W2", "Wn", "wf")), ops._p(hsum),
                   ops._p(gf), ops._p(vrow), B, C, d["W1"].shape[0], ops._stream())


def k_noise_bwd(d, hsum, gf, gW1, gW2, gWn, gwf, gavg, gmx):
    """the launch and, as NoiseMapFn.backward, the sum of the four per-sample partials over the batch"""
    ops = _ops()
    B, C = d["avg"].shape
    R = d["W1"].shape[0]
    dev = gavg.device
    parts = [torch.full((B, n), NAN, device=dev) for n in (R * C, C * R, C * C, C)]
    ops.lib().call("cidnet_noise_global_bwd", *(ops._p(d[k]) for k in ("avg", "mx", "W1", "W2", "Wn", "wf")), ops._p(hsum), ops._p(gf),
                   ops._p(d["gv"]), *(ops._p(p) for p in parts), ops._p(gavg), ops._p(gmx), B, C, R, ops._stream())
    for p, out in zip(parts, (gW1, gW2, gWn, gwf)):
        sum_rows(p, B, p.shape[1], out)


def run_noise(dev, C, R, B, zero_row=False):
    t, r = noise_case(C, R, B, zero_row)
    d = {k: v.to(dev) for k, v in t.items()}
    hsum, gf, vrow = twice(dev, lambda h, g, v: k_noise_fwd(d, h, g, v), ((B, R, 3), F32), ((B, C), F32), ((B, C), F32))
    close(hsum[..., 0], r["h"], what="h")
    assert torch.equal(hsum[..., 1:].cpu().double(), r["hsum"][..., 1:]), "relu masks"
    close(gf, r["gf"], what="gf")
    close(vrow, r["vrow"], what="vrow")
    hs, gfr = r["hsum"].float().to(dev), r["gf"].float().to(dev)
    outs = twice(dev, lambda *o: k_noise_bwd(d, hs, gfr, *o), ((R, C), F32), ((C, R), F32), ((C, C), F32), ((C,), F32),
                 ((B, C), F32), ((B, C), F32))
    for o, k in zip(outs, ("gW1", "gW2", "gWn", "gwf", "gavg", "gmx")):
        close(o, r[k], what=k)
    return hsum, outs


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,R", NOISE_CR, ids=_ids(NOISE_CR))
def test_noise_global(dev, C, R, B):
    run_noise(dev, C, R, B)


@gpu
def test_noise_global_relu_mask_at_zero(dev):
    """row 0 of W1 is zero: both pre-activations of unit 0 are exactly 0 in fp32 and fp64; its masks are 0, it adds nothing
    to h, and its row of gW1 is 0"""
    _, r = noise_case(12, 8, 3, True)
    assert bool((r["a"][:, 0] == 0).all()) and bool((r["m"][:, 0] == 0).all()) and bool((r["gW1"][0] == 0).all())
    hsum, outs = run_noise(dev, 12, 8, 3, True)
    assert bool((hsum[:, 0] == 0).all()) and bool((outs[0][0] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. cidnet_rowdot_sigmoid_fwd / bwd
# ---------------------------------------------------------------------------------------------------------------------
ROWDOT_PIX = LANES + BLOCK
ROWDOT_C = [1, 7, 12, 36]
ROWDOT_WRAP = (1, 1, 4_194_311)


@functools.lru_cache(maxsize=None)
def rowdot_case(B, C, HW):
    g = _gen(6, B, C, HW)
    t = dict(t=_half(g, B, C, HW), v=_randn(g, B, C) / C ** 0.5, gnm=_pos(g, B, HW))
    t64 = t["t"].double().requires_grad_(True)
    v64 = t["v"].double().requires_grad_(True)
    nm = torch.sigmoid((t64 * v64[..., None]).sum(1))
    gt, gv = torch.autograd.grad(nm, (t64, v64), t["gnm"].double())
    gl = (t["gnm"].double() * nm * (1 - nm)).detach()
    noncancelling(gv, (gl[:, None] * t64.detach()).abs().sum(-1), f"rowdot gv {B}x{C}x{HW}")
    return t, dict(nm=nm.detach(), gt=gt, gv=gv)


def k_rowdot_fwd(t, v, nm):
    ops = _ops()
    B, C, HW = t.shape
    ops.lib().call("cidnet_rowdot_sigmoid_fwd", ops._p(t), ops._p(v), ops._p(nm), B, C, HW, ops._stream())


def k_rowdot_bwd(gnm, nm, t, v, gt, gv):
    ops = _ops()
    B, C, HW = t.shape
    ops.lib().call("cidnet_rowdot_sigmoid_bwd", ops._p(gnm), ops._p(nm), ops._p(t), ops._p(v), ops._p(gt), ops._p(gv), B, C, HW,
                   ops._stream())


def run_rowdot(dev, B, C, HW):
    t, r = rowdot_case(B, C, HW)
    d = {k: v.to(dev) for k, v in t.items()}
    nm, = twice(dev, lambda o: k_rowdot_fwd(d["t"], d["v"], o), ((B, HW), F32))
    close(nm, r["nm"], what="noise map")
    nmr = r["nm"].float().to(dev)
    gt, gv = twice(dev, lambda a, b: k_rowdot_bwd(d["gnm"], nmr, d["t"], d["v"], a, b), ((B, C, HW), F32), ((B, C), F32))
    close(gt, r["gt"], what="rowdot gt")
    close(gv, r["gv"], what="rowdot gv")


@gpu
@pytest.mark.parametrize("C", ROWDOT_C)
@pytest.mark.parametrize("hw", ROWDOT_PIX, ids=_ids(ROWDOT_PIX))
def test_rowdot_sigmoid(dev, hw, C):
    for B in (1, 3):
        run_rowdot(dev, B, C, hw[0] * hw[1])


@gpu
def test_rowdot_sigmoid_144_channels(dev):
    run_rowdot(dev, 3, 144, 75)


@gpu
def test_rowdot_sigmoid_fwd_wraps_the_grid(dev):
    B, C, HW = ROWDOT_WRAP
    g = _gen(7)
    t, v = _randn(g, B, C, HW), torch.tensor([[1.5]])
    d = [x.to(dev) for x in (t, v)]
    nm, = twice(dev, lambda o: k_rowdot_fwd(*d, o), ((B, HW), F32))
    close(nm, torch.sigmoid(1.5 * t.double()[:, 0]), what="rowdot wrap")


# ---------------------------------------------------------------------------------------------------------------------
# 5. NoiseMapFn against the un-folded module
# ---------------------------------------------------------------------------------------------------------------------
NOISE_MAP_SHAPES = [(2, 12, 5, 15), (1, 36, 9, 14), (3, 7, 3, 43)]


def ref_noise_map(x, w1, w2, wdw, wpw, wf):
    """global branch: sigmoid(fc2(relu(fc1(avg pool))) + fc2(relu(fc1(max pool)))); local branch: depthwise 3x3,
    LeakyReLU(0.2), 1x1; their product through the final 1x1 to one channel, then sigmoid"""
    fc = lambda z: F.conv2d(F.relu(F.conv2d(z, w1)), w2)
    glob = torch.sigmoid(fc(F.adaptive_avg_pool2d(x, 1)) + fc(F.adaptive_max_pool2d(x, 1)))
    local = F.conv2d(F.leaky_relu(F.conv2d(x, wdw, padding=1, groups=x.shape[1]), 0.2), wpw)
    return torch.sigmoid(F.conv2d(glob * local, wf))


@functools.lru_cache(maxsize=None)
def noise_map_case(shape):
    B, C, H, W = shape
    R = max(8, C // 4)
    g = _gen(8, *shape)
    t = [torch.rand(B, C, H, W, generator=g), _randn(g, R, C, 1, 1) / C ** 0.5, _randn(g, C, R, 1, 1) / R ** 0.5,
         0.4 * _randn(g, C, 1, 3, 3), _randn(g, C, C, 1, 1) / C ** 0.5, _randn(g, 1, C, 1, 1)]
    up = _pos(g, B, 1, H, W)
    leaves = [v.double().requires_grad_(True) for v in t]
    nm = ref_noise_map(*leaves)
    return t, up, nm.detach(), torch.autograd.grad(nm, leaves, up.double())


@gpu
@pytest.mark.parametrize("shape", NOISE_MAP_SHAPES, ids=_ids(NOISE_MAP_SHAPES))
def test_noise_map_fn_against_the_unfolded_module(dev, shape):
    """the fold itself: noise_map = sigmoid(vrow . leaky(dw3x3(x))) with vrow from the global branch, against the module as
    written; output and the gradients of x and the five weights"""
    t, up, nm_ref, grads_ref = noise_map_case(shape)
    runs = []
    for _ in range(2):
        leaves = [v.to(dev).requires_grad_(True) for v in t]
        nm = _ops().NoiseMapFn.apply(*leaves)
        runs.append([nm.detach()] + list(torch.autograd.grad(nm, leaves, up.to(dev))))
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    for o, r, k in zip(runs[0], [nm_ref] + list(grads_ref), ("nm", "gx", "g_fc1", "g_fc2", "g_dw", "g_pw", "g_final")):
        assert o.shape == r.shape
        close(o, r, what=k)


# ---------------------------------------------------------------------------------------------------------------------
# 6. cidnet_modulate_fwd / bwd, 7. cidnet_blend_fwd / bwd
# ---------------------------------------------------------------------------------------------------------------------
STRADDLE = [(2, 60), (3, 90)]                 # C = 36 at 50x75: (B, rows handed to cidnet_sum_rows)
MOD_WRAP = (1, 129, 32_517)


@functools.lru_cache(maxsize=None)
def mod_case(B, C, HW):
    """v of mean 0.5 (gws sums g * v * k * (1 - k) * nm over samples and pixels), nm in [0, 1), ws of both signs"""
    g = _gen(9, B, C, HW)
    t = dict(v=_half(g, B, C, HW), nm=torch.rand(B, HW, generator=g), ws=_randn(g, C), g=_pos(g, B, C, HW))
    v, nm, ws = (t[k].double().requires_grad_(True) for k in ("v", "nm", "ws"))
    keep = torch.sigmoid(ws[None, :, None] * nm[:, None])
    out = v * keep
    gv, gnm, gws = torch.autograd.grad(out, (v, nm, ws), t["g"].double())
    terms = (t["g"].double() * v * keep * (1 - keep) * nm[:, None]).detach()
    noncancelling(gws, terms.abs().sum((0, 2)), f"modulate gws {B}x{C}x{HW}")
    return t, dict(out=out.detach(), gv=gv, gnm=gnm, gws=gws)


def k_mod_fwd(qkv, nm, ws, vout):
    """v is the last third of qkv (B, 3C, HW)"""
    ops = _ops()
    B, C, HW = vout.shape
    ops.lib().call("cidnet_modulate_fwd", ops._po(qkv, 2 * C * HW), 3 * C * HW, ops._p(nm), ops._p(ws), ops._p(vout), B, C, HW,
                   ops._stream())


def k_mod_bwd(qkv, nm, ws, g, dqkv, gnm, gws):
    """as NoiseCABResidualFn.backward: gv into the last third of dqkv, the partials summed by cidnet_sum_rows"""
    ops = _ops()
    B, C, HW = g.shape
    nws = mod_ws_floats(B, C, HW)
    part = torch.full((nws,), NAN, device=g.device)
    ops.lib().call("cidnet_modulate_bwd", ops._po(qkv, 2 * C * HW), 3 * C * HW, ops._p(nm), ops._p(ws), ops._p(g),
                   ops._po(dqkv, 2 * C * HW), 3 * C * HW, ops._p(gnm), ops._p(part), B, C, HW, ops._stream())
    sum_rows(part, nws // C, C, gws)


def run_modulate(dev, B, C, HW):
    t, r = mod_case(B, C, HW)
    d = {k: v.to(dev) for k, v in t.items()}
    qkv = torch.full((B, 3 * C, HW), NAN, device=dev)                  # q and k: poison if read
    qkv[:, 2 * C:] = d["v"]
    out, = twice(dev, lambda o: k_mod_fwd(qkv, d["nm"], d["ws"], o), ((B, C, HW), F32))
    close(out, r["out"], what="modulate fwd")
    dqkv, gnm, gws = twice(dev, lambda a, b, c: k_mod_bwd(qkv, d["nm"], d["ws"], d["g"], a, b, c), sliced(dev, B, 3 * C, 2 * C, 3 * C, HW),
                           ((B, HW), F32), ((C,), F32))
    untouched(dqkv, 2 * C, 3 * C)
    close(dqkv[:, 2 * C:], r["gv"], what="modulate gv")
    close(gnm, r["gnm"], what="modulate gnm")
    close(gws, r["gws"], what="modulate gws")


@gpu
@pytest.mark.parametrize("C", MOD_C)
@pytest.mark.parametrize("hw", ALL_PIX, ids=_ids(ALL_PIX))
def test_modulate(dev, hw, C):
    HW = hw[0] * hw[1]
    for B in (1, 3):
        assert mod_ws_floats(B, C, HW) == B * CHUNKS_OF[HW] * C
        run_modulate(dev, B, C, HW)


@gpu
def test_modulate_144_channels(dev):
    run_modulate(dev, 3, 144, 75)


@gpu
@pytest.mark.parametrize("B,rows", STRADDLE, ids=["narrow-60-rows", "wide-90-rows"])
def test_modulate_gws_on_either_side_of_the_sum_rows_switch(dev, B, rows):
    """C = 36 at 50x75 (938 quads, 30 chunks): 60 rows go to sum_rows_kernel, 90 to sum_rows_wide_kernel"""
    assert mod_ws_floats(B, 36, 3750) // 36 == rows
    run_modulate(dev, B, 36, 3750)


def _wrap_inputs(seed):
    B, C, HW = MOD_WRAP
    g = _gen(seed)
    return B, C, HW, g


@gpu
def test_modulate_fwd_wraps_the_grid(dev):
    B, C, HW, g = _wrap_inputs(10)
    v, nm, ws = _randn(g, B, C, HW), torch.rand(B, HW, generator=g), _randn(g, C)
    d = [x.to(dev) for x in (v, nm, ws)]
    ops = _ops()
    out, = twice(dev, lambda o: ops.lib().call("cidnet_modulate_fwd", ops._p(d[0]), C * HW, ops._p(d[1]), ops._p(d[2]), ops._p(o), B, C, HW,
                                               ops._stream()), ((B, C, HW), F32))
    close(out, v.double() * torch.sigmoid(ws.double()[None, :, None] * nm.double()[:, None]), what="modulate wrap")


@functools.lru_cache(maxsize=None)
def blend_case(B, C, HW):
    g = _gen(11, B, C, HW)
    t = dict(a=_randn(g, B, C, HW), d=_randn(g, B, C, HW), nm=torch.rand(B, HW, generator=g), g=_pos(g, B, C, HW))
    a, d, nm = (t[k].double().requires_grad_(True) for k in ("a", "d", "nm"))
    out = nm[:, None] * a + (1 - nm[:, None]) * d
    ga, gd, gnm = torch.autograd.grad(out, (a, d, nm), t["g"].double())
    return t, dict(out=out.detach(), ga=ga, gd=gd, gnm=gnm)


def k_blend_fwd(a, d, nm, out):
    ops = _ops()
    B, C, HW = a.shape
    ops.lib().call("cidnet_blend_fwd", ops._p(a), ops._p(d), ops._p(nm), ops._p(out), B, C, HW, ops._stream())


def k_blend_bwd(a, d, nm, g, ga, gd, gnm):
    ops = _ops()
    B, C, HW = a.shape
    ops.lib().call("cidnet_blend_bwd", ops._p(a), ops._p(d), ops._p(nm), ops._p(g), ops._p(ga), ops._p(gd), ops._p(gnm), B, C, HW,
                   ops._stream())


def run_blend(dev, B, C, HW):
    t, r = blend_case(B, C, HW)
    d = {k: v.to(dev) for k, v in t.items()}
    out, = twice(dev, lambda o: k_blend_fwd(d["a"], d["d"], d["nm"], o), ((B, C, HW), F32))
    close(out, r["out"], what="blend fwd")
    ga, gd, gnm = twice(dev, lambda x, y, z: k_blend_bwd(d["a"], d["d"], d["nm"], d["g"], x, y, z), ((B, C, HW), F32), ((B, C, HW), F32),
                        ((B, HW), F32))
    close(ga, r["ga"], what="blend ga")
    close(gd, r["gd"], what="blend gd")
    close(gnm, r["gnm"], what="blend gnm")


@gpu
@pytest.mark.parametrize("C", MOD_C)
@pytest.mark.parametrize("hw", ALL_PIX, ids=_ids(ALL_PIX))
def test_blend(dev, hw, C):
    for B in (1, 3):
        run_blend(dev, B, C, hw[0] * hw[1])


@gpu
def test_blend_144_channels_and_50x75(dev):
    run_blend(dev, 3, 144, 75)
    run_blend(dev, 2, 36, 3750)


@gpu
def test_blend_fwd_wraps_the_grid(dev):
    B, C, HW, g = _wrap_inputs(12)
    a, d, nm = _randn(g, B, C, HW), _randn(g, B, C, HW), torch.rand(B, HW, generator=g)
    dv = [x.to(dev) for x in (a, d, nm)]
    out, = twice(dev, lambda o: k_blend_fwd(*dv, o), ((B, C, HW), F32))
    n64 = nm.double()[:, None]
    close(out, n64 * a.double() + (1 - n64) * d.double(), what="blend wrap")


# ---------------------------------------------------------------------------------------------------------------------
# 8. cidnet_sum_rows
# ---------------------------------------------------------------------------------------------------------------------
SUM_NRED = [1, 63, 64, 65, 95, 96, 97, 128, 129, 944]
SUM_N = [1, 7, 8, 9, 36, 257, 1300]


@gpu
@pytest.mark.parametrize("n_red", SUM_NRED)
def test_sum_rows(dev, n_red):
    """out[i] = sum_r in[r][i]: sum_rows_kernel up to 64 rows, sum_rows_wide_kernel beyond (lane sl takes rows sl, sl + 32,
    sl + 64, ...: two per pass and one remainder row); all terms positive"""
    for n in SUM_N:
        x = _pos(_gen(13, n_red, n), n_red, n)
        xd = x.to(dev)
        out, = twice(dev, lambda o: sum_rows(xd, n_red, n, o), ((n,), F32))
        close(out, x.double().sum(0), what=f"sum_rows {n_red} x {n}")


# ---------------------------------------------------------------------------------------------------------------------
# 9. cidnet_resize_bilinear_fwd / bwd
# ---------------------------------------------------------------------------------------------------------------------
RESIZE = [((5, 7), (5, 7)),
          ((4, 6), (32, 48)), ((8, 12), (32, 48)), ((16, 24), (32, 48)),
          ((4, 6), (37, 51)), ((9, 12), (37, 51)), ((3, 5), (7, 129)),
          ((37, 40), (9, 13)), ((40, 33), (3, 2)), ((20, 28), (10, 14)),
          ((1, 1), (6, 9)), ((1, 7), (5, 7)), ((7, 5), (1, 1)), ((6, 1), (6, 4))]
RESIZE_IDS = ["%dx%d-%dx%d" % (a + b) for a, b in RESIZE]
RS_WRAP = ((1024, 1025), (2048, 2050))
RS_CTOT = 6                                   # two maps of 1 and 3 channels at offsets 0 and 1, then two sentinel channels


def ref_resize(x, size, gout=None):
    """F.interpolate(bilinear, align_corners=False) in fp64, and its adjoint applied to gout"""
    x = x.double().requires_grad_(True)
    y = F.interpolate(x, size, mode="bilinear", align_corners=False)
    if gout is None:
        return y.detach()
    return y.detach(), torch.autograd.grad(y, x, gout.double())[0]


def k_resize_fwd(src, dst, off, ctot, size):
    ops = _ops()
    B, C, Hi, Wi = src.shape
    Ho, Wo = size
    ops.lib().call("cidnet_resize_bilinear_fwd", ops._p(src), ops._po(dst, off * Ho * Wo), ctot * Ho * Wo, B, C, Hi, Wi, Ho, Wo,
                   ops._stream())


def k_resize_bwd(gdst, off, ctot, size, gsrc):
    ops = _ops()
    B, C, Hi, Wi = gsrc.shape
    Ho, Wo = size
    ops.lib().call("cidnet_resize_bilinear_bwd", ops._po(gdst, off * Ho * Wo), ctot * Ho * Wo, ops._p(gsrc), B, C, Hi, Wi, Ho, Wo,
                   ops._stream())


@functools.lru_cache(maxsize=None)
def resize_case(hi_wi, ho_wo, B):
    g = _gen(14, *hi_wi, *ho_wo, B)
    maps = [_randn(g, B, c, *hi_wi) for c in (1, 3)]
    gout = _pos(g, B, 4, *ho_wo)
    refs = [ref_resize(m, ho_wo, gout[:, off:off + m.shape[1]]) for m, off in zip(maps, (0, 1))]
    return maps, gout, refs


@gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hi_wi,ho_wo", RESIZE, ids=RESIZE_IDS)
def test_resize_bilinear(dev, hi_wi, ho_wo, B):
    """each map into its channel slice of (B, 6, Ho, Wo), the other channels bit-unchanged; the adjoint reads its slice of
    a gradient whose other channels are NaN"""
    maps, gout, refs = resize_case(hi_wi, ho_wo, B)
    Ho, Wo = ho_wo
    gd = torch.full((B, RS_CTOT, Ho, Wo), NAN, device=dev)
    gd[:, :4] = gout.to(dev)
    for m, off, (y_ref, g_ref) in zip(maps, (0, 1), refs):
        c = m.shape[1]
        md = m.to(dev)
        dst, = twice(dev, lambda o: k_resize_fwd(md, o, off, RS_CTOT, ho_wo), sliced(dev, B, RS_CTOT, off, off + c, Ho * Wo))
        untouched(dst, off, off + c)
        close(dst[:, off:off + c].reshape(B, c, Ho, Wo), y_ref, what=f"resize fwd, map at {off}")
        gsrc, = twice(dev, lambda o: k_resize_bwd(gd, off, RS_CTOT, ho_wo, o), (tuple(m.shape), F32))
        close(gsrc, g_ref, what=f"resize bwd, map at {off}")


@gpu
def test_resize_cat_fn(dev):
    """ResizeCatFn: maps of two sizes and channel counts into one tensor, and back"""
    g = _gen(15)
    maps = [_randn(g, 2, 1, 4, 6), _randn(g, 2, 3, 9, 12)]
    size = (37, 51)
    up = _pos(g, 2, 4, *size)
    refs = [ref_resize(m, size, up[:, off:off + m.shape[1]]) for m, off in zip(maps, (0, 1))]
    runs = []
    for _ in range(2):
        leaves = [m.to(dev).requires_grad_(True) for m in maps]
        out = _ops().ResizeCatFn.apply(*size, *leaves)
        runs.append([out.detach()] + list(torch.autograd.grad(out, leaves, up.to(dev))))
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    out, g0, g1 = runs[0]
    close(out, torch.cat([r[0] for r in refs], 1), what="resize-cat")
    close(g0, refs[0][1], what="resize-cat g0")
    close(g1, refs[1][1], what="resize-cat g1")


@gpu
def test_resize_fwd_and_its_adjoint_at_the_wrap_size(dev):
    """1x1x1024x1025 -> 2048x2050 (exact ratio 2): 4 198 400 outputs wrap the forward's 16384-block grid"""
    small, big = RS_WRAP
    g = _gen(16)
    x, gout = _randn(g, 1, 1, *small), _pos(g, 1, 1, *big)
    y_ref, g_ref = ref_resize(x, big, gout)
    xd, gd = x.to(dev), gout.to(dev)
    y, = twice(dev, lambda o: k_resize_fwd(xd, o, 0, 1, big), ((1, 1) + big, F32))
    close(y, y_ref, what="resize fwd wrap")
    gs, = twice(dev, lambda o: k_resize_bwd(gd, 0, 1, big, o), ((1, 1) + small, F32))
    close(gs, g_ref, what="adjoint of the wrap forward")


@gpu
def test_resize_adjoint_wraps_the_grid(dev):
    """the adjoint is a gather with one item per INPUT pixel, so it wraps its grid as the adjoint of the down-scale
    2048x2050 -> 1024x1025 (exact ratio 2): 4 198 400 gathered inputs"""
    small, big = RS_WRAP
    g = _gen(17)
    gout = _pos(g, 1, 1, *small)
    _, g_ref = ref_resize(torch.zeros(1, 1, *big), small, gout)
    gd = gout.to(dev)
    gs, = twice(dev, lambda o: k_resize_bwd(gd, 0, 1, small, o), ((1, 1) + big, F32))
    close(gs, g_ref, what="resize bwd wrap")


# ---------------------------------------------------------------------------------------------------------------------
# the fixture condition of every summed output, on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_sums_do_not_cancel():
    """builds the fixtures of the summed outputs (each asserts max|ref| >= 0.05 * max_i sum|terms_i| as it is built): pooled
    avg, noise_global's partials over the batch, rowdot's gv and modulate's gws at the small shapes"""
    for hw in POOL_PIX:
        for kind in POOL_KINDS:
            for B, C in POOL_BC:
                pool_case(kind, B, C, *hw)
    for C, R in NOISE_CR:
        for B in (1, 3):
            noise_case(C, R, B)
    noise_case(12, 8, 3, True)
    for hw in ROWDOT_PIX:
        for C in ROWDOT_C:
            rowdot_case(3, C, hw[0] * hw[1])
    for hw in ALL_PIX:
        for C in MOD_C:
            mod_case(3, C, hw[0] * hw[1])
    mod_case(3, 144, 75)
    rowdot_case(3, 144, 75)
