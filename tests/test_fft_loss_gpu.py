"""GPU: the frequency-domain training loss (csrc/fft_loss.hip, ops.FFTLossFn / rfft2_parts / rfft2_parts_adjoint / dft_table,
losses.FFTLoss, CIDNetLoss(fft_weight=)) against tests/fft_loss_ref.py: fp64 torch.fft.rfft2 + autograd on the CPU.

Every tolerance is 8 * E32 + 1e-30, E32 the largest deviation of the fp32 restatement from the fp64 reference on the same
input (fft_loss_ref).  The loss itself carries the bar of the L1 and TNSM terms, 2e-6 relative.  A sign must equal the fp64
sign wherever the fp64 part is exactly 0 or at least 8 E32 from 0; the n_near parts in between may flip, and each flip moves
a gradient element by at most 2 c, c = |g_up weight s| / (2 P H Wh).

Every direct call of the ABI gets NaN-filled outputs with four guard floats behind each, a NaN-filled workspace of exactly
the queried size (guarded too), must leave the guards NaN and write only finite values, and is repeated into fresh buffers,
which must come out bit-identical.

What the shapes (fft_loss_ref.shapes, from the plan query's tile MT x NT and chunk KC; 64 / 64 / 64 today) reach:
  (1,1,1)                              the smallest plane
  (2,3,4), (3,5,7)                     tiny planes; odd x odd has one purely real bin, even x even four
  (1,16,30), (1,16,31)                 Wh = 16 from an even and an odd width
  (1,63,124), (1,64,126), (1,65,129)   one short of, exactly, one past a tile in M and N; K = 2 H and W around 2 KC
  (1,32,63), (1,32,64), (1,32,65)      K one short of, exactly, one past a chunk in the row pass
  (3,21,33), (5,13,20)                 P H = 63 and 65: planes share a row tile in the row passes, never in the column passes
  (6,50,75)                            the coarsest training plane, ragged everywhere
  (1,400,600)                          the longest accumulation

Measured kernel error / E32, MI355X, per case (every shape above, the impulse and the constant plane): spectrum 1.00,
adjoint on normal and on +-1 / 0 cotangents 1.00, loss gradient under both norms 1.00 -- the errors agree with the
restatement's to the four digits printed (0 / 0 at (1,1,1)): v_mfma_f32_32x32x2f32 accumulates k in ascending order with
fused products, which is what the restatement does.  Loss: 3.8e-9 .. 6.0e-8 relative (bar 2e-6).  Signs: no flip outside the
near set; inside it 6 of 6 at (6,50,75) and 2 of 10 at (1,400,600), all at purely real bins, where the host's fp64 transform
returned 1e-17 in place of 0 (another host returned exact zeros and n_near = 0 / 8): the gradient does not depend on them.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_loss_ref as FR  # noqa: E402

import hvi_cidnet_amd as P  # noqa: E402
from hvi_cidnet_amd import ops  # noqa: E402
from hvi_cidnet_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 4
NFIELDS = 17
ARG, SHAPE, WS = -1, -2, -3


def _plan(P_, H, W):
    out = (ctypes.c_long * NFIELDS)()
    assert lib().raw("cidnet_fft_loss_plan")(P_, H, W, out, NFIELDS) == 0
    return list(out)


MT, NT, KC = _plan(1, 1, 1)[:3]
SHAPES = FR.shapes(MT, NT, KC)


def _ratio(err, e32):
    return err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))


# ---- the call protocol ----------------------------------------------------------------------------------------------------
def _nan(n, dev):
    return torch.full((n + GUARD,), NAN, device=dev)


def _abi(dev, name, shape, sizes, args, expect=0):
    """name(*args(outs, ws, ws_floats), P, H, W, stream), twice, by the protocol of the module's docstring.  sizes: the floats
    of each output, None for one passed as NULL.  -> the outputs of the first call (None where NULL).  expect != 0: a refusal,
    which must leave every output and the workspace all NaN."""
    P_, H, W = shape
    n_ws = max(int(lib().raw("cidnet_fft_loss_ws_floats")(P_, H, W)), 0) or 64
    runs = []
    for _ in range(1 if expect else 2):
        outs = [None if n is None else _nan(n, dev) for n in sizes]
        ws = _nan(n_ws, dev)
        rc = lib().raw(name)(*args([ops._p(o) for o in outs], ops._p(ws), n_ws), P_, H, W, ops._stream())
        torch.cuda.synchronize()
        assert rc == expect, (name, shape, rc)
        assert bool(torch.isnan(ws[n_ws:]).all())
        for o, n in zip(outs, sizes):
            if o is None:
                continue
            assert bool(torch.isnan(o[n:]).all()), (name, shape, "guard")
            if expect:
                assert bool(torch.isnan(o).all()) and bool(torch.isnan(ws).all()), (name, shape, "written on an error")
            else:
                assert bool(torch.isfinite(o[:n]).all()), (name, shape, "not finite")
        runs.append((outs, ws))
    if expect:
        return None
    for o0, o1, n in zip(runs[0][0], runs[1][0], sizes):
        if o0 is not None:
            assert torch.equal(o0[:n], o1[:n]), (name, shape, "two calls differ")
    return [None if o is None else o[:n] for o, n in zip(runs[0][0], sizes)], runs[0][1]


@functools.lru_cache(maxsize=None)
def _table(N, Nk, dev):
    t = _nan(2 * N * Nk, dev)
    again = _nan(2 * N * Nk, dev)
    for buf in (t, again):
        assert lib().raw("cidnet_dft_table")(N, Nk, ops._p(buf), ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(t[2 * N * Nk:]).all()) and bool(torch.isfinite(t[:2 * N * Nk]).all())
    assert torch.equal(t[:2 * N * Nk], again[:2 * N * Nk])
    return t[:2 * N * Nk]


def _tabs(shape, dev):
    _, H, W = shape
    return ops._p(_table(H, H, dev)), ops._p(_table(W, W // 2 + 1, dev))


def _spectrum(dev, x):
    """cidnet_rfft2_fwd on x (P,H,W) -> D (P,H,Wh,2) on the host"""
    shape = tuple(x.shape)
    P_, H, W = shape
    xd = x.to(dev).contiguous()
    th, tw = _tabs(shape, dev)
    (D,), _ = _abi(dev, "cidnet_rfft2_fwd", shape, [P_ * H * (W // 2 + 1) * 2],
                   lambda o, ws, n: (ops._p(xd), th, tw, o[0], ws, n))
    return D.cpu().view(P_, H, W // 2 + 1, 2)


def _adjoint(dev, S, W):
    P_, H = S.shape[:2]
    shape = (P_, H, W)
    Sd = S.to(dev).contiguous()
    th, tw = _tabs(shape, dev)
    (g,), _ = _abi(dev, "cidnet_rfft2_adj", shape, [P_ * H * W], lambda o, ws, n: (ops._p(Sd), th, tw, o[0], ws, n))
    return g.cpu().view(P_, H, W)


def _loss_fwd(dev, a, b, norm, want_S, weight=FR.WEIGHT):
    shape = tuple(a.shape)
    P_, H, W = shape
    ad, bd = a.to(dev).contiguous(), b.to(dev).contiguous()
    th, tw = _tabs(shape, dev)
    (loss, S), ws = _abi(dev, "cidnet_fft_loss_fwd", shape, [1, P_ * H * (W // 2 + 1) * 2 if want_S else None],
                         lambda o, ws, n: (ops._p(ad), ops._p(bd), th, tw, ctypes.c_float(weight), FR.NORMS.index(norm), o[0], o[1],
                                           ws, n))
    return loss.cpu()[0], (None if S is None else S.view(P_, H, W // 2 + 1, 2)), ws


def _loss_bwd(dev, S, W, norm, want_a, want_b, weight=FR.WEIGHT, g_up=FR.G_UP):
    P_, H = S.shape[:2]
    shape = (P_, H, W)
    th, tw = _tabs(shape, dev)
    gl = torch.tensor([g_up], dtype=torch.float32, device=dev)
    n = P_ * H * W
    (ga, gb), ws = _abi(dev, "cidnet_fft_loss_bwd", shape, [n if want_a else None, n if want_b else None],
                        lambda o, ws, nws: (ops._p(S), th, tw, ops._p(gl), ctypes.c_float(weight), FR.NORMS.index(norm), o[0], o[1],
                                            ws, nws))
    return (None if ga is None else ga.view(P_, H, W)), (None if gb is None else gb.view(P_, H, W)), ws


# ---- A. tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 600])
def test_tables(dev, N):
    for Nk in sorted({N, N // 2 + 1}):
        got = _table(N, Nk, dev).cpu().numpy().reshape(N, Nk, 2)
        want = FR.table64(N, Nk)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert bool((np.abs(got.astype(np.float64) - want) <= ulp).all()), (N, Nk)
        m = (np.arange(N)[:, None] * np.arange(Nk)[None, :]) % N
        q = (4 * m) % N == 0
        assert np.array_equal(got[q], want[q].astype(np.float32))             # the quarter turns: exactly 0 and +-1
        assert set(np.unique(got[q])) <= {-1.0, 0.0, 1.0}
        cached = ops.dft_table(N, Nk, dev)
        assert cached is ops.dft_table(N, Nk, dev) and np.array_equal(cached.cpu().numpy(), got)


# ---- B. the spectrum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_spectrum(dev, shape):
    x, D64, e32 = FR.spectrum_case(*shape)
    D = _spectrum(dev, x)
    err = float((D.double() - D64).abs().max())
    print(f"spectrum {shape}: err {err:.3e} E32 {e32:.3e} ratio {_ratio(err, e32):.2f}")
    assert err <= FR.tol(e32)
    P_, H, W = shape
    for ky in {0, H // 2 if H % 2 == 0 else 0}:                               # the purely real bins
        for kx in {0, W // 2 if W % 2 == 0 else 0}:
            assert torch.count_nonzero(D[:, ky, kx, 1]) == 0
    assert torch.equal(ops.rfft2_parts(x.to(dev)).cpu(), D)                   # the wrapper is the same two launches
    if P_ > 1:                                                                # a plane's spectrum does not depend on the others
        assert torch.equal(_spectrum(dev, x[1:2]), D[1:2])


def test_spectrum_of_an_impulse_and_of_a_constant(dev):
    P_, H, W = 2, 17, 33
    x = torch.zeros((P_, H, W))
    x[:, H - 1, W - 2] = 1.0
    D64 = FR.spectrum64(x)
    e32 = float(np.abs(FR.restate_spectrum(x.numpy()).astype(np.float64) - D64.numpy()).max())
    D = _spectrum(dev, x)
    err = float((D.double() - D64).abs().max())
    mod = float((D.double().pow(2).sum(-1).sqrt() - 1.0).abs().max())        # every |D| is 1
    print(f"impulse: err {err:.3e} | |D| - 1 | {mod:.3e} E32 {e32:.3e} ratio {_ratio(err, e32):.2f}")
    assert err <= FR.tol(e32) and mod <= 2 * FR.tol(e32)
    c = torch.full((1, 50, 75), 0.37)
    D64 = FR.spectrum64(c)
    e32 = float(np.abs(FR.restate_spectrum(c.numpy()).astype(np.float64) - D64.numpy()).max())
    D = _spectrum(dev, c)
    err = float((D.double() - D64).abs().max())
    rest = D.clone()
    rest[0, 0, 0] = 0
    print(f"constant: err {err:.3e} beside DC {float(rest.abs().max()):.3e} E32 {e32:.3e} ratio {_ratio(err, e32):.2f}")
    assert err <= FR.tol(e32)                                                 # everything but DC cancels to within the bound
    assert abs(float(D64[0, 0, 0, 0]) - 0.37 * 50 * 75) < 1e-3 and float(D64.abs().sum() - D64[0, 0, 0, 0].abs()) < 1e-6


def test_views_and_unaligned_inputs(dev):
    P_, H, W = 3, 21, 33
    x, D64, e32 = FR.spectrum_case(P_, H, W)
    want = _spectrum(dev, x)
    xd = x.to(dev)
    wide = torch.zeros((P_, H, 2 * W), device=dev)
    wide[:, :, ::2] = xd
    assert torch.equal(ops.rfft2_parts(wide[:, :, ::2]).cpu(), want)          # a strided view
    assert torch.equal(ops.rfft2_parts(xd.transpose(1, 2).contiguous().transpose(1, 2)).cpu(), want)
    pc = FR.pair_case(P_, H, W)
    crit = P.FFTLoss(FR.WEIGHT)
    base = crit(pc["a"].to(dev)[None], pc["b"].to(dev)[None])
    n = P_ * H * W
    for off in (1, 2, 3):                                                     # 4, 8 and 12 bytes off a 16-byte boundary
        buf = torch.zeros(n + 3, device=dev)
        v = buf[off:off + n].view(P_, H, W)
        v.copy_(xd)
        assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
        assert torch.equal(ops.rfft2_parts(v).cpu(), want)
        bufb = torch.zeros(n + 3, device=dev)
        vb = bufb[off:off + n].view(P_, H, W)
        vb.copy_(pc["b"].to(dev))
        v.copy_(pc["a"].to(dev))
        assert torch.equal(crit(v[None], vb[None]), base)


# ---- C. the adjoint -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "signs"])
@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint(dev, shape, kind):
    S, g64, e32 = FR.adjoint_case(*shape, kind)
    g = _adjoint(dev, S, shape[2])
    err = float((g.double() - g64).abs().max())
    print(f"adjoint {kind} {shape}: err {err:.3e} E32 {e32:.3e} ratio {_ratio(err, e32):.2f}")
    assert err <= FR.tol(e32)
    assert torch.equal(ops.rfft2_parts_adjoint(S.to(dev), shape[2]).cpu(), g)


# ---- D. the loss ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", FR.NORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_signs_and_gradient(dev, shape, norm):
    P_, H, W = shape
    pc, lc = FR.pair_case(*shape), FR.loss_case(*shape, norm)
    parts = pc["D64"].numel()
    assert pc["n_near"] <= FR.near_limit(parts) and (parts >= 2000 or pc["n_near"] == 0)     # the fixture condition
    loss, S, _ = _loss_fwd(dev, pc["a"], pc["b"], norm, True)
    ref = float(lc["loss"])
    lerr = abs(float(loss) - ref) / ref
    alone, none, _ = _loss_fwd(dev, pc["a"], pc["b"], norm, False)           # S == NULL: the loss, and nothing else
    assert none is None and torch.equal(alone, loss)
    # the signs: +-1 / 0, equal to the fp64 sign wherever that part is exactly 0 or clear of 0
    Sc = S.cpu()
    assert bool(((Sc == 0) | (Sc.abs() == 1)).all())
    sure = ~pc["near"]
    assert torch.equal(Sc[sure].double(), torch.sign(pc["D64"])[sure])
    flips = int((Sc.double() != torch.sign(pc["D64"])).sum())
    # the gradient, in the four forms the entry point has
    bound = FR.tol(lc["e32"]) + 2 * lc["c"] * pc["n_near"]
    ga, gb, _ = _loss_bwd(dev, S, W, norm, True, True)
    gerr = float((ga.cpu().double() - lc["ga"]).abs().max())
    print(f"loss {norm} {shape}: loss err {lerr:.3e}; gradient err {gerr:.3e} E32 {lc['e32']:.3e} ratio {_ratio(gerr, lc['e32']):.2f}; "
          f"n_near {pc['n_near']} flips {flips}")
    assert lerr <= 2e-6
    assert gerr <= bound
    assert float((gb.cpu().double() - lc["gb"]).abs().max()) <= bound
    assert torch.equal(gb.view(torch.int32), ga.view(torch.int32) ^ torch.tensor(-2 ** 31, dtype=torch.int32, device=dev))    # bit for bit -ga
    a_only, nb, _ = _loss_bwd(dev, S, W, norm, True, False)
    na, b_only, _ = _loss_bwd(dev, S, W, norm, False, True)
    assert nb is None and na is None and torch.equal(a_only, ga) and torch.equal(b_only, gb)
    na, nb, ws = _loss_bwd(dev, S, W, norm, False, False)
    assert na is None and nb is None and bool(torch.isnan(ws).all())         # nothing asked for: nothing launched


@pytest.mark.parametrize("norm", FR.NORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_module_and_function_in_the_four_requires_grad_combinations(dev, shape, norm):
    P_, H, W = shape
    pc = FR.pair_case(*shape)
    loss0, S, _ = _loss_fwd(dev, pc["a"], pc["b"], norm, True)
    ga0, gb0, _ = _loss_bwd(dev, S, W, norm, True, True)
    crit = P.FFTLoss(loss_weight=FR.WEIGHT, norm=norm)
    for ra, rb in [(True, True), (True, False), (False, True), (False, False)]:
        a = pc["a"].to(dev).view(1, P_, H, W).clone().requires_grad_(ra)
        b = pc["b"].to(dev).view(1, P_, H, W).clone().requires_grad_(rb)
        loss = crit(a, b) if ra else ops.FFTLossFn.apply(a, b, FR.WEIGHT, norm)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.equal(loss.detach().cpu(), loss0)
        assert loss.requires_grad == (ra or rb)
        if ra or rb:
            (loss * FR.G_UP).backward()
        assert (a.grad is not None) == ra and (b.grad is not None) == rb
        assert not ra or torch.equal(a.grad[0], ga0)
        assert not rb or torch.equal(b.grad[0], gb0)


def test_identical_images_give_exactly_zero(dev):
    for shape in [(2, 3, 4), (3, 21, 33), (6, 50, 75)]:
        x = FR.noise(*shape, 7).to(dev)[None]
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        loss = P.FFTLoss(0.3, "ortho")(a, b)
        loss.backward()
        assert float(loss.detach()) == 0.0 and torch.count_nonzero(a.grad) == 0 and torch.count_nonzero(b.grad) == 0


def test_second_backward_is_a_clear_error(dev):
    pc = FR.pair_case(2, 3, 4)
    a = pc["a"].to(dev)[None].requires_grad_(True)
    loss = P.FFTLoss()(a, pc["b"].to(dev)[None])
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="freed by the first backward"):
        loss.backward()


# ---- E. integration -------------------------------------------------------------------------------------------------------
def _model(dev, chans=(12, 12, 24, 48)):
    from oracle import cidnet_oracle as O
    m = P.CIDNet(channels=list(chans))
    p = O.make_params(21, channels=chans)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


def _step(m, loss_fn, x, gt):
    m.zero_grad(set_to_none=True)
    out = m(x)
    out.retain_grad()
    loss = loss_fn(out, gt)
    loss.backward()
    grads = {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None}
    return loss.detach().clone(), out.grad.detach().clone(), out.detach(), grads


def test_cidnet_loss_term(dev):
    from oracle import cidnet_oracle as O
    x = O.synthetic_batch(31, (2, 3, 32, 48)).to(dev)
    gt = O.synthetic_batch(32, (2, 3, 32, 48)).to(dev)
    m = _model(dev)
    m.two_streams = False
    base = _step(m, P.CIDNetLoss(m), x, gt)
    off = _step(m, P.CIDNetLoss(m, fft_weight=0.0), x, gt)
    assert torch.equal(base[0], off[0]) and torch.equal(base[1], off[1])      # the default objective did not move
    assert len(base[3]) > 50 and base[3].keys() == off[3].keys()
    for n, g in base[3].items():                                              # nor any parameter's gradient
        assert torch.equal(g, off[3][n]), n
    wgt, hvi_w = 0.3, 0.7
    base = _step(m, P.CIDNetLoss(m, HVI_weight=hvi_w), x, gt)
    on = _step(m, P.CIDNetLoss(m, HVI_weight=hvi_w, fft_weight=wgt), x, gt)
    # the term on its own: 0.3 (FFTLoss(rgb) + HVI_weight FFTLoss(hvi)), the HVI target not detached
    m.zero_grad(set_to_none=True)
    out = on[2].clone().requires_grad_(True)
    crit = P.FFTLoss()
    t_rgb, t_hvi = crit(out, gt), crit(m.HVIT(out), m.HVIT(gt))
    term = wgt * (t_rgb + hvi_w * t_hvi)
    term.backward()
    assert float(t_rgb.detach()) > 0 and float(t_hvi.detach()) > 0
    mags = abs(float(base[0])) + wgt * (float(t_rgb.detach()) + hvi_w * float(t_hvi.detach()))
    assert abs(float(on[0]) - (float(base[0]) + float(term.detach()))) <= 4 * 2.0 ** -24 * mags
    want = base[1].double() + out.grad.double()
    assert float((on[1].double() - want).abs().max()) <= 4 * 2.0 ** -24 * float((base[1].abs() + out.grad.abs()).max())
    assert float((on[1] - base[1]).abs().max()) > 0
    # density_k through the TARGET alone: the prediction's HVI map is a constant here, so only HVIT(gt) reaches the parameter
    k = m.trans.density_k
    k.grad = None
    with torch.no_grad():
        pred_hvi = m.HVIT(on[2])
    P.FFTLoss(wgt)(pred_hvi, m.HVIT(gt)).backward()
    assert k.grad is not None and float(k.grad.abs().max()) > 0
    assert not torch.equal(on[3]["trans.density_k"], base[3]["trans.density_k"])


def test_trainer_steps_with_the_term_eager_and_captured(dev):
    from oracle import cidnet_oracle as O
    from hvi_cidnet_amd.dp import DataParallelTrainer
    shape = (2, 3, 64, 64)
    batches = [(O.synthetic_batch(51 + i, shape).to(dev), O.synthetic_batch(61 + i, shape).to(dev)) for i in range(2)]
    res = []
    for use_graph in (False, True):
        m = _model(dev)
        loss_fn = P.CIDNetLoss(m, fft_weight=0.5, fft_norm="ortho")
        tr = DataParallelTrainer(m, lr=1e-3, n_buckets=3, use_graph=use_graph, loss_fn=loss_fn)
        losses = [float(tr.step(x, gt).item()) for x, gt in batches]
        torch.cuda.synchronize()
        res.append((losses, tr.flat_g.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    mb = _model(dev)
    base = DataParallelTrainer(mb, lr=1e-3, n_buckets=3, loss_fn=P.CIDNetLoss(mb))
    assert float(base.step(*batches[0]).item()) != res[0][0][0]              # the term is in the step


def test_first_use_of_a_shape_inside_a_capture(dev):
    """the trainer runs a step eagerly before it captures one, so there the tables exist by then; here the capture itself
    meets the shape first: the tables go into a buffer of the call's own and nothing is cached or synchronised"""
    B, C, H, W = 2, 3, 22, 26
    keys = [(dev.type, dev.index, H, H), (dev.type, dev.index, W, W // 2 + 1)]
    assert not any(k in ops._DFT_TABLES for k in keys)
    a0, b0 = FR.noise(B * C, H, W, 11), FR.noise(B * C, H, W, 12)
    a = a0.to(dev).view(B, C, H, W).clone().requires_grad_(True)
    b = b0.to(dev).view(B, C, H, W).clone().requires_grad_(True)
    crit = P.FFTLoss(FR.WEIGHT, "ortho")
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        warm = torch.rand((1, 1, 8, 10), device=dev, requires_grad=True)       # another shape: the stream's scratch buffer exists
        crit(warm, torch.rand((1, 1, 8, 10), device=dev)).backward()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        loss = crit(a, b)
        ga, gb = torch.autograd.grad(loss, (a, b))
    assert not any(k in ops._DFT_TABLES for k in keys)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), ga.clone(), gb.clone())
    a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    loss2 = crit(a2, b2)
    loss2.backward()
    assert all(k in ops._DFT_TABLES for k in keys)
    assert torch.equal(got[0], loss2.detach()) and torch.equal(got[1], a2.grad) and torch.equal(got[2], b2.grad)
    want = float(FR.reference(a0, b0, FR.WEIGHT, "ortho")[0])
    assert abs(float(got[0]) - want) <= 2e-6 * want


# ---- F. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(dev):
    shape = (2, 5, 6)
    P_, H, W = shape
    Wh = W // 2 + 1
    nS, nx = P_ * H * Wh * 2, P_ * H * W
    x = torch.rand(nx + 4, device=dev)
    S = torch.ones(nS + 4, device=dev)
    gl = torch.ones(4, device=dev)
    th, tw = _tabs(shape, dev)
    f, vp = ctypes.c_float, ctypes.c_void_p
    px, pS, pg = x.data_ptr(), S.data_ptr(), gl.data_ptr()

    def fwd(**k):
        d = dict(a=vp(px), b=vp(px), th=th, tw=tw, weight=f(1.0), norm=0, ws_off=0, short=0, S_off=0, loss_off=0, shape=shape)
        d.update(k)
        _abi(dev, "cidnet_fft_loss_fwd", d["shape"], [1, nS],
             lambda o, ws, n: (d["a"], d["b"], d["th"], d["tw"], d["weight"], d["norm"], vp(o[0].value + d["loss_off"]),
                               vp(o[1].value + d["S_off"]), vp(ws.value + d["ws_off"]), n - d["short"]), expect=d["code"])

    def bwd(**k):
        d = dict(S=vp(pS), th=th, tw=tw, g=vp(pg), weight=f(1.0), norm=0, ws_off=0, short=0, ga_off=0, shape=shape)
        d.update(k)
        _abi(dev, "cidnet_fft_loss_bwd", d["shape"], [nx, nx],
             lambda o, ws, n: (d["S"], d["th"], d["tw"], d["g"], d["weight"], d["norm"], vp(o[0].value + d["ga_off"]), o[1],
                               vp(ws.value + d["ws_off"]), n - d["short"]), expect=d["code"])

    common = [(dict(th=None), ARG), (dict(tw=None), ARG), (dict(th=vp(px + 2)), ARG), (dict(norm=2), ARG), (dict(norm=-1), ARG),
              (dict(weight=f(-1.0)), ARG), (dict(weight=f(NAN)), ARG), (dict(weight=f(float("inf"))), ARG), (dict(ws_off=4), ARG),
              (dict(short=1), WS), (dict(shape=(0, 5, 6)), ARG), (dict(shape=(2, 0, 6)), ARG), (dict(shape=(2, 5, 0)), ARG),
              (dict(shape=(2, 2049, 6)), SHAPE), (dict(shape=(2, 5, 2049)), SHAPE), (dict(shape=(65536, 5, 6)), SHAPE),
              (dict(shape=(600, 2048, 2048)), SHAPE)]
    for bad, code in common + [(dict(a=None), ARG), (dict(b=None), ARG), (dict(a=vp(px + 1)), ARG), (dict(b=vp(px + 3)), ARG),
                               (dict(S_off=2), ARG), (dict(loss_off=1), ARG)]:
        fwd(code=code, **bad)
    for bad, code in common + [(dict(S=None), ARG), (dict(g=None), ARG), (dict(S=vp(pS + 2)), ARG), (dict(ga_off=2), ARG)]:
        bwd(code=code, **bad)
    # the two linear maps: the same checks without weight and norm
    for name, src, n_out in (("cidnet_rfft2_fwd", px, nS), ("cidnet_rfft2_adj", pS, nx)):
        for bad, code in [(dict(src=None), ARG), (dict(src=vp(src + 2)), ARG), (dict(th=None), ARG), (dict(tw=None), ARG),
                          (dict(out_off=1), ARG), (dict(ws_off=4), ARG), (dict(short=1), WS), (dict(shape=(2, 5, 0)), ARG),
                          (dict(shape=(2, 5, 2049)), SHAPE)]:
            d = dict(src=vp(src), th=th, tw=tw, out_off=0, ws_off=0, short=0, shape=shape)
            d.update(bad)
            _abi(dev, name, d["shape"], [n_out],
                 lambda o, ws, n: (d["src"], d["th"], d["tw"], vp(o[0].value + d["out_off"]), vp(ws.value + d["ws_off"]),
                                   n - d["short"]), expect=code)
    # a NULL output where one is required
    _abi(dev, "cidnet_fft_loss_fwd", shape, [None, nS],
         lambda o, ws, n: (vp(px), vp(px), th, tw, f(1.0), 0, None, o[1], ws, n), expect=ARG)
    _abi(dev, "cidnet_rfft2_fwd", shape, [None], lambda o, ws, n: (vp(px), th, tw, None, ws, n), expect=ARG)
    _abi(dev, "cidnet_rfft2_adj", shape, [None], lambda o, ws, n: (vp(pS), th, tw, None, ws, n), expect=ARG)
    # the table kernel
    t = _nan(64, dev)
    for args, code in [((0, 1), ARG), ((4, 0), ARG), ((2049, 3), SHAPE), ((4, 5), SHAPE)]:
        assert lib().raw("cidnet_dft_table")(*args, ops._p(t), ops._stream()) == code
    assert lib().raw("cidnet_dft_table")(4, 3, None, ops._stream()) == ARG
    assert lib().raw("cidnet_dft_table")(4, 3, vp(t.data_ptr() + 2), ops._stream()) == ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())
    with pytest.raises(RuntimeError, match="does not take"):
        ops.rfft2_parts(torch.zeros((1, 1, 2049), device=dev))
