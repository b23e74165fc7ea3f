"""References for the frequency-domain training loss (include/cidnet_hip.h, "frequency-domain training loss").  Nothing of the
project runs here.

  * reference():  fp64 torch.fft.rfft2 + autograd on the CPU, the issue's definition word for word.
  * table64():    the twiddle table in fp64 with the integer reduction, exact at the quarter turns.
  * closed_form(): the definition written out with DFT matrices, the identities the kernels implement.
  * restate_spectrum() / restate_adjoint() ("restate32"): the four GEMMs of csrc/fft_loss.hip in numpy with an fp32 accumulator that takes k = 0, 1, 2, ... in
    ascending order (the kernel's chunks follow one another in that order and a lane's accumulator takes a chunk's k in
    order), each product fused into the sum (formed exactly in fp64, the sum rounded once to fp32), from the fp32 table.
  * E32 of a case: the largest deviation of restate32 from the fp64 reference on the same fp32 input.  Every tolerance of the
    GPU tests is 8 * E32 + 1e-30 (TOL), the factor tests/test_loss_kernels_gpu.py section A uses for the same construction.
  * the fixtures: uniform-noise planes, the pairs b = clamp(0.7 a + 0.3 n), and their seed rule (pair_case).
"""
import functools
import math

import numpy as np
import torch

MARGIN = 8.0
WEIGHT, G_UP = 0.3, 2.5                                      # the loss weight and the upstream factor of section D
NORMS = ("backward", "ortho")


def shapes(MT, NT, KC):
    """(P, H, W) of sections B, C and D for a kernel whose block tile is MT x NT with K chunks of KC (the plan query's first
    three fields); what each reaches is in tests/test_fft_loss_gpu.py.  With 64 / 64 / 64: ..., (1,63,124), (1,64,126),
    (1,65,129), (1,32,63), (1,32,64), (1,32,65), (3,21,33), (5,13,20), ..."""
    return [(1, 1, 1), (2, 3, 4), (3, 5, 7), (1, 16, 30), (1, 16, 31),
            (1, MT - 1, 2 * NT - 4), (1, MT, 2 * NT - 2), (1, MT + 1, 2 * NT + 1),
            (1, KC // 2, KC - 1), (1, KC // 2, KC), (1, KC // 2, KC + 1),
            (3, (MT - 1) // 3, 33), (5, (MT + 1) // 5, 20), (6, 50, 75), (1, 400, 600)]


def tol(e32):
    return MARGIN * e32 + 1e-30


def table64(N, Nk):
    """(N, Nk, 2) float64: (cos, -sin)(2 pi m / N) with m = n k mod N reduced in integers; exactly 0 / +-1 where 4 m is a
    multiple of N"""
    m = (np.arange(N, dtype=np.int64)[:, None] * np.arange(Nk, dtype=np.int64)[None, :]) % N
    ang = 2.0 * np.pi * m.astype(np.float64) / N
    c, s = np.cos(ang), -np.sin(ang)
    q = (4 * m) % N == 0                                      # quarter turns: 4 m / N in {0, 1, 2, 3}
    quarter = (4 * m) // N
    c = np.where(q, np.array([1.0, 0.0, -1.0, 0.0])[quarter % 4], c)
    s = np.where(q, np.array([0.0, -1.0, 0.0, 1.0])[quarter % 4], s)
    return np.stack([c, s], axis=-1)


def table32(N, Nk):
    return table64(N, Nk).astype(np.float32)


def scale_of(weight, norm, P, H, W):
    """weight s / (2 P H Wh) in fp64 from the fp32 weight, as the entry points form it"""
    s = 1.0 / math.sqrt(float(H) * float(W)) if norm == "ortho" else 1.0
    return float(np.float32(weight)) * s / (2.0 * P * H * (W // 2 + 1))


def spectrum64(x):
    """x (P,H,W) torch tensor -> (P,H,Wh,2) float64: the parts of the unnormalised half spectrum"""
    return torch.view_as_real(torch.fft.rfft2(x.double())).contiguous()


def adjoint64(S, W):
    """the fp64 vjp of x -> view_as_real(rfft2(x)) with cotangent S (P,H,Wh,2): what autograd gives"""
    P, H = S.shape[0], S.shape[1]
    x = torch.zeros((P, H, W), dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.view_as_real(torch.fft.rfft2(x)), x, S.double())
    return g


def reference(a, b, weight=WEIGHT, norm="backward", g_up=G_UP):
    """a, b fp32 (P,H,W) -> (loss, dloss/da, dloss/db) in fp64, the gradients of g_up * loss: the issue's definition,
    weight * F.l1_loss(view_as_real(rfft2(a, norm=norm)), view_as_real(rfft2(b, norm=norm))) with the fp32 weight"""
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    fa, fb = torch.fft.rfft2(a64, norm=norm), torch.fft.rfft2(b64, norm=norm)
    loss = float(np.float32(weight)) * torch.nn.functional.l1_loss(torch.view_as_real(fa), torch.view_as_real(fb))
    ga, gb = torch.autograd.grad(loss * g_up, (a64, b64))
    return loss.detach(), ga, gb


def closed_form(a, b, weight=WEIGHT, norm="backward", g_up=G_UP):
    """the same three values from the DFT matrices: D = sum d exp(-i t), loss = weight s / (2 P H Wh) sum |Re D| + |Im D|,
    gradient = g_up weight s / (2 P H Wh) sum sign(Re D) cos t - sign(Im D) sin t; also returns D (P,H,Wh,2)"""
    P, H, W = a.shape
    d = (a.double() - b.double()).numpy()
    th, tw = table64(H, H), table64(W, W // 2 + 1)
    Eh, Ew = th[..., 0] + 1j * th[..., 1], tw[..., 0] + 1j * tw[..., 1]          # exp(-i 2 pi y ky / H), exp(-i 2 pi x kx / W)
    D = np.einsum("yk,pyx,xl->pkl", Eh, d, Ew)
    c = scale_of(weight, norm, P, H, W)
    loss = c * (np.abs(D.real).sum() + np.abs(D.imag).sum())
    sr, si = np.sign(D.real), np.sign(D.imag)
    # d(Re D)/dd = cos t = Re(Eh Ew), d(Im D)/dd = -sin t = Im(Eh Ew)
    g = np.einsum("pkl,yk,xl->pyx", sr, Eh.real, Ew.real) - np.einsum("pkl,yk,xl->pyx", sr, Eh.imag, Ew.imag) \
        + np.einsum("pkl,yk,xl->pyx", si, Eh.imag, Ew.real) + np.einsum("pkl,yk,xl->pyx", si, Eh.real, Ew.imag)
    return loss, g_up * c * g, np.stack([D.real, D.imag], axis=-1)


# ---- the fp32 restatement -------------------------------------------------------------------------------------------------
def _gemm32(A, B):
    """A (..., M, K) @ B (..., K, N) with an fp32 accumulator over k ascending, each product fused into the sum"""
    K = A.shape[-1]
    acc = np.zeros(np.broadcast_shapes(A.shape[:-2], B.shape[:-2]) + (A.shape[-2], B.shape[-1]), dtype=np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    for k in range(K):
        acc = (acc.astype(np.float64) + A64[..., :, k, None] * B64[..., k, None, :]).astype(np.float32)
    return acc


def _rot(X, adjoint):
    """X (P,H,Wh,2) -> (P, 2 H, 2 Wh): row 2 y is X[y] with (re, im) interleaved; row 2 y + 1 is (-im, re), the adjoint's
    (im, -re)"""
    P, H, Wh, _ = X.shape
    even = X.reshape(P, H, 2 * Wh)
    odd = np.stack([X[..., 1], -X[..., 0]] if adjoint else [-X[..., 1], X[..., 0]], axis=-1).reshape(P, H, 2 * Wh)
    return np.stack([even, odd], axis=2).reshape(P, 2 * H, 2 * Wh)


def restate_spectrum(d):
    """d fp32 numpy (P,H,W) -> D (P,H,Wh,2) fp32: products (a) and (b)"""
    P, H, W = d.shape
    Wh = W // 2 + 1
    R = _gemm32(d.reshape(P * H, W), table32(W, Wh).reshape(W, 2 * Wh)).reshape(P, H, Wh, 2)
    return _gemm32(table32(H, H).reshape(H, 2 * H), _rot(R, False)).reshape(P, H, Wh, 2)


def restate_adjoint(S, W, f=None):
    """S fp32 numpy (P,H,Wh,2) -> g (P,H,W) fp32: products (c) and (d); f: the fp32 factor of (d)'s epilogue"""
    P, H, Wh, _ = S.shape
    G = _gemm32(table32(H, H).reshape(H, 2 * H), _rot(S, True))                      # (P, H, 2 Wh)
    g = _gemm32(G.reshape(P * H, 2 * Wh), table32(W, Wh).reshape(W, 2 * Wh).T.copy()).reshape(P, H, W)
    return g if f is None else g * np.float32(f)


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def noise(P, H, W, seed):
    return torch.rand((P, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _base_seed(P, H, W):
    return 1000 * P + 37 * H + W


@functools.lru_cache(maxsize=None)
def spectrum_case(P, H, W):
    """section B: x, its fp64 spectrum, E32.  Computed once and shared, read-only."""
    x = noise(P, H, W, _base_seed(P, H, W))
    D64 = spectrum64(x)
    e32 = float(np.abs(restate_spectrum(x.numpy()).astype(np.float64) - D64.numpy()).max())
    return x, D64, e32


@functools.lru_cache(maxsize=None)
def adjoint_case(P, H, W, kind):
    """section C: a spectrum-shaped cotangent ("normal": normal-distributed, "signs": +-1 / 0), its fp64 vjp, E32"""
    gen = torch.Generator().manual_seed(_base_seed(P, H, W) + (5 if kind == "normal" else 6))
    shape = (P, H, W // 2 + 1, 2)
    if kind == "normal":
        S = torch.randn(shape, generator=gen, dtype=torch.float32)
    else:
        S = torch.randint(-1, 2, shape, generator=gen).float()
    g64 = adjoint64(S, W)
    e32 = float(np.abs(restate_adjoint(S.numpy(), W).astype(np.float64) - g64.numpy()).max())
    return S, g64, e32


def near_limit(parts):
    """how many parts of a case may lie within 8 E32 of zero without being zero: 0.1 %, none under 2000 parts"""
    return 0 if parts < 2000 else parts // 1000


@functools.lru_cache(maxsize=None)
def pair_case(P, H, W):
    """section D: the pair a, b = clamp(0.7 a + 0.3 n) of the first seed from the base seed on whose fp64 spectrum has at most
    near_limit parts with 0 < |part| < 8 E32.  -> dict: a, b (fp32 (P,H,W)), D64 (the parts of rfft2(a - b)), e32 (of the
    spectrum), near (bool mask of those parts), n_near, seed"""
    for seed in range(_base_seed(P, H, W), _base_seed(P, H, W) + 50):
        a = noise(P, H, W, 2 * seed)
        b = (0.7 * a + 0.3 * noise(P, H, W, 2 * seed + 1)).clamp(0.0, 1.0)
        d = a - b                                             # fp32, as the kernel's staging forms it
        D64 = spectrum64(d)
        e32 = float(np.abs(restate_spectrum(d.numpy()).astype(np.float64) - D64.numpy()).max())
        near = (D64.abs() > 0) & (D64.abs() < tol(e32))
        if int(near.sum()) <= near_limit(D64.numel()):
            return dict(a=a, b=b, D64=D64, e32=e32, near=near, n_near=int(near.sum()), seed=seed)
    raise AssertionError(f"no seed gives a fixture for {(P, H, W)}")


@functools.lru_cache(maxsize=None)
def loss_case(P, H, W, norm):
    """section D, per norm: the fp64 loss and gradients of g_up * loss, the gradient's E32 (the restatement run on the fp64
    signs, so that it measures the products and not a flipped sign) and c = |g_up weight s| / (2 P H Wh)"""
    pc = pair_case(P, H, W)
    loss, ga, gb = reference(pc["a"], pc["b"], WEIGHT, norm, G_UP)
    c = scale_of(WEIGHT, norm, P, H, W)
    S64 = torch.sign(pc["D64"]).float().numpy()
    f = np.float32(c) * np.float32(G_UP)
    e32 = float(np.abs(restate_adjoint(S64, W, f).astype(np.float64) - ga.numpy()).max())
    return dict(loss=loss, ga=ga, gb=gb, e32=e32, c=abs(G_UP * c))
