"""csrc/attn.hip against fp64: the LCA channel attention (gram_kernel<TI, DT>, softmax_fwd_kernel, softmax_bwd_kernel) through
cidnet_attn_fwd, cidnet_attn_fwd_t and cidnet_attn_bwd, with normalize = 1 (CABResidualFn) and normalize = 0 (NoiseCABResidualFn),
compared with a plain torch fp64 CPU evaluation written from the math: q, k (B, C, HW) viewed per head, F.normalize(., dim=-1)
(eps 1e-12) when normalised, shat = qn kn^T, attn = softmax(shat * T), M_b[:, head block] = Wp[:, head block] attn_b; autograd of
sum(M * dM) supplies gq, gk, gT, gWp, and a loop over the samples the per-sample dWp_b and dT_b.  Nothing of the project is on the
reference side.

Every output and the workspace (exactly cidnet_attn_gram_ws_floats floats) are allocated NaN-filled, must be finite after the
call, and a second call into fresh buffers must be bit-identical.  The v third of the (B, 3C, HW) tensor is NaN: the attention
kernels must never read it.  Criterion: max|out - ref| <= 2e-5 * max|ref| + 1e-6 per output tensor (test_ops_gpu.close) for every
forward and backward output; nq and nk are exactly 1.0 when un-normalised.  A float32 CPU evaluation of the reference differs
from fp64 by at most 0.04 of this bound on every output at every case below but one, so the criterion leaves over 20x (the
kernels measured at most 0.07 of it).  The one: [gq; gk] at (36, 2), HW = 1, normalised.  A one-pixel row is its own direction, so the
normalisation's Jacobian annihilates every gradient and the fp64 reference is 0 up to 4.4e-16, while its terms G_ij k_j / (nq_i nk_j)
are O(1 / |q_i|) with |q_i| down to 0.045; what is compared is their rounding residue.  The float32 CPU evaluation of the
reference leaves 1.907e-6 there, above the criterion's absolute 1e-6 (the kernel's Wqk, multiplied out in fp64, leaves 1.384e-6),
so this one output at this one case is allowed 4 x 1.907e-6 = 7.63e-6 absolute in place of the 1e-6 (ZERO_GRADIENT_ATOL;
test_fixtures_do_not_cancel checks on the host that the float32 evaluation misses the 1e-6); the relative part stays.  The
un-normalised case at HW = 1 and every other output at HW = 1 keep the plain criterion.

The backward is fed the fp64 reference's forward outputs cast to fp32.  Wqk, the per-sample (2C x 2C) map [q; k] -> [gq; gk], must
be exactly 0 outside each head's own q / k blocks and, un-normalised, on the diagonal; Wqk.double() @ [q; k] evaluated in fp64 on
the CPU is compared with [gq; gk].

Fixture: q = randn; per head k = 0.6 R q_head + 0.8 randn with R a random orthogonal ch x ch matrix, so that S = q k^T is about
0.6 HW R^T and does not cancel; T cycles through 1.0, 0.37, 4.0, -2.0, 8.0, 0.5, 1.5, 3.0 per head; Wp = 0.3 randn; dM = randn; for
normalize = 0, q and k are each scaled by HW**-0.5 so |T S| stays O(10).  Every case asserts in fp64, before it compares,
max|S| >= 0.05 * max sum|q_i k_j| and the same for gT and gWp against the sums of their absolute terms (`noncancelling`);
test_fixtures_do_not_cancel does so for every case on the host.  gT is a sum of B * ch * ch terms of random sign, so a case
whose first seed left it near that bound takes a later one (SEED).

Channel tilings at HW = 130 (one chunk of 130 pixels, n_red = 4), B = 2, both modes:

  (C, heads)   ch   what it reaches
  (1, 1)        1   TI = 1: fifteen of sixteen tile rows clamped to row 0; one-element softmax
  (48, 8)       6   TI = 1, ten clamped rows; all eight temperatures, the negative one included
  (12, 1)      12   the small config, one head: its block is the whole of Wp and of Wqk's off-diagonal quarters
  (32, 2)      16   TI = 1, the tile exactly full: no clamped row
  (34, 2)      17   TI = 2 with one live row in the second tile, fifteen clamped
  (36, 2)      18   the model's, also with B = 3
  (72, 4)      18   the model's
  (144, 8)     18   the model's widest: the largest dynamic LDS of softmax_bwd_kernel
  (32, 1)      32   TI = 2, both tiles full: the limit
  (33, 1), (36, 5)  CIDNET_ERR_SHAPE from both entry points; a workspace one float short: CIDNET_ERR_WS; outputs stay NaN

Pixel counts at (C, heads) = (36, 2), B = 1, both modes (chunks of 512 pixels below 16384 pixels, of 2048 from there; a chunk's
four waves take 32 pixels each per 128-pixel step, a wave's four k-slots 8 each; n_red = 4 * chunks slabs):

  HW       what it reaches
  1, 5, 7  the checked loader only (chunk under 8 pixels)
  8        the narrowest wide chunk: k-slots 1..3 pulled back to pixel 0 and fully masked
  9        k-slot 1 pulled back by 7 pixels, `dup` = 7
  31, 32, 33       the wave boundary: wave 1 idle, idle, one pixel (dup = 7)
  127, 128, 129    the second loop iteration: wave 0 takes pixel 128
  511, 512         one chunk, nearly full and full
  513      a second chunk of 1 pixel: the checked loader beside a wide chunk
  519      a second chunk of 7 pixels
  520      a second chunk of exactly 8 pixels
  1001     the bf16 self-comparison's count
  2048     n_red = 16: one unrolled pass of the slab sum, no remainder
  2049     n_red = 20: 16 + 4
  16383    512-pixel chunks, n_red = 128; last chunk 511
  16384    the switch to 2048-pixel chunks, n_red = 32
  18435    2048-pixel chunks; last chunk of 3 pixels on the checked loader; n_red = 40 = 32 + 8
  16383, 16384, 18435 again at (34, 2): TI = 2 with fifteen clamped rows

bf16 storage (cidnet_attn_fwd_t, dt = bf16), forward only: HW in 5, 8, 33, 129, 513, 1001 at (34, 2) and (36, 2), both modes, against
the fp64 reference evaluated on the bf16-rounded values; the same criterion, since the products stay fp32.

Zero-norm rows: (36, 2), HW = 130, B = 2, normalised; in sample 1 row 3 of q (head 0) and row 5 of k (head 1) are exact zeros.
Their nq / nk must equal float32(1e-12) exactly and their shat row / column exactly 0; their gradient is divided by eps
(about 1e10), so the dead rows and the live rows of [gq; gk] are compared separately, each relative to its own maximum.

CABResidualFn (output and nine gradients) at (B, C, heads, H, W) = (2, 36, 2, 5, 15), (1, 12, 1, 9, 14), (1, 72, 4, 3, 43) and
NoiseCABResidualFn (output and eleven gradients) at the first two, against fp64 autograd of the block written with conv2d (1x1;
depthwise 3x3, padding 1), the attention math above and conv2d with Wp; for the noise block v is multiplied by
sigmoid(conv1x1(noise_map)) and the q / kv weights carry HW**-0.5 so that the raw logits stay O(1) (max|T S| <= 16 asserted).
Two runs, bit-identical and finite, every result through the same criterion.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ops_gpu import close  # noqa: E402
from test_tnsm_gpu import F32, NAN, _gen, _ids, _ops, noncancelling, twice  # noqa: E402

gpu = pytest.mark.gpu

EPS = 1e-12                                    # F.normalize's eps
T_CYCLE = (1.0, 0.37, 4.0, -2.0, 8.0, 0.5, 1.5, 3.0)
TILINGS = [(1, 1), (48, 8), (12, 1), (32, 2), (34, 2), (36, 2), (72, 4), (144, 8), (32, 1)]
TILING_HW = 130
BAD_SHAPES = [(33, 1), (36, 5)]
PIXELS = [1, 5, 7, 8, 9, 31, 32, 33, 127, 128, 129, 511, 512, 513, 519, 520, 1001, 2048, 2049, 16383, 16384, 18435]
PIXELS_TI2_CLAMPED = [16383, 16384, 18435]     # repeated at (34, 2)
BF16_HW = [5, 8, 33, 129, 513, 1001]
BF16_CH = [(34, 2), (36, 2)]
DEAD = dict(C=36, heads=2, HW=130, B=2, b=1, q_ch=3, k_ch=18 + 5, k_row=5)      # sample 1: row 3 of head 0 (q), row 5 of head 1 (k)
CAB_SHAPES = [(2, 36, 2, 5, 15), (1, 12, 1, 9, 14), (1, 72, 4, 3, 43)]
NOISE_CAB_SHAPES = [(2, 36, 2, 5, 15), (1, 12, 1, 9, 14)]
# gT sums B * ch * ch terms whose signs dM = randn leaves random, so at most seeds it sits near the 0.05 of `noncancelling`: these
# cases take the first seed at which every sum of the fixture clears it by 1.5x (0.075) in both modes and every kind
ZERO_GRADIENT_CASE = (36, 2, 1, 1, 1)           # (C, heads, HW, B, normalize): [gq; gk] is identically 0, see the docstring
ZERO_GRADIENT_ATOL = 4 * 1.907e-6
SEED = {(32, 1, 130, 2): 33, (36, 2, 130, 3): 2, (36, 2, 1, 1): 8, (36, 2, 8, 1): 1, (36, 2, 9, 1): 1, (36, 2, 31, 1): 1, (36, 2, 32, 1): 2,
        (36, 2, 128, 1): 1, (36, 2, 520, 1): 3, (36, 2, 1001, 1): 1, (36, 2, 16383, 1): 1, (34, 2, 18435, 1): 2, (34, 2, 129, 1): 3,
        (34, 2, 513, 1): 1}


def gram_pch(HW):
    """the chunking rule of csrc/attn.hip, restated"""
    return 2048 if HW >= 16384 else 512


def geometry(C, heads, HW):
    ch, pch = C // heads, gram_pch(HW)
    chunks = -(-HW // pch)
    return dict(ch=ch, TI=1 if ch <= 16 else 2, chunks=chunks, last=HW - (chunks - 1) * pch, n_red=4 * chunks)


def all_cases():
    """(C, heads, HW, B, kind) of every raw-entry-point case; each runs with normalize 1 and 0 unless it is the dead-row case"""
    cases = [(C, h, TILING_HW, 2, "f32") for C, h in TILINGS] + [(36, 2, TILING_HW, 3, "f32")]
    cases += [(36, 2, HW, 1, "f32") for HW in PIXELS] + [(34, 2, HW, 1, "f32") for HW in PIXELS_TI2_CLAMPED]
    cases += [(C, h, HW, 1, "bf16") for C, h in BF16_CH for HW in BF16_HW]
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def attn_math(q, k, T, heads, normalize):
    """q, k (B, C, HW), T (heads) -> shat, shat * T, softmax, each (B, heads, ch, ch)"""
    B, C, HW = q.shape
    ch = C // heads
    qh, kh = q.reshape(B, heads, ch, HW), k.reshape(B, heads, ch, HW)
    if normalize:
        qh, kh = F.normalize(qh, dim=-1), F.normalize(kh, dim=-1)
    shat = qh @ kh.transpose(-1, -2)
    logit = shat * T.reshape(1, heads, 1, 1)
    return shat, logit, torch.softmax(logit, -1)


def fold(Wp, attn):
    """M_b[:, head block] = Wp[:, head block] @ attn_b"""
    heads, ch = attn.shape[1:3]
    return torch.cat([Wp[:, h * ch:(h + 1) * ch] @ attn[:, h] for h in range(heads)], -1)


def ref_attn(q, k, T, Wp, dM, heads, normalize):
    q, k, T, Wp = (x.detach().clone().requires_grad_(True) for x in (q, k, T, Wp))
    B, C, HW = q.shape
    ch = C // heads
    shat, logit, attn = attn_math(q, k, T, heads, normalize)
    M = fold(Wp, attn)
    gq, gk, gT, gWp, gl = torch.autograd.grad((M * dM).sum(), (q, k, T, Wp, logit), retain_graph=True)
    per = [torch.autograd.grad((M[b] * dM[b]).sum(), (T, Wp), retain_graph=True) for b in range(B)]
    qh, kh = q.detach().reshape(B, heads, ch, HW), k.detach().reshape(B, heads, ch, HW)
    one = torch.ones(B, C, dtype=q.dtype)
    r = dict(shat=shat.detach(), attn=attn.detach(), M=M.detach(), gq=gq, gk=gk, gT=gT, gWp=gWp,
             dT_b=torch.stack([p[0] for p in per]), dWp_b=torch.stack([p[1] for p in per]),
             nq=qh.norm(dim=-1).clamp_min(EPS).reshape(B, C) if normalize else one,
             nk=kh.norm(dim=-1).clamp_min(EPS).reshape(B, C) if normalize else one,
             S=qh @ kh.transpose(-1, -2), S_abs=qh.abs() @ kh.abs().transpose(-1, -2), logit=logit.detach(),
             gT_abs=(gl * shat.detach()).abs().sum((0, 2, 3)),
             gWp_abs=torch.cat([(dM[:, :, h * ch:(h + 1) * ch].abs() @ attn.detach()[:, h].transpose(-1, -2)).sum(0)
                                for h in range(heads)], -1))
    return r


@functools.lru_cache(maxsize=None)
def attn_case(C, heads, HW, B, normalize, kind="f32"):
    """kind: "f32", "bf16" (q and k rounded to bf16 values) or "dead" (one zero row of q and one of k)"""
    g = _gen(41, C, heads, HW, B, SEED.get((C, heads, HW, B), 0))
    ch = C // heads
    q = torch.randn(B, C, HW, generator=g)
    k = torch.empty_like(q)
    for h in range(heads):
        R = torch.linalg.qr(torch.randn(ch, ch, generator=g)).Q
        k[:, h * ch:(h + 1) * ch] = 0.6 * (R @ q[:, h * ch:(h + 1) * ch]) + 0.8 * torch.randn(B, ch, HW, generator=g)
    if not normalize:
        q, k = q * HW ** -0.5, k * HW ** -0.5
    if kind == "bf16":
        q, k = q.bfloat16().float(), k.bfloat16().float()
    if kind == "dead":
        q[DEAD["b"], DEAD["q_ch"]] = 0.0
        k[DEAD["b"], DEAD["k_ch"]] = 0.0
    t = dict(q=q, k=k, T=torch.tensor([T_CYCLE[h % len(T_CYCLE)] for h in range(heads)]),
             Wp=0.3 * torch.randn(C, C, generator=g), dM=torch.randn(B, C, C, generator=g))
    r = ref_attn(*(t[n].double() for n in ("q", "k", "T", "Wp", "dM")), heads, normalize)
    what = f"C={C} heads={heads} HW={HW} B={B} normalize={normalize} {kind}"
    noncancelling(r["S"], r["S_abs"], "S " + what)
    noncancelling(r["gT"], r["gT_abs"], "gT " + what)
    noncancelling(r["gWp"], r["gWp_abs"], "gWp " + what)
    assert all(bool(torch.isfinite(v).all()) for v in r.values()), what
    return t, r


# ---------------------------------------------------------------------------------------------------------------------
# the case table and the fixtures, on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_it_claims():
    geo = {HW: geometry(36, 2, HW) for HW in PIXELS}
    assert any(1 <= v["last"] <= 7 and v["chunks"] > 1 for v in geo.values())          # checked loader beside wide chunks
    assert {HW for HW, v in geo.items() if v["last"] < 8 and v["chunks"] == 1} == {1, 5, 7}
    assert geo[520]["last"] == 8 and geo[520]["chunks"] == 2 and geo[8]["last"] == 8
    assert geo[513]["last"] == 1 and geo[519]["last"] == 7 and geo[18435]["last"] == 3 and geo[18435]["chunks"] == 10
    assert {HW: v["n_red"] for HW, v in geo.items() if HW >= 2048} == {2048: 16, 2049: 20, 16383: 128, 16384: 32, 18435: 40}
    assert {v["n_red"] % 16 for v in geo.values() if v["n_red"] >= 16} == {0, 4, 8}
    assert any(v["n_red"] < 16 for v in geo.values())
    assert geo[16383]["chunks"] == 32 and geo[16384]["chunks"] == 8                     # 512-pixel chunks, then 2048
    assert {C // h: geometry(C, h, TILING_HW)["TI"] for C, h in TILINGS} == {1: 1, 6: 1, 12: 1, 16: 1, 17: 2, 18: 2, 32: 2}
    assert all(geometry(C, h, HW)["TI"] == 2 for C, h in BF16_CH for HW in BF16_HW)
    for C, heads, HW, B, _ in all_cases():                                              # the library's own chunk count
        v = geometry(C, heads, HW)
        assert _ops()._raw("cidnet_attn_gram_ws_floats", B, C, heads, HW) == B * heads * v["n_red"] * (v["ch"] ** 2 + 2 * v["ch"])
    for C, heads in BAD_SHAPES:
        assert C % heads != 0 or C // heads > 32
    for B, C, heads, H, W in CAB_SHAPES + NOISE_CAB_SHAPES:
        assert C * (C // heads) <= 144 * 18


def test_fixtures_do_not_cancel():
    """builds every fixture of the table (each asserts the non-cancelling conditions and a finite reference as it is built)"""
    for C, heads, HW, B, kind in all_cases():
        for normalize in (1, 0):
            attn_case(C, heads, HW, B, normalize, kind)
    d = DEAD
    t, r = attn_case(d["C"], d["heads"], d["HW"], d["B"], 1, "dead")
    assert r["nq"][d["b"], d["q_ch"]] == EPS and r["nk"][d["b"], d["k_ch"]] == EPS
    assert bool((r["shat"][d["b"], 0, d["q_ch"]] == 0).all()) and bool((r["shat"][d["b"], 1, :, d["k_row"]] == 0).all())
    assert r["gq"][d["b"], d["q_ch"]].abs().max() > 1e8 and r["gk"][d["b"], d["k_ch"]].abs().max() > 1e8
    C, heads, HW, B, normalize = ZERO_GRADIENT_CASE                  # the one widened bound: 4x the float32 reference's own error
    t, r = attn_case(C, heads, HW, B, normalize)
    r32 = ref_attn(*(t[n] for n in ("q", "k", "T", "Wp", "dM")), heads, normalize)
    ref = torch.cat([r["gq"], r["gk"]], 1)
    e32 = (torch.cat([r32["gq"], r32["gk"]], 1).double() - ref).abs().max().item()
    assert ref.abs().max() < 1e-14 and 1e-6 < e32 <= ZERO_GRADIENT_ATOL <= 1e-4, e32        # measured: e32 = 1.907e-6
    for shape in CAB_SHAPES:
        block_case(shape, False)
    for shape in NOISE_CAB_SHAPES:
        block_case(shape, True)


# ---------------------------------------------------------------------------------------------------------------------
# the raw entry points
# ---------------------------------------------------------------------------------------------------------------------
def check(o, r, what, atol=None):
    """test_ops_gpu.close, after printing the figures; atol replaces its absolute 1e-6 (ZERO_GRADIENT_CASE only)"""
    o64, r64 = o.detach().cpu().double(), r.detach().cpu().double()
    d, m = (o64 - r64).abs().max().item(), r64.abs().max().item()
    print(f"{what}: max|diff| {d:.3e}, max|ref| {m:.3e}")
    assert o64.shape == r64.shape, what
    if atol is None:
        close(o, r, what=what)
    else:
        assert d <= 2e-5 * m + atol, f"{what}: max diff {d:.3e} > tol {2e-5 * m + atol:.3e}"


def fwd_specs(B, C, heads):
    ch = C // heads
    return ((B, heads, ch, ch), F32), ((B, heads, ch, ch), F32), ((B, C), F32), ((B, C), F32), ((B, C, C), F32)


def k_attn_fwd(qkv, T, Wp, heads, normalize, outs, short=0, typed=False):
    """attn, shat, nq, nk, M = outs; a NaN-filled workspace of exactly the floats the library asks for (less `short`)"""
    ops = _ops()
    B, C3, HW = qkv.shape
    C = C3 // 3
    n = ops._raw("cidnet_attn_gram_ws_floats", B, C, heads, HW) - short
    ws = torch.full((n,), NAN, device=qkv.device)
    tail = (ops._p(T), ops._p(Wp), *(ops._p(o) for o in outs), ops._p(ws), n, B, C, heads, HW, normalize, ops._stream())
    if typed or qkv.dtype == torch.bfloat16:
        ops.lib().call("cidnet_attn_fwd_t", ops._p(qkv), ops._dt(qkv), *tail)
    else:
        ops.lib().call("cidnet_attn_fwd", ops._p(qkv), *tail)


def k_attn_bwd(dM, Wp, attn, shat, nq, nk, T, heads, normalize, outs):
    """dWp_b, dT_b, Wqk = outs"""
    ops = _ops()
    B, C = nq.shape
    ops.lib().call("cidnet_attn_bwd", *(ops._p(x) for x in (dM, Wp, attn, shat, nq, nk, T)), *(ops._p(o) for o in outs), B, C, heads,
                   normalize, ops._stream())


def k_sum_rows(part, n_red, n, out):
    ops = _ops()
    ops.lib().call("cidnet_sum_rows", ops._p(part), n_red, n, ops._p(out), ops._stream())


def make_qkv(dev, t, kind):
    """(B, 3C, HW) with q, k and a NaN v"""
    q, k = t["q"], t["k"]
    B, C, HW = q.shape
    qkv = torch.full((B, 3 * C, HW), NAN)
    qkv[:, :C], qkv[:, C:2 * C] = q, k
    qkv = qkv.to(dev)
    return qkv.to(torch.bfloat16) if kind == "bf16" else qkv


def own_blocks(C, heads):
    """(2C, 2C) mask of the entries of Wqk a head may write: its diagonal and its own k (for q rows) / q (for k rows) block"""
    ch = C // heads
    m = torch.eye(2 * C, dtype=torch.bool)
    for h in range(heads):
        s = slice(h * ch, (h + 1) * ch)
        ks = slice(C + h * ch, C + (h + 1) * ch)
        m[s, ks] = True
        m[ks, s] = True
    return m


def run_attn(dev, C, heads, HW, B, normalize, kind="f32"):
    t, r = attn_case(C, heads, HW, B, normalize, kind)
    what = f"C={C} heads={heads} HW={HW} B={B} normalize={normalize} {kind}: "
    qkv = make_qkv(dev, t, kind)
    T, Wp, dM = (t[n].to(dev) for n in ("T", "Wp", "dM"))
    outs = twice(dev, lambda *o: k_attn_fwd(qkv, T, Wp, heads, normalize, o), *fwd_specs(B, C, heads))
    for o, n in zip(outs, ("attn", "shat", "nq", "nk", "M")):
        check(o, r[n], what + n)
    nq, nk = outs[2].cpu(), outs[3].cpu()
    if not normalize:
        assert bool((nq == 1.0).all()) and bool((nk == 1.0).all()), "un-normalised nq / nk are not exactly 1"
    if kind == "dead":
        d = DEAD
        eps32 = torch.tensor(EPS, dtype=F32)
        assert nq[d["b"], d["q_ch"]] == eps32 and nk[d["b"], d["k_ch"]] == eps32, "nq / nk of a zero row is not eps"
        assert int((nq == eps32).sum()) == 1 and int((nk == eps32).sum()) == 1
        shat = outs[1].cpu()
        assert bool((shat[d["b"], 0, d["q_ch"]] == 0).all()) and bool((shat[d["b"], 1, :, d["k_row"]] == 0).all())
    if kind == "bf16":
        return outs
    # backward, fed the reference's forward outputs
    fed = [r[n].float().to(dev) for n in ("attn", "shat", "nq", "nk")]
    dWp_b, dT_b, Wqk = twice(dev, lambda *o: k_attn_bwd(dM, Wp, *fed, T, heads, normalize, o), ((B, C, C), F32), ((B, heads), F32),
                             ((B, 2 * C, 2 * C), F32))
    check(dWp_b, r["dWp_b"], what + "dWp_b")
    check(dT_b, r["dT_b"], what + "dT_b")
    gWp, gT = twice(dev, lambda a, b: (k_sum_rows(dWp_b, B, C * C, a), k_sum_rows(dT_b, B, heads, b)), ((C, C), F32), ((heads,), F32))
    check(gWp, r["gWp"], what + "gWp")
    check(gT, r["gT"], what + "gT")
    W = Wqk.cpu()
    assert bool((W[:, ~own_blocks(C, heads)] == 0).all()), "Wqk is not zero outside the heads' own blocks"
    if not normalize:
        assert bool((W.diagonal(dim1=1, dim2=2) == 0).all()), "un-normalised Wqk has a diagonal"
    got = W.double() @ torch.cat([t["q"], t["k"]], 1).double()
    ref = torch.cat([r["gq"], r["gk"]], 1)
    if kind == "dead":
        dead = torch.zeros(B, 2 * C, dtype=torch.bool)
        dead[DEAD["b"], DEAD["q_ch"]] = dead[DEAD["b"], C + DEAD["k_ch"]] = True
        assert ref[dead].abs().max() > 1e8 > 1e3 > ref[~dead].abs().max()
        check(got[dead], ref[dead], what + "[gq; gk], zero-norm rows")
        check(got[~dead], ref[~dead], what + "[gq; gk], live rows")
    else:
        widened = (C, heads, HW, B, normalize) == ZERO_GRADIENT_CASE
        check(got, ref, what + "[gq; gk]", ZERO_GRADIENT_ATOL if widened else None)
    return outs


@gpu
@pytest.mark.parametrize("C,heads", TILINGS, ids=_ids(TILINGS))
def test_attn_channel_tilings(dev, C, heads):
    for normalize in (1, 0):
        outs = run_attn(dev, C, heads, TILING_HW, 2, normalize)
        t, _ = attn_case(C, heads, TILING_HW, 2, normalize)             # the typed entry point at fp32: the same kernels
        qkv, T, Wp = make_qkv(dev, t, "f32"), t["T"].to(dev), t["Wp"].to(dev)
        typed = twice(dev, lambda *o: k_attn_fwd(qkv, T, Wp, heads, normalize, o, typed=True), *fwd_specs(2, C, heads))
        for a, b in zip(outs, typed):
            assert torch.equal(a, b), "cidnet_attn_fwd_t at fp32 differs from cidnet_attn_fwd"


@gpu
def test_attn_three_samples(dev):
    for normalize in (1, 0):
        run_attn(dev, 36, 2, TILING_HW, 3, normalize)


@gpu
@pytest.mark.parametrize("HW", PIXELS)
def test_attn_pixel_counts(dev, HW):
    for normalize in (1, 0):
        run_attn(dev, 36, 2, HW, 1, normalize)


@gpu
@pytest.mark.parametrize("HW", PIXELS_TI2_CLAMPED)
def test_attn_large_pixel_counts_with_clamped_rows(dev, HW):
    for normalize in (1, 0):
        run_attn(dev, 34, 2, HW, 1, normalize)


@gpu
@pytest.mark.parametrize("C,heads", BF16_CH, ids=_ids(BF16_CH))
@pytest.mark.parametrize("HW", BF16_HW)
def test_attn_fwd_bf16_storage(dev, HW, C, heads):
    for normalize in (1, 0):
        run_attn(dev, C, heads, HW, 1, normalize, "bf16")


@gpu
def test_attn_zero_norm_rows(dev):
    d = DEAD
    run_attn(dev, d["C"], d["heads"], d["HW"], d["B"], 1, "dead")


@gpu
@pytest.mark.parametrize("C,heads", BAD_SHAPES, ids=_ids(BAD_SHAPES))
def test_attn_rejects_unsupported_shapes(dev, C, heads):
    """ch > 32 or heads not dividing C: CIDNET_ERR_SHAPE from both entry points, nothing written"""
    B, HW = 2, TILING_HW
    ch = -(-C // heads)
    g = _gen(42, C, heads)
    qkv = torch.randn(B, 3 * C, HW, generator=g).to(dev)
    T, Wp, dM = torch.ones(heads).to(dev), torch.randn(C, C, generator=g).to(dev), torch.randn(B, C, C, generator=g).to(dev)
    for normalize in (1, 0):
        outs = [torch.full(s, NAN, device=dev) for s in ((B, heads, ch, ch), (B, heads, ch, ch), (B, C), (B, C), (B, C, C))]
        with pytest.raises(RuntimeError, match="CIDNET_ERR_SHAPE"):
            k_attn_fwd(qkv, T, Wp, heads, normalize, outs)
        fed = [torch.rand(s, generator=g).to(dev) + 0.5 for s in ((B, heads, ch, ch), (B, heads, ch, ch), (B, C), (B, C))]
        bouts = [torch.full(s, NAN, device=dev) for s in ((B, C, C), (B, heads), (B, 2 * C, 2 * C))]
        with pytest.raises(RuntimeError, match="CIDNET_ERR_SHAPE"):
            k_attn_bwd(dM, Wp, *fed, T, heads, normalize, bouts)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs + bouts), "an output was written despite the error"


@gpu
def test_attn_rejects_a_short_workspace(dev):
    C, heads, HW, B = 36, 2, 520, 2
    t, _ = attn_case(C, heads, HW, 1, 1)
    qkv = make_qkv(dev, t, "f32").repeat(B, 1, 1)
    for kind in ("f32", "bf16"):
        x = qkv.to(torch.bfloat16) if kind == "bf16" else qkv
        outs = [torch.full(s, NAN, device=dev) for s, _ in fwd_specs(B, C, heads)]
        with pytest.raises(RuntimeError, match="CIDNET_ERR_WS"):
            k_attn_fwd(x, t["T"].to(dev), t["Wp"].to(dev), heads, 1, outs, short=1)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs), "an output was written despite the error"


# ---------------------------------------------------------------------------------------------------------------------
# CABResidualFn and NoiseCABResidualFn
# ---------------------------------------------------------------------------------------------------------------------
CAB_NAMES = ("x_res", "xn", "yn", "T", "wq", "wq_dw", "wkv", "wkv_dw", "wp")
NOISE_CAB_NAMES = ("x_res", "xn", "yn", "nm", "T", "wq", "wq_dw", "wkv", "wkv_dw", "w_scaler", "wp")


def ref_block(p, heads, noise):
    """x_res + project_out(attn @ v): q = dw3x3(conv1x1(xn)), k | v = dw3x3(conv1x1(yn)); the noise block skips the
    normalisation and multiplies v by sigmoid(conv1x1(noise_map))"""
    B, C, H, W = p["xn"].shape
    q = F.conv2d(F.conv2d(p["xn"], p["wq"]), p["wq_dw"], padding=1, groups=C)
    k, v = F.conv2d(F.conv2d(p["yn"], p["wkv"]), p["wkv_dw"], padding=1, groups=2 * C).chunk(2, 1)
    if noise:
        v = v * torch.sigmoid(F.conv2d(p["nm"], p["w_scaler"]))
    _, logit, attn = attn_math(q.flatten(2), k.flatten(2), p["T"].flatten(), heads, not noise)
    out = (attn @ v.reshape(B, heads, C // heads, H * W)).reshape(B, C, H, W)
    return p["x_res"] + F.conv2d(out, p["wp"]), logit


@functools.lru_cache(maxsize=None)
def block_case(shape, noise):
    """yn and the k half of the kv weights are mixtures with xn and the q weights, so the logits are not noise around 0"""
    B, C, heads, H, W = shape
    g = _gen(43, C, heads, H, W, noise)
    rn = lambda *s: torch.randn(*s, generator=g)
    s = (H * W) ** -0.5 if noise else 1.0
    xn = rn(B, C, H, W)
    wq, wq_dw = rn(C, C, 1, 1) / C ** 0.5, 0.4 * rn(C, 1, 3, 3)
    wkv, wkv_dw = rn(2 * C, C, 1, 1) / C ** 0.5, 0.4 * rn(2 * C, 1, 3, 3)
    wkv[:C] = 0.7 * wq + 0.7 * wkv[:C]
    wkv_dw[:C] = 0.7 * wq_dw + 0.7 * wkv_dw[:C]
    t = dict(x_res=rn(B, C, H, W), xn=xn, yn=0.7 * xn + 0.7 * rn(B, C, H, W),
             T=torch.tensor([T_CYCLE[h % len(T_CYCLE)] for h in range(heads)]).reshape(heads, 1, 1),
             wq=wq * s, wq_dw=wq_dw, wkv=wkv * s, wkv_dw=wkv_dw, wp=rn(C, C, 1, 1) / C ** 0.5)
    if noise:
        t["nm"], t["w_scaler"] = torch.rand(B, 1, H, W, generator=g), rn(C, 1, 1, 1)
    names = NOISE_CAB_NAMES if noise else CAB_NAMES
    up = rn(B, C, H, W)
    leaves = {n: t[n].double().requires_grad_(True) for n in names}
    out, logit = ref_block(leaves, heads, noise)
    grads = torch.autograd.grad(out, [leaves[n] for n in names], up.double())
    peak = logit.detach().abs().max().item()
    assert 0.5 <= peak <= 16, f"block {shape} noise={noise}: max|T S| = {peak:.3e}"
    assert all(bool(torch.isfinite(x).all()) for x in grads)
    return t, up, out.detach(), grads


def run_block(dev, shape, noise):
    heads = shape[2]
    names = NOISE_CAB_NAMES if noise else CAB_NAMES
    t, up, out_ref, grads_ref = block_case(shape, noise)
    fn = _ops().NoiseCABResidualFn if noise else _ops().CABResidualFn
    runs = []
    for _ in range(2):
        leaves = [t[n].to(dev).requires_grad_(True) for n in names]
        out = fn.apply(*leaves, heads)
        runs.append([out.detach()] + list(torch.autograd.grad(out, leaves, up.to(dev))))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    for o, r, n in zip(runs[0], [out_ref] + list(grads_ref), ("out",) + tuple("g_" + n for n in names)):
        check(o, r, f"{'Noise' if noise else ''}CABResidualFn {shape}: {n}")


@gpu
@pytest.mark.parametrize("shape", CAB_SHAPES, ids=_ids(CAB_SHAPES))
def test_cab_residual_fn(dev, shape):
    """output and the gradients of x_res, xn, yn, T, wq, wq_dw, wkv, wkv_dw, wp"""
    run_block(dev, shape, False)


@gpu
@pytest.mark.parametrize("shape", NOISE_CAB_SHAPES, ids=_ids(NOISE_CAB_SHAPES))
def test_noise_cab_residual_fn(dev, shape):
    """output and the gradients of x_res, xn, yn, noise_map, T, wq, wq_dw, wkv, wkv_dw, w_scaler, wp"""
    run_block(dev, shape, True)
