"""csrc/dw.hip against fp64: the depthwise 3x3 kernels (forward, flipped, weight gradient, fused backward) and the IEL gate
kernels (gate forward / backward, fused dwconv + gate forward, fused gate + dwconv1/2 backward), each compared with a plain
torch fp64 CPU evaluation of the same formula (autograd supplies the gradients; nothing of the project is on the reference
side), across the strip tilings pick_tiling takes.

Every case first asserts, through the host-only query cidnet_dw_tiling, the (rows, nstrips, chunks) it is there for, so a
retuned cost model fails the case instead of silently moving it to another tiling.  Every output is allocated NaN-filled,
must be finite after the call, and a second call into a fresh NaN-filled buffer must be bit-identical (fixed-order
reductions).  fp32 criterion: max|out - ref| <= 2e-5 * max|ref| + 1e-6 per output tensor (test_ops_gpu.close).

Tilings reached (family 0: dw3x3, iel_gate_fwd/bwd; 1: iel_dw_gate_fwd; 2: dw3x3_wgrad / dw3x3_bwd; 3: iel_gate_dw_bwd;
"last" = rows of the last strip, "=" an exact last strip, "-" a single strip; C = 2h):

  rows  family 0                    family 1                    family 2                      family 3
  1-3   H = 1, 2, 3 (-)             H = 1, 2, 3 (-)             H = 1, 2, 3 (-)               H = 1, 2, 3 (-)
  4     4x8 (-)                     4x8 (-)                     4x8 (-), 5x9 last 1,          4x8 (-), 5x9 last 1,
                                                                6x5 last 2, 7x7 last 3        6x5 last 2, 7x7 last 3
  5     5x9 (-), 9x85 last 4        5x9 (-), 9x85 last 4        9x85 last 4, 21x41 last 1     9x85 last 4, 21x41 last 1
  6     6x5 (-), 11x86 last 5       6x5 (-), 11x86 last 5       11x86 last 5, 113x10 last 5   11x86 last 5, 113x10 last 5
  7     7x7 (-), 13x87 last 6,      7x7 (-), 13x87 last 6,      13x87 last 6,                 13x87 last 6
        21x41 =                     21x41 =                     117x299 last 5 (chunks 2)
  8     15x88 last 7, 16x85 =,      15x88 last 7, 16x85 =,      15x88 last 7, 16x85 =,        15x88 last 7, 16x85 =,
        113x10 last 1,              113x10 last 1,              229x299 last 5 (chunks 3)     117x299 last 5 (chunks 2),
        117x299, 229x299 last 5     117x299, 229x299 last 5                                   229x299 last 5 (chunks 3)
  9     2x6554x58x37 last 4         2x3745x58x37 last 4         2x5462x50x37 last 5           2x2185x49x37 last 4
        (dw3x3 and the gate)                                                                  (row-loop exits 2 and 0)
  17    2x11469x68x37 = (dw3x3)     2x6554x68x37 =              2x6302x68x50 =                2x2521x68x50 = (exit 1)

(the tanh_fast case, 2x5x19x27, adds rows 7 last 5 to families 0 and 1 and rows 4 last 3 to family 3; chunks is 1 wherever
it is not given; the small shapes are HxW of (B, h, H, W) in SMALL, the tall ones BxCxHxW or BxhxHxW.)

The rows 9 and 17 cases are the smallest problems that reach those heights (one plane fewer and the query reports a shorter
strip); they hold 10 M to 60 M pixels per tensor, so the fp64 reference covers five channels only (see _subset).
"""
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ops_gpu import close  # noqa: E402

gpu = pytest.mark.gpu          # the two tests that only read the case tables through the host-side query carry no mark

NAN = float("nan")
F32, BF16 = 0, 1


# ---------------------------------------------------------------------------------------------------------------------
# reference: plain torch, fp64, CPU
# ---------------------------------------------------------------------------------------------------------------------
def ref_dw(x, w, addend=None, flip=False):
    conv = F.conv_transpose2d if flip else F.conv2d
    y = conv(x, w, padding=1, groups=x.shape[1])
    return y if addend is None else y + addend


def ref_dw_wgrad(x, gout):
    C = x.shape[1]
    return torch.nn.grad.conv2d_weight(x, (C, 1, 3, 3), gout, padding=1, groups=C)


def ref_gate(w1, w2, dg, u=None, pin=None, w_dw=None):
    """g = (tanh(a1) + u1) * (tanh(a2) + u2), a_i = dw_i(u_i), [u1; u2] = u (or dw(pin) when pin is given), and its
    gradients for the output gradient dg: du, gw1, gw2 through the whole formula; da_i, ds_i at a_i and at the `+ u_i`
    branch, with a_i and a detached copy of u_i as separate leaves"""
    h = w1.shape[0]
    out = {}
    if pin is not None:
        u = F.conv2d(pin, w_dw, padding=1, groups=2 * h)
        out["u"] = u
    ur = u.detach().clone().requires_grad_(True)
    w1r, w2r = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    a1 = F.conv2d(ur[:, :h], w1r, padding=1, groups=h)
    a2 = F.conv2d(ur[:, h:], w2r, padding=1, groups=h)
    g = (torch.tanh(a1) + ur[:, :h]) * (torch.tanh(a2) + ur[:, h:])
    g.backward(dg)
    out.update(g=g.detach(), du=ur.grad, gw1=w1r.grad, gw2=w2r.grad, a=torch.cat([a1, a2], 1).detach())
    al = [a.detach().clone().requires_grad_(True) for a in (a1, a2)]
    sl = [u[:, :h].detach().clone().requires_grad_(True), u[:, h:].detach().clone().requires_grad_(True)]
    ((torch.tanh(al[0]) + sl[0]) * (torch.tanh(al[1]) + sl[1])).backward(dg)
    out.update(da=torch.cat([a.grad for a in al], 1), ds=torch.cat([s.grad for s in sl], 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the raw ABI
# ---------------------------------------------------------------------------------------------------------------------
def tiling(family, planes, H, W):
    from hvi_cidnet_amd._lib import lib
    r, n, c = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib().raw("cidnet_dw_tiling")(family, planes, H, W, ctypes.byref(r), ctypes.byref(n), ctypes.byref(c)) == 0
    return r.value, n.value, c.value


def twice(dev, call, *specs):
    """run `call` on fresh NaN-filled outputs (shape, dtype) twice: finite everywhere, bit-identical between the runs"""
    runs = []
    for _ in range(2):
        bufs = [torch.full(shape, NAN, device=dev, dtype=dt) for shape, dt in specs]
        call(*bufs)
        runs.append(bufs)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()), "elements left unwritten or not finite"
        assert torch.equal(a, b), "two runs differ"
    return runs[0]


def _dtc(t):
    return BF16 if t.dtype == torch.bfloat16 else F32


def k_dw3x3(x, w1, w2, csplit, addend, out, flip):
    from hvi_cidnet_amd import ops
    B, C, H, W = x.shape
    if x.dtype == torch.float32:
        ops.lib().call("cidnet_dw3x3", ops._p(x), ops._p(w1), ops._p(w2), csplit, ops._p(addend), ops._p(out), flip, B, C, H, W,
                       ops._stream())
    else:
        ops.lib().call("cidnet_dw3x3_t", ops._p(x), ops._p(w1), ops._p(w2), csplit, ops._p(addend), ops._p(out), _dtc(x), flip,
                       B, C, H, W, ops._stream())


def _wgrad_ws(x):
    from hvi_cidnet_amd import ops
    n = ops._raw("cidnet_dw3x3_wgrad_ws_floats", *x.shape)
    return torch.full((max(n, 1),), NAN, device=x.device), n


def k_dw3x3_wgrad(x, gout, gw1, gw2, csplit):
    from hvi_cidnet_amd import ops
    ws, n = _wgrad_ws(x)
    ops.lib().call("cidnet_dw3x3_wgrad", ops._p(x), ops._p(gout), ops._p(gw1), ops._p(gw2), csplit, ops._p(ws), n, *x.shape,
                   ops._stream())


def k_dw3x3_bwd(x, gout, w1, w2, csplit, addend, gin, gw1, gw2):
    from hvi_cidnet_amd import ops
    ws, n = _wgrad_ws(x)
    if x.dtype == torch.float32:
        ops.lib().call("cidnet_dw3x3_bwd", ops._p(x), ops._p(gout), ops._p(w1), ops._p(w2), csplit, ops._p(addend), ops._p(gin),
                       ops._p(gw1), ops._p(gw2), ops._p(ws), n, *x.shape, ops._stream())
    else:
        ops.lib().call("cidnet_dw3x3_bwd_t", ops._p(x), ops._p(gout), ops._p(w1), ops._p(w2), csplit, ops._p(addend), ops._p(gin),
                       _dtc(x), ops._p(gw1), ops._p(gw2), ops._p(ws), n, *x.shape, ops._stream())


def k_gate_fwd(u, w1, w2, g):
    from hvi_cidnet_amd import ops
    B, h, H, W = g.shape
    ops.lib().call("cidnet_iel_gate_fwd", ops._p(u), ops._p(w1), ops._p(w2), ops._p(g), B, h, H, W, ops._stream())


def k_gate_bwd(u, w1, w2, dg, da, ds):
    from hvi_cidnet_amd import ops
    B, h, H, W = dg.shape
    ops.lib().call("cidnet_iel_gate_bwd", ops._p(u), ops._p(w1), ops._p(w2), ops._p(dg), ops._p(da), ops._p(ds), B, h, H, W,
                   ops._stream())


def k_dw_gate_fwd(pin, w_dw, w1, w2, u, g):
    from hvi_cidnet_amd import ops
    B, h, H, W = g.shape
    if pin.dtype == torch.float32:
        ops.lib().call("cidnet_iel_dw_gate_fwd", ops._p(pin), ops._p(w_dw), ops._p(w1), ops._p(w2), ops._p(u), ops._p(g), B, h, H, W,
                       ops._stream())
    else:
        ops.lib().call("cidnet_iel_dw_gate_fwd_t", ops._p(pin), ops._p(w_dw), ops._p(w1), ops._p(w2), ops._p(u), ops._p(g),
                       _dtc(pin), B, h, H, W, ops._stream())


def k_gate_dw_bwd(u, w1, w2, dg, du, gw1, gw2):
    from hvi_cidnet_amd import ops
    B, h, H, W = dg.shape
    n = ops._raw("cidnet_iel_gate_dw_bwd_ws_floats", B, h, H, W)
    ws = torch.full((max(n, 1),), NAN, device=u.device)
    if u.dtype == torch.float32:
        ops.lib().call("cidnet_iel_gate_dw_bwd", ops._p(u), ops._p(w1), ops._p(w2), ops._p(dg), ops._p(du), ops._p(gw1),
                       ops._p(gw2), ops._p(ws), n, B, h, H, W, ops._stream())
    else:
        ops.lib().call("cidnet_iel_gate_dw_bwd_t", ops._p(u), ops._p(w1), ops._p(w2), ops._p(dg), ops._p(du), _dtc(u), ops._p(gw1),
                       ops._p(gw2), ops._p(ws), n, B, h, H, W, ops._stream())


def close_bf16(out, ref, what):
    """a bf16-stored output of fp32 arithmetic, per element: one bf16 ulp of the reference (round to nearest, plus an fp32
    error that crosses a rounding boundary) on top of the fp32 criterion"""
    assert out.dtype == torch.bfloat16
    o, r = out.detach().cpu().double(), ref.double()
    excess = ((o - r).abs() - (2.0 ** -8 * r.abs() + 2e-5 * r.abs().max().item() + 1e-6)).max().item()
    assert excess <= 0, f"{what}: an element is {excess:.3e} past one bf16 ulp + the fp32 criterion"


# ---------------------------------------------------------------------------------------------------------------------
# small cases.  (B, h, H, W) -> the tilings of families 0..3 (planes B*2h, B*h, B*2h, B*h); below the lane thresholds
# the tiling depends on H and W only, so the depthwise kernels (C = 2h) and the gate kernels share a family-0 entry.
# ---------------------------------------------------------------------------------------------------------------------
SMALL = {
    (2, 3, 1, 9):      ((1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1)),        # H < 4: one strip shorter than the minimum
    (2, 1, 2, 3):      ((2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1)),        # W < 8: the NARROW instantiation
    (2, 3, 3, 11):     ((3, 1, 1), (3, 1, 1), (3, 1, 1), (3, 1, 1)),
    (2, 3, 2, 1):      ((2, 1, 1), (2, 1, 1), (2, 1, 1), (2, 1, 1)),
    (2, 1, 3, 2):      ((3, 1, 1), (3, 1, 1), (3, 1, 1), (3, 1, 1)),
    (2, 3, 6, 5):      ((6, 1, 1), (6, 1, 1), (4, 2, 1), (4, 2, 1)),
    (2, 1, 7, 7):      ((7, 1, 1), (7, 1, 1), (4, 2, 1), (4, 2, 1)),
    (3, 95, 4, 8):     ((4, 1, 1), (4, 1, 1), (4, 1, 1), (4, 1, 1)),        # the narrowest fast-path width
    (2, 95, 5, 9):     ((5, 1, 1), (5, 1, 1), (4, 2, 1), (4, 2, 1)),        # families 2, 3: a last strip of one row
    (2, 3, 9, 85):     ((5, 2, 1), (5, 2, 1), (5, 2, 1), (5, 2, 1)),        # W % 4 = 1, 2, 3 at W >= 8: the last lane of a row
    (2, 3, 11, 86):    ((6, 2, 1), (6, 2, 1), (6, 2, 1), (6, 2, 1)),        # is pulled back over 3, 2, 1 pixels of its neighbour
    (2, 3, 13, 87):    ((7, 2, 1), (7, 2, 1), (7, 2, 1), (7, 2, 1)),
    (2, 1, 15, 88):    ((8, 2, 1), (8, 2, 1), (8, 2, 1), (8, 2, 1)),
    (2, 1, 16, 85):    ((8, 2, 1), (8, 2, 1), (8, 2, 1), (8, 2, 1)),        # exact last strip
    (2, 3, 21, 41):    ((7, 3, 1), (7, 3, 1), (5, 5, 1), (5, 5, 1)),        # families 2, 3: one-row last strip at rows 5
    (2, 1, 113, 10):   ((8, 15, 1), (8, 15, 1), (6, 19, 1), (6, 19, 1)),    # families 0, 1: a last strip of one row
    (2, 1, 117, 299):  ((8, 15, 1), (8, 15, 1), (7, 17, 2), (8, 15, 2)),    # two blocks per plane, the second partly filled
    (2, 1, 229, 299):  ((8, 29, 1), (8, 29, 1), (8, 29, 3), (8, 29, 3)),    # three blocks per plane: 2175 items, 127 in the last
}
SMALL_IDS = ["x".join(map(str, s)) for s in SMALL]
BF16_CASES = [(2, 1, 7, 7), (2, 95, 5, 9), (2, 3, 13, 87), (2, 1, 117, 299)]


def assert_tiling(shape, family, planes_per_sample=None):
    """planes: B*C = B*2h for the depthwise kernels (families 0, 2), B*h for the gate kernels (0, 1, 3)"""
    B, h, H, W = shape
    planes = B * (planes_per_sample or (2 * h if family in (0, 2) else h))
    got = tiling(family, planes, H, W)
    assert got == SMALL[shape][family], f"family {family} takes (rows, nstrips, chunks) = {got} at {shape}, not {SMALL[shape][family]}"
    rows, nstrips, _ = got
    assert rows * nstrips >= H > rows * (nstrips - 1)
    return got


def test_small_cases_reach_what_the_table_claims():
    """the case list, read through the query: every family sees every strip height 4..8, H in {1, 2, 3}, a ragged last
    strip including one of a single row, and families 2 and 3 two and three blocks per plane"""
    for family in range(4):
        rows_seen, last_seen, chunks_seen = set(), set(), set()
        for shape in SMALL:
            rows, nstrips, chunks = assert_tiling(shape, family)
            H = shape[2]
            rows_seen.add(rows)
            chunks_seen.add(chunks)
            if nstrips > 1 and H % rows:
                last_seen.add(H % rows)
        assert rows_seen >= set(range(1, 9)), (family, rows_seen)
        assert 1 in last_seen and len(last_seen) >= 3, (family, last_seen)
        assert chunks_seen >= ({1, 2, 3} if family >= 2 else {1}), (family, chunks_seen)
    widths = {s[3] for s in SMALL}
    assert widths >= {1, 2, 3, 5, 7} and {w % 4 for w in widths if w >= 8} == {0, 1, 2, 3}
    assert {s[1] for s in SMALL} == {1, 3, 95} and all(s[0] > 1 for s in SMALL)


@functools.lru_cache(maxsize=None)
def small_inputs(shape, bf16=False):
    """seeded fp32 CPU inputs of a case (rounded to bf16 first in the bf16 cases): x serves as `in`, u and pin"""
    B, h, H, W = shape
    g = torch.Generator().manual_seed(1000 * H + W + (7 if bf16 else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(x=1.5 * r(B, 2 * h, H, W), gout=r(B, 2 * h, H, W), addend=r(B, 2 * h, H, W), dg=r(B, h, H, W),
             w=0.4 * r(2 * h, 1, 3, 3), w1=0.5 * r(h, 1, 3, 3), w2=0.5 * r(h, 1, 3, 3))
    if bf16:
        for k in ("x", "gout", "addend", "dg"):
            t[k] = t[k].to(torch.bfloat16).float()
    return t


@functools.lru_cache(maxsize=None)
def small_refs(shape, bf16=False):
    """every fp64 reference of a case, computed once and shared by its tests"""
    t = {k: v.double() for k, v in small_inputs(shape, bf16).items()}
    x, w = t["x"], t["w"]
    r = dict(fwd=ref_dw(x, w), flip_add=ref_dw(x, w, t["addend"], flip=True), gw=ref_dw_wgrad(x, t["gout"]),
             gin=ref_dw(t["gout"], w, flip=True), gin_add=ref_dw(t["gout"], w, t["addend"], flip=True))
    r["gate"] = ref_gate(t["w1"], t["w2"], t["dg"], u=x)
    r["dw_gate"] = ref_gate(t["w1"], t["w2"], t["dg"], pin=x, w_dw=w)
    return r


def on(dev, t, bf16=False):
    return {k: v.to(dev).to(torch.bfloat16 if bf16 and k in ("x", "gout", "addend", "dg") else torch.float32) for k, v in t.items()}


def check(out, ref, what):
    (close_bf16 if out.dtype == torch.bfloat16 else close)(out, ref, what=what)


def run_dw3x3_fwd(dev, shape, bf16):
    B, h, H, W = shape
    C = 2 * h
    d, r = on(dev, small_inputs(shape, bf16), bf16), small_refs(shape, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    spec = ((B, C, H, W), dt)
    cs = max(1, C // 3)
    w1, w2 = d["w"][:cs].contiguous(), d["w"][cs:].contiguous()
    y, = twice(dev, lambda o: k_dw3x3(d["x"], d["w"], None, C, None, o, 0), spec)
    check(y, r["fwd"], "plain")
    y, = twice(dev, lambda o: k_dw3x3(d["x"], d["w"], None, C, d["addend"], o, 1), spec)
    check(y, r["flip_add"], "flip + addend")
    y, = twice(dev, lambda o: k_dw3x3(d["x"], w1, w2, cs, None, o, 0), spec)
    check(y, r["fwd"], "csplit inside C")
    y, = twice(dev, lambda o: k_dw3x3(d["x"], d["w"], None, C + 5, None, o, 0), spec)
    check(y, r["fwd"], "csplit beyond C, w2 NULL")


def run_dw3x3_bwd(dev, shape, bf16):
    B, h, H, W = shape
    C = 2 * h
    d, r = on(dev, small_inputs(shape, bf16), bf16), small_refs(shape, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    cs = max(1, C // 3)
    w1, w2 = d["w"][:cs].contiguous(), d["w"][cs:].contiguous()
    gin, gw = twice(dev, lambda o, g: k_dw3x3_bwd(d["x"], d["gout"], d["w"], None, C, None, o, g, None),
                    ((B, C, H, W), dt), ((C, 1, 3, 3), torch.float32))
    check(gin, r["gin"], "bwd gin")
    close(gw, r["gw"], what="bwd gw")
    gin, g1, g2 = twice(dev, lambda o, a, b: k_dw3x3_bwd(d["x"], d["gout"], w1, w2, cs, d["addend"], o, a, b),
                        ((B, C, H, W), dt), ((cs, 1, 3, 3), torch.float32), ((C - cs, 1, 3, 3), torch.float32))
    check(gin, r["gin_add"], "bwd gin + addend")
    close(torch.cat([g1, g2]), r["gw"], what="bwd gw, csplit inside C")


@gpu
@pytest.mark.parametrize("shape", list(SMALL), ids=SMALL_IDS)
def test_dw3x3_forward(dev, shape):
    """cidnet_dw3x3: plain, flip = 1 with an addend, csplit strictly inside C, csplit >= C with a NULL w2"""
    assert_tiling(shape, 0)
    run_dw3x3_fwd(dev, shape, False)


@gpu
@pytest.mark.parametrize("shape", list(SMALL), ids=SMALL_IDS)
def test_dw3x3_wgrad_and_fused_backward(dev, shape):
    """cidnet_dw3x3_wgrad and cidnet_dw3x3_bwd (without / with an addend): the weight gradients must not count the pixels a
    pulled-back last lane shares with its neighbour twice, and must sum every block of a plane and every sample"""
    B, h, H, W = shape
    C = 2 * h
    assert_tiling(shape, 2)
    d, r = on(dev, small_inputs(shape)), small_refs(shape)
    cs = max(1, C // 3)
    g1, g2 = twice(dev, lambda a, b: k_dw3x3_wgrad(d["x"], d["gout"], a, b, cs), ((cs, 1, 3, 3), torch.float32),
                   ((C - cs, 1, 3, 3), torch.float32))
    close(torch.cat([g1, g2]), r["gw"], what="wgrad")
    gw, = twice(dev, lambda a: k_dw3x3_wgrad(d["x"], d["gout"], a, None, C), ((C, 1, 3, 3), torch.float32))
    close(gw, r["gw"], what="wgrad, gw2 NULL")
    run_dw3x3_bwd(dev, shape, False)


def run_gate_fwd_bwd(dev, d, r, shape):
    B, h, H, W = shape
    g, = twice(dev, lambda o: k_gate_fwd(d["x"], d["w1"], d["w2"], o), ((B, h, H, W), torch.float32))
    close(g, r["g"], what="gate fwd")
    da, ds = twice(dev, lambda a, s: k_gate_bwd(d["x"], d["w1"], d["w2"], d["dg"], a, s), ((B, 2 * h, H, W), torch.float32),
                   ((B, 2 * h, H, W), torch.float32))
    close(da, r["da"], what="gate bwd da")
    close(ds, r["ds"], what="gate bwd ds")
    return g, da, ds


@gpu
@pytest.mark.parametrize("shape", list(SMALL), ids=SMALL_IDS)
def test_iel_gate_fwd_and_bwd(dev, shape):
    """cidnet_iel_gate_fwd / cidnet_iel_gate_bwd against (tanh(dw1(u1)) + u1) * (tanh(dw2(u2)) + u2) and its gradients at
    a_i and at the `+ u_i` branch"""
    assert_tiling(shape, 0, shape[1])
    run_gate_fwd_bwd(dev, on(dev, small_inputs(shape)), small_refs(shape)["gate"], shape)


def run_dw_gate_fwd(dev, d, r, shape, bf16=False):
    B, h, H, W = shape
    dt = torch.bfloat16 if bf16 else torch.float32
    u, g = twice(dev, lambda a, b: k_dw_gate_fwd(d["x"], d["w"], d["w1"], d["w2"], a, b), ((B, 2 * h, H, W), dt), ((B, h, H, W), dt))
    check(u, r["u"], "dw+gate u")
    check(g, r["g"], "dw+gate g")
    g0, = twice(dev, lambda b: k_dw_gate_fwd(d["x"], d["w"], d["w1"], d["w2"], None, b), ((B, h, H, W), dt))
    check(g0, r["g"], "dw+gate g, u NULL")
    assert torch.equal(g0, g)
    return u, g


@gpu
@pytest.mark.parametrize("shape", list(SMALL), ids=SMALL_IDS)
def test_iel_dw_gate_fwd(dev, shape):
    """cidnet_iel_dw_gate_fwd with u written and with u NULL (the same g either way)"""
    assert_tiling(shape, 1)
    run_dw_gate_fwd(dev, on(dev, small_inputs(shape)), small_refs(shape)["dw_gate"], shape)


def run_gate_dw_bwd(dev, d, r, shape, bf16=False):
    B, h, H, W = shape
    dt = torch.bfloat16 if bf16 else torch.float32
    du, g1, g2 = twice(dev, lambda a, b, c: k_gate_dw_bwd(d["x"], d["w1"], d["w2"], d["dg"], a, b, c), ((B, 2 * h, H, W), dt),
                       ((h, 1, 3, 3), torch.float32), ((h, 1, 3, 3), torch.float32))
    check(du, r["du"], "gate+dw bwd du")
    close(g1, r["gw1"], what="gate+dw bwd gw1")
    close(g2, r["gw2"], what="gate+dw bwd gw2")
    return du, g1, g2


@gpu
@pytest.mark.parametrize("shape", list(SMALL), ids=SMALL_IDS)
def test_iel_gate_dw_bwd(dev, shape):
    """cidnet_iel_gate_dw_bwd: du through the gate and both depthwise convs, and their weight gradients summed over the
    strips, the blocks of a plane and the batch"""
    assert_tiling(shape, 3)
    run_gate_dw_bwd(dev, on(dev, small_inputs(shape)), small_refs(shape)["gate"], shape)


@gpu
@pytest.mark.parametrize("shape", BF16_CASES, ids=["x".join(map(str, s)) for s in BF16_CASES])
def test_bf16_typed_entry_points(dev, shape):
    """cidnet_dw3x3_t, cidnet_dw3x3_bwd_t, cidnet_iel_dw_gate_fwd_t and cidnet_iel_gate_dw_bwd_t with dt = CIDNET_BF16: the
    fp64 reference runs on the bf16-rounded inputs; the kernels compute in fp32 and round once on store, so every stored
    element lies within 2**-8 * |ref| + the fp32 criterion of it, and the fp32 weight gradients keep the fp32 criterion"""
    for family in range(4):
        assert_tiling(shape, family)
    d, r = on(dev, small_inputs(shape, True), True), small_refs(shape, True)
    assert d["x"].dtype == torch.bfloat16
    run_dw3x3_fwd(dev, shape, True)
    run_dw3x3_bwd(dev, shape, True)
    run_dw_gate_fwd(dev, d, r["dw_gate"], shape, True)
    run_gate_dw_bwd(dev, d, r["gate"], shape, True)


# ---------------------------------------------------------------------------------------------------------------------
# tanh_fast regimes
# ---------------------------------------------------------------------------------------------------------------------
TANH_SHAPE = (2, 5, 19, 27)
TANH_NORMS = (0.05, 0.2, 2.5, 60.0)          # 2-norm of a channel's taps = standard deviation of its pre-activation


@functools.lru_cache(maxsize=None)
def tanh_case():
    """u ~ N(0, 1) with a block of exact zeros; channel c < 4 of both gate convolutions has taps of 2-norm TANH_NORMS[c],
    so its pre-activations are N(0, norm^2): inside the Taylor branch, around the 0.2 switch, 1..5, and saturated beyond
    20 (exp2 overflows to inf at |a| > 44).  Channel 4: dw1 all zero (a1 = 0 exactly), dw2 ordinary.  The depthwise conv
    of the fused forward is the identity tap, so its u equals pin bit for bit and it sees the same pre-activations."""
    B, h, H, W = TANH_SHAPE
    g = torch.Generator().manual_seed(20)
    x = torch.randn(B, 2 * h, H, W, generator=g)
    x[:, :, 4:10, 5:12] = 0.0
    ws = []
    for _ in range(2):
        w = torch.randn(h, 1, 3, 3, generator=g)
        for c, n in enumerate(TANH_NORMS):
            w[c] *= n / w[c].norm()
        ws.append(w)
    ws[0][4] = 0.0
    ws[1][4] *= 0.3
    ident = torch.zeros(2 * h, 1, 3, 3)
    ident[:, 0, 1, 1] = 1.0
    t = dict(x=x, dg=torch.randn(B, h, H, W, generator=g), w=ident, w1=ws[0], w2=ws[1])
    t64 = {k: v.double() for k, v in t.items()}
    r = ref_gate(t64["w1"], t64["w2"], t64["dg"], u=t64["x"])
    r["u"] = t64["x"]
    return t, r


def test_tanh_regimes_are_populated():
    """on the reference side: each regime of tanh_fast holds at least 5 % of the pre-activations, and exact zeros occur"""
    _, r = tanh_case()
    a = r["a"].abs()
    frac = lambda m: m.double().mean().item()
    assert frac(a < 0.2) >= 0.05 and frac((a > 0) & (a < 0.2)) >= 0.05
    assert frac((a >= 0.1) & (a <= 0.3)) >= 0.05
    assert frac((a >= 0.15) & (a < 0.2)) > 0 and frac((a >= 0.2) & (a <= 0.25)) > 0      # both sides of the switch
    assert frac((a >= 1) & (a <= 5)) >= 0.05
    assert frac(a > 20) >= 0.05 and frac(a > 45) > 0
    assert frac(a == 0) >= 0.05


@gpu
def test_tanh_fast_regimes(dev):
    """forward and backward of the four gate kernels with pre-activations in every regime of tanh_fast: the Taylor branch,
    the switch at 0.2, 1..5 where 1 - t*t cancels, saturation with exp2 at inf, and exact zeros.  The fp32 criterion, per
    output tensor as everywhere, and also per channel pair: each channel is one regime, and the saturated channels would
    otherwise set the scale for the small ones"""
    B, h, H, W = TANH_SHAPE
    for family, planes in ((0, B * h), (1, B * h), (3, B * h)):
        rows, nstrips, _ = tiling(family, planes, H, W)
        assert nstrips > 1 and rows * nstrips >= H > rows * (nstrips - 1)
    t, r = tanh_case()
    d = on(dev, t)
    g, da, ds = run_gate_fwd_bwd(dev, d, r, TANH_SHAPE)
    _, g_fused = run_dw_gate_fwd(dev, d, r, TANH_SHAPE)
    du, g1, g2 = run_gate_dw_bwd(dev, d, r, TANH_SHAPE)
    for c in range(h):
        pair = [c, h + c]
        close(g[:, c], r["g"][:, c], what=f"g, channel {c}")
        close(g_fused[:, c], r["g"][:, c], what=f"fused g, channel {c}")
        close(da[:, pair], r["da"][:, pair], what=f"da, channels {pair}")
        close(ds[:, pair], r["ds"][:, pair], what=f"ds, channels {pair}")
        close(du[:, pair], r["du"][:, pair], what=f"du, channels {pair}")
        close(torch.stack([g1[c], g2[c]]), torch.stack([r["gw1"][c], r["gw2"][c]]), what=f"gw, channel {c}")


# ---------------------------------------------------------------------------------------------------------------------
# tall strips: the smallest problems whose lane count lets pick_tiling go above 8 rows
# ---------------------------------------------------------------------------------------------------------------------
def _subset(n):
    """The channels the fp64 reference covers in a tall-strip case: the first, the last and three in between, all samples,
    full planes (so every strip boundary of those planes is compared).  A cost measure: the planes of a launch differ only
    in their base pointer; all other planes are checked for finiteness and run-to-run equality."""
    return sorted({0, n // 4, n // 2 + 1, (3 * n) // 4, n - 1})


def _randn(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return lambda *s: torch.randn(*s, device=dev, generator=g)


def _tall_inputs(dev, seed, B, h, H, W):
    r = _randn(dev, seed)
    return dict(x=1.5 * r(B, 2 * h, H, W), dg=r(B, h, H, W), w=0.4 * r(2 * h, 1, 3, 3), w1=0.5 * r(h, 1, 3, 3), w2=0.5 * r(h, 1, 3, 3))


def _tall_tiling(family, planes, H, W, expect, band):
    got = tiling(family, planes, H, W)
    assert got == expect and band[0] <= got[0] <= band[1], (got, expect)
    assert tiling(family, planes - 2, H, W)[0] < got[0], "not the smallest problem that reaches this strip height"
    return got


def _c64(t, idx=None):
    return (t if idx is None else t[:, idx]).cpu().double()


@gpu
@pytest.mark.parametrize("B,C,H,W,expect,band", [(2, 6554, 58, 37, (9, 7, 1), (9, 16)), (2, 11469, 68, 37, (17, 4, 1), (17, 24))],
                         ids=["rows9-last4", "rows17-exact"])
def test_tall_strips_dw3x3(dev, B, C, H, W, expect, band):
    """family 0 above 8 rows: cidnet_dw3x3 with csplit inside C; fp64 on the channels of _subset"""
    _tall_tiling(0, B * C, H, W, expect, band)
    r = _randn(dev, 31)
    x, w = 1.5 * r(B, C, H, W), 0.4 * r(C, 1, 3, 3)
    cs = C // 3
    w1, w2 = w[:cs].contiguous(), w[cs:].contiguous()
    y, = twice(dev, lambda o: k_dw3x3(x, w1, w2, cs, None, o, 0), ((B, C, H, W), torch.float32))
    idx = _subset(C)
    close(y[:, idx], ref_dw(_c64(x, idx), w[idx].cpu().double()), what="tall dw3x3")


@gpu
def test_tall_strips_gate_fwd_bwd(dev):
    """family 0 above 8 rows through iel_gate_kernel: 9-row strips with a last strip of 4"""
    B, h, H, W = 2, 6554, 58, 37
    _tall_tiling(0, B * h, H, W, (9, 7, 1), (9, 16))
    t = _tall_inputs(dev, 32, B, h, H, W)
    idx = _subset(h)
    pair = idx + [h + c for c in idx]
    r = ref_gate(t["w1"][idx].cpu().double(), t["w2"][idx].cpu().double(), _c64(t["dg"], idx), u=_c64(t["x"], pair))
    g, = twice(dev, lambda o: k_gate_fwd(t["x"], t["w1"], t["w2"], o), ((B, h, H, W), torch.float32))
    close(g[:, idx], r["g"], what="tall gate fwd")
    del g
    da, ds = twice(dev, lambda a, s: k_gate_bwd(t["x"], t["w1"], t["w2"], t["dg"], a, s), ((B, 2 * h, H, W), torch.float32),
                   ((B, 2 * h, H, W), torch.float32))
    close(da[:, pair], r["da"], what="tall gate bwd da")
    close(ds[:, pair], r["ds"], what="tall gate bwd ds")


@gpu
@pytest.mark.parametrize("B,h,H,W,expect,band", [(2, 3745, 58, 37, (9, 7, 1), (9, 16)), (2, 6554, 68, 37, (17, 4, 1), (17, 24))],
                         ids=["rows9-last4", "rows17-exact"])
def test_tall_strips_dw_gate_fwd(dev, B, h, H, W, expect, band):
    """family 1 above 8 rows: the rolling three-slot windows and the row loop unrolled by three, halo rows of u recomputed
    across each strip boundary"""
    _tall_tiling(1, B * h, H, W, expect, band)
    t = _tall_inputs(dev, 33, B, h, H, W)
    idx = _subset(h)
    pair = idx + [h + c for c in idx]
    r = ref_gate(t["w1"][idx].cpu().double(), t["w2"][idx].cpu().double(), _c64(t["dg"], idx), pin=_c64(t["x"], pair),
                 w_dw=t["w"][pair].cpu().double())
    u, g = twice(dev, lambda a, b: k_dw_gate_fwd(t["x"], t["w"], t["w1"], t["w2"], a, b), ((B, 2 * h, H, W), torch.float32),
                 ((B, h, H, W), torch.float32))
    close(u[:, pair], r["u"], what="tall dw+gate u")
    close(g[:, idx], r["g"], what="tall dw+gate g")


@gpu
@pytest.mark.parametrize("B,C,H,W,expect,band", [(2, 5462, 50, 37, (9, 6, 1), (9, 16)), (2, 6302, 68, 50, (17, 4, 1), (17, 24))],
                         ids=["rows9-last5", "rows17-exact"])
def test_tall_strips_dw3x3_wgrad_bwd(dev, B, C, H, W, expect, band):
    """family 2 above 8 rows: cidnet_dw3x3_wgrad and cidnet_dw3x3_bwd; a channel's weight gradient sums B planes"""
    _tall_tiling(2, B * C, H, W, expect, band)
    r = _randn(dev, 34)
    x, gout, w = 1.5 * r(B, C, H, W), r(B, C, H, W), 0.4 * r(C, 1, 3, 3)
    cs = C // 3
    w1, w2 = w[:cs].contiguous(), w[cs:].contiguous()
    idx = _subset(C)
    x64, g64, w64 = _c64(x, idx), _c64(gout, idx), w[idx].cpu().double()
    gw_ref = ref_dw_wgrad(x64, g64)
    g1, g2 = twice(dev, lambda a, b: k_dw3x3_wgrad(x, gout, a, b, cs), ((cs, 1, 3, 3), torch.float32), ((C - cs, 1, 3, 3), torch.float32))
    close(torch.cat([g1, g2])[idx], gw_ref, what="tall wgrad")
    gin, g1, g2 = twice(dev, lambda o, a, b: k_dw3x3_bwd(x, gout, w1, w2, cs, None, o, a, b), ((B, C, H, W), torch.float32),
                        ((cs, 1, 3, 3), torch.float32), ((C - cs, 1, 3, 3), torch.float32))
    close(gin[:, idx], ref_dw(g64, w64, flip=True), what="tall bwd gin")
    close(torch.cat([g1, g2])[idx], gw_ref, what="tall bwd gw")


@gpu
@pytest.mark.parametrize("B,h,H,W,expect,band", [(2, 2185, 49, 37, (9, 6, 1), (9, 16)), (2, 2521, 68, 50, (17, 4, 1), (17, 24))],
                         ids=["rows9-last4", "rows17-exact"])
def test_tall_strips_gate_dw_bwd(dev, B, h, H, W, expect, band):
    """family 3 above 8 rows.  The row loop is unrolled by three and leaves through one of three exits according to
    (strip rows + 2) % 3: the 9-row strips take exit 2 and their 4-row last strip exit 0, the 17-row strips exit 1"""
    rows, nstrips, _ = _tall_tiling(3, B * h, H, W, expect, band)
    exits = {(rows + 2) % 3, (H - (nstrips - 1) * rows + 2) % 3}
    assert exits == ({0, 2} if rows == 9 else {1}), exits
    t = _tall_inputs(dev, 36, B, h, H, W)
    idx = _subset(h)
    pair = idx + [h + c for c in idx]
    r = ref_gate(t["w1"][idx].cpu().double(), t["w2"][idx].cpu().double(), _c64(t["dg"], idx), u=_c64(t["x"], pair))
    du, g1, g2 = twice(dev, lambda a, b, c: k_gate_dw_bwd(t["x"], t["w1"], t["w2"], t["dg"], a, b, c), ((B, 2 * h, H, W), torch.float32),
                       ((h, 1, 3, 3), torch.float32), ((h, 1, 3, 3), torch.float32))
    close(du[:, pair], r["du"], what="tall gate+dw bwd du")
    close(g1[idx], r["gw1"], what="tall gate+dw bwd gw1")
    close(g2[idx], r["gw2"], what="tall gate+dw bwd gw2")
