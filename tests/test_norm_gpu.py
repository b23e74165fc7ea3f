"""The channels-first LayerNorm kernels (csrc/norm.hip) against fp64 on every dispatch path.  References, the case table, the
restatement of the launcher's dispatch and the criteria live in tests/norm_ref.py; tests/test_norm_cpu.py checks on the host that
the table reaches every kernel instantiation and every boundary named below, so this file only has to run the table.

Every case goes through the C ABI with raw pointers.  All outputs (y, y2, mean, rstd, gx, gw, gb, gw2, gb2) start as NaN and carry
16 NaN floats behind their end which must stay NaN; workspaces have exactly the size the entry point demands, followed in the same
allocation by such a guard.  Every call runs twice into fresh buffers and must give the same bits (the reductions are fixed-order).
The backward takes mean and rstd from the kernels' own forward, as the op layer does.

Input classes (norm_ref.inputs), each on every path but the grid-wrap cases, which take `random` only:
  random      x in [-2, 2), w = 1 + 0.2 r, b = 0.1 r, gy in [-1, 1)
  offset      x = 8 + [-1, 1): a one-pass variance or a lossy mean would show
  zero        a stripe of pixels with x exactly 0 in all channels (u = 0, rs = 1 / sqrt(eps)): y must equal the bias bit for bit
              there, and gx (1000 x the scale of the other pixels) is compared under its own mask with its own max|ref|
  constg      gy constant over the channels, w = 1: gx vanishes in exact arithmetic
  scale_up, scale_down    x * 1e3, x * 1e-3 (eps inside the sqrt matters for the second)
Criteria: random, zero, scale_*: the project's 2e-5 * max|ref| + 1e-6 against fp64 for y, mean, gx, gw, gb, and 2e-5 + 1e-6
relative for rstd.  offset, constg: max(that, 4 * E32), E32 the error of the fp32 CPU oracle (forward and autograd) against fp64 on
the same inputs; 4 because the kernels sum the C terms serially per lane and the pixels in a fixed tree where torch sums pairwise.
bf16 outputs: the fp64 y rounded to bf16, within 2^-8 * max|y| plus the fp32 bar.  bf16 gy: the reference takes the rounded values.

Paths (B, C, H, W are listed in norm_ref.py):
  forward     register kernels C = 36 / 72 / 144 at HW = 1, 2, 3, 5, 35, 96, B = 3 on odd planes, with statistics and with mean = rstd =
              nullptr (y bit-equal); the generic kernel at C = 1, 2, 35, 37, 73, 145 and HW = 1, 3, 4, 5, 6, 63; both wrapped
              (524,900 pixels of C = 36; 524,538 quads of C = 2); bf16 output; two modules (bit-equal to two single calls)
  backward, full workspace   the four fused kernels with 1, 32, 33, 64, 65 and (wrapped) 1024 block rows for ln_wb2_reduce_kernel;
              shapes without a fused kernel: reg<36,2,true>, reg<72,1,true>, reg<144,1,false> (512 x 513, nchunk 15), the generic
              kernel (C = 1, 12, 36 odd, 37; nchunk 56); each with and without addend and with accumulate 0 / 1 (1: bit-equal to
              the fp32 sum of the prefill and the accumulate-0 result)
  backward, 2 C nchunk floats   reg<36,2,true>, reg<72,1,true>, quad<36,true> on fused shapes: the bar, and gx within twice the bar
              of the fused gx; one float fewer: CIDNET_ERR_WS
  gx == nullptr, bf16 gy (four fused variants), cidnet_ln_cf_bwd2 (four variants, accumulate and accumulate2 varied separately),
  views one float inside larger buffers (bit-equal to the aligned run), the error returns, and the op layer on top.

Measured on the MI355X (the module prints this report at its end; every figure is the largest over the cases and outputs of a
path).  `random err/bar`: share of the project bar used on class random, at most 0.023 on any fp32 path (the bf16-output rows
are dominated by the half ulp of bf16).  `err/E32`: kernel error over the fp32 CPU oracle's on the same inputs, where E32 >= 1e-9;
a figure above 4 belongs to an output whose 4 E32 lies below the project bar, which then is the bar (E32 of a few 1e-8).  For
constg torch's autograd cancels exactly (E32 of gx is 0 to 1e-17), so the kernels' largest |gx| is listed: the bar there is 1e-6.

  kernel                                          random err/bar  offset err/E32  constg err/E32  constg max|gx|
  ln_fwd_reg_kernel<36,1>                         0.013           2.09            6.17            -
  ln_fwd_reg_kernel<72,1>                         0.022           7.52            6.38            -
  ln_fwd_reg_kernel<144,1>                        0.015           8.75            10.00           -
  ln_fwd_reg_kernel<36,1>+y2                      0.009           1.57            1.52            -
  ln_fwd_reg_kernel<72,1>+y2                      0.009           2.41            1.37            -
  ln_fwd_reg_kernel<144,1>+y2                     0.016           3.17            2.66            -
  ln_fwd_reg_kernel<36,1,bf16_t>                  0.386           1.48            1.42            -
  ln_fwd_reg_kernel<72,1,bf16_t>                  0.449           2.41            1.37            -
  ln_fwd_reg_kernel<144,1,bf16_t>                 0.876           3.17            2.66            -
  ln_fwd_kernel                                   0.017           10.25           24.04           -
  ln_bwd_quad_fused_kernel<9,4,4>                 0.014           2.17            2.43            3.5e-07
  ln_bwd_quad_fused_kernel<9,2,8>                 0.018           3.16            3.00            3.1e-07
  ln_bwd_quad_fused_kernel<18,2,8>                0.020           4.48            8.00            3.7e-07
  ln_bwd_quad_fused_kernel<18,1,8>                0.022           3.61            6.33            3.7e-07
  ln_bwd_quad_fused_kernel<9,4,4,false,bf16_t>    0.011           2.26            1.13            9.7e-08
  ln_bwd_quad_fused_kernel<9,2,8,false,bf16_t>    0.014           3.05            1.36            2.0e-07
  ln_bwd_quad_fused_kernel<18,2,8,false,bf16_t>   0.015           3.33            0.71            7.4e-08
  ln_bwd_quad_fused_kernel<18,1,8,false,bf16_t>   0.016           2.54            1.36            7.3e-08
  ln_bwd_quad_fused_kernel<9,2,4,true>            0.011           2.75            9.00            4.1e-07
  ln_bwd_quad_fused_kernel<9,2,8,true>            0.012           2.74            1.67            3.3e-07
  ln_bwd_quad_fused_kernel<18,2,8,true>           0.014           3.35            1.30            2.7e-07
  ln_bwd_quad_fused_kernel<18,1,8,true>           0.014           3.91            1.59            3.7e-07
  ln_bwd_reg_kernel<36,2,true>                    0.012           2.32            17.00           5.1e-07
  ln_bwd_reg_kernel<72,1,true>                    0.016           2.68            6.33            3.2e-07
  ln_bwd_reg_kernel<144,1,false>                  0.023           3.14            1.57            6.3e-07
  ln_bwd_quad_kernel<36,true>                     0.019           3.24            1.59            5.1e-07
  ln_bwd_kernel                                   0.013           2.58            20.00           7.4e-07
  ln_wb_kernel (gx == nullptr)                    0.010           3.24            17.00           -

Two findings of these tests were kernel defects and are fixed in csrc/norm.hip.  (1) ln_bwd_kernel formed g * w twice, rounded in the
channel sum and contracted into an FMA in the output, so gw - mean_c(gw) kept the product's rounding residue times rstd: for C = 1,
where gx is exactly 0, it returned up to 2.9e-5 on class random (bar 1e-6); the product is now rounded once (also in
ln_bwd_reg_kernel<144,1,false>).  (2) ln_bwd_reg_kernel summed its C terms in one serial chain; at C = 144 on 512 x 513 class constg
came to 2.1e-6 = 5.07 E32 against the bar 4 E32 = 1.67e-6; with four partial sums and a tree it is 6.3e-7 = 1.57 E32.  One finding
was a fixture at a rounding kink: a bf16 y whose fp64 value lies within the fp32 bar of the midpoint of two bf16 neighbours may round
to either, a whole ulp from the rounded reference ((2, 144, 6, 6) offset: 1.56e-2 against 8.9e-3); such entries (under 20 %, asserted)
are held to the same bound against the unrounded fp64 value, all others to it against the rounded one.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 16
F32, BF16 = torch.float32, torch.bfloat16


# --------------------------------------------------------------------------------------------------------------------------
# buffers, figures
# --------------------------------------------------------------------------------------------------------------------------
class Arena:
    """NaN-filled device buffers with a NaN guard behind (and, for views, the offset floats in front); keeps every tensor alive
    while its raw pointer is in flight"""

    def __init__(self, dev):
        self.dev, self.held = dev, []

    def new(self, n, dtype=F32, off=0):
        full = torch.full((off + n + GUARD,), NAN, dtype=dtype, device=self.dev)
        self.held.append((full, off, n))
        return full[off:off + n]

    def check(self, what):
        torch.cuda.synchronize()
        for full, off, n in self.held:
            assert bool(torch.isnan(full[:off]).all()) and bool(torch.isnan(full[off + n:]).all()), f"{what}: guard overwritten"


def place(dev, v, off=0):
    """the CPU or device tensor v in a device buffer of its own, `off` elements inside it"""
    full = torch.empty(off + v.numel(), dtype=v.dtype, device=dev)
    full[off:].copy_(v.reshape(-1))
    return full[off:]


FIG = {}


def note(kernel, cls, name, e, b, e32):
    f = FIG.setdefault((kernel, cls), {"share": 0.0, "ratio": 0.0, "gx0": 0.0})
    f["share"] = max(f["share"], e / b if b > 0 else 0.0)
    if e32 is not None and e32 >= 1e-9:          # below: torch's own result is exact (constg: its autograd cancels exactly)
        f["ratio"] = max(f["ratio"], e / e32)
    if cls == "constg" and name == "gx":
        f["gx0"] = max(f["gx0"], e)


@pytest.fixture(scope="module", autouse=True)
def report():
    assert "CIDNET_LN_UNFUSED" not in os.environ, "the case table assumes the fused backward is enabled"
    yield
    print("\nNORM-REPORT kernel | class | largest err / bar | largest err / E32 | largest |gx| of constg")
    for (k, c), f in sorted(FIG.items()):
        print(f"NORM-REPORT {k} | {c} | {f['share']:.3f} | {f['ratio']:.2f} | {f['gx0']:.1e}")


_CACHE = {}


def get(dev, case, cls, dual=False, gy_bf16=False, on_device=False):
    """-> (t: fp32 CPU inputs, d: the same on the device, ref: fp64 on the device incl. gx_add, E: E32 per output or None)"""
    key = (case, cls, dual, gy_bf16)
    if key in _CACHE:
        return _CACHE[key]
    t = R.inputs(case, cls, dual=dual, addend=True)
    if gy_bf16:
        t["gy"] = R.bf16_round(t["gy"])
    ref = R.reference(t, dual=dual, device=dev if on_device else None)
    ref["gx_add"] = ref["gx"] + t["addend"].to(ref["gx"].device).double()
    E = R.e32(t, ref, dual) if cls in R.MEASURED else None
    val = (t, {k: v.to(dev) for k, v in t.items()}, {k: v.to(dev) for k, v in ref.items()}, E)
    if t["x"].numel() <= 100_000:
        _CACHE[key] = val
    return val


def compare(kernel, case, cls, name, got, ref, E, bf16_out=False):
    """one output against its fp64 reference under the bar of its class; the zero class splits y and gx by its pixel mask"""
    B, C, H, W = case
    what = f"{kernel} {case} {cls} {name}"
    assert bool(torch.isfinite(got.float()).all()), f"{what}: not finite"
    refname = "gx" if name in ("gx", "gx_add") else name
    got = got.double().view(ref.shape)
    parts = [(got, ref, "")]
    if cls == "zero" and name in ("gx", "gx_add", "y", "y2"):
        m = R.zero_pixels(H * W).to(got.device)
        g3, r3 = got.view(B, C, H * W), ref.view(B, C, H * W)
        parts = [(g3[:, :, m], r3[:, :, m], " zero pixels"), (g3[:, :, ~m], r3[:, :, ~m], " live pixels")]
    for g, r, tag in parts:
        if r.numel() == 0:
            continue
        b = R.bar(name, r, cls, E)
        e32 = E[name] if E is not None and not bf16_out else None
        if bf16_out:
            # the fp64 value rounded to bf16, within half a bf16 ulp of max|y| plus the fp32 bar.  Where the fp64 value lies within
            # the fp32 bar of a rounding tie (the midpoint of two bf16 neighbours) an fp32 result inside its bar may round to
            # either neighbour, a whole ulp apart: those entries are held to the same bound against the unrounded value
            rb = r.to(BF16).double()
            half = torch.ldexp(torch.ones_like(r), torch.frexp(r.abs())[1] - 9)            # half a bf16 ulp at |r|
            kink = half - (r - rb).abs() <= b
            assert kink.double().mean().item() <= 0.2, f"{what}{tag}: too few entries off the rounding ties"
            b = b + 2.0 ** -8 * r.abs().max().item()
            e = max(R.err(refname, g[~kink], rb[~kink]), R.err(refname, g[kink], r[kink]))
        else:
            e = R.err(refname, g, r)
        print(f"NORM-FIG {what}{tag}: err {e:.3e} bar {b:.3e}" + (f" E32 {e32:.3e}" if e32 is not None else ""))
        note(kernel, cls, name, e, b, e32)
        assert e <= b, f"{what}{tag}: err {e:.3e} > bar {b:.3e}"


def same(a, b, what):
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs between two runs"


# --------------------------------------------------------------------------------------------------------------------------
# the entry points
# --------------------------------------------------------------------------------------------------------------------------
def run_fwd(dev, d, case, stats="both", y_dt=0, dual=False, off=0):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    HW, n = H * W, B * C * H * W
    a = Arena(dev)
    ydt = BF16 if y_dt == 1 else F32
    o = {"y": a.new(n, ydt, 0 if y_dt == 1 else off), "y2": a.new(n, ydt) if dual else None,
         "mean": a.new(B * HW) if stats in ("both", "mean") else None, "rstd": a.new(B * HW) if stats in ("both", "rstd") else None}
    p = ops._p
    if dual:
        rc = ops._raw("cidnet_ln_cf_fwd2", p(d["x"]), p(d["w"]), p(d["b"]), p(o["y"]), p(d["w2"]), p(d["b2"]), p(o["y2"]), p(o["mean"]),
                      p(o["rstd"]), B, C, HW, ops._f(R.EPS), ops._stream())
    else:
        rc = ops._raw("cidnet_ln_cf_fwd_t", p(d["x"]), p(d["w"]), p(d["b"]), p(o["y"]), y_dt, p(o["mean"]), p(o["rstd"]), B, C, HW,
                      ops._f(R.EPS), ops._stream())
    a.check(f"fwd {case}")
    return rc, o


def run_bwd(dev, d, st, case, ws_floats, gx=True, addend=False, acc=0, gy_bf16=False, off=0, prefill=None):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    HW, n = H * W, B * C * H * W
    a = Arena(dev)
    o = {"gx": a.new(n, off=off) if gx else None, "gw": a.new(C), "gb": a.new(C)}
    if prefill is not None:
        o["gw"].copy_(prefill[0]); o["gb"].copy_(prefill[1])
    ws = a.new(ws_floats)
    gy = d["gy"].to(BF16) if gy_bf16 else d["gy"]
    p = ops._p
    rc = ops._raw("cidnet_ln_cf_bwd_res_t", p(d["x"]), p(d["w"]), p(gy), 1 if gy_bf16 else 0, p(st["mean"]), p(st["rstd"]),
                  p(d["addend"]) if addend else None, p(o["gx"]), p(o["gw"]), p(o["gb"]), acc, p(ws), ws_floats, B, C, HW, ops._stream())
    a.check(f"bwd {case}")
    return rc, o


def run_bwd2(dev, d, st, case, ws_floats, addend=False, acc=0, acc2=0, off=0, prefill=None):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    HW, n = H * W, B * C * H * W
    a = Arena(dev)
    o = {"gx": a.new(n, off=off), "gw": a.new(C), "gb": a.new(C), "gw2": a.new(C), "gb2": a.new(C)}
    if prefill is not None:
        for k, v in zip(("gw", "gb", "gw2", "gb2"), prefill):
            o[k].copy_(v)
    ws = a.new(ws_floats)
    p = ops._p
    rc = ops._raw("cidnet_ln_cf_bwd2", p(d["x"]), p(d["w"]), p(d["gy"]), p(d["w2"]), p(d["gy2"]), p(st["mean"]), p(st["rstd"]),
                  p(d["addend"]) if addend else None, p(o["gx"]), p(o["gw"]), p(o["gb"]), acc, p(o["gw2"]), p(o["gb2"]), acc2, p(ws),
                  ws_floats, B, C, HW, ops._stream())
    a.check(f"bwd2 {case}")
    return rc, o


def all_nan(o):
    return all(bool(torch.isnan(v.float()).all()) for v in o.values() if v is not None)


def prefills(dev, C, k=2):
    return [(3.0 * R.rnd(900 + i, (C,))).to(dev) for i in range(k)]


# --------------------------------------------------------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------------------------------------------------------
def check_fwd(dev, case, cls, off=0):
    B, C, H, W = case
    kernel = R.fwd_path(B, C, H * W).kernel
    t, d, ref, E = get(dev, case, cls)
    if off:
        d = dict(d, x=place(dev, d["x"], off))
    rc, o = run_fwd(dev, d, case, off=off)
    assert rc == 0
    rc2, o2 = run_fwd(dev, d, case, off=off)
    same(o, o2, f"{kernel} {case} {cls}")
    for k in ("y", "mean", "rstd"):
        compare(kernel, case, cls, k, o[k], ref[k], E)
    rc3, o3 = run_fwd(dev, d, case, stats="none", off=off)
    assert rc3 == 0 and torch.equal(o3["y"], o["y"]), f"{kernel} {case} {cls}: y differs without the statistics"
    if cls == "zero":
        m = R.zero_pixels(H * W).to(dev)
        assert torch.equal(o["y"].view(B, C, H * W)[:, :, m], d["b"].view(1, C, 1).expand(B, C, int(m.sum()))), "y != bias on zero columns"
    return o


@pytest.mark.parametrize("case", R.FWD_REG + R.FWD_GENERIC, ids=str)
def test_forward(dev, case):
    for cls in R.CLASSES:
        check_fwd(dev, case, cls)


@pytest.mark.parametrize("case", R.FWD_WRAP, ids=str)
def test_forward_grid_wrap(dev, case):
    assert R.fwd_path(case[0], case[1], R.hw(case)).trips == 2
    check_fwd(dev, case, "random")


@pytest.mark.parametrize("case", R.FWD_BF16, ids=str)
def test_forward_bf16_output(dev, case):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    assert ops._raw("cidnet_ln_cf_typed_supported", B, C, H * W) == R.typed_supported(B, C, H * W) == 1
    kernel = R.fwd_path(B, C, H * W, y_dt=1).kernel
    for cls in R.CLASSES:
        t, d, ref, E = get(dev, case, cls)
        rc, o = run_fwd(dev, d, case, y_dt=1)
        assert rc == 0 and o["y"].dtype == BF16
        same(o, run_fwd(dev, d, case, y_dt=1)[1], f"{kernel} {case} {cls}")
        compare(kernel, case, cls, "y", o["y"], ref["y"], E, bf16_out=True)
        for k in ("mean", "rstd"):
            compare(kernel, case, cls, k, o[k], ref[k], E)
        o32 = run_fwd(dev, d, case)[1]
        assert torch.equal(o["y"], o32["y"].to(BF16)) and torch.equal(o["mean"], o32["mean"]) and torch.equal(o["rstd"], o32["rstd"])
        assert torch.equal(run_fwd(dev, d, case, stats="none", y_dt=1)[1]["y"], o["y"])
        if cls == "zero":
            m = R.zero_pixels(H * W).to(dev)
            assert torch.equal(o["y"].view(B, C, H * W)[:, :, m], d["b"].to(BF16).view(1, C, 1).expand(B, C, int(m.sum())))


@pytest.mark.parametrize("case", R.FWD_DUAL, ids=str)
def test_forward_two_modules(dev, case):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    assert ops._raw("cidnet_ln_cf_dual_supported", B, C, H * W) == R.dual_supported(B, C, H * W) == 1
    kernel = R.fwd_path(B, C, H * W, dual=True).kernel
    for cls in R.CLASSES:
        t, d, ref, E = get(dev, case, cls, dual=True)
        rc, o = run_fwd(dev, d, case, dual=True)
        assert rc == 0
        same(o, run_fwd(dev, d, case, dual=True)[1], f"{kernel} {case} {cls}")
        for k in ("y", "y2", "mean", "rstd"):
            compare(kernel, case, cls, k, o[k], ref[k], E)
        oa = run_fwd(dev, d, case)[1]
        ob = run_fwd(dev, dict(d, w=d["w2"], b=d["b2"]), case)[1]
        assert torch.equal(o["y"], oa["y"]) and torch.equal(o["y2"], ob["y"])
        assert torch.equal(o["mean"], oa["mean"]) and torch.equal(o["rstd"], oa["rstd"])


def test_forward_errors(dev):
    from hvi_cidnet_amd import ops
    case = (2, 36, 8, 12)
    _, d, _, _ = get(dev, case, "random", dual=True)
    for stats in ("mean", "rstd"):
        rc, o = run_fwd(dev, d, case, stats=stats)
        assert rc == R.ERR_ARG and all_nan(o)
    rc, o = run_fwd(dev, d, case, y_dt=2)
    assert rc == R.ERR_ARG and all_nan(o)
    for c in R.FWD_UNSUPPORTED:
        B, C, H, W = c
        assert ops._raw("cidnet_ln_cf_typed_supported", B, C, H * W) == R.typed_supported(B, C, H * W) == 0
        assert ops._raw("cidnet_ln_cf_dual_supported", B, C, H * W) == R.dual_supported(B, C, H * W) == 0
        _, d, _, _ = get(dev, c, "random", dual=True)
        rc, o = run_fwd(dev, d, c, y_dt=1)
        assert rc == R.ERR_SHAPE and all_nan(o)
        rc, o = run_fwd(dev, d, c, dual=True)
        assert rc == R.ERR_SHAPE and all_nan(o)


# --------------------------------------------------------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------------------------------------------------------
def check_bwd(dev, case, cls, ws_floats, gy_bf16=False, on_device=False, off=0):
    """one case and class on the path (ws_floats, gy type) selects: with and without addend, accumulate 0 (twice) and 1"""
    B, C, H, W = case
    pth = R.path(B, C, H * W, ws_floats, True, 1 if gy_bf16 else 0)
    assert not pth.kernel.startswith("ERR")
    kernel = pth.kernel
    t, d, ref, E = get(dev, case, cls, gy_bf16=gy_bf16, on_device=on_device)
    if off:
        d = dict(d, x=place(dev, d["x"], off), gy=place(dev, d["gy"], off if not gy_bf16 else 0))
    rc, st = run_fwd(dev, d, case)
    assert rc == 0
    pre = prefills(dev, C)
    out = {}
    for addend in (False, True):
        what = f"{kernel} {case} {cls} addend={addend}"
        rc, o = run_bwd(dev, d, st, case, ws_floats, addend=addend, gy_bf16=gy_bf16, off=off)
        assert rc == 0, what
        same(o, run_bwd(dev, d, st, case, ws_floats, addend=addend, gy_bf16=gy_bf16, off=off)[1], what)
        compare(kernel, case, cls, "gx_add" if addend else "gx", o["gx"], ref["gx_add" if addend else "gx"], E)
        compare(kernel, case, cls, "gw", o["gw"], ref["gw"], E)
        compare(kernel, case, cls, "gb", o["gb"], ref["gb"], E)
        rc, o1 = run_bwd(dev, d, st, case, ws_floats, addend=addend, acc=1, gy_bf16=gy_bf16, off=off, prefill=pre)
        assert rc == 0, what
        assert torch.equal(o1["gx"], o["gx"]), what
        assert torch.equal(o1["gw"], pre[0] + o["gw"]) and torch.equal(o1["gb"], pre[1] + o["gb"]), f"{what}: accumulate"
        out[addend] = o
    assert torch.equal(out[False]["gw"], out[True]["gw"]) and torch.equal(out[False]["gb"], out[True]["gb"])
    return st, out


@pytest.mark.parametrize("case", R.BWD_FUSED + R.BWD_UNFUSED, ids=str)
def test_backward_full_workspace(dev, case):
    from hvi_cidnet_amd import ops
    assert ops._raw("cidnet_ln_cf_bwd_ws_floats", case[1]) == R.bwd_ws_floats(case[1])
    for cls in R.CLASSES:
        check_bwd(dev, case, cls, R.bwd_ws_floats(case[1]))


@pytest.mark.parametrize("case", R.BWD_FUSED_WRAP, ids=str)
def test_backward_fused_grid_wrap(dev, case):
    p = R.path(case[0], case[1], R.hw(case), R.bwd_ws_floats(case[1]))
    assert p.trips == 2 and p.nblk == R.K_FUSED_BLOCKS
    check_bwd(dev, case, "random", R.bwd_ws_floats(case[1]))


@pytest.mark.parametrize("cls", R.CLASSES)
def test_backward_large_plane(dev, cls):
    """C = 144 beyond 2^18 pixels: ln_bwd_reg_kernel<144,1,false> and ln_wb_kernel with nchunk at its cap; the fp64 reference
    is evaluated with plain torch float64 ops on the device"""
    case = R.BWD_LARGE
    p = R.path(case[0], case[1], R.hw(case), R.bwd_ws_floats(144))
    assert (p.kernel, p.nchunk) == ("ln_bwd_reg_kernel<144,1,false>", 15)
    check_bwd(dev, case, cls, R.bwd_ws_floats(144), on_device=True)


@pytest.mark.parametrize("case", R.BWD_SHORT, ids=str)
def test_backward_short_workspace(dev, case):
    B, C, H, W = case
    n = R.ws_short(case)
    kernel = R.path(B, C, H * W, n).kernel
    assert kernel in ("ln_bwd_reg_kernel<36,2,true>", "ln_bwd_reg_kernel<72,1,true>", "ln_bwd_quad_kernel<36,true>")
    for cls in R.CLASSES:
        st, short = check_bwd(dev, case, cls, n)
        t, d, ref, E = get(dev, case, cls)
        for addend in (False, True):
            name = "gx_add" if addend else "gx"
            rc, full = run_bwd(dev, d, st, case, R.bwd_ws_floats(C), addend=addend)
            assert rc == 0
            diff = (short[addend]["gx"].double() - full["gx"].double()).abs()
            if cls == "zero":
                m = R.zero_pixels(H * W).to(dev)
                parts = [(diff.view(B, C, -1)[:, :, m], ref[name].view(B, C, -1)[:, :, m]), (diff.view(B, C, -1)[:, :, ~m], ref[name].view(B, C, -1)[:, :, ~m])]
            else:
                parts = [(diff, ref[name])]
            for dd, rr in parts:
                if rr.numel():
                    assert dd.max().item() <= 2 * R.bar(name, rr, cls, E), f"{kernel} {case} {cls}: gx of the unfused and the fused path"
        rc, o = run_bwd(dev, d, st, case, n - 1)
        assert rc == R.ERR_WS and all_nan(o)


@pytest.mark.parametrize("case", R.BWD_NOGX, ids=str)
def test_backward_parameter_gradients_only(dev, case):
    B, C, H, W = case
    n = R.ws_short(case)
    assert R.path(B, C, H * W, n, gx=False).kernel == "ln_wb_kernel"
    for cls in R.CLASSES:
        t, d, ref, E = get(dev, case, cls)
        st = run_fwd(dev, d, case)[1]
        rc, o = run_bwd(dev, d, st, case, n, gx=False)
        assert rc == 0
        same(o, run_bwd(dev, d, st, case, n, gx=False)[1], f"ln_wb_kernel {case} {cls}")
        for k in ("gw", "gb"):
            compare("ln_wb_kernel", case, cls, k, o[k], ref[k], E)
        w = run_bwd(dev, d, st, case, n, gx=True)[1]
        assert torch.equal(o["gw"], w["gw"]) and torch.equal(o["gb"], w["gb"])
        pre = prefills(dev, C)
        o1 = run_bwd(dev, d, st, case, n, gx=False, acc=1, prefill=pre)[1]
        assert torch.equal(o1["gw"], pre[0] + o["gw"]) and torch.equal(o1["gb"], pre[1] + o["gb"])
    rc, o = run_bwd(dev, d, st, case, R.bwd_ws_floats(C), gx=False, gy_bf16=True)
    assert rc == R.ERR_SHAPE and all_nan(o)


@pytest.mark.parametrize("case", R.BWD_BF16, ids=str)
def test_backward_bf16_gradient(dev, case):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    assert ops._raw("cidnet_ln_cf_typed_supported", B, C, H * W) == R.typed_supported(B, C, H * W) == 1
    for cls in R.CLASSES:
        st, out = check_bwd(dev, case, cls, R.bwd_ws_floats(C), gy_bf16=True)
        t, d, ref, E = get(dev, case, cls, gy_bf16=True)
        f32 = run_bwd(dev, d, st, case, R.bwd_ws_floats(C))[1]              # the fp32 kernel on the same (representable) values
        same(out[False], f32, f"bf16 gy {case} {cls}")
    rc, o = run_bwd(dev, d, st, case, R.ws_short(case), gy_bf16=True)
    assert rc == R.ERR_SHAPE and all_nan(o)
    rc, o = run_bwd(dev, d, st, case, 2 * C * R.K_FUSED_BLOCKS - 1, gy_bf16=True)
    assert rc == R.ERR_SHAPE and all_nan(o)


def check_bwd2(dev, case, cls, off=0):
    B, C, H, W = case
    n = R.bwd2_ws_floats(C)
    kernel = R.path2(B, C, H * W, n).kernel
    t, d, ref, E = get(dev, case, cls, dual=True)
    if off:
        d = dict(d, x=place(dev, d["x"], off), gy=place(dev, d["gy"], off), gy2=place(dev, d["gy2"], off))
    st = run_fwd(dev, d, case, dual=True)[1]
    pre = prefills(dev, C, 4)
    for addend in (False, True):
        what = f"{kernel} {case} {cls} addend={addend}"
        rc, o = run_bwd2(dev, d, st, case, n, addend=addend, off=off)
        assert rc == 0, what
        same(o, run_bwd2(dev, d, st, case, n, addend=addend, off=off)[1], what)
        compare(kernel, case, cls, "gx_add" if addend else "gx", o["gx"], ref["gx_add" if addend else "gx"], E)
        for k in ("gw", "gb", "gw2", "gb2"):
            compare(kernel, case, cls, k, o[k], ref[k], E)
        for acc, acc2 in ((0, 1), (1, 0)):
            o1 = run_bwd2(dev, d, st, case, n, addend=addend, acc=acc, acc2=acc2, off=off, prefill=pre)[1]
            assert torch.equal(o1["gx"], o["gx"]), what
            for k, v, a in (("gw", pre[0], acc), ("gb", pre[1], acc), ("gw2", pre[2], acc2), ("gb2", pre[3], acc2)):
                assert torch.equal(o1[k], v + o[k] if a else o[k]), f"{what}: {k} with accumulate={acc}, accumulate2={acc2}"
    return d, st


@pytest.mark.parametrize("case", R.BWD2, ids=str)
def test_backward_two_modules(dev, case):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    assert ops._raw("cidnet_ln_cf_dual_supported", B, C, H * W) == R.dual_supported(B, C, H * W) == 1
    assert ops._raw("cidnet_ln_cf_bwd2_ws_floats", C) == R.bwd2_ws_floats(C)
    for cls in R.CLASSES:
        d, st = check_bwd2(dev, case, cls)
    rc, o = run_bwd2(dev, d, st, case, R.bwd2_ws_floats(C) - 1)
    assert rc == R.ERR_WS and all_nan(o)


def test_backward_two_modules_unsupported_shapes(dev):
    from hvi_cidnet_amd import ops
    for case in R.BWD2_UNSUPPORTED:
        B, C, H, W = case
        assert ops._raw("cidnet_ln_cf_dual_supported", B, C, H * W) == R.dual_supported(B, C, H * W) == 0
        t, d, ref, E = get(dev, case, "random", dual=True)
        st = run_fwd(dev, d, case)[1]
        rc, o = run_bwd2(dev, d, st, case, R.bwd2_ws_floats(C))
        assert rc == R.ERR_SHAPE and all_nan(o)


# --------------------------------------------------------------------------------------------------------------------------
# views: x, gy, gx (and y) four bytes off their allocation's alignment
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.VIEW_FWD, ids=str)
def test_forward_views(dev, case):
    o = check_fwd(dev, case, "random", off=1)
    assert o["y"].data_ptr() % 8 == 4
    same(o, check_fwd(dev, case, "random"), f"view {case}")


@pytest.mark.parametrize("case,ws", R.VIEW_BWD, ids=str)
def test_backward_views(dev, case, ws):
    n = R.bwd_ws_floats(case[1]) if ws == "full" else R.ws_short(case)
    _, a = check_bwd(dev, case, "random", n, off=1)
    _, b = check_bwd(dev, case, "random", n)
    assert a[True]["gx"].data_ptr() % 8 == 4
    for addend in (False, True):
        same(a[addend], b[addend], f"view {case} {ws}")


@pytest.mark.parametrize("case", R.VIEW_BWD2, ids=str)
def test_backward_two_modules_views(dev, case):
    check_bwd2(dev, case, "random", off=1)


# --------------------------------------------------------------------------------------------------------------------------
# the op layer
# --------------------------------------------------------------------------------------------------------------------------
def _leaves(d, names, grad=True):
    return [d[k].clone().requires_grad_(grad) for k in names]


@pytest.mark.parametrize("case", [(2, 36, 8, 12), (2, 36, 5, 7), (3, 144, 5, 7), (1, 72, 25, 41)], ids=str)
def test_op_layer_single_module(dev, case):
    from hvi_cidnet_amd import ops
    B, C, H, W = case
    for cls in ("random", "zero"):
        t, d, ref, E = get(dev, case, cls)
        x, w, b = _leaves(d, ("x", "w", "b"))
        y = ops.LayerNormCFFn.apply(x, w, b, R.EPS)
        y.backward(d["gy"])
        for name, got in (("y", y.detach()), ("gx", x.grad), ("gw", w.grad), ("gb", b.grad)):
            compare("LayerNormCFFn", case, cls, name, got, ref[name], E)
        # needs_input_grad[0] == False: gx = nullptr, the parameter gradients alone
        w2, b2 = _leaves(d, ("w", "b"))
        ops.LayerNormCFFn.apply(d["x"], w2, b2, R.EPS).backward(d["gy"])
        compare("LayerNormCFFn, x without grad", case, cls, "gw", w2.grad, ref["gw"], E)
        compare("LayerNormCFFn, x without grad", case, cls, "gb", b2.grad, ref["gb"], E)
        # the residual form: the addend arrives in the kernel; then only the residual output used (gy is None, or zeros
        # where autograd materialises it: either way gx is the residual's gradient and the parameter gradients vanish)
        x, w, b = _leaves(d, ("x", "w", "b"))
        y, xres = ops.LayerNormResFn.apply(x, w, b, R.EPS)
        torch.autograd.backward([y, xres], [d["gy"], d["addend"]])
        for name, got in (("y", y.detach()), ("gx_add", x.grad), ("gw", w.grad), ("gb", b.grad)):
            compare("LayerNormResFn", case, cls, name, got, ref[name], E)
        x, w, b = _leaves(d, ("x", "w", "b"))
        y, xres = ops.LayerNormResFn.apply(x, w, b, R.EPS)
        xres.backward(d["addend"])
        assert torch.equal(x.grad, d["addend"])
        assert float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0


@pytest.mark.parametrize("case", [(2, 36, 8, 12), (3, 144, 5, 7), (1, 36, 7, 9)], ids=str)
def test_op_layer_two_modules(dev, case):
    from hvi_cidnet_amd import ops
    import hvi_cidnet_amd as P
    B, C, H, W = case
    t, d, ref, E = get(dev, case, "random", dual=True)
    na, nb = P.LayerNorm(C).to(dev), P.LayerNorm(C).to(dev)
    with torch.no_grad():
        na.weight.copy_(d["w"]); na.bias.copy_(d["b"]); nb.weight.copy_(d["w2"]); nb.bias.copy_(d["b2"])
    x = d["x"].clone().requires_grad_(True)
    assert bool(ops.ln_dual_supported(x)) == bool(R.dual_supported(B, C, H * W))
    ya, yb, xres = na.forward_dual(x, nb)
    torch.autograd.backward([ya, yb, xres], [d["gy"], d["gy2"], d["addend"]])
    for name, got in (("y", ya.detach()), ("y2", yb.detach()), ("gx_add", x.grad), ("gw", na.weight.grad), ("gb", na.bias.grad),
                      ("gw2", nb.weight.grad), ("gb2", nb.bias.grad)):
        compare("LayerNorm.forward_dual", case, "random", name, got, ref[name], E)
    if R.dual_supported(B, C, H * W):
        x2, wa, ba, wb, bb = _leaves(d, ("x", "w", "b", "w2", "b2"))
        oa, ob, xr = ops.LayerNormDualFn.apply(x2, wa, ba, wb, bb, R.EPS)
        torch.autograd.backward([oa, ob, xr], [d["gy"], d["gy2"], d["addend"]])
        assert torch.equal(oa, ya) and torch.equal(ob, yb) and torch.equal(x2.grad, x.grad)
        assert torch.equal(wa.grad, na.weight.grad) and torch.equal(bb.grad, nb.bias.grad)
