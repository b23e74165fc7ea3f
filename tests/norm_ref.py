"""References, case table and criteria for the channels-first LayerNorm kernels (csrc/norm.hip); used by tests/test_norm_cpu.py
and tests/test_norm_gpu.py.  Nothing of the project is on the reference side: the formulas below are written from the math in
fp64 torch, and tests/test_norm_cpu.py checks them against the oracle's autograd.

    u = mean_c x,  var = mean_c (x - u)^2 (biased),  rs = 1 / sqrt(var + eps),  xhat = (x - u) rs,  y = w xhat + b
    gx = rs (g w - mean_c(g w) - xhat mean_c(g w xhat)) [+ addend],   gw = sum_{b,p} g xhat,   gb = sum_{b,p} g
    two modules on one tensor: g w + g2 w2 in place of g w for gx, (gw, gb) and (gw2, gb2) per module

`path`, `fwd_path` and `path2` restate the launcher's dispatch (cidnet_ln_cf_fwd_t, cidnet_ln_cf_bwd_res_t, cidnet_ln_cf_bwd2,
wb_chunks, grid_for) in plain Python, with CIDNET_LN_UNFUSED unset; kernel names are spelled as in norm.hip without blanks.
"""
import collections

import torch

from oracle import cidnet_oracle as O

EPS = 1e-6
ERR_ARG, ERR_SHAPE, ERR_WS = -1, -2, -3

# --------------------------------------------------------------------------------------------------------------------------
# the launcher's dispatch
# --------------------------------------------------------------------------------------------------------------------------
K_THREADS, K_MAX_BLOCKS, K_FUSED_BLOCKS = 256, 2048, 1024

Path = collections.namedtuple("Path", "kernel nblk nchunk trips")


def _cdiv(a, b):
    return -(-a // b)


def grid_for(items):
    return min(max(_cdiv(items, K_THREADS), 1), K_MAX_BLOCKS)


def wb_chunks(B, C, HW):
    per = _cdiv(_cdiv(HW, 4), K_THREADS)
    want = _cdiv(2048, C)
    return max(min(per, want), 1)


def wb_trips(B, C, HW):
    """passes of ln_wb_kernel's pixel loop per sample"""
    return _cdiv(_cdiv(HW, 4), wb_chunks(B, C, HW) * K_THREADS)


def typed_supported(B, C, HW):
    return int(B > 0 and HW > 0 and ((C == 36 and HW % 4 == 0) or (C == 72 and HW % 2 == 0) or (C == 144 and B * HW <= 1 << 18)))


dual_supported = typed_supported


def bwd_ws_floats(C):
    return max(2 * 2048 + 4 * C * 64, 2 * C * K_FUSED_BLOCKS)


def bwd2_ws_floats(C):
    return 4 * C * K_FUSED_BLOCKS


def fwd_path(B, C, HW, y_dt=0, dual=False):
    """-> Path(kernel, blocks, None, trips of the grid-stride loop) of cidnet_ln_cf_fwd_t / cidnet_ln_cf_fwd2"""
    if y_dt not in (0, 1):
        return Path("ERR_ARG", 0, None, 0)
    if (y_dt or dual) and not typed_supported(B, C, HW):
        return Path("ERR_SHAPE", 0, None, 0)
    if C in (36, 72, 144):
        g = grid_for(B * HW)
        name = "ln_fwd_reg_kernel<%d,1%s>%s" % (C, ",bf16_t" if y_dt else "", "+y2" if dual else "")
        return Path(name, g, None, _cdiv(B * HW, g * K_THREADS))
    items = B * _cdiv(HW, 4)
    g = grid_for(items)
    return Path("ln_fwd_kernel", g, None, _cdiv(items, g * K_THREADS))


def _fused(B, C, HW, dual, bf16):
    """(CQ, VEC, LPP), blocks, trips of ln_bwd_quad_fused_kernel"""
    lanes = B * HW if C == 36 else (B * HW * 4 if C == 72 or HW % 2 == 0 else B * HW * 8)
    nblk = min(_cdiv(lanes, K_THREADS), K_FUSED_BLOCKS)
    if C == 36:
        cq, vec, lpp = (9, 2, 4) if dual else (9, 4, 4)
    elif C == 72:
        cq, vec, lpp = 9, 2, 8
    else:
        cq, vec, lpp = (18, 2, 8) if HW % 2 == 0 else (18, 1, 8)
    tail = ",true" if dual else (",false,bf16_t" if bf16 else "")
    name = "ln_bwd_quad_fused_kernel<%d,%d,%d%s>" % (cq, vec, lpp, tail)
    return name, nblk, _cdiv(B * (HW // vec), nblk * K_THREADS // lpp)


def path(B, C, HW, ws_floats, gx=True, gy_dt=0):
    """cidnet_ln_cf_bwd_res_t -> Path(gx kernel, its blocks, nchunk of ln_wb_kernel or None when the fused kernel forms the
    parameter gradients (ln_wb2_reduce_kernel then sums `nblk` rows), trips of the gx kernel's grid-stride loop)"""
    nchunk = wb_chunks(B, C, HW)
    if ws_floats < 2 * C * nchunk:
        return Path("ERR_WS", 0, nchunk, 0)
    shape_ok = bool(typed_supported(B, C, HW))
    if gy_dt:
        if not gx or not shape_ok or ws_floats < 2 * C * K_FUSED_BLOCKS:
            return Path("ERR_SHAPE", 0, nchunk, 0)
        name, nblk, trips = _fused(B, C, HW, False, True)
        return Path(name, nblk, None, trips)
    if gx and shape_ok and ws_floats >= 2 * C * K_FUSED_BLOCKS:
        name, nblk, trips = _fused(B, C, HW, False, False)
        return Path(name, nblk, None, trips)
    if not gx:
        return Path("ln_wb_kernel", 0, nchunk, 0)
    if C == 36 and HW % 2 == 0:
        g = grid_for(B * HW // 2)
        return Path("ln_bwd_reg_kernel<36,2,true>", g, nchunk, _cdiv(B * HW // 2, g * K_THREADS))
    if C == 72:
        g = grid_for(B * HW)
        return Path("ln_bwd_reg_kernel<72,1,true>", g, nchunk, _cdiv(B * HW, g * K_THREADS))
    if C == 144 and B * C * HW < 1 << 31 and B * HW <= 1 << 18:
        g = grid_for(B * HW * 4)
        return Path("ln_bwd_quad_kernel<36,true>", g, nchunk, _cdiv(B * HW, g * K_THREADS // 4))
    if C == 144:
        g = grid_for(B * HW)
        return Path("ln_bwd_reg_kernel<144,1,false>", g, nchunk, _cdiv(B * HW, g * K_THREADS))
    items = B * _cdiv(HW, 4)
    g = grid_for(items)
    return Path("ln_bwd_kernel", g, nchunk, _cdiv(items, g * K_THREADS))


def path2(B, C, HW, ws_floats):
    """cidnet_ln_cf_bwd2"""
    if not dual_supported(B, C, HW):
        return Path("ERR_SHAPE", 0, None, 0)
    if ws_floats < bwd2_ws_floats(C):
        return Path("ERR_WS", 0, None, 0)
    name, nblk, trips = _fused(B, C, HW, True, False)
    return Path(name, nblk, None, trips)


# every instantiation the launchers of norm.hip name ("+y2": the same forward kernel with its second output)
ALL_KERNELS = frozenset(
    ["ln_fwd_kernel", "ln_bwd_kernel", "ln_wb_kernel", "ln_wb_reduce_kernel", "ln_wb2_reduce_kernel",
     "ln_bwd_reg_kernel<36,2,true>", "ln_bwd_reg_kernel<72,1,true>", "ln_bwd_reg_kernel<144,1,false>", "ln_bwd_quad_kernel<36,true>"]
    + ["ln_fwd_reg_kernel<%d,1%s>" % (c, t) for c in (36, 72, 144) for t in ("", ",bf16_t")]
    + ["ln_bwd_quad_fused_kernel<%s%s>" % (k, t) for k in ("9,4,4", "9,2,8", "18,2,8", "18,1,8") for t in ("", ",false,bf16_t")]
    + ["ln_bwd_quad_fused_kernel<%s,true>" % k for k in ("9,2,4", "9,2,8", "18,2,8", "18,1,8")])

# --------------------------------------------------------------------------------------------------------------------------
# the case table: (B, C, H, W); any factorisation of H*W serves, the kernels see B, C and H*W only
# --------------------------------------------------------------------------------------------------------------------------
_HW = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (2, 2), 5: (1, 5), 6: (2, 3), 35: (5, 7), 63: (7, 9), 96: (8, 12)}

FWD_REG = ([(1, C) + _HW[hw] for C in (36, 72, 144) for hw in (1, 2, 3, 5, 35, 96)]
           + [(3, C) + _HW[hw] for C in (36, 72, 144) for hw in (1, 3, 5, 35)])
FWD_GENERIC = [(1 + (i + j) % 2, C) + _HW[hw] for i, C in enumerate((1, 2, 35, 37, 73, 145)) for j, hw in enumerate((1, 3, 4, 5, 6, 63))]        # tails 1, 3, none, 1, 2, 3
FWD_WRAP = [(1, 36, 724, 725), (1, 2, 1448, 1449)]
FWD_BF16 = [(2, 36, 8, 12), (1, 72, 5, 6), (2, 144, 6, 6), (3, 144, 5, 7)]
FWD_DUAL = [(2, 36, 8, 12), (1, 72, 5, 6), (1, 144, 6, 6), (3, 144, 5, 7)]
FWD_UNSUPPORTED = [(1, 36, 2, 3), (1, 72, 1, 5), (2, 12, 7, 9)]          # typed and dual calls: CIDNET_ERR_SHAPE

# backward with the full workspace cidnet_ln_cf_bwd_ws_floats(C)
BWD_FUSED = ([(1, 36, 2, 2), (2, 36, 64, 64), (3, 36, 4, 683), (1, 36, 128, 128), (1, 36, 68, 241)]          # B HW = 4, 8192, 8196, 16384, 16388
             + [(1, C, 1, 2) for C in (72, 144)] + [(2, C, 32, 32) for C in (72, 144)] + [(1, C, 2, 1025) for C in (72, 144)]
             + [(1, C, 64, 64) for C in (72, 144)] + [(3, C, 2, 683) for C in (72, 144)]                     # 2, 2048, 2050, 4096, 4098
             + [(1, 144, 1, 1), (3, 144, 5, 7), (1, 144, 1, 1023), (1, 144, 25, 41), (1, 144, 1, 2047), (1, 144, 3, 683)])
BWD_FUSED_WRAP = [(1, 36, 512, 513), (1, 72, 256, 258), (1, 144, 256, 258), (1, 144, 181, 183)]
BWD_UNFUSED = ([(1, 36, 1, 2), (2, 36, 2, 3), (1, 36, 27, 38)]                       # reg<36,2,true>; HW = 1026: nchunk 2
               + [(1, 36, 1, 1), (1, 36, 1, 3), (2, 36, 5, 7)]                       # C = 36, HW odd: the generic backward
               + [(1, 72, 1, 1), (3, 72, 5, 7), (1, 72, 25, 41)]                     # reg<72,1,true>; HW = 1025: nchunk 2
               + [(1, 1, 1, 1), (2, 1, 3, 5), (2, 12, 7, 9), (1, 12, 1, 6), (3, 37, 1, 3), (1, 37, 17, 3313)])   # generic; HW = 56321: nchunk 56
BWD_LARGE = (1, 144, 512, 513)                                                       # reg<144,1,false>, nchunk 15

# backward with exactly 2 C nchunk floats: the unfused kernels on shapes the fused kernel covers
BWD_SHORT = [(2, 36, 8, 12), (1, 72, 5, 6), (2, 144, 6, 6), (3, 144, 5, 7), (1, 72, 32, 34)]
BWD_NOGX = [(2, 36, 8, 12), (1, 72, 5, 6), (2, 144, 6, 6), (2, 12, 7, 9), (1, 36, 27, 38), (1, 72, 25, 41)]
BWD_BF16 = [(2, 36, 8, 12), (1, 72, 5, 6), (2, 144, 6, 6), (3, 144, 5, 7), (3, 72, 2, 683)]
BWD2 = [(2, 36, 8, 12), (1, 72, 5, 6), (1, 144, 6, 6), (3, 144, 5, 7), (2, 36, 64, 64), (1, 72, 2, 1025)]
BWD2_UNSUPPORTED = [(1, 36, 2, 3), (1, 72, 1, 5), (2, 12, 7, 9)]

# one view case per kernel family: x, gy, gx (and y) one float inside larger buffers
VIEW_FWD = [(2, 36, 8, 12), (3, 72, 5, 7), (2, 37, 7, 9)]
VIEW_BWD = [((2, 36, 8, 12), "full"), ((1, 72, 5, 6), "full"), ((3, 144, 5, 7), "full"),      # fused VEC 4 / 2 / 1
            ((2, 36, 8, 12), "short"), ((1, 72, 5, 6), "short"), ((3, 144, 5, 7), "short"),   # reg VEC 2 / 1, quad
            ((2, 12, 7, 9), "full")]                                                          # generic, ln_wb_kernel
VIEW_BWD2 = [(2, 36, 8, 12)]

CLASSES = ("random", "offset", "zero", "constg", "scale_up", "scale_down")
MEASURED = ("offset", "constg")          # classes whose bar is max(project bar, 4 E32)


def hw(case):
    return case[2] * case[3]


def ws_short(case):
    B, C = case[:2]
    return 2 * C * wb_chunks(B, C, hw(case))


# --------------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------------
def rnd(seed, shape, scale=1.0):
    return (O.synthetic_batch(seed, shape) - 0.5) * (2 * scale)


def zero_pixels(HW):
    """bool [HW]: the stripe of pixels whose whole column is exactly 0 in class `zero`"""
    m = torch.zeros(HW, dtype=torch.bool)
    m[HW // 3: HW // 3 + max(1, HW // 4)] = True
    return m


def inputs(case, cls, dual=False, addend=True, seed=0):
    """fp32 CPU tensors of one case: x, w, b, gy [, addend] [, w2, b2, gy2]"""
    B, C, H, W = case
    shape = (B, C, H, W)
    assert cls in CLASSES
    if cls == "offset":
        x = 8.0 + rnd(seed + 7, shape, 1.0)
    else:
        x = rnd(seed + 7, shape, 2.0)
    if cls == "scale_up":
        x = x * 1e3
    elif cls == "scale_down":
        x = x * 1e-3
    elif cls == "zero":
        x.view(B, C, H * W)[:, :, zero_pixels(H * W)] = 0.0
    t = {"x": x, "w": 1 + rnd(seed + 8, (C,), 0.2), "b": rnd(seed + 9, (C,), 0.1)}
    plane = (B, 1, H, W) if cls == "constg" else shape
    t["gy"] = rnd(seed + 10, plane).expand(shape).contiguous()
    if cls == "constg":
        t["w"] = torch.ones(C)
    if addend:
        t["addend"] = rnd(seed + 58, shape)
    if dual:
        t["w2"] = torch.ones(C) if cls == "constg" else 1 + rnd(seed + 54, (C,), 0.3)
        t["b2"] = rnd(seed + 55, (C,), 0.2)
        t["gy2"] = rnd(seed + 57, plane).expand(shape).contiguous()
    return t


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


# --------------------------------------------------------------------------------------------------------------------------
# fp64 references (any device)
# --------------------------------------------------------------------------------------------------------------------------
def ln_fwd_ref(x, w, b, eps=EPS):
    """x [B,C,H,W], w, b [C], all fp64 -> y, mean [B,H,W], rstd [B,H,W], xhat"""
    assert x.dtype == torch.float64
    C = x.shape[1]
    u = x.sum(1, keepdim=True) / C
    d = x - u
    var = (d * d).sum(1, keepdim=True) / C
    rs = 1.0 / torch.sqrt(var + eps)
    xhat = d * rs
    y = w.view(1, C, 1, 1) * xhat + b.view(1, C, 1, 1)
    return y, u[:, 0], rs[:, 0], xhat


def ln_bwd_ref(x, w, gy, addend=None, w2=None, gy2=None, eps=EPS):
    """-> gx, gw, gb [, gw2, gb2]"""
    assert x.dtype == torch.float64 and gy.dtype == torch.float64
    C = x.shape[1]
    _, _, rs, xhat = ln_fwd_ref(x, w, w, eps)
    rs = rs[:, None]
    g = gy * w.view(1, C, 1, 1)
    if gy2 is not None:
        g = g + gy2 * w2.view(1, C, 1, 1)
    gx = rs * (g - g.sum(1, keepdim=True) / C - xhat * ((g * xhat).sum(1, keepdim=True) / C))
    if addend is not None:
        gx = gx + addend
    out = [gx, (gy * xhat).sum((0, 2, 3)), gy.sum((0, 2, 3))]
    if gy2 is not None:
        out += [(gy2 * xhat).sum((0, 2, 3)), gy2.sum((0, 2, 3))]
    return out


def reference(t, dual=False, addend=False, gy_bf16=False, device=None):
    """fp64 reference of everything the kernels produce for the fp32 inputs t -> dict of fp64 tensors"""
    d = {k: (v.to(device) if device is not None else v).double() for k, v in t.items()}
    if gy_bf16:
        d["gy"] = bf16_round(t["gy"]).to(d["x"].device).double()
    r = {}
    r["y"], r["mean"], r["rstd"], _ = ln_fwd_ref(d["x"], d["w"], d["b"])
    if dual:
        r["y2"] = ln_fwd_ref(d["x"], d["w2"], d["b2"])[0]
        r["gx"], r["gw"], r["gb"], r["gw2"], r["gb2"] = ln_bwd_ref(d["x"], d["w"], d["gy"], d["addend"] if addend else None, d["w2"], d["gy2"])
    else:
        r["gx"], r["gw"], r["gb"] = ln_bwd_ref(d["x"], d["w"], d["gy"], d["addend"] if addend else None)
    return r


def oracle_eval(t, dtype, dual=False, addend=False):
    """the oracle's LayerNorm and its autograd in `dtype` on the CPU -> the same dict as reference()"""
    x, w, b = (t[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "b"))
    r = {}
    outs, grads = [O.layernorm_cf(x, w, b, EPS)], [t["gy"].to(dtype)]
    if dual:
        w2, b2 = (t[k].to(dtype).clone().requires_grad_(True) for k in ("w2", "b2"))
        outs.append(O.layernorm_cf(x, w2, b2, EPS))
        grads.append(t["gy2"].to(dtype))
    if addend:
        outs.append(x * 1.0)
        grads.append(t["addend"].to(dtype))
    torch.autograd.backward(outs, grads)
    with torch.no_grad():
        u = x.mean(1, keepdim=True)
        r["mean"] = u[:, 0]
        r["rstd"] = (1.0 / torch.sqrt((x - u).pow(2).mean(1, keepdim=True) + EPS))[:, 0]
    r["y"], r["gx"], r["gw"], r["gb"] = outs[0].detach(), x.grad, w.grad, b.grad
    if dual:
        r["y2"], r["gw2"], r["gb2"] = outs[1].detach(), w2.grad, b2.grad
    return r


# --------------------------------------------------------------------------------------------------------------------------
# criteria
# --------------------------------------------------------------------------------------------------------------------------
def err(name, got, ref):
    """the error figure of one output: max |got - ref|, for rstd max |got / ref - 1|"""
    got, ref = got.double(), ref.double()
    if got.numel() == 0:
        return 0.0
    if name == "rstd":
        return ((got - ref).abs() / ref.abs()).max().item()
    return (got - ref).abs().max().item()


def project_bar(name, ref):
    """2e-5 * max|ref| + 1e-6 against fp64 (rstd: relative, so max|ref| is 1)"""
    if ref.numel() == 0:
        return 0.0
    return 2e-5 * (1.0 if name == "rstd" else ref.abs().max().item()) + 1e-6


def e32(t, ref, dual=False):
    """error of the fp32 CPU evaluation of the oracle (forward and autograd) against the fp64 reference, per output of `ref`;
    `gx_add` is the input gradient with the residual's gradient added, which autograd forms as this one fp32 sum"""
    o = oracle_eval(t, torch.float32, dual, False)
    if "addend" in t:
        o["gx_add"] = o["gx"] + t["addend"]
    return {k: err(k, o[k].to(ref[k].device), ref[k]) for k in o if k in ref}


def bar(name, ref, cls, E32=None):
    p = project_bar(name, ref)
    return max(p, 4.0 * E32[name]) if cls in MEASURED else p
