"""Host checks of tests/norm_ref.py: the fp64 formulas against the oracle's autograd, the case table against the dispatch of
csrc/norm.hip (every kernel instantiation its launchers name, every boundary tests/test_norm_gpu.py promises), the fixtures."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as R  # noqa: E402

NORM_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hvi-cidnet_amd", "csrc", "norm.hip")


@pytest.mark.parametrize("case", [(2, 5, 3, 4), (1, 36, 2, 2), (3, 12, 1, 5), (1, 1, 2, 3), (2, 72, 1, 1)])
@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("dual,addend", [(False, False), (False, True), (True, False), (True, True)])
def test_formulas_equal_oracle_autograd_in_fp64(case, cls, dual, addend):
    t = R.inputs(case, cls, dual=dual, addend=addend)
    ref = R.reference(t, dual=dual, addend=addend)
    orc = R.oracle_eval(t, torch.float64, dual=dual, addend=addend)
    assert set(orc) == set(ref)
    for k in ref:
        scale = max(ref[k].abs().max().item(), orc[k].abs().max().item(), 1e-300)
        if cls == "constg" and k == "gx" and not addend:
            scale = t["gy"].abs().max().item()                   # gx vanishes: relative to the terms that cancel
        assert (ref[k] - orc[k]).abs().max().item() <= 1e-12 * scale, (k, cls)


def test_bf16_gradient_reference_takes_the_rounded_values():
    t = R.inputs((1, 36, 2, 2), "random")
    a, b = R.reference(t, gy_bf16=True), R.reference(dict(t, gy=R.bf16_round(t["gy"])))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["gb"], R.reference(t)["gb"])


def _launched_kernels():
    """every kernel (with its template arguments) that a hipLaunchKernelGGL of norm.hip names, macros expanded"""
    src = open(NORM_HIP).read()
    names = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\(?\s*(\w+)\s*(<[^>]*>)?", src):
        names.add(m.group(1) + (m.group(2) or "").replace(" ", ""))
    out = set()
    for n in names:
        if "CC" in n:
            out |= {n.replace("CC", c) for c in re.findall(r"CIDNET_LN_FWD_H\((\d+)\)", src)}
        elif "CQ,VEC,LPP" in n:
            out |= {n.replace("CQ,VEC,LPP", "%s,%s,%s" % a) for a in re.findall(r"CIDNET_LN_BWD_H\((\d+), (\d+), (\d+)\)", src)}
        else:
            out.add(n)
    return out


def test_all_kernels_lists_what_the_launchers_name():
    assert _launched_kernels() == set(R.ALL_KERNELS)


def _reached():
    """{kernel: [Path, ...]} over the whole case table, through the dispatch restatement"""
    got = {}

    def add(p):
        assert not p.kernel.startswith("ERR"), p
        got.setdefault(p.kernel, []).append(p)

    for c in R.FWD_REG + R.FWD_GENERIC + R.FWD_WRAP + R.VIEW_FWD:
        add(R.fwd_path(c[0], c[1], R.hw(c)))
    for c in R.FWD_BF16:
        add(R.fwd_path(c[0], c[1], R.hw(c), y_dt=1))
    for c in R.FWD_DUAL:
        add(R.fwd_path(c[0], c[1], R.hw(c), dual=True))
    full = lambda c: R.bwd_ws_floats(c[1])
    for c in R.BWD_FUSED + R.BWD_FUSED_WRAP + R.BWD_UNFUSED + [R.BWD_LARGE]:
        add(R.path(c[0], c[1], R.hw(c), full(c)))
    for c in R.BWD_SHORT:
        add(R.path(c[0], c[1], R.hw(c), R.ws_short(c)))
    for c in R.BWD_NOGX:
        add(R.path(c[0], c[1], R.hw(c), R.ws_short(c), gx=False))
    for c in R.BWD_BF16:
        add(R.path(c[0], c[1], R.hw(c), full(c), gy_dt=1))
    for c in R.BWD2:
        add(R.path2(c[0], c[1], R.hw(c), R.bwd2_ws_floats(c[1])))
    for p in [q for v in got.values() for q in v]:
        if p.nchunk is not None:
            got.setdefault("ln_wb_reduce_kernel", []).append(p)
            if p.kernel != "ln_wb_kernel":
                got.setdefault("ln_wb_kernel", []).append(p)
        elif "fused" in p.kernel:
            got.setdefault("ln_wb2_reduce_kernel", []).append(p)
    return got


def test_case_table_reaches_every_kernel_and_boundary():
    got = _reached()
    assert set(got) - {k for k in got if k.endswith("+y2")} == set(R.ALL_KERNELS)
    assert {k for k in got if k.endswith("+y2")} == {"ln_fwd_reg_kernel<%d,1>+y2" % c for c in (36, 72, 144)}
    nblk = lambda k: {p.nblk for p in got[k]}
    trips = lambda k: {p.trips for p in got[k]}
    # grid-stride second trips: both forwards, all four fused backwards; the dual C = 36 kernel always makes two
    for k in ("ln_fwd_reg_kernel<36,1>", "ln_fwd_kernel", "ln_bwd_quad_fused_kernel<9,4,4>", "ln_bwd_quad_fused_kernel<9,2,8>",
              "ln_bwd_quad_fused_kernel<18,2,8>", "ln_bwd_quad_fused_kernel<18,1,8>"):
        assert {1, 2} <= trips(k), k
    assert trips("ln_bwd_quad_fused_kernel<9,2,4,true>") == {2}
    # ln_wb2_reduce_kernel's two-at-a-time loop: one row, the step's edges, the cap
    for k in ("ln_bwd_quad_fused_kernel<9,4,4>", "ln_bwd_quad_fused_kernel<9,2,8>", "ln_bwd_quad_fused_kernel<18,2,8>"):
        assert {1, 32, 33, 64, 65, 1024} <= nblk(k), k
    assert {1, 32, 33, 64, 65, 1024} <= nblk("ln_bwd_quad_fused_kernel<18,1,8>")
    assert {1, 32, 33, 64, 65, 1024} <= nblk("ln_wb2_reduce_kernel")
    assert {32, 33} <= nblk("ln_bwd_quad_fused_kernel<9,2,4,true>") | nblk("ln_bwd_quad_fused_kernel<9,2,8,true>")
    # ln_wb_kernel / ln_wb_reduce_kernel: one chunk, two, the caps ceil(2048 / C) for C = 144 and C = 37
    chunks = lambda C: {p.nchunk for p, c in _wb_cases() if c[1] == C}
    assert {1, 2} <= chunks(36) and {1, 2} <= chunks(72) and {1, 15} <= chunks(144) and {1, 56} <= chunks(37)
    assert 15 == -(-2048 // 144) and 56 == -(-2048 // 37)
    assert R.path(*_bcw(R.BWD_LARGE), R.bwd_ws_floats(144)) == R.Path("ln_bwd_reg_kernel<144,1,false>", 1026, 15, 1)
    # the unfused register kernels both ways: by shape under the full workspace, by a short workspace on fused shapes
    for k, by_shape, by_ws in (("ln_bwd_reg_kernel<36,2,true>", R.BWD_UNFUSED, R.BWD_SHORT), ("ln_bwd_reg_kernel<72,1,true>", R.BWD_UNFUSED, R.BWD_SHORT)):
        assert any(R.path(*_bcw(c), R.bwd_ws_floats(c[1])).kernel == k for c in by_shape)
        assert any(R.path(*_bcw(c), R.ws_short(c)).kernel == k for c in by_ws)
    for c in R.BWD_SHORT:
        assert R.ws_short(c) < 2 * c[1] * R.K_FUSED_BLOCKS and R.typed_supported(*_bcw(c))
        assert R.path(*_bcw(c), R.ws_short(c) - 1).kernel == "ERR_WS"
        assert "fused" in R.path(*_bcw(c), R.bwd_ws_floats(c[1])).kernel
    assert any(c[0] > 1 and R.hw(c) % 2 for c in R.BWD_SHORT if c[1] == 144)           # quad kernel, B > 1, odd plane
    assert any(R.path(*_bcw(c), R.ws_short(c)).nblk > 1 for c in R.BWD_SHORT if c[1] == 144)
    # planes of 1, 2, 3 pixels and B > 1 on odd planes in the register forward; tails 1, 2, 3 and none in the generic kernels
    for C in (36, 72, 144):
        assert {1, 2, 3} <= {R.hw(c) for c in R.FWD_REG if c[1] == C and c[0] == 1}
        assert any(c[0] == 3 and R.hw(c) % 2 for c in R.FWD_REG if c[1] == C)
    assert {c[1] for c in R.FWD_GENERIC} == {1, 2, 35, 37, 73, 145}
    assert {R.hw(c) % 4 for c in R.FWD_GENERIC} == {0, 1, 2, 3}
    assert {R.hw(c) % 4 for c in R.BWD_UNFUSED if R.path(*_bcw(c), R.bwd_ws_floats(c[1])).kernel == "ln_bwd_kernel"} == {1, 2, 3}
    assert {c[1] for c in R.BWD_UNFUSED if R.path(*_bcw(c), R.bwd_ws_floats(c[1])).kernel == "ln_bwd_kernel"} == {1, 12, 36, 37}
    assert any(c[1] == 144 and c[0] == 3 and R.hw(c) % 2 for c in R.BWD_FUSED)          # <18,1,8> with B > 1
    assert any(c[1] == 144 and R.hw(c) == 1 for c in R.BWD_FUSED)
    # a parameter-gradient-only call with nchunk > 1; every view family
    assert {1, 2} <= {R.path(*_bcw(c), R.ws_short(c), gx=False).nchunk for c in R.BWD_NOGX}
    fam = {R.path(*_bcw(c), R.bwd_ws_floats(c[1]) if ws == "full" else R.ws_short(c)).kernel for c, ws in R.VIEW_BWD}
    assert fam == {"ln_bwd_quad_fused_kernel<9,4,4>", "ln_bwd_quad_fused_kernel<9,2,8>", "ln_bwd_quad_fused_kernel<18,1,8>",
                   "ln_bwd_reg_kernel<36,2,true>", "ln_bwd_reg_kernel<72,1,true>", "ln_bwd_quad_kernel<36,true>", "ln_bwd_kernel"}
    assert {R.fwd_path(*_bcw(c)).kernel for c in R.VIEW_FWD} == {"ln_fwd_reg_kernel<36,1>", "ln_fwd_reg_kernel<72,1>", "ln_fwd_kernel"}


def _bcw(c):
    return c[0], c[1], R.hw(c)


def _wb_cases():
    for c in R.BWD_UNFUSED + [R.BWD_LARGE]:
        yield R.path(*_bcw(c), R.bwd_ws_floats(c[1])), c
    for c in R.BWD_SHORT + R.BWD_NOGX:
        yield R.path(*_bcw(c), R.ws_short(c)), c


def test_expected_support_and_errors_of_the_table():
    """what the GPU test asserts of cidnet_ln_cf_typed_supported / _dual_supported and of the error returns, stated once here"""
    for c in R.FWD_BF16 + R.FWD_DUAL + R.BWD_BF16 + R.BWD2 + R.BWD_SHORT:
        assert R.typed_supported(*_bcw(c)) == 1 and R.dual_supported(*_bcw(c)) == 1
    for c in R.FWD_UNSUPPORTED + R.BWD2_UNSUPPORTED:
        assert R.typed_supported(*_bcw(c)) == 0
        assert R.fwd_path(*_bcw(c), y_dt=1).kernel == "ERR_SHAPE" and R.fwd_path(*_bcw(c), dual=True).kernel == "ERR_SHAPE"
        assert R.path2(*_bcw(c), R.bwd2_ws_floats(c[1])).kernel == "ERR_SHAPE"
    assert {(c[1], R.hw(c)) for c in R.FWD_UNSUPPORTED} >= {(36, 6), (72, 5)} and any(c[1] == 12 for c in R.FWD_UNSUPPORTED)
    assert R.typed_supported(*_bcw(R.BWD_LARGE)) == 0
    assert R.fwd_path(1, 36, 4, y_dt=2).kernel == "ERR_ARG"
    for c in R.BWD_BF16:
        assert R.path(*_bcw(c), R.bwd_ws_floats(c[1]), gx=False, gy_dt=1).kernel == "ERR_SHAPE"
        assert R.path(*_bcw(c), R.ws_short(c), gy_dt=1).kernel == "ERR_SHAPE"
    assert {R.path(*_bcw(c), R.bwd_ws_floats(c[1]), gy_dt=1).kernel for c in R.BWD_BF16} == {
        "ln_bwd_quad_fused_kernel<%s,false,bf16_t>" % k for k in ("9,4,4", "9,2,8", "18,2,8", "18,1,8")}
    for c in R.BWD2:
        assert R.path2(*_bcw(c), R.bwd2_ws_floats(c[1]) - 1).kernel == "ERR_WS"


def test_zero_column_fixtures_hold_exact_zeros():
    every = (R.FWD_REG + R.FWD_GENERIC + R.FWD_BF16 + R.FWD_DUAL + R.BWD_FUSED + R.BWD_UNFUSED + R.BWD_SHORT + R.BWD_NOGX
             + R.BWD_BF16 + R.BWD2)
    for c in sorted(set(every)):
        B, C, H, W = c
        m = R.zero_pixels(H * W)
        assert 1 <= int(m.sum()) <= max(1, H * W // 4)
        x = R.inputs(c, "zero", addend=False)["x"].view(B, C, H * W)
        assert (x[:, :, m] == 0).all()
        assert H * W < 4 or (x[:, :, ~m] != 0).any(1).all()          # and the other columns are live
        ref = R.reference({"x": x.view(B, C, H, W), "w": torch.ones(C), "b": torch.zeros(C), "gy": torch.ones(B, C, H, W)})
        assert (ref["mean"].view(B, -1)[:, m] == 0).all() and (ref["y"].view(B, C, -1)[:, :, m] == 0).all()
        assert torch.allclose(ref["rstd"].view(B, -1)[:, m], torch.tensor(1e3, dtype=torch.float64), rtol=1e-12)


def test_constant_gradient_class_has_zero_input_gradient():
    for c in ((2, 36, 8, 12), (3, 144, 5, 7), (2, 12, 7, 9)):
        t = R.inputs(c, "constg", dual=True)
        assert (t["w"] == 1).all() and (t["w2"] == 1).all() and (t["gy"] == t["gy"][:, :1]).all()
        assert R.reference(t, dual=True)["gx"].abs().max().item() <= 1e-14
        assert torch.equal(R.reference(t, dual=True, addend=True)["gx"], R.reference(t, dual=True)["gx"] + t["addend"].double())
