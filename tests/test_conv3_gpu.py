"""The dense 3x3 convolution family against fp64: csrc/conv3.hip (fp32 MFMA forward / data gradient, weight gradient, replicate
fix), csrc/conv3_thin.hip (a side with four channels or fewer), csrc/conv3x.hip (bf16x3 forward / data gradient) and
csrc/conv3xw.hip (bf16x3 weight gradient), each compared with plain torch in fp64 on the CPU -- F.conv2d(padding=1),
F.conv_transpose2d for the data gradient, torch.nn.grad.conv2d_weight for the weight gradient, F.pad(mode="replicate") + a
valid convolution for the replicate forms; nothing of the project is on the reference side -- across the tilings the
launchers' cost models take.

Every case first asserts, through the host-only query cidnet_conv3x3_tiling, the tiling it is there for, so a retuned cost
model fails the case instead of silently moving it to another code path (test_case_tables_reach_their_tilings does the same
for every table without a GPU).  Every output is allocated NaN-filled, must be finite after the call, and a second call into
fresh NaN-filled buffers must be bit-identical.  Criteria: fp32 paths and bf16x3 with three levels, test_ops_gpu.close
(max|out - ref| <= 2e-5 max|ref| + 1e-6); bf16x3 forward with three levels additionally no worse than 1.5 x the fp32-MFMA
kernel's error; bf16x3 forward level modes 3e-6 max|ref| + 1e-6 against the fp64 convolution of the bf16-rounded operands;
bf16x3 one-level weight gradient 1e-5 max|ref| + 1e-6 likewise.

Tilings reached (B x M x K x H x W; M = output channels / dY planes, K = input channels / X planes):

  conv3_kernel (fp32 forward / data gradient), TILES and the sweeps
    LOGX 4 / 3 / 2 at tpb 1         1x12x12 at 8x16 / 9x16 / 17x16
    tpb 2, LOGX 2 / 3 / 4           4x12x12x289x196 (10 row tiles: exact), 4x12x12x225x260 (15: ragged), 4x12x12x257x228 (33: ragged)
    tpb 3                           3x12x12x417x388 (LOGX 2, 14 row tiles), 3x100x12x225x228 (LOGX 4, 29, blocks of 36 = (2,1))
    tpb 4                           3x100x12x417x196 (LOGX 2, 14 row tiles, blocks of 36 = (2,1))
    (MT, LEFT) x nmb                M 5, 13 -> (1,0); 17 -> (1,1); 21 -> (1,2); 29, 32 -> (2,0); 33 -> (2,1); 37 -> (3,0);
                                    50 -> (2,0) x 2 (18 live rows in the last); 97 -> (2,1) x 3; 145 -> (3,0) x 4 (1 live row),
                                    each with K 5 (a k-group that is not full), 12, 36, 37 and 72 (the K > 36 re-staging path)
    plane edges                     W 8, 9, 13, 63, 65 and NARROW W 5, 7, each at H 1, 2, 3; plain / flip x zero / replicate
    slices                          x_bs, y_bs and r_bs wider than the planes the call covers
  conv3_wgrad_kernel (fp32 weight gradient)
    input-channel tiles             N 8 (padded, N < 16), 16 (nfull 1), 20 (ngrp 1), 24 (ngrp 2), 28 (padded), 36 (2 + ngrp 1), 44
                                    (padded), each with every M above
    rows per chunk                  rr = H single chunk (H 1, 7, 14); rr 8 last 7 (H 15), last 1 (H 57); rr 9 last 8 (H 17); rr 10
                                    last 9 (H 19); work items 1, 2, 3, 6, 16, 24 (not multiples of 4 among them)
    narrow kernel                   W 1, 5, 7
  conv3_thin.hip
    M-side kernel                   M 1 (8-row strips), 2, 3, 4 (4-row strips) x K 1, 4, 5, 36, 85, 86, 144, 256; dynamic LDS up to
                                    98,304 B (M 4, K 256), above 64 KB from K 86 (M 4) and K 200 (M 3)
    K-side kernel                   K 1, 2, 3, 4 x M 5, 36, 256 (8-row strips)
    strips                          H 1, 4, 5, 8, 9, 17 x W 3, 5, 7 (NARROW), 8, 9, 66: single, exact and ragged last strips
    weight gradients                both kinds at every (M, K) above; 16-row strips, 2 chunks at 17x516 (258 strip items)
  conv3x_kernel (bf16x3 forward / data gradient)
    persistent loop, remap          1x100x36x50x780 and 1x100x72x49x779: 525 work items on 512 blocks; 1x100x36x9x5473 with one
                                    activation level: 1032 on 1024 blocks
    one item per block              27 items (no remap), 16 items (remap), kchunks 2 and 4, M 1, 47, 49, W 1, 2, 3, H 1
  conv3xw_kernel (bf16x3 weight gradient)
    nt 1                            W 4, 5, 31, 33 with H % 4 = 1, 2, 3, 1
    nt 2 and 3 in one launch        1x144x144x12x352 (33 tiles on 16 blocks per pair), 1x144x144x13x350 with one level (44 tiles)
    nt 4 and 5 in one launch        1x288x144x12x352 (33 tiles on 8 blocks per pair), 1x288x144x11x350 with one level
    more than 256 tiles, one pair   2x36x36x36x480 (270 tiles on 256 blocks: nt 1 and 2)

The thin M-side launches above 64 KB of dynamic LDS (M 4 with K >= 86, M 3 with K >= 200) run without raising the kernel's
dynamic-LDS limit; the M 3 / M 4 cases with K 86, 144 and 256 are the ones that tell whether that is enough on the device.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ops_gpu import close  # noqa: E402

gpu = pytest.mark.gpu          # the test that only reads the case tables through the host-side query carries no mark

NAN = float("nan")
FIELDS = (("thin", "MT", "LEFT", "nmb", "LOGX", "tpb", "narrow", "ntiles", "xt", "gy"),
          ("path", "MT", "LEFT", "nmb", "nfull", "ngrp", "rr", "last", "chunks", "nitems"),
          ("kside", "rows", "nstrips", "last", "lds"),
          ("chunks", "rows", "nstrips", "last"),
          ("tiles_x", "tiles_y", "mchunks", "kchunks", "nwork", "grid", "remap", "maxitems"),
          ("pairs", "nblk", "ntiles", "nt_min", "nt_max"))
FWD, WGRAD, THIN, THIN_WGRAD, X3, X3W = range(6)


def tiling(kind, B, M, K, H, W, levels=3):
    from hvi_cidnet_amd._lib import lib
    out = (ctypes.c_int * 10)(*([-1] * 10))
    rc = lib().raw("cidnet_conv3x3_tiling")(kind, B, M, K, H, W, levels, out, 10)
    assert rc == 0, (kind, B, M, K, H, W, levels, rc)
    return dict(zip(FIELDS[kind], out))


def expect(kind, shape, levels=3, **want):
    t = tiling(kind, *shape, levels)
    got = {k: t[k] for k in want}
    assert got == want, (kind, shape, got, want)
    return t


# (MT, LEFT, nmb) of the output-channel split, shared by the fp32 forward and weight-gradient kernels
SPLIT = {5: (1, 0, 1), 13: (1, 0, 1), 17: (1, 1, 1), 21: (1, 2, 1), 29: (2, 0, 1), 32: (2, 0, 1), 33: (2, 1, 1), 37: (3, 0, 1),
         50: (2, 0, 2), 97: (2, 1, 3), 145: (3, 0, 4)}
KS = (5, 12, 36, 37, 72)


# ---------------------------------------------------------------------------------------------------------------------
# references: plain torch, fp64, CPU
# ---------------------------------------------------------------------------------------------------------------------
def rand(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def ref_conv(x, wt, flip, rep):
    """x (B, K, H, W); wt (M, K, 3, 3), or for flip the forward layer's weight (K, M, 3, 3) whose data gradient is taken"""
    if rep:
        wk = wt.transpose(0, 1).flip(2, 3) if flip else wt
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), wk)
    return F.conv_transpose2d(x, wt, padding=1) if flip else F.conv2d(x, wt, padding=1)


def ref_wgrad(x, gy, rep):
    M, N = gy.shape[1], x.shape[1]
    if rep:
        return torch.nn.grad.conv2d_weight(F.pad(x, (1, 1, 1, 1), mode="replicate"), (M, N, 3, 3), gy)
    return torch.nn.grad.conv2d_weight(x, (M, N, 3, 3), gy, padding=1)


def conv_inputs(seed, B, M, K, H, W, flip, add):
    x = rand(seed, B, K, H, W)
    wt = rand(seed + 1, *((K, M, 3, 3) if flip else (M, K, 3, 3)), scale=1.0 / (3 * K ** 0.5))
    r = rand(seed + 2, B, M, H, W) if add else None
    return x, wt, r


# ---------------------------------------------------------------------------------------------------------------------
# the raw ABI
# ---------------------------------------------------------------------------------------------------------------------
def twice(dev, call, *shapes):
    """run `call` on fresh NaN-filled fp32 outputs twice: finite everywhere, bit-identical between the runs"""
    runs = []
    for _ in range(2):
        bufs = [torch.full(shape, NAN, device=dev) for shape in shapes]
        call(*bufs)
        runs.append(bufs)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert bool(torch.isfinite(a).all()), "elements left unwritten or not finite"
        assert torch.equal(a, b), "two runs differ"
    return runs[0]


def k_conv(x, wt, r, y, flip, rep, B, M, K, H, W, x_bs=None, r_bs=None, y_bs=None, x_off=0, r_off=0, y_off=0):
    """cidnet_conv3x3_add: the fp32 kernels (MFMA, or the streaming ones when a side has four channels or fewer)"""
    from hvi_cidnet_amd import ops
    w_ms, w_ks = (9, 9 * M) if flip else (9 * K, 9)
    ops.lib().call("cidnet_conv3x3_add", ops._pe(x, x_off), K * H * W if x_bs is None else x_bs, ops._p(wt), w_ms, w_ks, int(flip),
                   int(rep), None if r is None else ops._pe(r, r_off), M * H * W if r_bs is None else r_bs, ops._pe(y, y_off),
                   M * H * W if y_bs is None else y_bs, B, M, K, H, W, ops._stream())


def k_wgrad(gy, x, dw, rep, B, M, N, H, W):
    """cidnet_conv3x3_wgrad with a NaN-filled workspace of exactly the size the library asks for"""
    from hvi_cidnet_amd import ops
    n = ops._raw("cidnet_conv3x3_wgrad_ws_floats", B, M, N, H, W)
    ws = torch.full((max(n, 1),), NAN, device=x.device)
    ops.lib().call("cidnet_conv3x3_wgrad", ops._p(gy), M * H * W, ops._p(x), N * H * W, int(rep), ops._p(dw), ops._p(ws), n, B, M, N,
                   H, W, ops._stream())


def k_x3(x, wt, r, y, flip, B, M, K, H, W, wl, xl):
    """cidnet_conv3x3_bf16x3_prep + _pre_lv"""
    from hvi_cidnet_amd import ops
    w_ms, w_ks = (9, 9 * M) if flip else (9 * K, 9)
    n = ops._raw("cidnet_conv3x3_bf16x3_ws_floats", M, K)
    ws = torch.full((n,), NAN, device=x.device)
    ops.lib().call("cidnet_conv3x3_bf16x3_prep", ops._p(wt), w_ms, w_ks, int(flip), ops._p(ws), n, M, K, ops._stream())
    ops.lib().call("cidnet_conv3x3_bf16x3_pre_lv", ops._p(x), K * H * W, ops._p(ws), ops._p(r), M * H * W, ops._p(y), M * H * W, B, M, K,
                   H, W, wl, xl, ops._stream())


def k_x3w(gy, x, dw, B, M, N, H, W, levels):
    from hvi_cidnet_amd import ops
    n = ops._raw("cidnet_conv3x3_wgrad_bf16x3_ws_floats", B, M, N, H, W)
    ws = torch.full((n,), NAN, device=x.device)
    ops.lib().call("cidnet_conv3x3_wgrad_bf16x3_lv", ops._p(gy), M * H * W, ops._p(x), N * H * W, ops._p(dw), ops._p(ws), n, B, M, N, H,
                   W, levels, ops._stream())


def check_conv(dev, seed, B, M, K, H, W, flip, rep, add, what=""):
    x, wt, r = conv_inputs(seed, B, M, K, H, W, flip, add)
    ref = ref_conv(x.double(), wt.double(), flip, rep)
    if add:
        ref = ref + r.double()
    xd, wd, rd = x.to(dev), wt.to(dev), None if r is None else r.to(dev)
    y, = twice(dev, lambda y: k_conv(xd, wd, rd, y, flip, rep, B, M, K, H, W), (B, M, H, W))
    close(y, ref, what=f"{what} {B}x{M}x{K}x{H}x{W} flip={int(flip)} rep={int(rep)} add={int(add)}")


def check_wgrad(dev, seed, B, M, N, H, W, rep, what=""):
    x, gy = rand(seed, B, N, H, W), rand(seed + 1, B, M, H, W)
    ref = ref_wgrad(x.double(), gy.double(), rep)
    xd, gd = x.to(dev), gy.to(dev)
    dw, = twice(dev, lambda dw: k_wgrad(gd, xd, dw, rep, B, M, N, H, W), (M, N, 3, 3))
    close(dw, ref, what=f"{what} wgrad {B}x{M}x{N}x{H}x{W} rep={int(rep)}")


# ---------------------------------------------------------------------------------------------------------------------
# case tables (shape, what the query must report, variant)
# ---------------------------------------------------------------------------------------------------------------------
# fp32 forward tiles: (B, M, K, H, W), expected, (flip, rep, add)
TILES = [((1, 12, 12, 8, 16), dict(LOGX=4, tpb=1, ntiles=1), (0, 0, 0)),
         ((1, 12, 12, 9, 16), dict(LOGX=3, tpb=1, ntiles=1), (1, 0, 1)),
         ((1, 12, 12, 17, 16), dict(LOGX=2, tpb=1, ntiles=1), (0, 1, 0)),
         ((4, 12, 12, 289, 196), dict(LOGX=2, tpb=2, ntiles=10, gy=5), (0, 0, 1)),
         ((4, 12, 12, 225, 260), dict(LOGX=3, tpb=2, ntiles=15, gy=8), (1, 0, 0)),
         ((4, 12, 12, 257, 228), dict(LOGX=4, tpb=2, ntiles=33, gy=17), (0, 1, 0)),
         ((3, 12, 12, 417, 388), dict(LOGX=2, tpb=3, ntiles=14, gy=5), (0, 0, 0)),
         ((3, 100, 12, 225, 228), dict(MT=2, LEFT=1, nmb=3, LOGX=4, tpb=3, ntiles=29, gy=10), (0, 0, 1)),
         ((3, 100, 12, 417, 196), dict(MT=2, LEFT=1, nmb=3, LOGX=2, tpb=4, ntiles=14, gy=4), (1, 1, 0))]
EDGE_W = (8, 9, 13, 63, 65, 5, 7)
EDGE_H = (1, 2, 3)
# fp32 weight gradient rows: (B, M, N, H, W), expected, replicate
WG_ROWS = [((1, 12, 12, 1, 40), dict(rr=1, last=1, chunks=1, nitems=2), 0),
           ((2, 36, 36, 7, 70), dict(rr=7, last=7, chunks=1, nitems=3, ngrp=1), 1),
           ((1, 12, 12, 14, 8), dict(rr=14, last=14, chunks=1, nitems=1), 0),
           ((2, 36, 36, 15, 70), dict(rr=8, last=7, chunks=2, nitems=6, ngrp=1), 0),
           ((1, 12, 20, 57, 40), dict(rr=8, last=1, chunks=4, nitems=16, ngrp=1), 1),
           ((1, 12, 12, 17, 40), dict(rr=9, last=8, chunks=1, nitems=4), 0),
           ((1, 50, 24, 19, 70), dict(rr=10, last=9, chunks=2, nitems=6, ngrp=2, nmb=2), 1),
           ((1, 12, 12, 57, 70), dict(rr=8, last=1, chunks=6, nitems=24), 0)]
WG_N = {8: (1, 0), 16: (1, 0), 20: (1, 1), 24: (1, 2), 28: (2, 0), 36: (2, 1), 44: (3, 0)}     # N -> (nfull, ngrp)
WG_NARROW = [((2, 12, 20, 5, 5), 0), ((1, 37, 8, 3, 7), 1), ((1, 5, 5, 4, 1), 1), ((2, 13, 36, 1, 7), 0)]
THIN_M_K = (1, 4, 5, 36, 85, 86, 144, 256)
THIN_K_M = (5, 36, 256)
STRIP_H = (1, 4, 5, 8, 9, 17)
STRIP_W = (3, 5, 7, 8, 9, 66)
# bf16x3 forward: (B, M, K, H, W), (flip, add), (w levels, x levels), expected
X3_CASES = [((1, 100, 36, 50, 780), (0, 1), (3, 3), dict(nwork=525, grid=512, remap=1, maxitems=2, mchunks=3)),
            ((1, 100, 72, 49, 779), (1, 0), (3, 3), dict(nwork=525, grid=512, remap=1, maxitems=2, kchunks=2)),
            ((1, 100, 36, 9, 5473), (0, 1), (3, 1), dict(nwork=1032, grid=1024, remap=1, maxitems=2)),
            ((1, 100, 36, 9, 5473), (1, 0), (1, 1), dict(nwork=1032, grid=1024, remap=1, maxitems=2)),
            ((1, 100, 36, 17, 65), (0, 0), (3, 3), dict(nwork=27, grid=27, remap=0, maxitems=1)),
            ((1, 100, 36, 17, 65), (1, 1), (3, 1), dict(nwork=27, grid=27, remap=0, maxitems=1)),
            ((2, 49, 36, 15, 34), (1, 1), (3, 3), dict(nwork=16, grid=16, remap=1, maxitems=1, mchunks=2)),
            ((2, 49, 72, 15, 34), (0, 1), (1, 1), dict(nwork=16, grid=16, remap=1, kchunks=2)),
            ((2, 49, 72, 15, 34), (1, 0), (3, 1), dict(nwork=16, grid=16, remap=1, kchunks=2)),
            ((1, 47, 72, 9, 33), (0, 1), (3, 3), dict(nwork=4, kchunks=2, mchunks=1)),
            ((1, 47, 144, 7, 35), (1, 0), (3, 3), dict(nwork=2, kchunks=4, mchunks=1)),
            ((1, 1, 144, 1, 3), (1, 0), (3, 3), dict(nwork=1, kchunks=4)),
            ((1, 49, 36, 1, 2), (0, 1), (3, 3), dict(nwork=2, mchunks=2)),
            ((3, 47, 36, 7, 1), (0, 0), (3, 3), dict(nwork=3, remap=0)),
            ((3, 47, 36, 7, 1), (0, 1), (1, 1), dict(nwork=3, remap=0))]
# bf16x3 weight gradient: (B, M, N, H, W), levels, expected
X3W_CASES = [((1, 36, 36, 5, 4), 3, dict(nt_min=1, nt_max=1)),
             ((1, 72, 36, 6, 5), 3, dict(nt_min=1, nt_max=1, pairs=2)),
             ((1, 36, 72, 7, 31), 1, dict(nt_min=1, nt_max=1, pairs=2)),
             ((2, 36, 36, 9, 33), 3, dict(nt_min=1, nt_max=1, ntiles=12)),
             ((1, 144, 144, 12, 352), 3, dict(pairs=16, nblk=16, ntiles=33, nt_min=2, nt_max=3)),
             ((1, 144, 144, 13, 350), 1, dict(pairs=16, nblk=16, ntiles=44, nt_min=2, nt_max=3)),
             ((1, 288, 144, 12, 352), 3, dict(pairs=32, nblk=8, ntiles=33, nt_min=4, nt_max=5)),
             ((1, 288, 144, 11, 350), 1, dict(pairs=32, nblk=8, ntiles=33, nt_min=4, nt_max=5)),
             ((2, 36, 36, 36, 480), 3, dict(pairs=1, nblk=256, ntiles=270, nt_min=1, nt_max=2))]


def thin_m_expect(M, K, H):
    rows = 8 if M == 1 else 4
    return dict(kside=0, rows=rows, nstrips=-(-H // rows), last=H - (-(-H // rows) - 1) * rows,
                lds=K * M * 48 + 3 * rows * M * 1024)


def test_case_tables_reach_their_tilings():
    """every table above, through the host-only query alone (no GPU): a retuned cost model fails here first"""
    for shape, want, _ in TILES:
        expect(FWD, shape, thin=0, narrow=0, **want)
    for M, (mt, left, nmb) in SPLIT.items():
        for K in KS:
            expect(FWD, (2, M, K, 5, 13), thin=0, MT=mt, LEFT=left, nmb=nmb)
            assert nmb * (16 * mt + 4 * left) >= M > (nmb - 1) * (16 * mt + 4 * left)
        for N, (nfull, ngrp) in WG_N.items():
            expect(WGRAD, (2, M, N, 9, 13), path=0, MT=mt, LEFT=left, nmb=nmb, nfull=nfull, ngrp=ngrp, rr=9, nitems=1)
    assert {v[:2] for v in SPLIT.values()} == {(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0)}      # every instantiation
    for W in EDGE_W:
        for H in EDGE_H:
            expect(FWD, (2, 20, 12, H, W), thin=0, MT=1, LEFT=1, narrow=int(W < 8), ntiles=1)
    for shape, want, _ in WG_ROWS:
        expect(WGRAD, shape, path=0, **want)
    for shape, _ in WG_NARROW:
        expect(WGRAD, shape, path=1)
    for M in (1, 2, 3, 4):
        for K in THIN_M_K:
            t = expect(THIN, (2, M, K, 9, 9), **thin_m_expect(M, K, 9))
            assert (t["lds"] > 65536) == ((M == 4 and K >= 86) or (M == 3 and K >= 200))
            expect(FWD, (2, M, K, 9, 9), thin=1)
            expect(WGRAD, (2, M, K, 9, 9), path=2, chunks=1)
    assert tiling(THIN, 1, 4, 256, 9, 9)["lds"] == 98304 and tiling(THIN, 1, 3, 200, 9, 9)["lds"] > 65536
    for K in (1, 2, 3, 4):
        for M in THIN_K_M:
            expect(THIN, (2, M, K, 9, 9), kside=1, rows=8, nstrips=2, last=1, lds=M * K * 48)
    for H in STRIP_H:
        for W in STRIP_W:
            expect(THIN, (1, 1, 5, H, W), **thin_m_expect(1, 5, H))
            expect(THIN, (1, 3, 5, H, W), **thin_m_expect(3, 5, H))
            expect(THIN, (1, 5, 3, H, W), kside=1, rows=8, nstrips=-(-H // 8), last=H - (-(-H // 8) - 1) * 8)
            expect(THIN_WGRAD, (1, 3, 5, H, W), chunks=1, rows=16, nstrips=-(-H // 16), last=H - (-(-H // 16) - 1) * 16)
    expect(THIN_WGRAD, (1, 3, 36, 17, 516), chunks=2, rows=16, nstrips=2, last=1)
    for shape, _, (wl, xl), want in X3_CASES:
        expect(X3, shape, levels=xl, **want)
    for shape, lv, want in X3W_CASES:
        expect(X3W, shape, levels=lv, **want)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 MFMA forward / data gradient
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,want,variant", TILES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 5 else None)
def test_fp32_forward_tile_shapes(dev, shape, want, variant):
    """conv3_kernel at every tile width, with 1 to 4 row tiles per block (the `tile < tile_end` loop and its ragged end)"""
    expect(FWD, shape, thin=0, narrow=0, **want)
    check_conv(dev, 100, *shape, *variant, what="tiles")


@gpu
@pytest.mark.parametrize("M", sorted(SPLIT))
def test_fp32_forward_channel_splits(dev, M):
    """every (MT, LEFT) instantiation, M not a multiple of 4, partly empty last m-blocks; K 5 (a k-group that is not full),
    12, 36, 37 and 72 (re-staging); forward and data-gradient forms, zero and replicate padding, with and without the addend"""
    mt, left, nmb = SPLIT[M]
    for i, K in enumerate(KS):
        expect(FWD, (2, M, K, 5, 13), thin=0, MT=mt, LEFT=left, nmb=nmb)
        check_conv(dev, 200 + M + K, 2, M, K, 5, 13, flip=False, rep=bool(i & 1), add=bool(i & 2), what="split")
        check_conv(dev, 300 + M + K, 2, M, K, 5, 13, flip=True, rep=not (i & 1), add=not (i & 2), what="split")


@gpu
@pytest.mark.parametrize("W", EDGE_W)
def test_fp32_forward_plane_edges(dev, W):
    """widths around the 4-pixel quad and the 64-pixel tile, the NARROW instantiation (W < 8), one to three rows"""
    for H in EDGE_H:
        expect(FWD, (2, 20, 12, H, W), thin=0, MT=1, LEFT=1, narrow=int(W < 8), ntiles=1)
        for flip in (False, True):
            for rep in (False, True):
                check_conv(dev, 400 + W + H, 2, 20, 12, H, W, flip, rep, add=(H == 2) != flip, what="edges")


@gpu
@pytest.mark.parametrize("B,Co,Ci,H,W", [(2, 20, 12, 1, 9), (1, 12, 20, 5, 1), (1, 13, 5, 3, 8), (2, 36, 36, 9, 13), (1, 37, 12, 2, 5)])
def test_fp32_replicate_data_gradient(dev, B, Co, Ci, H, W):
    """the data gradient of ReplicationPad2d(1) + valid conv = the zero-pad data gradient (flip) + the border fix, against
    autograd through F.pad(mode="replicate") in fp64"""
    from hvi_cidnet_amd import ops
    x, w, gy = rand(1, B, Ci, H, W), rand(2, Co, Ci, 3, 3, scale=1.0 / (3 * Ci ** 0.5)), rand(3, B, Co, H, W)
    xr = x.double().requires_grad_(True)
    F.conv2d(F.pad(xr, (1, 1, 1, 1), mode="replicate"), w.double()).backward(gy.double())
    wd, gd = w.to(dev), gy.to(dev)

    def call(dx):
        k_conv(gd, wd, None, dx, True, False, B, Ci, Co, H, W)
        ops.lib().call("cidnet_conv3x3_replicate_dgrad_fix", ops._p(gd), ops._p(wd), ops._p(dx), B, Co, Ci, H, W, ops._stream())
    dx, = twice(dev, call, (B, Ci, H, W))
    close(dx, xr.grad, what="replicate dgrad")


@gpu
@pytest.mark.parametrize("M,K,add", [(20, 12, True), (20, 12, False), (50, 37, True), (3, 12, False), (12, 3, False)])
@pytest.mark.parametrize("flip,rep", [(False, False), (True, True)])
def test_fp32_forward_slices(dev, M, K, add, flip, rep):
    """x_bs / y_bs / r_bs: the call reads K planes out of a wider input, adds M planes of a wider addend and writes M planes
    of a wider output, whose other planes keep their contents (MFMA kernel, and both streaming kernels)"""
    B, H, W = 2, 6, 11
    expect(FWD, (B, M, K, H, W), thin=int(min(M, K) <= 4))
    HW = H * W
    x, wt, r = conv_inputs(500 + M, B, M, K, H, W, flip, add)
    ref = ref_conv(x.double(), wt.double(), flip, rep) + (r.double() if add else 0)
    xw = torch.full((B, K + 3, H, W), NAN, device=dev)
    xw[:, 2:2 + K] = x.to(dev)
    rw = None
    if add:
        rw = torch.full((B, M + 2, H, W), NAN, device=dev)
        rw[:, 1:1 + M] = r.to(dev)
    wd = wt.to(dev)
    outs = []
    for _ in range(2):
        yw = torch.full((B, M + 5, H, W), 7.25, device=dev)
        yw[:, 4:4 + M] = NAN
        k_conv(xw, wd, rw, yw, flip, rep, B, M, K, H, W, x_bs=(K + 3) * HW, r_bs=(M + 2) * HW, y_bs=(M + 5) * HW, x_off=2 * HW,
               r_off=HW, y_off=4 * HW)
        outs.append(yw)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][:, :4] == 7.25).all()) and bool((outs[0][:, 4 + M:] == 7.25).all()), "planes outside the slice were written"
    assert bool(torch.isfinite(outs[0]).all())
    close(outs[0][:, 4:4 + M], ref, what="slices")


# ---------------------------------------------------------------------------------------------------------------------
# fp32 MFMA weight gradient
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", sorted(WG_N))
def test_fp32_wgrad_channel_tiles(dev, N):
    """conv3_wgrad_kernel: full 16-wide input tiles, the NLEFT launch for a remainder of 1..8 (ngrp 1, 2), the padded tile
    otherwise; with every output-channel split"""
    nfull, ngrp = WG_N[N]
    for i, (M, (mt, left, nmb)) in enumerate(sorted(SPLIT.items())):
        expect(WGRAD, (2, M, N, 9, 13), path=0, MT=mt, LEFT=left, nmb=nmb, nfull=nfull, ngrp=ngrp, rr=9, nitems=1)
        check_wgrad(dev, 600 + M + N, 2, M, N, 9, 13, rep=bool((i + N // 4) & 1), what="tiles")


@gpu
@pytest.mark.parametrize("shape,want,rep", WG_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_fp32_wgrad_row_chunks(dev, shape, want, rep):
    """rows per chunk: the whole plane, 8 with last chunks of 1 and 7 rows, more than 8; work-item counts that do not fill the
    last block's four waves"""
    expect(WGRAD, shape, path=0, **want)
    check_wgrad(dev, 700, *shape, rep=bool(rep), what="rows")


@gpu
@pytest.mark.parametrize("shape,rep", WG_NARROW, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_fp32_wgrad_narrow(dev, shape, rep):
    expect(WGRAD, shape, path=1)
    check_wgrad(dev, 800, *shape, rep=bool(rep), what="narrow")


# ---------------------------------------------------------------------------------------------------------------------
# thin kernels
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", (1, 2, 3, 4))
def test_thin_m_side(dev, M):
    """c3_thin_m_kernel with 1 to 256 input planes (dynamic LDS up to 98,304 B: more than 64 KB at M 3 / K 256 and at M 4 /
    K 86, 144, 256), forward, flip and replicate, and the weight gradient of the same layer (dY thin: N <= 4 takes the n kernel)"""
    B, H, W = 2, 9, 9
    for i, K in enumerate(THIN_M_K):
        expect(THIN, (B, M, K, H, W), **thin_m_expect(M, K, H))
        check_conv(dev, 900 + K, B, M, K, H, W, flip=False, rep=bool(i & 1), add=False, what="thin m")
        check_conv(dev, 950 + K, B, M, K, H, W, flip=True, rep=not (i & 1), add=False, what="thin m")
        expect(WGRAD, (B, M, K, H, W), path=2, chunks=1)
        check_wgrad(dev, 970 + K, B, M, K, H, W, rep=bool(i & 2), what="thin m")


@gpu
@pytest.mark.parametrize("K", (1, 2, 3, 4))
def test_thin_k_side(dev, K):
    """c3_thin_k_kernel with 5 to 256 output planes, and the weight gradient of the same layer (X thin)"""
    B, H, W = 2, 9, 9
    for i, M in enumerate(THIN_K_M):
        expect(THIN, (B, M, K, H, W), kside=1, rows=8, nstrips=2, last=1, lds=M * K * 48)
        check_conv(dev, 1000 + M, B, M, K, H, W, flip=False, rep=bool(i & 1), add=False, what="thin k")
        check_conv(dev, 1050 + M, B, M, K, H, W, flip=True, rep=not (i & 1), add=False, what="thin k")
        expect(WGRAD, (B, M, K, H, W), path=2, chunks=1)
        check_wgrad(dev, 1070 + M, B, M, K, H, W, rep=not (i & 1), what="thin k")


@gpu
@pytest.mark.parametrize("W", STRIP_W)
def test_thin_strips(dev, W):
    """strip heights 8 (M 1, and the K side) and 4 (M 3) with single, exact and ragged last strips; the NARROW
    instantiations (W < 8); the weight gradients of both kinds on the same planes"""
    for H in STRIP_H:
        rep = bool((H + W) & 1)
        for M, K in ((1, 5), (3, 5), (5, 3)):
            if M <= 4:
                expect(THIN, (1, M, K, H, W), **thin_m_expect(M, K, H))
            else:
                expect(THIN, (1, M, K, H, W), kside=1, rows=8, nstrips=-(-H // 8), last=H - (-(-H // 8) - 1) * 8)
            check_conv(dev, 1100 + H, 1, M, K, H, W, flip=(M == 3), rep=rep, add=False, what="strips")
            expect(THIN_WGRAD, (1, M, K, H, W), chunks=1, rows=16, nstrips=-(-H // 16), last=H - (-(-H // 16) - 1) * 16)
            check_wgrad(dev, 1150 + H, 1, M, K, H, W, rep=not rep, what="strips")


@gpu
@pytest.mark.parametrize("M,N,rep", [(3, 36, False), (36, 3, True), (1, 5, True), (5, 1, False)])
def test_thin_wgrad_two_chunks(dev, M, N, rep):
    """258 strip items = two 256-item chunks per sample, the second nearly empty"""
    expect(THIN_WGRAD, (2, M, N, 17, 516), chunks=2, rows=16, nstrips=2, last=1)
    check_wgrad(dev, 1200, 2, M, N, 17, 516, rep=rep, what="two chunks")


# ---------------------------------------------------------------------------------------------------------------------
# bf16x3 forward / data gradient
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,variant,levels,want", X3_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) in (2, 5) else None)
def test_bf16x3_forward(dev, shape, variant, levels, want):
    """conv3x_kernel: blocks that walk several work items (LDS reuse behind the leading barrier, the XCD remap of the first
    item), ragged tiles and channel chunks, the k-chunk loop; three levels against fp64 (and no worse than 1.5 x the fp32-MFMA
    kernel), the bf16 level modes against the fp64 convolution of the rounded operands"""
    B, M, K, H, W = shape
    (flip, add), (wl, xl) = variant, levels
    expect(X3, shape, levels=xl, **want)
    x, wt, r = conv_inputs(1300 + M + K + H, B, M, K, H, W, flip, add)
    exact = ref_conv(x.double(), wt.double(), flip, False) + (r.double() if add else 0)
    xd, wd, rd = x.to(dev), wt.to(dev), None if r is None else r.to(dev)
    y, = twice(dev, lambda y: k_x3(xd, wd, rd, y, flip, B, M, K, H, W, wl, xl), (B, M, H, W))
    if (wl, xl) == (3, 3):
        close(y, exact, what="bf16x3")
        y32 = torch.full((B, M, H, W), NAN, device=dev)
        k_conv(xd, wd, rd, y32, flip, False, B, M, K, H, W)
        e3, e32 = (y.double().cpu() - exact).abs().max().item(), (y32.double().cpu() - exact).abs().max().item()
        assert e3 <= 1.5 * e32 + 1e-6 * exact.abs().max().item(), (e3, e32)
    else:
        ref = ref_conv(bf16_round(x), bf16_round(wt) if wl == 1 else wt.double(), flip, False) + (r.double() if add else 0)
        err = (y.double().cpu() - ref).abs().max().item()
        assert err <= 3e-6 * ref.abs().max().item() + 1e-6, err
        # and it is NOT the fp32 product: the rounding of the operands is visible (a silently ignored mode would pass above
        # only if rounding changed nothing)
        assert (y.double().cpu() - exact).abs().max().item() > 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# bf16x3 weight gradient
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,levels,want", X3W_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_bf16x3_wgrad(dev, shape, levels, want):
    """conv3xw_kernel: one to five tiles per block through the two alternating LDS buffers (from the third tile on a buffer
    is overwritten after use), blocks of one launch with different tile counts, ragged tiles; three levels and one"""
    B, M, N, H, W = shape
    expect(X3W, shape, levels=levels, **want)
    from hvi_cidnet_amd import ops
    assert ops._raw("cidnet_conv3x3_wgrad_bf16x3_ws_floats", B, M, N, H, W) == want.get("pairs", (M // 36) * (N // 36)) * \
        tiling(X3W, *shape)["nblk"] * 108 * 108
    x, gy = rand(1400 + W, B, N, H, W), rand(1401 + W, B, M, H, W)
    xd, gd = x.to(dev), gy.to(dev)
    dw, = twice(dev, lambda dw: k_x3w(gd, xd, dw, B, M, N, H, W, levels), (M, N, 3, 3))
    if levels == 3:
        close(dw, ref_wgrad(x.double(), gy.double(), False), what="bf16x3 wgrad")
    else:
        ref = ref_wgrad(bf16_round(x), bf16_round(gy), False)
        err = (dw.double().cpu() - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item() + 1e-6, err
