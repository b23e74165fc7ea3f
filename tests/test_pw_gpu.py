"""The 1x1 convolution family against fp64: csrc/pw.hip (fp32-MFMA forward / data gradient in its split-K, register-resident,
LDS and tail forms, the NormUpsample epilogue, the weight gradient), csrc/pwx.hip (bf16x3 forward) and csrc/pwb.hip (fused
backward), each compared with plain torch in fp64 on the CPU -- torch.bmm / torch.einsum for the products,
F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) and F.prelu for the NormUpsample tail; nothing of the
project is on the reference side -- across the paths the dispatch takes.

Every case first asserts, through the host-only query cidnet_pw_plan, the plan it is there for, so a retuned threshold fails
the case instead of silently moving it to another kernel (test_case_tables_reach_their_plans does the same for every table
without a GPU).  Every output is allocated NaN-filled, must be finite after the call, and a second call into fresh buffers must
be bit-identical.  Tensors are passed as slices of wider buffers wherever the ABI has a stride (x_bs, y_bs, r_bs, w_bs,
dw_ld, gy_bs, gx_bs larger than what the call covers, and a front offset); everything outside the covered planes holds a
sentinel that must be unchanged afterwards.

Two criteria per case:
  exact    operands are small integers (X, R in [-8, 8], W in [-4, 4]; weight gradients shrink the ranges so that
           max|dY| max|X| B HW < 2^24), so every product and every partial sum in any order is an integer below 2^24: exact in
           fp32 and at every bf16 level.  The output must EQUAL the fp64 result (its bf16 rounding for bf16 outputs).  The bound
           is asserted on the reference side.  One wrong row, pixel, k-step or chunk anywhere in the plane fails it.
  rounded  random operands, weights scaled by 1 / sqrt(K), under the tolerances the suite already uses for each path:
           test_ops_gpu.close (2e-5 max|ref| + 1e-6) for the fp32-MFMA and three-level paths; 3e-6 max|ref| + 1e-6 against
           the fp64 product of the bf16-rounded operands for the one-level forward and 1e-5 max|ref| + 1e-6 for the one-level
           weight gradient; 2^-8 max|ref| + 1e-6 for bf16 outputs; the bf16x3 forward no worse than 3 x the fp32-MFMA kernel's
           own error + 2e-6 max|ref|; the fused backward no worse than 2 x the two separate kernels + 1e-6 max|ref|.
           (cidnet_pw_conv_up_prelu has only this one: its bilinear tap weights are not integers.)

Paths reached (B x M x K x HW; M = output channels / dY planes, K = input channels / X planes), all asserted in the case:

  pw_conv_rega_kernel (register-resident weights)
    (MT, LEFT, KS)                  (1,1,9) M 20, (2,1,9) M 36, (3,1,9) M 52, (3,0,9) M 96 x 2 blocks, (4,0,9) M 190 x 3, (5,0,9) M 72,
                                    each 2 x M x 36 x 1028; LEFT flips at M 33 (1 live row), 36 (4), 37 (5 -> a padded tile)
    KS 18                           K 37, 60: M 64 (2,0,18) x 2, M 95 (3,0,18) x 2, M 72 (5,0,18), M 36 (2,1,18)
    KS 24 (K 73..96 AND HW > 8192)  1x36x73x8196 (2,1,24), 1x48x96x8196 (3,0,24)
    k-step that is not full         K 1, 3, 5 at M 36
    store_heavy block target        72x36 -> 1024, 71x36 -> 512 (M >= 2 K fails), 190x36 -> 1024
    tpb 2 / 3, ragged last block    6x36x36x23808 (93 tiles, 47 blocks), 3x36x36x89600 (350 tiles, 117 blocks)
    tpb clamped at 8                1x4x4x921856 (3601 tiles, 451 blocks, the last walks one)
  tail kernel (pw_conv_kernel<TAIL>)
    streaming tile + tail launch    HW 257, 258, 259;  tail only (path 3): HW 1, 2, 3, 5, 255;  none: HW 256, 260
  pw_conv_splitk_kernel
    KSW 9 / 18 / 24                 K 64, 100 (9), 190 (18), 383, 384 (24) at 2 x 50 x K x 130
    two launches around K = 384     K 385 (second launch K = 1, KSW 9), 400 (9), 768 (24)
    MT 1, 2, 3 and m-blocks         M 10 (1), 20 (2), 50 (3 x 2 blocks, 2 live rows in the last), 100 (3 x 3 blocks)
                                    and MT 1 at KSW 18 (2x10x190x130), MT 2 at KSW 24 (2x20x384x61): all nine (MT, KSW)
    groups past the plane's end     HW 16, 61, 65, 130
    tpb 2                           2x144x100x8192 (128 groups x 3 m-blocks x 2)
    thresholds                      K 100: HW 8192 split-K, 8196 LDS;  K 400: HW 16384 split-K twice, 16388 LDS in two K chunks
  pw_conv_kernel (weight panel in LDS)
    MT 1 .. 6                       1x16 (1), 1x32 (2), 4x190 (3), 8x128 (4), 6x190 (5) x 100 x 8196; 2x96x100x65536 (6: 512 blocks)
    one panel, tpb 2, ragged        1x766x144x8196 (MT 3, 33 tiles on 17 blocks)
    panel re-staged (K > kc)        K 772 in three chunks of 320, 320, 132 at HW 300 (none), 301 (tile + tail), 70 (tail only);
                                    K 400 at HW 16388 in two
    ldA padding                     even MT 2, 4, 6 (MB + 16) and odd 1, 3, 5
  types                             fp32 -> bf16 and bf16 -> fp32 on each of the three kernels; K 400 with a bf16 output falls
                                    from split-K through to the LDS kernel; bf16 -> bf16 is CIDNET_ERR_SHAPE
  per-sample weights                B 3 on each of the three kernels (w_bs wider than M K)
  cidnet_pw_conv_up_prelu (EPI 2)
    register route                  Co 36 (2,1,9) and Co 72 (5,0,9) at zw 8 (W % 4 == 0, zw >= 4); zh 1 at zw 64
    LDS fall-back                   zw 3 and zw 5 (W % 4 != 0); Co 144 (ks 36: always LDS)
    Ypre NULL and non-NULL give an equal Y; w_ms = 2 Co (second half of the concat weight); slopes of both signs.  (The ABI
    takes ONE slope -- nn.PReLU() of the reference's NormUpsample has a single parameter -- so there is no per-channel form.)
  pw_wgrad_kernel + reduce_slabs_kernel
    (MT, NT)                        all nine pairs from M, N in {5, 16, 17, 36, 48, 95, 190}
    pch 512                         HW 12, 127, 128, 129, 513 (last chunk 1)
    larger pch                      1x190x190x20001 (768, last chunk 33), 1x190x190x40063 (1536, last chunk 127)
    flags                           three-level, FP32_MFMA, BF16_1LEVEL with the four storage-type pairs
    per_sample 0 / 1                at B 1 and 3
    ACCUMULATE                      dW prefilled with integers; exact criterion: result = prefill + gradient
    dw_ld > N                       sentinel columns untouched
    ws one float short              CIDNET_ERR_WS, nothing launched (outputs still NaN)
  pwx_kernel (bf16x3 forward)
    WM 1 / 2 / 4, chunks 2          M 17 (MTW 2), 48 (3), 64 (4), 80 (5); 96 (WM 2, MTW 3); 161 (WM 4, MTW 3), 320 (WM 4, MTW 5);
                                    336 (chunks 2, MTW 3).  MTW 1 cannot be reached: M <= 16 is refused by _supported.
    cpg 6 / 8                       K 1, 23, 24, 33 (6); 25, 95 (8)
    planes                          HW 64, 65, 127, 130
    residual, per-sample prepared weights, levels (3,3) and (1,1), the bf16 type combinations; M 16 and HW 63 refused
  pwb_kernel (fused backward)
    grid-stride loop + prefetch     the four instantiated shapes (190x36, 36x95, 36x36, 72x36) with more than 512 chunks:
                                    1 x HW 16420 (514 chunks on 512 blocks: two blocks walk 2), 3 x HW 5508 (519: a block's chunks
                                    lie in different samples), 2 x HW 16420 (1028: blocks walk 2 and 3)
    small planes                    HW 4 and 36;  channel counts inside a tile: 181x33
"""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ops_gpu import close  # noqa: E402

gpu = pytest.mark.gpu          # the test that only reads the case tables through the host-side query carries no mark

NAN = float("nan")
SENT = -4096.0                 # exact in bf16
OFF, PAD = 32, 64              # front offset and per-sample slack of every strided buffer, in elements
FIELDS = (("path", "launches", "MT", "LEFT", "KS", "KS2", "kc", "nkc", "tpb", "gx", "gy", "tail", "target", "lds"),
          ("MT", "NT", "nmb", "nnb", "pch", "chunks", "last", "n_red", "n_red_ps"),
          ("cpg", "KB", "MT", "WM", "chunks", "MTW", "tiles"),
          ("MT", "NT", "chunks", "blocks", "most"))
FWD, WGRAD, X3, FUSED = range(4)
SPLITK, REGA, LDS, TAIL_ONLY = range(4)
ACCUMULATE, FP32_MFMA, ONE_LEVEL = 1, 2, 4
ERR_SHAPE, ERR_WS = -2, -3


def plan(kind, B, M, K, HW, W=0, zw=0, xdt=0, ydt=0, epi=0):
    from hvi_cidnet_amd._lib import lib
    out = (ctypes.c_int * 14)(*([-1] * 14))
    rc = lib().raw("cidnet_pw_plan")(kind, B, M, K, HW, W, zw, xdt, ydt, epi, out, 14)
    assert rc == 0, (kind, B, M, K, HW, W, zw, xdt, ydt, epi, rc)
    return dict(zip(FIELDS[kind], out))


def expect(kind, shape, want, **kw):
    t = plan(kind, *shape, **kw)
    got = {k: t[k] for k in want}
    assert got == want, (kind, shape, kw, got, want)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# case tables: shape, what the query must report, variant
# ---------------------------------------------------------------------------------------------------------------------
def _rega(mt, left, ks, **kw):
    return dict(path=REGA, launches=1, MT=mt, LEFT=left, KS=ks, **kw)


def _sk(mt, ks, ks2=0, **kw):
    return dict(path=SPLITK, launches=2 if ks2 else 1, MT=mt, KS=ks, KS2=ks2, tail=0, **kw)


def _lds(mt, **kw):
    return dict(path=LDS, launches=1, MT=mt, LEFT=0, **kw)


# cidnet_pw_conv_t: (B, M, K, HW), expected plan, options (xdt, ydt, ps = per-sample weights)
FWD_CASES = [
    # register-resident kernel: every (MT, LEFT) at KS 9
    ((2, 20, 36, 1028), _rega(1, 1, 9, gy=1, tail=0, tpb=1, gx=5), {}),
    ((2, 36, 36, 1028), _rega(2, 1, 9, gy=1), {}),
    ((2, 52, 36, 1028), _rega(3, 1, 9, gy=1), {}),
    ((2, 96, 36, 1028), _rega(3, 0, 9, gy=2), {}),
    ((2, 190, 36, 1028), _rega(4, 0, 9, gy=3, target=1024), {}),
    ((2, 72, 36, 1028), _rega(5, 0, 9, gy=1, target=1024), {}),
    ((2, 71, 36, 1028), _rega(5, 0, 9, gy=1, target=512), {}),
    ((2, 33, 36, 1028), _rega(2, 1, 9), {}),
    ((2, 37, 36, 1028), _rega(3, 0, 9, gy=1), {}),
    # KS 18 and 24
    ((2, 64, 37, 1028), _rega(2, 0, 18, gy=2), {}),
    ((2, 95, 37, 1028), _rega(3, 0, 18, gy=2), {}),
    ((2, 72, 37, 1028), _rega(5, 0, 18, gy=1), {}),
    ((2, 64, 60, 1028), _rega(2, 0, 18, gy=2), {}),
    ((2, 95, 60, 1028), _rega(3, 0, 18, gy=2), {}),
    ((2, 72, 60, 1028), _rega(5, 0, 18, gy=1), {}),
    ((2, 36, 60, 1028), _rega(2, 1, 18, gy=1), {}),
    ((1, 36, 73, 8196), _rega(2, 1, 24, gy=1, gx=33), {}),
    ((1, 48, 96, 8196), _rega(3, 0, 24, gy=1, gx=33), {}),
    # a k-step that is not full
    ((2, 36, 1, 1028), _rega(2, 1, 9), {}),
    ((2, 36, 3, 1028), _rega(2, 1, 9), {}),
    ((2, 36, 5, 1028), _rega(2, 1, 9), {}),
    # tiles per block: 2 and 3 with a ragged last block, 8 clamped
    ((6, 36, 36, 23808), _rega(2, 1, 9, tpb=2, gx=47, target=512), {}),
    ((3, 36, 36, 89600), _rega(2, 1, 9, tpb=3, gx=117, target=512), {}),
    ((1, 4, 4, 921856), _rega(1, 0, 9, tpb=8, gx=451, target=512), {}),
    # tail: a streaming tile plus the tail launch; the tail kernel alone; none
    ((2, 36, 36, 257), _rega(2, 1, 9, tail=1, gx=1), {}),
    ((2, 36, 36, 258), _rega(2, 1, 9, tail=1, gx=1), {}),
    ((2, 36, 36, 259), _rega(2, 1, 9, tail=1, gx=1), {}),
    ((2, 36, 36, 1), dict(path=TAIL_ONLY, launches=0, MT=3, tail=1, nkc=1), {}),
    ((2, 36, 36, 2), dict(path=TAIL_ONLY, launches=0, MT=3, tail=1), {}),
    ((2, 36, 36, 3), dict(path=TAIL_ONLY, launches=0, MT=3, tail=1), {}),
    ((2, 36, 36, 5), dict(path=TAIL_ONLY, launches=0, MT=3, tail=1), {}),
    ((2, 36, 36, 255), dict(path=TAIL_ONLY, launches=0, MT=3, tail=1), {}),
    ((2, 36, 36, 256), _rega(2, 1, 9, tail=0, gx=1), {}),
    ((2, 36, 36, 260), _rega(2, 1, 9, tail=0, gx=2), {}),
    # split-K: register depth, two launches around K = 384
    ((2, 50, 64, 130), _sk(3, 9, gy=2, gx=3, tpb=1), {}),
    ((2, 50, 100, 130), _sk(3, 9, gy=2), {}),
    ((2, 50, 190, 130), _sk(3, 18, gy=2), {}),
    ((2, 50, 383, 130), _sk(3, 24, gy=2), {}),
    ((2, 50, 384, 130), _sk(3, 24, gy=2), {}),
    ((2, 50, 385, 130), _sk(3, 24, 9, gy=2), {}),
    ((2, 50, 400, 130), _sk(3, 24, 9, gy=2), {}),
    ((2, 50, 768, 130), _sk(3, 24, 24, gy=2), {}),
    # split-K: channel tiles, groups past the end of the plane, two groups per block
    ((2, 10, 100, 61), _sk(1, 9, gy=1, gx=1), {}),
    ((2, 20, 190, 65), _sk(2, 18, gy=1, gx=2), {}),
    ((2, 100, 383, 16), _sk(3, 24, gy=3, gx=1), {}),
    ((2, 10, 400, 65), _sk(1, 24, 9, gy=1, gx=2), {}),
    ((2, 20, 100, 16), _sk(2, 9, gy=1, gx=1), {}),
    ((2, 10, 190, 130), _sk(1, 18, gy=1, gx=3), {}),
    ((2, 20, 384, 61), _sk(2, 24, gy=1, gx=1), {}),
    ((2, 144, 100, 8192), _sk(3, 9, gy=3, tpb=2, gx=64), {}),
    # split-K thresholds
    ((1, 36, 100, 8192), _sk(3, 9, gy=1, tpb=1, gx=128), {}),
    ((1, 36, 100, 8196), _lds(2, tail=0, nkc=1, kc=100, tpb=1, gx=33, gy=2), {}),
    ((1, 36, 400, 16384), _sk(3, 24, 9, gy=1, gx=256), {}),
    ((1, 36, 400, 16388), _lds(2, tail=0, kc=320, nkc=2, tpb=1, gx=65, gy=2), {}),
    # LDS kernel: channel tiles 1 .. 6 (even: ldA = MB + 16)
    ((1, 16, 100, 8196), _lds(1, gy=1, kc=100, lds=100 * 16 * 4), {}),
    ((1, 32, 100, 8196), _lds(2, gy=1, lds=100 * 48 * 4), {}),
    ((4, 190, 100, 8196), _lds(3, gy=4, lds=100 * 48 * 4), {}),
    ((8, 128, 100, 8196), _lds(4, gy=2, lds=100 * 80 * 4), {}),
    ((6, 190, 100, 8196), _lds(5, gy=3, lds=100 * 80 * 4), {}),
    ((2, 96, 100, 65536), _lds(6, gy=1, tpb=1, gx=256, lds=100 * 112 * 4), {}),
    ((1, 766, 144, 8196), _lds(3, gy=16, tpb=2, gx=17, nkc=1), {}),
    # LDS kernel: the weight panel re-staged per tile (K > kc)
    ((2, 40, 772, 300), _lds(2, kc=320, nkc=3, tail=0, tpb=1, gx=2, gy=2), {}),
    ((2, 40, 772, 301), _lds(2, kc=320, nkc=3, tail=1, tpb=1, gx=1, gy=2), {}),
    ((2, 40, 772, 70), dict(path=TAIL_ONLY, launches=0, MT=2, kc=320, nkc=3, tail=1), {}),
    # storage types on each kernel
    ((2, 36, 36, 1028), _rega(2, 1, 9), dict(ydt=1)),
    ((2, 36, 36, 1029), _rega(2, 1, 9, tail=1), dict(xdt=1)),
    ((2, 50, 190, 131), _sk(3, 18), dict(ydt=1)),
    ((2, 50, 190, 130), _sk(3, 18), dict(xdt=1)),
    ((2, 50, 400, 130), _sk(3, 24, 9), dict(xdt=1)),
    ((2, 50, 400, 518), _lds(2, kc=320, nkc=2, tail=1, gy=2, gx=2), dict(ydt=1)),
    ((1, 40, 100, 8197), _lds(2, tail=1), dict(ydt=1)),
    ((1, 40, 100, 8196), _lds(2, tail=0), dict(xdt=1)),
    # per-sample weights on each kernel
    ((3, 36, 36, 1029), _rega(2, 1, 9, tail=1), dict(ps=1)),
    ((3, 50, 400, 130), _sk(3, 24, 9), dict(ps=1)),
    ((3, 40, 772, 301), _lds(2, nkc=3, tail=1), dict(ps=1)),
]

# cidnet_pw_conv_up_prelu: (B, Co, K, zh, zw), expected plan, slope
UP_CASES = [
    ((2, 36, 36, 8, 8), _rega(2, 1, 9, tail=0), 0.25),
    ((2, 72, 72, 8, 8), _rega(5, 0, 18, tail=0), -0.5),
    ((1, 72, 36, 9, 8), _rega(5, 0, 9, tail=0), 0.1),
    ((2, 36, 36, 1, 64), _rega(2, 1, 9, tail=0), -0.3),
    ((2, 36, 36, 22, 3), _lds(3, tail=0, nkc=1), 0.25),
    ((2, 36, 36, 13, 5), _lds(3, tail=0, nkc=1), -0.25),
    ((1, 144, 144, 8, 8), _lds(2, tail=0, nkc=1), 0.2),
    ((1, 144, 144, 13, 5), _lds(2, tail=0, nkc=1), -0.2),
]

# cidnet_pw_wgrad_t: (B, M, N, HW), expected plan, (flags, dY type, X type, per_sample)
_T = {5: 1, 16: 1, 17: 2, 36: 3, 48: 3, 95: 3, 190: 3}       # channels -> 16-row tiles per block
WG_CASES = [
    ((2, 5, 5, 129), dict(MT=1, NT=1, pch=512, chunks=1, last=129), (0, 0, 0, 0)),
    ((2, 16, 17, 129), dict(MT=1, NT=2), (FP32_MFMA, 0, 0, 0)),
    ((2, 5, 190, 129), dict(MT=1, NT=3, nnb=4), (0, 0, 0, 1)),
    ((2, 17, 16, 129), dict(MT=2, NT=1), (0, 0, 0, 0)),
    ((2, 17, 17, 129), dict(MT=2, NT=2), (ONE_LEVEL, 0, 0, 0)),
    ((2, 17, 95, 129), dict(MT=2, NT=3, nnb=2), (0, 0, 0, 0)),
    ((2, 36, 5, 129), dict(MT=3, NT=1), (0, 0, 0, 0)),
    ((2, 48, 17, 129), dict(MT=3, NT=2), (FP32_MFMA, 0, 0, 1)),
    ((2, 190, 36, 129), dict(MT=3, NT=3, nmb=4, nnb=1), (0, 0, 0, 0)),
    ((3, 95, 48, 129), dict(MT=3, NT=3, nmb=2, nnb=1), (0, 0, 0, 1)),
    # pixels per block 512: planes below one step, around one wave step, a last chunk of one pixel
    ((1, 36, 36, 12), dict(pch=512, chunks=1, last=12), (0, 0, 0, 0)),
    ((3, 36, 36, 127), dict(pch=512, chunks=1, last=127), (0, 0, 0, 1)),
    ((1, 36, 36, 128), dict(pch=512, chunks=1, last=128), (FP32_MFMA, 0, 0, 1)),
    ((3, 36, 36, 513), dict(pch=512, chunks=2, last=1, n_red=6, n_red_ps=2), (0, 0, 0, 0)),
    ((1, 36, 36, 513), dict(pch=512, chunks=2, last=1), (ONE_LEVEL, 0, 0, 1)),
    # larger blocks as the cost model picks them
    ((1, 190, 190, 20001), dict(pch=768, chunks=27, last=33), (0, 0, 0, 0)),
    ((1, 190, 190, 40063), dict(pch=1536, chunks=27, last=127), (FP32_MFMA, 0, 0, 0)),
    # one level with the four storage-type pairs
    ((2, 36, 95, 641), dict(MT=3, NT=3, chunks=2, last=129), (ONE_LEVEL, 0, 0, 0)),
    ((2, 36, 95, 641), dict(MT=3, NT=3, chunks=2, last=129), (ONE_LEVEL, 1, 0, 0)),
    ((2, 36, 95, 641), dict(MT=3, NT=3, chunks=2, last=129), (ONE_LEVEL, 0, 1, 1)),
    ((2, 36, 95, 641), dict(MT=3, NT=3, chunks=2, last=129), (ONE_LEVEL, 1, 1, 0)),
]

# bf16x3 forward: (B, M, K, HW), expected plan, (residual, per-sample weights, levels, x type, y type)
X3_CASES = [
    ((2, 17, 1, 64), dict(cpg=6, KB=1, MT=2, WM=1, chunks=1, MTW=2, tiles=1), (0, 0, 3, 0, 0)),
    ((2, 48, 23, 65), dict(cpg=6, KB=1, WM=1, chunks=1, MTW=3, tiles=1), (1, 0, 3, 0, 0)),
    ((2, 64, 24, 127), dict(cpg=6, KB=1, WM=1, chunks=1, MTW=4, tiles=1), (0, 0, 3, 0, 0)),
    ((2, 80, 25, 130), dict(cpg=8, KB=1, WM=1, chunks=1, MTW=5, tiles=1), (1, 0, 3, 0, 0)),
    ((2, 96, 33, 130), dict(cpg=6, KB=2, WM=2, chunks=1, MTW=3, tiles=2), (1, 1, 3, 0, 0)),
    ((2, 161, 95, 65), dict(cpg=8, KB=3, WM=4, chunks=1, MTW=3, tiles=2), (0, 0, 3, 0, 0)),
    ((1, 320, 33, 127), dict(cpg=6, KB=2, WM=4, chunks=1, MTW=5, tiles=2), (1, 0, 3, 0, 0)),
    ((2, 336, 25, 130), dict(cpg=8, KB=1, WM=4, chunks=2, MTW=3, tiles=3), (1, 0, 3, 0, 0)),
    ((3, 336, 24, 64), dict(cpg=6, KB=1, WM=4, chunks=2, MTW=3, tiles=1), (0, 1, 3, 0, 0)),
    ((2, 130, 72, 333), dict(cpg=6, KB=3, WM=2, chunks=1, MTW=5, tiles=3), (1, 0, 3, 0, 0)),
    # one level, and the bf16 storage types
    ((2, 96, 33, 130), dict(WM=2, MTW=3), (1, 0, 1, 0, 0)),
    ((2, 336, 95, 127), dict(WM=4, chunks=2, MTW=3), (0, 0, 1, 0, 0)),
    ((2, 80, 25, 130), dict(WM=1, MTW=5), (1, 0, 1, 1, 0)),
    ((2, 161, 23, 65), dict(WM=4, MTW=3), (0, 0, 1, 0, 1)),
    ((3, 96, 95, 127), dict(WM=2, MTW=3), (1, 1, 1, 1, 1)),
]
X3_REFUSED = [(1, 16, 36, 64), (1, 36, 36, 63)]

# fused backward: (B, M, N, HW), expected plan
FUSED_CASES = [
    ((1, 190, 36, 16420), dict(MT=12, NT=3, chunks=514, blocks=512, most=2)),
    ((3, 36, 95, 5508), dict(MT=3, NT=6, chunks=173, blocks=512, most=2)),
    ((2, 36, 36, 16420), dict(MT=3, NT=3, chunks=514, blocks=512, most=3)),
    ((3, 72, 36, 5508), dict(MT=5, NT=3, chunks=173, blocks=512, most=2)),
    ((2, 181, 33, 36), dict(MT=12, NT=3, chunks=2, blocks=4, most=1)),
    ((3, 36, 36, 4), dict(MT=3, NT=3, chunks=1, blocks=3, most=1)),
    ((1, 72, 36, 36), dict(MT=5, NT=3, chunks=2, blocks=2, most=1)),
    ((2, 36, 95, 4), dict(MT=3, NT=6, chunks=1, blocks=2, most=1)),
]


def _fwd_kw(opt):
    return dict(xdt=opt.get("xdt", 0), ydt=opt.get("ydt", 0))


def _up_shape(case):
    B, Co, K, zh, zw = case
    return (B, Co, K, 4 * zh * zw), dict(W=2 * zw, zw=zw, epi=2)


def test_case_tables_reach_their_plans():
    """every table above, through the host-only query alone (no GPU): a retuned threshold fails here first"""
    from hvi_cidnet_amd._lib import lib
    L = lib()
    seen = set()
    for shape, want, opt in FWD_CASES:
        for epi in (0, 1):
            t = expect(FWD, shape, want, epi=epi, **_fwd_kw(opt))
        seen.add((t["path"], t["MT"], t["LEFT"], t["KS"]))
    # every register-resident and split-K instantiation, every channel-tile count of the LDS kernel
    assert {(REGA, mt, left, ks) for mt, left, ks in ((1, 1, 9), (2, 1, 9), (3, 1, 9), (3, 0, 9), (4, 0, 9), (5, 0, 9), (2, 0, 18),
                                                     (3, 0, 18), (5, 0, 18), (2, 1, 18), (2, 1, 24), (3, 0, 24), (1, 0, 9))} <= seen
    assert {(SPLITK, mt, 0, ks) for mt in (1, 2, 3) for ks in (9, 18, 24)} <= seen
    assert {(LDS, mt, 0, 0) for mt in range(1, 7)} <= seen
    out = (ctypes.c_int * 14)()
    assert L.raw("cidnet_pw_plan")(FWD, 1, 36, 36, 1028, 0, 0, 1, 1, 0, out, 14) == ERR_SHAPE          # bf16 -> bf16
    for case, want, _ in UP_CASES:
        shape, kw = _up_shape(case)
        t = expect(FWD, shape, want, **kw)
        assert t["path"] != SPLITK
    for shape, want, _ in WG_CASES:
        B, M, N, HW = shape
        t = expect(WGRAD, shape, {**want, "MT": _T[M], "NT": _T[N]})
        assert L.raw("cidnet_pw_wgrad_ws_floats")(B, M, N, HW) == B * t["chunks"] * M * N
    assert {(_T[s[1]], _T[s[2]]) for s, _, _ in WG_CASES} == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    assert {plan(WGRAD, *s)["pch"] for s, _, _ in WG_CASES} >= {512, 768, 1536}
    for shape, want, _ in X3_CASES:
        expect(X3, shape, want)
    assert {(plan(X3, *s)["WM"], plan(X3, *s)["MTW"]) for s, _, _ in X3_CASES} >= {(1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (2, 5), (4, 3), (4, 5)}
    for shape in X3_REFUSED:
        assert L.raw("cidnet_pw_plan")(X3, *shape, 0, 0, 0, 0, 0, out, 14) == ERR_SHAPE
    for shape, want in FUSED_CASES:
        expect(FUSED, shape, want)


# ---------------------------------------------------------------------------------------------------------------------
# operands and strided buffers
# ---------------------------------------------------------------------------------------------------------------------
def ints(seed, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def rand(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


class Slab:
    """B blocks of n elements inside a wider buffer: block b starts at OFF + b * bs with bs = n + PAD; the rest is SENT"""

    def __init__(self, dev, B, n, dtype=torch.float32, src=None, pad=PAD, off=OFF):
        self.B, self.n, self.bs, self.off = B, n, n + pad, off
        self.buf = torch.full((off + B * self.bs,), SENT, device=dev, dtype=dtype)
        self.view().copy_(src.reshape(B, n).to(dev)) if src is not None else self.view().fill_(NAN)

    def view(self):
        return self.buf[self.off:].view(self.B, self.bs)[:, :self.n]

    def ptr(self):
        from hvi_cidnet_amd import ops
        return ops._pe(self.buf, self.off)

    def dt(self):
        return int(self.buf.dtype == torch.bfloat16)

    def check(self):
        """-> the covered part (B, n) in fp64 on the CPU; finite there, the sentinel everywhere else"""
        rest = self.buf[self.off:].view(self.B, self.bs)[:, self.n:]
        assert bool((rest == SENT).all()) and bool((self.buf[:self.off] == SENT).all()), "wrote outside the planes it covers"
        v = self.view().double().cpu()
        assert bool(torch.isfinite(v).all()), "elements left unwritten or not finite"
        return v


def same(a, b):
    assert torch.equal(a, b), "two runs differ"
    return a


def tdt(flag):
    return torch.bfloat16 if flag else torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# cidnet_pw_conv_t
# ---------------------------------------------------------------------------------------------------------------------
def run_pw(dev, B, M, K, HW, x, w, r, trans, xdt, ydt):
    """x (B, K, HW), w (nb, M, K) with nb = 1 or B (per-sample), r (B, M, HW) or None -> y (B, M * HW) fp64, run twice"""
    from hvi_cidnet_amd import ops
    nb = w.shape[0]
    xs = Slab(dev, B, K * HW, tdt(xdt), x)
    ws = Slab(dev, nb, M * K, src=w.transpose(1, 2).contiguous() if trans else w, pad=4)     # stored (K, M) for the data gradient
    rs = Slab(dev, B, M * HW, src=r) if r is not None else None
    w_ms, w_ks = (1, M) if trans else (K, 1)
    runs = []
    for _ in range(2):
        ys = Slab(dev, B, M * HW, tdt(ydt))
        ops.lib().call("cidnet_pw_conv_t", xs.ptr(), xdt, xs.bs, ws.ptr(), ws.bs if nb > 1 else 0, w_ms, w_ks, ys.ptr(), ydt, ys.bs,
                       rs.ptr() if rs else None, rs.bs if rs else 0, B, M, K, HW, ops._stream())
        runs.append(ys)
    torch.cuda.synchronize()
    for s in (xs, ws) + ((rs,) if rs else ()):
        s.check()                                                    # inputs and their slack untouched
    return same(runs[0].check(), runs[1].check())


def ref_pw(x, w, r):
    ref = torch.matmul(w.double(), x.double())                       # (nb, M, K) x (B, K, HW), nb broadcasts
    return (ref + r.double() if r is not None else ref).reshape(x.shape[0], -1)


@gpu
@pytest.mark.parametrize("shape,want,opt", FWD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pw_conv_paths(dev, shape, want, opt):
    B, M, K, HW = shape
    xdt, ydt, nb = opt.get("xdt", 0), opt.get("ydt", 0), B if opt.get("ps") else 1
    for epi in (0, 1):
        expect(FWD, shape, want, epi=epi, xdt=xdt, ydt=ydt)
    # exact: forward strides with a residual, transposed (data-gradient) strides without
    x, w, r = ints(1, 8, B, K, HW), ints(2, 4, nb, M, K), ints(3, 8, B, M, HW)
    for trans, res in ((0, r), (1, None)):
        ref = ref_pw(x, w, res)
        assert float(torch.matmul(w.double().abs(), x.double().abs()).max()) + 8 < 2 ** 24       # every partial sum is exact
        y = run_pw(dev, B, M, K, HW, x, w, res, trans, xdt, ydt)
        want_y = bf16_round(ref) if ydt else ref
        bad = (y != want_y).nonzero()
        assert bad.numel() == 0, f"exact, trans={trans}: {bad.shape[0]} wrong elements, first (b, m * HW + p) = {bad[0].tolist()}"
    # rounded: transposed strides with a residual
    x, w, r = rand(4, B, K, HW), rand(5, nb, M, K, scale=K ** -0.5), rand(6, B, M, HW)
    if xdt:
        x = x.to(torch.bfloat16).float()                             # the stored values ARE the operand
    ref = ref_pw(x, w, r)
    y = run_pw(dev, B, M, K, HW, x, w, r, 1, xdt, ydt)
    if ydt:
        err, bar = (y - ref).abs().max().item(), 2.0 ** -8 * ref.abs().max().item() + 1e-6       # half an ulp of the largest value
        assert err <= bar, (err, bar)
    else:
        close(y, ref, what=f"rounded {shape} {opt}")


@gpu
def test_pw_conv_bf16_to_bf16_is_refused(dev):
    from hvi_cidnet_amd import ops
    B, M, K, HW = 1, 36, 36, 260
    x = torch.zeros(B, K, HW, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(M, K, device=dev)
    y = torch.full((B, M, HW), NAN, device=dev, dtype=torch.bfloat16)
    rc = ops._raw("cidnet_pw_conv_t", ops._p(x), 1, K * HW, ops._p(w), 0, K, 1, ops._p(y), 1, M * HW, None, 0, B, M, K, HW, ops._stream())
    torch.cuda.synchronize()
    assert rc == ERR_SHAPE and bool(torch.isnan(y.float()).all())


# ---------------------------------------------------------------------------------------------------------------------
# cidnet_pw_conv_up_prelu
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,want,slope", UP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pw_conv_up_prelu(dev, case, want, slope):
    """Y = prelu(W_skip skip + up2(Z), slope), Ypre = the argument of the PReLU; W_skip is the second half of a (Co, 2 Co)
    concat weight (w_ms = 2 Co), the skip tensor is a slice of a wider buffer"""
    from hvi_cidnet_amd import ops
    B, Co, K, zh, zw = case
    shape, kw = _up_shape(case)
    expect(FWD, shape, want, **kw)
    HW = shape[3]
    skip, z = rand(11, B, K, 2 * zh, 2 * zw), rand(12, B, Co, zh, zw)
    wcat = rand(13, Co, 2 * K, scale=K ** -0.5)
    pre_ref = F.conv2d(skip.double(), wcat[:, K:].double().reshape(Co, K, 1, 1)) \
        + F.interpolate(z.double(), scale_factor=2, mode="bilinear", align_corners=True)
    y_ref = F.prelu(pre_ref, torch.tensor([slope], dtype=torch.float64))
    assert float((pre_ref < 0).double().mean()) > 0.2                # the slope matters
    xs = Slab(dev, B, K * HW, src=skip)
    wd, zd, sd = wcat.to(dev), z.to(dev), torch.tensor([slope], device=dev)
    outs = []
    for with_pre in (True, True, False):
        y = torch.full((B, Co, HW), NAN, device=dev)
        pre = torch.full((B, Co, HW), NAN, device=dev) if with_pre else None
        ops.lib().call("cidnet_pw_conv_up_prelu", xs.ptr(), xs.bs, ops._pe(wd, K), 2 * K, 1, ops._p(zd), ops._p(sd), ops._p(y),
                       ops._p(pre), B, Co, K, zh, zw, ops._stream())
        outs.append((y, pre))
    torch.cuda.synchronize()
    xs.check()
    for y, pre in outs:
        assert bool(torch.isfinite(y).all()) and (pre is None or bool(torch.isfinite(pre).all()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two runs differ"
    assert torch.equal(outs[0][0], outs[2][0]), "Y depends on whether Ypre is written"
    close(outs[0][1].reshape(pre_ref.shape), pre_ref, what=f"Ypre {case}")
    close(outs[0][0].reshape(y_ref.shape), y_ref, what=f"Y {case}")


# ---------------------------------------------------------------------------------------------------------------------
# cidnet_pw_wgrad_t
# ---------------------------------------------------------------------------------------------------------------------
def run_wgrad(dev, B, M, N, HW, gy, x, flags, ddt, xdt, per_sample, prefill=None, short=0):
    """-> (status, dW (nout, M, N) fp64) run twice; dW rows are N + 3 wide, the workspace is NaN-filled and exactly as large
    as the library asks (minus `short`)"""
    from hvi_cidnet_amd import ops
    gs, xs = Slab(dev, B, M * HW, tdt(ddt), gy), Slab(dev, B, N * HW, tdt(xdt), x)
    n = ops._raw("cidnet_pw_wgrad_ws_floats", B, M, N, HW)
    nout, ld = (B if per_sample else 1), N + 3
    runs = []
    for _ in range(2):
        dw = torch.full((nout, M, ld), SENT, device=dev)
        dw[:, :, :N] = NAN if prefill is None else prefill.to(dev)
        ws = torch.full((n,), NAN, device=dev)
        rc = ops._raw("cidnet_pw_wgrad_t", gs.ptr(), ddt, gs.bs, xs.ptr(), xdt, xs.bs, ops._p(dw), ld, int(per_sample), flags, ops._p(ws),
                      n - short, B, M, N, HW, ops._stream())
        runs.append(dw)
    torch.cuda.synchronize()
    gs.check(), xs.check()
    assert torch.equal(runs[0][:, :, :N], runs[1][:, :, :N]) or rc != 0, "two runs differ"
    assert bool((runs[0][:, :, N:] == SENT).all()), "wrote past column N of dW"
    return rc, runs[0][:, :, :N].double().cpu()


def ref_wgrad(gy, x, per_sample):
    r = torch.einsum("bmp,bnp->bmn", gy.double(), x.double())
    return r if per_sample else r.sum(0, keepdim=True)


@gpu
@pytest.mark.parametrize("shape,want,var", WG_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pw_wgrad_paths(dev, shape, want, var):
    B, M, N, HW = shape
    flags, ddt, xdt, ps = var
    expect(WGRAD, shape, {**want, "MT": _T[M], "NT": _T[N]})
    # exact, accumulating onto an integer prefill: max|dY| max|X| B HW < 2^24
    lim = max(1, min(8, math.isqrt((2 ** 24 - 9) // (B * HW))))
    gy, x = ints(21, lim, B, M, HW), ints(22, lim, B, N, HW)
    pre = ints(23, 8, (B if ps else 1), M, N)
    assert lim * lim * B * HW + 8 < 2 ** 24
    ref = ref_wgrad(gy, x, ps)
    assert float(torch.einsum("bmp,bnp->mn", gy.double().abs(), x.double().abs()).max()) + 8 < 2 ** 24
    rc, dw = run_wgrad(dev, B, M, N, HW, gy, x, flags, ddt, xdt, ps)
    assert rc == 0 and bool(torch.isfinite(dw).all())
    bad = (dw != ref).nonzero()
    assert bad.numel() == 0, f"exact: {bad.shape[0]} wrong elements, first (b, m, n) = {bad[0].tolist()}"
    rc, dw = run_wgrad(dev, B, M, N, HW, gy, x, flags | ACCUMULATE, ddt, xdt, ps, prefill=pre)
    assert rc == 0 and torch.equal(dw, ref + pre.double()), "CIDNET_WGRAD_ACCUMULATE: not prefill + gradient"
    # rounded
    gy, x = rand(24, B, M, HW), rand(25, B, N, HW)
    if flags & ONE_LEVEL or ddt:
        gy = gy.to(torch.bfloat16).float()
    if flags & ONE_LEVEL or xdt:
        x = x.to(torch.bfloat16).float()
    ref = ref_wgrad(gy, x, ps)
    rc, dw = run_wgrad(dev, B, M, N, HW, gy, x, flags, ddt, xdt, ps)
    assert rc == 0 and bool(torch.isfinite(dw).all())
    if flags & ONE_LEVEL:
        err = (dw - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item() + 1e-6, err
    else:
        close(dw, ref, what=f"rounded wgrad {shape} {var}")


@gpu
def test_pw_wgrad_short_workspace_launches_nothing(dev):
    B, M, N, HW = 2, 36, 36, 513
    rc, dw = run_wgrad(dev, B, M, N, HW, ints(31, 4, B, M, HW), ints(32, 4, B, N, HW), 0, 0, 0, 0, short=1)
    assert rc == ERR_WS and bool(torch.isnan(dw).all())


# ---------------------------------------------------------------------------------------------------------------------
# bf16x3 forward
# ---------------------------------------------------------------------------------------------------------------------
def run_x3(dev, B, M, K, HW, x, w, r, lv, xdt, ydt, one_shot=False):
    """cidnet_pw_conv_bf16x3_prep + _pre_t (or the one-call form), weights (nb, M, K), run twice -> y (B, M * HW) fp64"""
    from hvi_cidnet_amd import ops
    nb = w.shape[0]
    xs = Slab(dev, B, K * HW, tdt(xdt), x)
    wsl = Slab(dev, nb, M * K, src=w, pad=4)
    rs = Slab(dev, B, M * HW, src=r) if r is not None else None
    n = ops._raw("cidnet_pw_conv_bf16x3_ws_floats", B, M, K, int(nb > 1))
    p = plan(X3, B, M, K, HW)
    assert n == nb * p["KB"] * p["MT"] * 3 * 256
    runs = []
    for _ in range(2):
        ys = Slab(dev, B, M * HW, tdt(ydt))
        ws = torch.full((n,), NAN, device=dev)
        if one_shot:
            ops.lib().call("cidnet_pw_conv_bf16x3", xs.ptr(), xs.bs, wsl.ptr(), wsl.bs if nb > 1 else 0, K, 1, ys.ptr(), ys.bs,
                           rs.ptr() if rs else None, rs.bs if rs else 0, ops._p(ws), n, B, M, K, HW, ops._stream())
        else:
            ops.lib().call("cidnet_pw_conv_bf16x3_prep", wsl.ptr(), wsl.bs if nb > 1 else 0, K, 1, ops._p(ws), n, nb, M, K, ops._stream())
            ops.lib().call("cidnet_pw_conv_bf16x3_pre_t", xs.ptr(), xdt, xs.bs, ops._p(ws), int(nb > 1), ys.ptr(), ydt, ys.bs,
                           rs.ptr() if rs else None, rs.bs if rs else 0, B, M, K, HW, lv, lv, ops._stream())
        runs.append(ys)
    torch.cuda.synchronize()
    for s in (xs, wsl) + ((rs,) if rs else ()):
        s.check()
    return same(runs[0].check(), runs[1].check())


@gpu
@pytest.mark.parametrize("shape,want,var", X3_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pw_conv_bf16x3_paths(dev, shape, want, var):
    B, M, K, HW = shape
    res, ps, lv, xdt, ydt = var
    expect(X3, shape, want)
    nb = B if ps else 1
    x, w, r = ints(41, 8, B, K, HW), ints(42, 4, nb, M, K), ints(43, 8, B, M, HW) if res else None
    ref = ref_pw(x, w, r)
    assert float(torch.matmul(w.double().abs(), x.double().abs()).max()) + 8 < 2 ** 24
    y = run_x3(dev, B, M, K, HW, x, w, r, lv, xdt, ydt)
    bad = (y != (bf16_round(ref) if ydt else ref)).nonzero()
    assert bad.numel() == 0, f"exact: {bad.shape[0]} wrong elements, first (b, m * HW + p) = {bad[0].tolist()}"
    if lv == 3:
        assert torch.equal(run_x3(dev, B, M, K, HW, x, w, r, lv, 0, 0, one_shot=True), y)
    # rounded
    x, w, r = rand(44, B, K, HW), rand(45, nb, M, K, scale=K ** -0.5), rand(46, B, M, HW) if res else None
    y = run_x3(dev, B, M, K, HW, x, w, r, lv, xdt, ydt)
    if lv == 1:                                                      # the fp64 product of the bf16-rounded operands
        ref = ref_pw(x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), r)
        err, bar = (y - ref).abs().max().item(), (2.0 ** -8 if ydt else 3e-6) * ref.abs().max().item() + 1e-6
        assert err <= bar, (err, bar)
    else:                                                            # no worse than the fp32-MFMA kernel
        ref = ref_pw(x, w, r)
        e32 = (run_pw(dev, B, M, K, HW, x, w, r, 0, 0, 0) - ref).abs().max().item()
        es = (y - ref).abs().max().item()
        assert es <= 3 * e32 + 2e-6 * ref.abs().max().item(), (es, e32)
        close(y, ref, what=f"rounded bf16x3 {shape}")


@gpu
@pytest.mark.parametrize("shape", X3_REFUSED)
def test_pw_conv_bf16x3_refuses_unsupported(dev, shape):
    from hvi_cidnet_amd import ops
    B, M, K, HW = shape
    assert not ops._raw("cidnet_pw_conv_bf16x3_supported", M, K, HW)
    x, w = torch.zeros(B, K, HW, device=dev), torch.zeros(M, K, device=dev)
    y = torch.full((B, M, HW), NAN, device=dev)
    n = ops._raw("cidnet_pw_conv_bf16x3_ws_floats", B, M, K, 0)
    ws = torch.zeros(n, device=dev)
    rc = ops._raw("cidnet_pw_conv_bf16x3_pre_t", ops._p(x), 0, K * HW, ops._p(ws), 0, ops._p(y), 0, M * HW, None, 0, B, M, K, HW, 3, 3,
                  ops._stream())
    rc2 = ops._raw("cidnet_pw_conv_bf16x3", ops._p(x), K * HW, ops._p(w), 0, K, 1, ops._p(y), M * HW, None, 0, ops._p(ws), n, B, M, K, HW,
                   ops._stream())
    torch.cuda.synchronize()
    assert rc == ERR_SHAPE and rc2 == ERR_SHAPE and bool(torch.isnan(y).all())


# ---------------------------------------------------------------------------------------------------------------------
# fused backward
# ---------------------------------------------------------------------------------------------------------------------
def run_fused(dev, B, M, N, HW, gy, x, w):
    """-> gx (B, N * HW), dW (M, N) in fp64, run twice; workspace NaN-filled and exactly as large as the library asks"""
    from hvi_cidnet_amd import ops
    gs, xs = Slab(dev, B, M * HW, src=gy), Slab(dev, B, N * HW, src=x)
    wd = w.to(dev)
    n = ops._raw("cidnet_pw_bwd_fused_ws_floats", B, M, N, HW)
    runs = []
    for _ in range(2):
        gx, dw = Slab(dev, B, N * HW), torch.full((M, N), NAN, device=dev)
        ws = torch.full((n,), NAN, device=dev)
        ops.lib().call("cidnet_pw_bwd_fused", gs.ptr(), gs.bs, xs.ptr(), xs.bs, ops._p(wd), gx.ptr(), gx.bs, ops._p(dw), ops._p(ws), n,
                       B, M, N, HW, ops._stream())
        runs.append((gx, dw))
    torch.cuda.synchronize()
    gs.check(), xs.check()
    assert torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    assert bool(torch.isfinite(runs[0][1]).all())
    return same(runs[0][0].check(), runs[1][0].check()), runs[0][1].double().cpu()


@gpu
@pytest.mark.parametrize("shape,want", FUSED_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pw_bwd_fused_paths(dev, shape, want):
    from hvi_cidnet_amd import ops
    B, M, N, HW = shape
    t = expect(FUSED, shape, want)
    assert ops._raw("cidnet_pw_bwd_fused_supported", M, N, HW) and t["blocks"] * t["most"] >= B * t["chunks"] > t["blocks"] * (t["most"] - 1)
    gy, x, w = ints(51, 8, B, M, HW), ints(52, 8, B, N, HW), ints(53, 4, M, N)
    gx_ref = torch.einsum("mn,bmp->bnp", w.double(), gy.double()).reshape(B, -1)
    dw_ref = torch.einsum("bmp,bnp->mn", gy.double(), x.double())
    assert 64 * B * HW < 2 ** 24 and 32 * M < 2 ** 24
    gx, dw = run_fused(dev, B, M, N, HW, gy, x, w)
    for name, got, ref in (("gx", gx, gx_ref), ("dW", dw, dw_ref)):
        bad = (got != ref).nonzero()
        assert bad.numel() == 0, f"exact {name}: {bad.shape[0]} wrong elements, first {bad[0].tolist()}"
    # rounded, and no less accurate than the two separate kernels
    gy, x, w = rand(54, B, M, HW), rand(55, B, N, HW), rand(56, M, N, scale=0.3)
    gx_ref = torch.einsum("mn,bmp->bnp", w.double(), gy.double()).reshape(B, -1)
    dw_ref = torch.einsum("bmp,bnp->mn", gy.double(), x.double())
    gx, dw = run_fused(dev, B, M, N, HW, gy, x, w)
    close(gx, gx_ref, what=f"gx {shape}")
    close(dw, dw_ref, what=f"dW {shape}")
    gx2 = run_pw(dev, B, N, M, HW, gy, w.t().reshape(1, N, M).contiguous(), None, 0, 0, 0)
    rc, dw2 = run_wgrad(dev, B, M, N, HW, gy, x, 0, 0, 0, 0)
    assert rc == 0
    for a, b, ref in ((gx, gx2, gx_ref), (dw, dw2[0], dw_ref)):
        ea, eb = (a - ref).abs().max().item(), (b - ref).abs().max().item()
        assert ea <= 2.0 * eb + 1e-6 * ref.abs().max().item(), (ea, eb)
