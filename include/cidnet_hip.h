/* cidnet_hip.h -- C ABI of libcidnet_hip.so: the MI355X (gfx950) kernels of the CIDNet
 * forward/backward hot path.
 *
 * The reference (KitaharaH/HVI-CIDNet) has no FFI: its boundary is the Python nn.Module API of
 * net/CIDNet.py.  Each entry point below replaces the group of ATen eager ops that one reference
 * call site executes (cited per function); hvi-cidnet_amd/ops.py wraps them as
 * torch.autograd.Function and hvi-cidnet_amd/{hvi_transform,transformer_utils,lca,cidnet}.py
 * re-expose the reference's module names on top.
 *
 * Conventions
 *   - all tensors are fp32, NCHW-contiguous device memory unless a stride argument says otherwise;
 *     "HW" planes are H*W floats; pointers are plain device pointers owned by the caller;  the one
 *     exception are the evaluation metrics (cidnet_metric_*), whose images are uint8 (B,3,h,w) and
 *     whose results are fp64 device buffers, the training-batch kernel (cidnet_augment_*), which reads a uint8 arena, and
 *     the image ingest / egress kernels (cidnet_image_*), whose byte side is interleaved (h,w,3) uint8 and whose
 *     tiled forms take int32 origin lists;
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream; NULL = default);
 *   - functions are stateless and re-entrant, never allocate, never synchronise and never copy to
 *     the host, so a caller may capture them into a hipGraph;  scratch memory comes in through
 *     `ws` / `ws_floats` arguments whose required size the matching *_ws_floats() reports;
 *   - return 0 on success, a negative CIDNET_ERR_* for rejected arguments, or a positive
 *     hipError_t if the launch failed.  Kernels never abort the process.
 */
#ifndef CIDNET_HIP_H
#define CIDNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIDNET_ABI_VERSION 29

int cidnet_abi_version(void);

/* element-type codes of the typed (`_t`) entry points: a tensor passed as `void*` with an `int <name>_dt` is stored as fp32
 * or bfloat16; strides and offsets stay in ELEMENTS */
#define CIDNET_F32 0
#define CIDNET_BF16 1

/* ---- K1: RGB -> HVI  (RGB_HVI.HVIT, net/HVI_transform.py:16-47; CIDNet.HVIT, net/CIDNet.py:124) --
 * rgb, hvi: (B,3,H,W).  density_k: device pointer to the scalar parameter (read on the device, so
 * the reference's k.item() host sync at :38 disappears).  branch_code (optional, B*H*W bytes):
 * bits0-1 hue branch (0 gray,1 R,2 G,3 B), bits2-3 arg-max channel, bits4-5 arg-min channel,
 * bit6 value==0 -- the mask decisions of :23-27,31, exported for the bit-exactness test. */
int cidnet_hvit_fwd(const float* rgb, const float* density_k, float* hvi, uint8_t* branch_code,
                    int B, int H, int W, void* stream);

/* Backward of HVIT: g_rgb (B,3,H,W, optional) and g_k (1 float, optional; fixed-order reduction,
 * bitwise reproducible).  ws: >= cidnet_hvit_bwd_ws_floats() floats when g_k != NULL. */
long cidnet_hvit_bwd_ws_floats(void);
int cidnet_hvit_bwd(const float* rgb, const float* density_k, const float* g_hvi, float* g_rgb,
                    float* g_k, float* ws, long ws_floats, int B, int H, int W, void* stream);

/* ---- K2: HVI -> RGB  (RGB_HVI.PHVIT, net/HVI_transform.py:49-122) ---------------------------
 * Input is hvi (B,3,H,W); when hv (B,2,H,W) and iv (B,1,H,W) are non-NULL the residual form of
 * net/CIDNet.py:119, cat([hv, iv], 1) + hvi, is evaluated in registers.  k = *k_dev if k_dev !=
 * NULL else k_host (`this_k`, a python float in the reference: no gradient reaches density_k).
 * gated/alpha_s, gated2/alpha: the inference-time scales of :69-70,120-121.  sextant (optional,
 * B*H*W bytes): floor(6h) per pixel, 6 = the black-pixel case. */
int cidnet_phvit_fwd(const float* hv, const float* iv, const float* hvi, const float* k_dev,
                     float k_host, int gated, float alpha_s, int gated2, float alpha, float* rgb,
                     uint8_t* sextant, int B, int H, int W, void* stream);

/* Backward of PHVIT wrt its (summed) input: g_hvi (B,3,H,W) and/or the same gradient split as
 * g_hv (B,2,H,W) + g_iv (B,1,H,W) for the two decoder heads. */
int cidnet_phvit_bwd(const float* hv, const float* iv, const float* hvi, const float* k_dev,
                     float k_host, int gated, float alpha_s, int gated2, float alpha,
                     const float* g_rgb, float* g_hvi, float* g_hv, float* g_iv, int B, int H, int W,
                     void* stream);

/* ---- K3: channels-first LayerNorm  (LayerNorm.forward, net/transformer_utils.py:24-29) ---------
 * x,y: (B,C,HW).  mean/rstd (B,HW each, optional pair) are saved for the backward. */
int cidnet_ln_cf_fwd(const float* x, const float* weight, const float* bias, float* y, float* mean,
                     float* rstd, int B, int C, long HW, float eps, void* stream);
long cidnet_ln_cf_bwd_ws_floats(int C);
/* gx optional (NULL: parameter gradients only); gw, gb: (C) each, overwritten. */
int cidnet_ln_cf_bwd(const float* x, const float* weight, const float* gy, const float* mean,
                     const float* rstd, float* gx, float* gw, float* gb, float* ws, long ws_floats,
                     int B, int C, long HW, void* stream);
/* Typed forms for the bf16 mode: the LayerNorm OUTPUT (it only feeds 1x1 convs, net/LCA.py:22-23,60) and the incoming
 * gradient (an output of those convs' data-gradient launches) may be stored as bf16; x, the statistics, gx and the
 * parameter gradients stay fp32.  bf16 only for cidnet_ln_cf_typed_supported shapes (C = 36 / 72 / 144), else
 * CIDNET_ERR_SHAPE. */
int cidnet_ln_cf_typed_supported(int B, int C, long HW);
int cidnet_ln_cf_fwd_t(const float* x, const float* weight, const float* bias, void* y, int y_dt, float* mean, float* rstd,
                       int B, int C, long HW, float eps, void* stream);
int cidnet_ln_cf_bwd_res_t(const float* x, const float* weight, const void* gy, int gy_dt, const float* mean,
                           const float* rstd, const float* addend, float* gx, float* gw, float* gb, int accumulate,
                           float* ws, long ws_floats, int B, int C, long HW, void* stream);
/* same, with gx += addend (the gradient that reaches x through the residual branch of the pre-norm block,
 * net/LCA.py:79,80,91,92): saves the separate accumulation pass.  addend may be NULL.  accumulate != 0: gw / gb are
 * added to instead of overwritten -- one LayerNorm module is applied two or three times per LCA (LCA.py:79-80,91-92)
 * and its uses then sum their parameter gradients in place, in backward order. */
int cidnet_ln_cf_bwd_res(const float* x, const float* weight, const float* gy, const float* mean, const float* rstd,
                         const float* addend, float* gx, float* gw, float* gb, int accumulate, float* ws,
                         long ws_floats, int B, int C, long HW, void* stream);

/* Two LayerNorm MODULES applied to one tensor (the x-norm of an LCA block and the y-norm of its partner block read the same
 * input, net/LCA.py:79-80,91-92 with net/CIDNet.py:83-84): one pass reads x and writes both outputs; one backward pass reads
 * x once and returns gx = LN'(gy*w + gy2*w2) (+ addend) and both modules' parameter gradients (each with its own
 * accumulate flag).  _supported: the shapes of the register-resident kernels (C = 36 with HW % 4 == 0, C = 72 with HW % 2 == 0,
 * C = 144 on planes of at most 2^18 pixels per batch); otherwise CIDNET_ERR_SHAPE -- call the single-module entry points. */
int cidnet_ln_cf_dual_supported(int B, int C, long HW);
long cidnet_ln_cf_bwd2_ws_floats(int C);
int cidnet_ln_cf_fwd2(const float* x, const float* weight, const float* bias, float* y, const float* weight2,
                      const float* bias2, float* y2, float* mean, float* rstd, int B, int C, long HW, float eps,
                      void* stream);
int cidnet_ln_cf_bwd2(const float* x, const float* weight, const float* gy, const float* weight2, const float* gy2,
                      const float* mean, const float* rstd, const float* addend, float* gx, float* gw, float* gb,
                      int accumulate, float* gw2, float* gb2, int accumulate2, float* ws, long ws_floats, int B, int C,
                      long HW, void* stream);

/* ---- K4: pointwise (1x1) convolution on the fp32 MFMA -----------------------------------------
 * (nn.Conv2d(k=1): net/LCA.py:13,15,17,51,57; net/transformer_utils.py:60)
 * Per sample b:  Y[b] (M x HW) = A_b (M x K) * X[b] (K x HW)  [+ R[b]],
 *   A_b[m][k] = Wt[b*w_bs + m*w_ms + k*w_ks]   (w_bs = 0: shared weights; forward: w_ms=K,w_ks=1;
 *   data gradient: w_ms=1, w_ks=<Cin>), X[b] at X + b*x_bs with channel stride HW (same for Y, R),
 *   so channel slices of wider tensors can be read / written in place.  R may alias Y. */
#ifdef CIDNET_DEBUG
/* timing-study switches for cidnet_pw_conv (bit0: no stores, bit1: no K loop; bit7: force the weight-gradient
 * kernel to (flags >> 8) * 128 pixels per block); 0 = production.  Only in -DCIDNET_DEBUG builds. */
void cidnet_debug_pw_flags(int flags);
#endif
/* Element-type codes of the `_t` entry points (row J1, bf16 storage mode): a tensor argument declared `void*` with an
 * `int <name>_dt` is fp32 (CIDNET_F32) or bfloat16 (CIDNET_BF16); strides stay in ELEMENTS.  Arithmetic is fp32 in
 * every kernel: bf16 is a storage format of activations / saved tensors (round to nearest even on store). */
int cidnet_pw_conv_t(const void* X, int x_dt, long x_bs, const float* Wt, long w_bs, long w_ms, long w_ks, void* Y,
                     int y_dt, long y_bs, const float* R, long r_bs, int B, int M, int K, long HW, void* stream);
int cidnet_pw_conv(const float* X, long x_bs, const float* Wt, long w_bs, long w_ms, long w_ks,
                   float* Y, long y_bs, const float* R, long r_bs, int B, int M, int K, long HW,
                   void* stream);
/* The same product on the BF16 matrix cores with exact three-way split operands (csrc/pwx.hip; fp32 tensors only): for
 * launches bound by the fp32 MFMA rate or by that kernel's instruction issue.  _supported: M > 16, HW >= 64 (any HW
 * from there: the last 64-pixel group of a plane is pulled back to the plane's end), K * HW and M * HW below 2^31.
 * ws: cidnet_pw_conv_bf16x3_ws_floats(B, M, K, w_bs != 0) floats, 16-byte aligned (the weights, split once per call into
 * MFMA fragment order). */
int cidnet_pw_conv_bf16x3_supported(int M, int K, long HW);
long cidnet_pw_conv_bf16x3_ws_floats(int B, int M, int K, int per_sample);
int cidnet_pw_conv_bf16x3(const float* X, long x_bs, const float* Wt, long w_bs, long w_ms, long w_ks, float* Y, long y_bs,
                          const float* R, long r_bs, float* ws, long ws_floats, int B, int M, int K, long HW, void* stream);
/* The same call in two halves, for callers that keep the prepared weight operand across calls (weights change once per
 * optimizer step, but are used by a forward and -- transposed -- a backward launch, and by every inference call):
 * _prep splits Wt into ws (nb sets: B for per-sample weights, w_bs != 0; else 1; ws as above with per_sample = 1 and
 * B = nb), _pre runs the product from it.  cidnet_pw_conv_bf16x3 == _prep + _pre.  _prep_batch prepares n shared (not
 * per-sample) weight tensors in ONE launch: `table` is a device array of n rows of 8 x int64 {Wt pointer, ws pointer,
 * M, K, w_ms, w_ks, first block of the row, 0}; a row takes cidnet_pw_conv_bf16x3_prep_blocks(M, K) blocks, rows in
 * ascending block order, total_blocks = their sum. */
int cidnet_pw_conv_bf16x3_prep(const float* Wt, long w_bs, long w_ms, long w_ks, float* ws, long ws_floats, int nb, int M,
                               int K, void* stream);
int cidnet_pw_conv_bf16x3_pre(const float* X, long x_bs, const float* Wprep, int per_sample, float* Y, long y_bs,
                              const float* R, long r_bs, int B, int M, int K, long HW, void* stream);
/* w_levels / x_levels: how many bf16 levels of the weights / activations enter the products (all pairs i + j <= 2):
 * (3, 3) = _pre, the fp32-exact six products; (1, 1) both operands rounded to nearest bf16 and ONE product -- the
 * arithmetic of a bf16 autocast convolution with fp32 accumulation and fp32 output (BASELINE.json configs[2]'s "bf16"
 * mode; the activation split disappears and the matrix-core work drops to a sixth).  Other pairs: CIDNET_ERR_ARG (the
 * 3x3 conv below also takes (3, 1): exact weights, rounded activations, three products).  The prepared operand is the
 * same for every pair. */
int cidnet_pw_conv_bf16x3_pre_lv(const float* X, long x_bs, const float* Wprep, int per_sample, float* Y, long y_bs,
                                 const float* R, long r_bs, int B, int M, int K, long HW, int w_levels, int x_levels,
                                 void* stream);
/* ... with typed activations / output (x_dt, y_dt: CIDNET_F32 / CIDNET_BF16, defined below; strides in elements): a tensor
 * STORED as bf16 is read without conversion (its one level) / written rounded to nearest; bf16 types need (1, 1) levels.
 * R stays fp32 (the residual stream). */
int cidnet_pw_conv_bf16x3_pre_t(const void* X, int x_dt, long x_bs, const float* Wprep, int per_sample, void* Y, int y_dt,
                                long y_bs, const float* R, long r_bs, int B, int M, int K, long HW, int w_levels,
                                int x_levels, void* stream);
long cidnet_pw_conv_bf16x3_prep_blocks(int M, int K);
int cidnet_pw_conv_bf16x3_prep_batch(const long long* table, int n, long total_blocks, void* stream);
/* Backward of a 1x1 convolution Y = W X (W: (M, N) contiguous) in one kernel: gX (B, N, HW) = W^T gY and dW (M, N) = sum over
 * samples and pixels of gY X^T (overwritten; partial sums combined in fixed order).  gY is read from HBM once instead of once
 * by the data-gradient launch (cidnet_pw_conv* with transposed strides) and once by cidnet_pw_wgrad*.  fp32 tensors, split
 * bf16 products as cidnet_pw_conv_bf16x3.  _supported: the IEL / CAB layer shapes of the 36-channel level (M x N tiles
 * 12x3, 3x6, 3x3, 5x3) with HW a multiple of 4; other shapes CIDNET_ERR_SHAPE -- use the two separate entry points. */
int cidnet_pw_bwd_fused_supported(int M, int N, long HW);
long cidnet_pw_bwd_fused_ws_floats(int B, int M, int N, long HW);
int cidnet_pw_bwd_fused(const float* gY, long gy_bs, const float* X, long x_bs, const float* Wt, float* gX, long gx_bs,
                        float* dW, float* ws, long ws_floats, int B, int M, int N, long HW, void* stream);
/* NormUpsample tail (net/transformer_utils.py:64-66): pre = Wt*X + bilinear_x2(Z), Y = PReLU(pre).
 * Z: (B,M,zh,zw) low-resolution, X: skip tensor (B,K,2zh,2zw), Y/Ypre: (B,M,2zh,2zw); Ypre may be NULL (inference). */
int cidnet_pw_conv_up_prelu(const float* X, long x_bs, const float* Wt, long w_ms, long w_ks,
                            const float* Z, const float* slope, float* Y, float* Ypre, int B, int M,
                            int K, int zh, int zw, void* stream);
/* Weight gradient dW[m][n] = sum_{b,p} dY[b][m][p] X[b][n][p]; per_sample: dW is (B,M,N) without
 * the batch sum.  dw_ld = row stride of dW (>= N).  Fixed-order reduction (reproducible).
 * flags: CIDNET_WGRAD_ACCUMULATE adds to dW instead of overwriting it; with fp32 operands the products run on the
 * BF16 matrix cores as six exact bf16 cross products each (results within fp32 rounding, see cidnet_conv3x3_bf16x3)
 * unless CIDNET_WGRAD_FP32_MFMA is set. */
#define CIDNET_WGRAD_ACCUMULATE 1
#define CIDNET_WGRAD_FP32_MFMA 2
/* both operands rounded to nearest bf16, one product per term (the bf16 mode; any storage types) */
#define CIDNET_WGRAD_BF16_1LEVEL 4
long cidnet_pw_wgrad_ws_floats(int B, int M, int N, long HW);
int cidnet_pw_wgrad_t(const void* dY, int dy_dt, long dy_bs, const void* X, int x_dt, long x_bs, float* dW, long dw_ld,
                      int per_sample, int flags, float* ws, long ws_floats, int B, int M, int N, long HW,
                      void* stream);
int cidnet_pw_wgrad(const float* dY, long dy_bs, const float* X, long x_bs, float* dW, long dw_ld,
                    int per_sample, int flags, float* ws, long ws_floats, int B, int M, int N,
                    long HW, void* stream);
/* The launch plan the 1x1 convolution launchers take for a problem; host only, launches nothing and touches no device.
 * Computed by the functions the launchers themselves call.  Writes the fields of `kind` to out[0..] (n_out >= 14 always
 * suffices):
 *  0  cidnet_pw_conv_t (epi 0; epi 1 with a residual R) and cidnet_pw_conv_up_prelu (epi 2: HW = 4 zh zw, W = 2 zw; W and zw
 *     are read by epi 2 only) with x_dt -> y_dt tensors: path (0 split-K kernel, 1 register-resident kernel, 2 LDS kernel,
 *     3 a ragged plane below one 256-pixel tile: only the checked tail kernel runs), main launches (2: split-K around
 *     K = 384; 0 for path 3), MT, LEFT (a block owns 16 MT + 4 LEFT output channels; the tail kernel MT + LEFT tiles),
 *     KS (k-steps in registers: KS of the register kernel, KSW of the first split-K launch; 0 otherwise), KS2 (KSW of the
 *     second split-K launch), kc (K rows per staged weight chunk of the LDS and tail kernels; 0 for split-K), K chunks,
 *     tpb (256-pixel tiles -- split-K: 64-pixel groups -- a block walks), grid x, grid y (grid z = B), tail (1: the
 *     plane's last tile, HW % 4 != 0 or HW < 4, follows in a launch of the checked kernel), the block count tpb aimed for
 *     (512 or 1024), dynamic LDS bytes (split-K: the reduction buffer; otherwise the weight chunk of the LDS / tail kernel)
 *  1  cidnet_pw_wgrad_t (dY M planes, X K planes): MT, NT (16-row tiles per block), nmb, nnb (blocks along M, N), pch (pixels
 *     per block), chunks (blocks along the plane), pixels of the last chunk, slabs summed per output without and with
 *     per_sample (B chunks, chunks); workspace = B chunks M K floats
 *  2  cidnet_pw_conv_bf16x3_pre_t: cpg (channels per lane group: 6 or 8; a k-block is 4 cpg channels), KB (k-blocks), MT
 *     (16-row tiles of M), WM (waves of a block on one pixel group), chunks (grid y), MTW (tiles per wave), block pixel
 *     tiles per sample (of 4 / WM x 64 pixels); prepared weights = KB MT 3 x 256 floats per set
 *  3  cidnet_pw_bwd_fused (gY M planes, X K planes): MT, NT, 32-pixel chunks per sample, blocks, most chunks of one block
 *     (block x walks chunks x, x + blocks, ... of the B samples' chunks)
 * x_dt, y_dt and epi are read by kind 0 only.  CIDNET_ERR_SHAPE where the path does not take the problem (kind 0: bf16 ->
 * bf16, epi 2 with a bf16 tensor; 2, 3: the *_supported predicates).  The tests assert through it that a case runs the
 * path it is there for. */
int cidnet_pw_plan(int kind, int B, int M, int K, long HW, int W, int zw, int x_dt, int y_dt, int epi, int* out, int n_out);

/* ---- K5 / K8: depthwise 3x3 (zero pad) and the IEL gate  (net/LCA.py:14,16,53-55,62-65) --------
 * out = dw3x3(in) [+ addend]; channel c uses w1[c] if c < csplit else w2[c-csplit] (weights (.,1,3,3));
 * flip != 0 applies the 180-degree rotated taps (= data gradient of the forward). */
#ifdef CIDNET_DEBUG
/* timing-study switch: force the strip height of the depthwise / gate kernels (0 = automatic) */
void cidnet_debug_dw_rows(int rows);
#endif
/* the strip tiling a dw.hip kernel family takes for this problem; launches nothing.
 * family: 0 forward (dw3x3, iel_gate_fwd/bwd), 1 iel_dw_gate_fwd, 2 dw3x3_wgrad / dw3x3_bwd, 3 iel_gate_dw_bwd.
 * planes is B*C (families 0, 2) or B*h (1, 3).  A lane owns `rows` rows of a 4-pixel column; nstrips = ceil(H / rows).
 * chunks = blocks per plane of the fused backward kernels (1 for families 0 and 1; cidnet_dw3x3_wgrad alone, which
 * reduces once per 256 items, launches four times as many).  The tests assert through it that a shape reaches the
 * strip height / chunk count it is there for. */
int cidnet_dw_tiling(int family, long planes, int H, int W, int* rows, int* nstrips, int* chunks);
int cidnet_dw3x3(const float* in, const float* w1, const float* w2, int csplit, const float* addend,
                 float* out, int flip, int B, int C, int H, int W, void* stream);
/* in / addend / out stored as fp32 or bf16 (one type, dt): the CAB's q / kv depthwise convs in the bf16 mode */
int cidnet_dw3x3_t(const void* in, const float* w1, const float* w2, int csplit, const void* addend, void* out, int dt,
                   int flip, int B, int C, int H, int W, void* stream);
/* ---- K8 fused: tile-resident IEL forward (net/LCA.py:60-67 [+ the residual of I_LCA, LCA.py:92]) -------------
 * out = [res +] W_out * ((tanh(dw1 u1) + u1) * (tanh(dw2 u2) + u2)),  [u1; u2] = dw(W_in * xn), in ONE kernel: the
 * hidden tensors live in LDS only (csrc/iel.hip).  xn, res, out: (B,C,H,W); w_in (2h,C), w_dw (2h,1,3,3),
 * w_dw1 / w_dw2 (h,1,3,3), w_out (C,h).  u (B,2h,H,W) is written when non-NULL (the backward reads it); res may be
 * NULL.  cidnet_iel_fwd_supported: channel counts the kernel is instantiated for (others: CIDNET_ERR_SHAPE). */
int cidnet_iel_fwd_supported(int C, int h);
int cidnet_iel_fwd(const float* xn, const float* res, const float* w_in, const float* w_dw, const float* w_dw1,
                   const float* w_dw2, const float* w_out, float* u, float* out, int B, int C, int h, int H, int W,
                   void* stream);
long cidnet_dw3x3_wgrad_ws_floats(int B, int C, int H, int W);
int cidnet_dw3x3_wgrad(const float* in, const float* gout, float* gw1, float* gw2, int csplit,
                       float* ws, long ws_floats, int B, int C, int H, int W, void* stream);
/* fused backward: gin = dw3x3(gout, flipped) [+ addend] and gw in ONE pass over (in, gout) */
int cidnet_dw3x3_bwd(const float* in, const float* gout, const float* w1, const float* w2, int csplit,
                     const float* addend, float* gin, float* gw1, float* gw2, float* ws,
                     long ws_floats, int B, int C, int H, int W, void* stream);
/* g = (tanh(dw1(u1)) + u1) * (tanh(dw2(u2)) + u2);  u: (B,2h,H,W) = [u1;u2], g: (B,h,H,W). */
/* u = dw3x3(pin, wdw) (2h channels) and g = gate(u) in one pass (net/LCA.py:61-65): u is written once and never re-read.
 * u may be NULL: inference, where only the backward would read u -- the kernel then stores g alone. */
int cidnet_iel_dw_gate_fwd(const float* pin, const float* wdw, const float* w1, const float* w2, float* u, float* g,
                           int B, int h, int H, int W, void* stream);
/* bf16 storage mode (row J1): the same three kernels with the IEL's hidden tensors (pin, u, g; dg, du; in, gout, gin)
 * stored in the element type `dt` (CIDNET_F32 / CIDNET_BF16); weights, weight gradients and arithmetic stay fp32. */
int cidnet_iel_dw_gate_fwd_t(const void* pin, const float* wdw, const float* w1, const float* w2, void* u, void* g, int dt,
                             int B, int h, int H, int W, void* stream);
int cidnet_iel_gate_dw_bwd_t(const void* u, const float* w1, const float* w2, const void* dg, void* du, int dt, float* gw1,
                             float* gw2, float* ws, long ws_floats, int B, int h, int H, int W, void* stream);
int cidnet_dw3x3_bwd_t(const void* in, const void* gout, const float* w1, const float* w2, int csplit, const void* addend,
                       void* gin, int dt, float* gw1, float* gw2, float* ws, long ws_floats, int B, int C, int H, int W,
                       void* stream);
int cidnet_iel_gate_fwd(const float* u, const float* w1, const float* w2, float* g, int B, int h,
                        int H, int W, void* stream);
/* da = d(dw1/2 output), ds = d(s1/s2) both (B,2h,H,W); du = ds + dw3x3(da, flipped) by the caller. */
int cidnet_iel_gate_bwd(const float* u, const float* w1, const float* w2, const float* dg, float* da,
                        float* ds, int B, int h, int H, int W, void* stream);
/* fused: du = ds + dw^T(da) with da, ds recomputed on the fly, plus the dwconv1/dwconv2 weight gradients;
 * HBM traffic: read dg (h) + u (2h), write du (2h) -- the unfused pair moved 15h channel passes */
long cidnet_iel_gate_dw_bwd_ws_floats(int B, int h, int H, int W);
int cidnet_iel_gate_dw_bwd(const float* u, const float* w1, const float* w2, const float* dg, float* du,
                           float* gw1, float* gw2, float* ws, long ws_floats, int B, int h, int H, int W,
                           void* stream);

/* ---- K9/K10/K11: dense 3x3 convolution, pad 1, fp32 MFMA implicit GEMM -------------------------
 * (net/transformer_utils.py:39,58 zero pad; net/CIDNet.py:21-24,32-35,39-42,50-53 replicate pad)
 * Y[b][m] = sum_{k,tap} Wt[m*w_ms + k*w_ks + tap'] * Xpad[b][k] ; forward: w_ms=9K, w_ks=9, flip=0;
 * data gradient of the zero-pad conv: X=dY, M=Cin, K=Cout, w_ms=9, w_ks=9*Cin, flip=1. */
#ifdef CIDNET_DEBUG
/* timing-study switches for cidnet_conv3x3 (1 no stores, 2 no window prefetch loads, 4 constant weights,
 * 8 MFMA path even for thin (<= 4 channel) layers, 16 padded 16-row tiles instead of 4x4x1 row groups,
 * 128 weight gradient: input-channel remainder as a padded 16-column tile instead of the 4-column-group launch) */
void cidnet_debug_c3_flags(int flags);
#endif
int cidnet_conv3x3(const float* X, long x_bs, const float* Wt, long w_ms, long w_ks, int flip,
                   int replicate, float* Y, long y_bs, int B, int M, int K, int H, int W, void* stream);
/* The same zero-pad convolution (net/transformer_utils.py:39,58 and its data gradient) with its fp32 operands split
 * into three bf16 values each and the six significant cross products run on the BF16 matrix cores (csrc/conv3x.hip):
 * results within fp32 rounding of cidnet_conv3x3 (products exact, fp32 accumulation, dropped terms <= 2^-25 relative),
 * on a pipe the VALU does not contend for.  R optional addend (batch stride r_bs).  ws (cidnet_conv3x3_bf16x3_ws_floats
 * floats, 16-byte aligned) receives the split weights in MFMA fragment order.  _supported: K a multiple of 36. */
int cidnet_conv3x3_bf16x3_supported(int M, int K);
long cidnet_conv3x3_bf16x3_ws_floats(int M, int K);
int cidnet_conv3x3_bf16x3(const float* X, long x_bs, const float* Wt, long w_ms, long w_ks, int flip, const float* R,
                          long r_bs, float* Y, long y_bs, float* ws, long ws_floats, int B, int M, int K, int H,
                          int W, void* stream);
/* In two halves (see cidnet_pw_conv_bf16x3_prep): _prep writes the prepared weights (flip folded in) to ws, _pre convolves
 * from them; _prep_batch: rows {Wt pointer, ws pointer, M, K, w_ms, w_ks, first block, flip},
 * cidnet_conv3x3_bf16x3_prep_blocks(M, K) blocks per row. */
int cidnet_conv3x3_bf16x3_prep(const float* Wt, long w_ms, long w_ks, int flip, float* ws, long ws_floats, int M, int K,
                               void* stream);
int cidnet_conv3x3_bf16x3_pre(const float* X, long x_bs, const float* Wprep, const float* R, long r_bs, float* Y, long y_bs,
                              int B, int M, int K, int H, int W, void* stream);
int cidnet_conv3x3_bf16x3_pre_lv(const float* X, long x_bs, const float* Wprep, const float* R, long r_bs, float* Y,
                                 long y_bs, int B, int M, int K, int H, int W, int w_levels, int x_levels, void* stream);
long cidnet_conv3x3_bf16x3_prep_blocks(int M, int K);
int cidnet_conv3x3_bf16x3_prep_batch(const long long* table, int n, long total_blocks, void* stream);
/* Y = conv3x3(X) + R (R of Y's shape, batch stride r_bs; NULL = plain conv).  Used by the data gradient of
 * NormDownsample when its input also feeds a skip connection (net/CIDNet.py:80-81,85-86): the skip's gradient is
 * added in the epilogue instead of by a separate pass over the tensor.  Layers with <= 4 channels on a side
 * (streaming kernels) do not take an addend: CIDNET_ERR_ARG. */
int cidnet_conv3x3_add(const float* X, long x_bs, const float* Wt, long w_ms, long w_ks, int flip,
                       int replicate, const float* R, long r_bs, float* Y, long y_bs, int B, int M, int K,
                       int H, int W, void* stream);
long cidnet_conv3x3_wgrad_ws_floats(int B, int M, int N, int H, int W);
int cidnet_conv3x3_wgrad(const float* dY, long dy_bs, const float* X, long x_bs, int replicate,
                         float* dW, float* ws, long ws_floats, int B, int M, int N, int H, int W,
                         void* stream);
/* The zero-pad weight gradient with split operands on the BF16 matrix cores (csrc/conv3xw.hip; arithmetic as
 * cidnet_conv3x3_bf16x3, partial sums combined in fixed order: run-to-run identical).  dW (M, N, 3, 3) contiguous is
 * overwritten.  _supported: N (input channels) a multiple of 36, W >= 4. */
int cidnet_conv3x3_wgrad_bf16x3_supported(int M, int N, int H, int W);
long cidnet_conv3x3_wgrad_bf16x3_ws_floats(int B, int M, int N, int H, int W);
int cidnet_conv3x3_wgrad_bf16x3(const float* dY, long dy_bs, const float* X, long x_bs, float* dW, float* ws,
                                long ws_floats, int B, int M, int N, int H, int W, void* stream);
/* levels: bf16 levels of BOTH operands that enter the products: 3 = the call above (six products, fp32-exact); 1 = operands
 * rounded to nearest bf16, one product (the bf16 mode, see cidnet_pw_conv_bf16x3_pre_lv) */
int cidnet_conv3x3_wgrad_bf16x3_lv(const float* dY, long dy_bs, const float* X, long x_bs, float* dW, float* ws,
                                   long ws_floats, int B, int M, int N, int H, int W, int levels, void* stream);
#ifdef CIDNET_DEBUG
/* timing-study switches for cidnet_conv3x3_wgrad_bf16x3 (1 stage only a block's first tile, 2 no fragment reads / MFMAs) */
void cidnet_debug_c3xw_flags(int flags);
#endif
/* Adds to gX (computed by the zero-pad data gradient) the taps that read replicated border pixels. */
/* The tiling the 3x3 convolution launchers take for a problem; host only, launches nothing and touches no device.  Computed
 * by the functions the launchers themselves call.  Writes the fields of `kind` to out[0..] (n_out >= 10 always suffices):
 *  0  cidnet_conv3x3 / _add (M outputs, K inputs): thin (1: the streaming kernels of kind 2 run instead), MT, LEFT, nmb
 *     (a block owns 16 MT + 4 LEFT output channels, nmb blocks cover M), LOGX (tile = 4 << LOGX pixels x 128 >> LOGX
 *     rows), tpb (row tiles a block walks), narrow (W < 8), row tiles, tiles across, blocks down (grid = across x down x B nmb)
 *  1  cidnet_conv3x3_wgrad (dY M planes, X K planes): path (0 MFMA, 1 narrow W < 8, 2 streaming kernels), MT, LEFT, nmb,
 *     nfull (16-wide input tiles), ngrp (4-wide groups of the input remainder, their own launch), rr (rows per chunk),
 *     rows of the last row chunk, chunks (workspace = B chunks M K 9 floats), work items (column tile x row chunk)
 *  2  the streaming forward kernels (min(M, K) <= 4): kernel (0 M-side, 1 K-side), strip rows, strips, rows of the last
 *     strip, dynamic LDS bytes
 *  3  the streaming weight-gradient kernels: chunks (workspace = B chunks M K 9 floats), strip rows, strips, rows of the last
 *  4  cidnet_conv3x3_bf16x3_pre_lv with `levels` activation levels (1 or 3): tiles_x, tiles_y, mchunks, kchunks, nwork (work
 *     items), grid blocks, 1 if the kernel deals work ids XCD-wise (grid a multiple of 8), most work items of a block
 *  5  cidnet_conv3x3_wgrad_bf16x3_lv (dY M planes, X K planes): chunk pairs, blocks per pair, tiles, fewest and most tiles
 *     of a block (workspace = pairs x blocks per pair x 108 x 108 floats)
 * `levels` is read by kinds 4 and 5 only.  CIDNET_ERR_SHAPE where the path does not take the shape (kinds 2, 3: not a thin
 * layer; 4, 5: the *_supported predicates).  The tests assert through it that a case runs the tiling it is there for. */
int cidnet_conv3x3_tiling(int kind, int B, int M, int K, int H, int W, int levels, int* out, int n_out);
int cidnet_conv3x3_replicate_dgrad_fix(const float* gY, const float* Wt, float* gX, int B, int Co,
                                       int Ci, int H, int W, void* stream);

/* ---- resampling / PReLU pieces of NormDownsample, NormUpsample ---------------------------------
 * (nn.UpsamplingBilinear2d == bilinear, align_corners=True; nn.PReLU with one slope) */
/* pre (the pre-activation, read only by cidnet_prelu_bwd) may be NULL: inference. */
int cidnet_down_prelu_fwd(const float* t, const float* slope, float* pre, float* out, int B, int C,
                          int H, int W, void* stream);
long cidnet_prelu_bwd_ws_floats(void);
int cidnet_prelu_bwd(const float* dout, const float* pre, const float* slope, float* dpre,
                     float* dslope, float* ws, long ws_floats, long n, void* stream);
/* adjoint of bilinear (Hi,Wi)->(Ho,Wo): din (B,C,Hi,Wi) from dout (B,C,Ho,Wo), gather form. */
long cidnet_bilinear_bwd_ws_floats(int Hi, int Wi);
int cidnet_bilinear_bwd(const float* dout, float* din, float* ws, long ws_floats, int B, int C, int Hi,
                        int Wi, int Ho, int Wo, void* stream);
/* In two halves: the per-axis tap tables depend on the four sizes only (cidnet_bilinear_bwd_ws_floats(Hi, Wi) floats), so a
 * caller may compute them once per shape (_tabs) and run the adjoint from them (_pre). */
int cidnet_bilinear_bwd_tabs(float* tabs, long tabs_floats, int Hi, int Wi, int Ho, int Wo, void* stream);
int cidnet_bilinear_bwd_pre(const float* dout, float* din, const float* tabs, int B, int C, int Hi, int Wi, int Ho, int Wo,
                            void* stream);
int cidnet_add(const float* a, const float* b, float* y, long n, void* stream);

/* ---- K7: channel attention of CAB  (net/LCA.py:26-38) -------------------------------------------
 * qkv: (B,3C,HW) = [q;k;v] after the depthwise convs.  Produces attn = softmax(normalize(q)
 * normalize(k)^T * temperature) per (b,head), the normalised logits shat, the row norms nq,nk (B,C)
 * and M[b] = Wp * blockdiag(attn[b]) (B,C,C) so that project_out(attn @ v) = M[b] * v[b].
 * normalize = 0 gives the TNSM attention (net/TNSM.py:98-104): raw q k^T logits, no L2 normalisation. */
long cidnet_attn_gram_ws_floats(int B, int C, int heads, long HW);
int cidnet_attn_fwd(const float* qkv, const float* temperature, const float* Wp, float* attn,
                    float* shat, float* nq, float* nk, float* M, float* ws, long ws_floats, int B,
                    int C, int heads, long HW, int normalize, void* stream);
/* qkv stored as fp32 or bf16 (qkv_dt: CIDNET_F32 / CIDNET_BF16); the Gram products stay on the fp32 MFMA */
int cidnet_attn_fwd_t(const void* qkv, int qkv_dt, const float* temperature, const float* Wp, float* attn, float* shat,
                      float* nq, float* nk, float* M, float* ws, long ws_floats, int B, int C, int heads, long HW,
                      int normalize, void* stream);
/* From dM (B,C,C): per-sample dWp_b (B,C,C), dT_b (B,heads), and Wqk (B,2C,2C) with
 * [dq;dk][b] = Wqk[b] * [q;k][b]  (softmax + L2-normalisation backward folded). */
int cidnet_attn_bwd(const float* dM, const float* Wp, const float* attn, const float* shat,
                    const float* nq, const float* nk, const float* temperature, float* dWp_b,
                    float* dT_b, float* Wqk, int B, int C, int heads, int normalize, void* stream);
/* out[i] = sum_r in[r*n + i] (fixed order) */
int cidnet_sum_rows(const float* in, int n_red, long n, float* out, void* stream);

/* ---- training-step pieces (train.py:56-73) ------------------------------------------------------
 * loss = mean(|out - gt|) (L1Loss, loss/losses.py:10-20) and grad = sign(out - gt)/n in one pass. */
long cidnet_l1_loss_ws_floats(void);
int cidnet_l1_loss(const float* out, const float* gt, float* grad, float* loss, float* ws,
                   long ws_floats, long n, void* stream);
/* y = x * s[0] * mult (s: device scalar, may be null = 1): the upstream factor d(total)/d(loss) of a loss's
 * backward, and the sign flip that gives the gradient wrt the target (train.py:62: gt_hvi = model.HVIT(gt_rgb)
 * is NOT detached, so density_k receives gradient through the target of every HVI-space term) */
int cidnet_scale(const float* x, const float* s, float mult, float* y, long n, void* stream);
/* Gradient of the HVI image at its three-way fan-out (net/CIDNet.py:73-77: `i = hvi[:,2,:,:].unsqueeze(1)` feeds the I stem,
 * hvi the HV stem; :119 `+ hvi` the output residual): out (B,3,HW) = ga + gc, plane 2 also + gi (B,1,HW).  Null inputs
 * count as zero.  Replaces autograd's two accumulation passes and the slice backward (fill + copy). */
int cidnet_hvi_grad_sum(const float* ga, const float* gc, const float* gi, float* out, int B, long HW, void* stream);
/* SSIM loss ("next" row f1): SSIM.forward, loss/losses.py:166-190 with map_ssim, loss/loss_utils.py:125-145:
 * 11x11 Gaussian window (sigma 1.5), zero padding 5, depthwise; loss = (1 - mean(ssim_map)) * weight (1 float on the
 * device).  dA/dB/dC (B,C,H,W each) are the per-pixel derivative maps the backward filters; ws: block partials.
 * The backward gives d(total)/d(img1) for a device scalar gloss = d(total)/d(loss); img2 (the ground truth) gets none. */
long cidnet_ssim_ws_floats(int B, int C, int H, int W);
int cidnet_ssim_fwd(const float* img1, const float* img2, float weight, float* loss, float* dA, float* dB,
                    float* dC, float* ws, long ws_floats, int B, int C, int H, int W, void* stream);
int cidnet_ssim_bwd(const float* img1, const float* img2, const float* dA, const float* dB, const float* dC,
                    const float* gloss, float weight, float* gimg1, int B, int C, int H, int W, void* stream);
/* EdgeLoss ("next" row f1): EdgeLoss.forward, loss/losses.py:41-65: laplacian(z) = z - G(U(G(z))) with G the 5x5
 * replicate-padded blur outer([.05 .25 .4 .25 .05]) and U = even pixels x4; loss = mean((lap(x) - lap(y))^2) * weight.
 * fwd saves lap = laplacian(x - y) (B,C,H,W); bwd gives d(total)/dx = gloss * 2 weight / n * (lap - G^T U G^T lap).
 * ws: B*C*H*W + 2048 floats. */
long cidnet_edge_ws_floats(int B, int C, int H, int W);
int cidnet_edge_fwd(const float* x, const float* y, float weight, float* loss, float* lap, float* ws,
                    long ws_floats, int B, int C, int H, int W, void* stream);
int cidnet_edge_bwd(const float* lap, const float* gloss, float weight, float* gx, float* ws, long ws_floats,
                    int B, int C, int H, int W, void* stream);
/* ---- "next" row f4: VGG19 perceptual loss pieces (loss/vgg_arch.py:217-239, loss/losses.py:126-142; the 3x3
 * convolutions are cidnet_conv3x3).  The VGG weights are frozen (requires_grad=False, vgg_arch.py:203-206): data
 * gradients only.
 * normalize: y = ((range_norm ? (x + 1) / 2 : x) - mean[c]) / std[c], x (B,3,HW), ImageNet mean / std (:211-214).
 * bias_relu: x += bias[c] in place (the 'convN_M' feature, taken BEFORE the ReLU), act = max(x, 0) (act may be NULL,
 *   or x itself for an in-place ReLU).  relu_bwd: gx = act > 0 ? g : 0.
 * maxpool2: nn.MaxPool2d(2, 2) (:196), output floor(H/2) x floor(W/2); bwd routes to the first maximum in scan order.
 * mse_loss: loss (+)= weight * mean((a - b)^2), grad = weight * 2 (a - b) / n (criterion 'mse', train.py:192). */
int cidnet_vgg_normalize(const float* x, float* y, int range_norm, int B, long HW, void* stream);
int cidnet_vgg_normalize_bwd(const float* g, float* gx, int range_norm, int B, long HW, void* stream);
int cidnet_bias_relu(float* x, const float* bias, float* act, int B, int C, long HW, void* stream);
int cidnet_relu_bwd(const float* g, const float* act, float* gx, long n, void* stream);
int cidnet_maxpool2_fwd(const float* x, float* y, long planes, int H, int W, void* stream);
int cidnet_maxpool2_bwd(const float* x, const float* gy, float* gx, long planes, int H, int W, void* stream);
long cidnet_mse_ws_floats(void);
int cidnet_mse_loss(const float* a, const float* b, float* grad, float* loss, float weight, int accumulate, float* ws,
                    long ws_floats, long n, void* stream);
/* torch.optim.Adam step (train.py:166) over one flat buffer; g is multiplied by grad_scale first
 * (1/world_size after a sum all-reduce).  step = 1-based update count. */
int cidnet_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_scale,
                     void* stream);
/* Guard in front of the Adam step, decided on the device (csrc/guard.hip).  g[0..n): the flat gradient after the all-reduce.
 *   sum   = sum of g[i]^2 in fp64: per-block partials in fixed slots of ws (cidnet_grad_guard_ws_doubles() doubles), added in
 *           a fixed order by one block in a second launch; no atomics, repeated calls are bit-identical
 *   norm  = sqrt(sum) * grad_scale            (the 2-norm of the averaged gradient, what clip_grad_norm_ sees under DDP)
 *   coef  = min(1, max_norm / (norm + 1e-6))  (torch's formula, norm_type = 2); 1 when max_norm <= 0 or is not finite
 *   apply = isfinite(sum) || !skip_nonfinite  (one NaN or +-Inf element makes the sum non-finite)
 * state  (2 int64, device, owned by the caller, zero at the start of a run): [0] steps applied, [1] steps skipped; the one
 *        matching `apply` is incremented.
 * record (4 fp32, device): [0] apply as 1.0 / 0.0, [1] grad_scale * coef, [2] 1 - beta1^t, [3] sqrt(1 - beta2^t) with t the
 *        applied count after this step (powers in fp64); read by cidnet_adam_step_dev.
 * log_row (4 fp64, device, may be NULL): [0] loss[0] (NaN when loss is NULL), [1] norm, [2] coef, [3] the applied count after
 *        this step when it was applied, -(applied count + 1) when it was skipped (so a skipped row is strictly negative).
 * loss: the step's scalar fp32 loss on the device, or NULL. */
long cidnet_grad_guard_ws_doubles(void);
int cidnet_grad_guard(const float* g, long n, float grad_scale, float max_norm, int skip_nonfinite, float beta1,
                      float beta2, const float* loss, double* ws, long ws_doubles, long* state, float* record,
                      double* log_row, void* stream);
/* cidnet_adam_step with grad_scale and the two bias corrections read from a cidnet_grad_guard record; when the record's
 * apply is 0, p, m and v are not touched. */
int cidnet_adam_step_dev(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, const float* record, void* stream);
/* Elementwise passes over slices of the trainer's flat fp32 buffers (csrc/accum.hip).  Common contract: any n >= 1, bases
 * aligned to 4 bytes only (a scalar head up to the first 16-byte boundary of the written buffer, 16-byte accesses in the
 * grid-stride body, a scalar tail); nothing outside [0, n) is read or written; no atomics; every fp32 operation is rounded
 * on its own (no fma), so repeated calls and a numpy fp32 restatement are bit-identical.
 *   grad_accumulate: dst[i] = first ? src[i] : dst[i] + src[i].  The gradient sum of an accumulated update (pass order is
 *                    the caller's launch order) and, with n = 1, the sum of its scalar losses.
 *   ema_update:      ema[i] = ema[i] + w * (p[i] - ema[i]) (three roundings), w = fp32(1 - decay) formed by the caller in
 *                    double.  record: a cidnet_grad_guard record or NULL; with a record whose apply ([0]) is 0 every block
 *                    returns before it touches ema (a skipped step does not pull the average towards unchanged weights).
 *                    A launch of its own behind cidnet_adam_step / cidnet_adam_step_dev on the same stream.
 *   swap:            exchanges a[0..n) and b[0..n) in place; the two ranges must not overlap (CIDNET_ERR_ARG).  Twice is the
 *                    identity, bit for bit. */
int cidnet_grad_accumulate(float* dst, const float* src, long n, int first, void* stream);
int cidnet_ema_update(float* ema, const float* p, long n, float w, const float* record, void* stream);
int cidnet_swap(float* a, float* b, long n, void* stream);
/* Per-tensor statistics of a flat fp32 buffer (csrc/tensor_stats.hip): which slice of the trainer's gradient / weight arena
 * went non-finite, and which one carries the norm.  The reference's tools for this are host-side (--grad_detect:
 * torch.autograd.set_detect_anomaly, train.py:47; the per-epoch preview image, train.py:84-89); the contract is this text.
 * buf[0..n) and T segments (off[t], len[t]), in ELEMENTS: any order, adjacent or not, overlapping or not, aligned to 4 bytes
 * only.  Nothing outside a segment is read.  With x_i = buf[off[t] + i] and s = scale, row t of out (T x 4 doubles) is
 *   [0] norm      = sqrt(sum of (double) x_i^2 over the FINITE x_i) * (double) s   (one NaN does not erase the rest)
 *   [1] maxabs    = max of |x_i| over the finite x_i (0 when none is finite) * (double) s
 *   [2] nonfinite = how many x_i are NaN or +-Inf, exact
 *   [3] first     = the smallest i with a non-finite x_i, -1 when there is none
 * An element is classified by its exponent bits first and then either added or counted; no fmax carries a NaN.
 * Tiles: segment t is cut into ceil(len[t] / 4096) tiles of 4096 elements (the last one shorter); the tiles of all segments,
 * segment after segment, are numbered 0 .. tiles - 1.  table (T + 2 tiles int32): table[t] = the number of segment t's
 * first tile; table[T + 2 j], table[T + 2 j + 1] = segment and index inside the segment of tile j.
 * Launch 1, one block of 256 threads per tile: thread h reads elements 1024 q + 4 h + 0..3 of the tile for q = 0..3 (one
 *   unaligned 16-byte load where all four are inside the tile, scalar loads for the tile's last 1..3), adds the squares in
 *   that order onto 0.0 in fp64 (the square of an fp32 value is exact there); in each wave of 64 the butterfly v += v[lane ^
 *   32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1, then ((wave 0 + wave 1) + wave 2) + wave 3 -> slot j of ws (32 bytes: sum, max, count, first).
 * Launch 2, one wave per segment: lane l adds the segment's slots l, l + 64, ... in that order onto 0.0, the same butterfly,
 *   and lane 0 writes the row.
 * No atomics, no hand-off between blocks inside a launch: bit-identical from call to call, and a segment's row does not depend
 * on which other segments the call has.
 * plan: host only, launches nothing; the function the launcher itself calls.  off, len: T host values.  Writes out[0..2] =
 *   tiles, workspace bytes (32 tiles), table length in int32 (T + 2 tiles); seg_tiles (T int32, may be NULL) = tiles per
 *   segment; table (may be NULL: sizes only) = the table above, table_ints its capacity.  off / len / out NULL, n_out < 3,
 *   T < 1, n < 1, a len < 1, an off < 0, off + len > n, or a table shorter than T + 2 tiles is CIDNET_ERR_ARG; T or tiles above
 *   2^30 is CIDNET_ERR_SHAPE (the tile numbers are int32, with room for a grid).  On an error nothing is written; never writes
 *   past out[2], seg_tiles[T - 1], table[T + 2 tiles - 1].
 * The launcher takes the HOST off / len (checked as by plan on every call; the device is not asked) and their device copies
 *   off_dev / len_dev (T int64 each), table_dev (the uploaded table), out (T x 4 doubles, device) and ws (32 tiles bytes,
 *   8-byte aligned).  A NULL pointer, a misaligned out or ws, or a scale that is negative, NaN or infinite is CIDNET_ERR_ARG
 *   (a norm has no sign to give; the trainer's 1 / (world passes) is positive), with plan's errors; a short workspace
 *   CIDNET_ERR_WS.  What off_dev / len_dev / table_dev hold is the caller's word: THEY MUST BE THE COPIES OF WHAT WAS CHECKED. */
int cidnet_tensor_stats_plan(const long* off, const long* len, long T, long n, long* out, int n_out, int* seg_tiles, int* table,
                             long table_ints);
int cidnet_tensor_stats(const float* buf, long n, const long* off, const long* len, long T, const long* off_dev,
                        const long* len_dev, const int* table_dev, float scale, double* out, void* ws, long ws_bytes,
                        void* stream);

/* ---- K13: SpatialAttention of the MSSA variant (net/CIDNet_MSSA.py:10-25) ------------------------
 * out = x * sigmoid(conv7x7([mean_c x, max_c x])), w: (1,2,7,7).  stats (B,2,H,W), amax (B,H,W int32)
 * and att (B,1,H,W) are saved for the backward. */
int cidnet_sa_fwd(const float* x, const float* w, float* stats, int* amax, float* att, float* out,
                  int B, int C, int H, int W, void* stream);
long cidnet_sa_bwd_ws_floats(int B, int H, int W);
int cidnet_sa_bwd(const float* x, const float* w, const float* stats, const int* amax,
                  const float* att, const float* g, float* gx, float* gw, float* ws, long ws_floats,
                  int B, int C, int H, int W, void* stream);

/* ---- K14: pieces of the TNSM variant (net/TNSM.py) ----------------------------------------------
 * adaptive avg + max pool to 1x1 (:39-40); amax = flat index of the maximum per (b,c) plane */
int cidnet_global_pool_fwd(const float* x, float* avg, float* mx, int* amax, int B, int C, long HW,
                           void* stream);
int cidnet_global_pool_bwd(const float* gavg, const float* gmx, const int* amax, float* gx, int B, int C,
                           long HW, void* stream);
/* DynamicNoiseMap global branch (:43-47) folded with noise_branch[2] (Wn) and final_conv (wf):
 * gf = sigmoid(W2 (relu(W1 avg) + relu(W1 mx))), vrow[k] = sum_c wf[c] gf[c] Wn[c][k], so that
 * noise_map = sigmoid(vrow . leaky(dw3x3(x))).  hsum: (B,R,3) saved for the backward. */
int cidnet_noise_global_fwd(const float* avg, const float* mx, const float* W1, const float* W2,
                            const float* Wn, const float* wf, float* hsum, float* gf, float* vrow,
                            int B, int C, int R, void* stream);
/* per-sample parameter-gradient partials (sum over B with cidnet_sum_rows) + gavg, gmx (B,C) */
int cidnet_noise_global_bwd(const float* avg, const float* mx, const float* W1, const float* W2,
                            const float* Wn, const float* wf, const float* hsum, const float* gf,
                            const float* gvrow, float* gW1_b, float* gW2_b, float* gWn_b, float* gwf_b,
                            float* gavg, float* gmx, int B, int C, int R, void* stream);
/* mode 0: y = leaky_relu(a, 0.2); 1: y = a * (b > 0 ? 1 : 0.2) (a = grad, b = forward output);
 * 2: y = sigmoid(a); 3: y = a * b * (1 - b) (a = grad, b = forward output) */
int cidnet_elementwise(int mode, const float* a, const float* b, float* y, long n, void* stream);
/* nm[b][p] = sigmoid(sum_c v[b][c] t[b][c][p]) and its backward (gt (B,C,HW), gv (B,C)) */
int cidnet_rowdot_sigmoid_fwd(const float* t, const float* v, float* nm, int B, int C, long HW,
                              void* stream);
int cidnet_rowdot_sigmoid_bwd(const float* gnm, const float* nm, const float* t, const float* v,
                              float* gt, float* gv, int B, int C, long HW, void* stream);
/* v' = v * sigmoid(ws[c] * nm) (:103-112); vin may be a channel slice (batch stride vin_bs) */
int cidnet_modulate_fwd(const float* vin, long vin_bs, const float* nm, const float* ws, float* vout,
                        int B, int C, long HW, void* stream);
long cidnet_modulate_bwd_ws_floats(int B, int C, long HW);
int cidnet_modulate_bwd(const float* vin, long vin_bs, const float* nm, const float* ws,
                        const float* gvout, float* gvin, long gvin_bs, float* gnm, float* gws_part,
                        int B, int C, long HW, void* stream);
/* out = nm * a + (1 - nm) * d (AdaptiveFilter :165-166) and its backward */
int cidnet_blend_fwd(const float* a, const float* d, const float* nm, float* out, int B, int C, long HW,
                     void* stream);
int cidnet_blend_bwd(const float* a, const float* d, const float* nm, const float* g, float* ga,
                     float* gd, float* gnm, int B, int C, long HW, void* stream);
/* F.interpolate(bilinear, align_corners=False) (CIDNet_TNSM.py:258); dst / gdst may be channel
 * slices of a wider tensor (batch stride in floats) */
int cidnet_resize_bilinear_fwd(const float* src, float* dst, long dst_bs, int B, int C, int Hi, int Wi,
                               int Ho, int Wo, void* stream);
int cidnet_resize_bilinear_bwd(const float* gdst, long gdst_bs, float* gsrc, int B, int C, int Hi,
                               int Wi, int Ho, int Wo, void* stream);

/* ---- the TNSM variant's extra objective (train_tnsm.py:68-72) ---------------------------------------------------
 * loss = weight * (mean|noise_map - (1 - sigmoid(mean_c|out_rgb - im|))| + mean|d_x noise_map| + mean|d_y noise_map|),
 * noise_map (B,C,H,W) = the fused noise map CIDNet_TNSM.forward returns in train mode (C = 3), out_rgb / im (B,3,H,W).
 * One pass: loss (device scalar) and the gradients wrt noise_map and out_rgb (either may be NULL).
 * ws: cidnet_tnsm_noise_loss_ws_floats() floats. */
long cidnet_tnsm_noise_loss_ws_floats(void);
int cidnet_tnsm_noise_loss(const float* noise_map, const float* out_rgb, const float* im, float weight, float* loss,
                           float* g_noise, float* g_out, float* ws, long ws_floats, int B, int C, int H, int W,
                           void* stream);

/* ---- Evaluation metrics (eval.py:40-80 + measure.py:23-150 of the reference): quantize the model output, then PSNR and
 * SSIM against the ground truth, optionally after the "GT mean" rescale (gt_mean_scale).  Images are uint8 (B,3,h,w) device tensors;
 * results are one fp64 value per image in caller-owned device buffers (double* -- no host scalar, no synchronisation).
 * to_uint8: q = (uint8) trunc(clamp(x, 0, 1) * 255.0f) of the top-left h x w crop of x (B,3,Hp,Wp) (eval.py:69-73 with
 *   ToPILImage's pic.mul(255).byte(); NaN -> 0).
 * psnr_ssim: psnr[b] = 10 log10(255^2 / (mean((a - g)^2) + 1e-8)) over the 3 h w values (measure.py:66-71; squared errors
 *   summed exactly); ssim[b] = mean over the three planes of the mean SSIM map on the valid region of the 11 x 11
 *   Gaussian window (sigma 1.5), C1 = (0.01 255)^2, C2 = (0.03 255)^2, fp64 (measure.py:23-64).  scale NULL: plain.  scale =
 *   B doubles on the device (GT mean; what gt_mean_scale forms): a is first replaced by clip(a * scale[b], 0, 255) (fp64; PSNR
 *   reads its fp32 cast).  psnr or ssim may be NULL; with ssim, h < 11 or w < 11 is CIDNET_ERR_SHAPE.  Fixed-order
 *   reductions: bit-identical results from call to call, and an image's values do not depend on the rest of the batch.
 *   ws: cidnet_metric_ws_floats(B, h, w) floats (the tile partials), 8-byte aligned.
 * gt_mean_scale: the "GT mean" rescale of measure.py:138-141, formed once for every paired metric (psnr_ssim here, the LPIPS
 *   ingest and CIEDE2000 below): scale[b] = mean(gray(gt_b)) / mean(gray(restored_b)), gray = (4899 R + 9617 G + 1868 B + 8192)
 *   >> 14 on the 8-bit values, summed exactly in integers, then ((double) sum_gt / n) / ((double) sum_restored / n) with n = h w.
 *   An image whose gray mean is 0 gets an infinite or NaN scale; the users clip in fp64 and let a NaN through, as np.clip
 *   does.  Any h, w >= 1.  B > 65535 is CIDNET_ERR_SHAPE.  ws: cidnet_metric_gt_mean_scale_ws_floats(B, h, w) = 2 * B * chunks
 *   * 2 floats (16384 pixels per chunk), 8-byte aligned. */
int cidnet_metric_to_uint8(const float* x, uint8_t* q, int B, int Hp, int Wp, int h, int w, void* stream);
long cidnet_metric_gt_mean_scale_ws_floats(int B, int h, int w);
int cidnet_metric_gt_mean_scale(const uint8_t* restored, const uint8_t* gt, double* scale, float* ws, long ws_floats, int B, int h,
                                int w, void* stream);
long cidnet_metric_ws_floats(int B, int h, int w);
int cidnet_metric_psnr_ssim(const uint8_t* restored, const uint8_t* gt, const double* scale, double* psnr, double* ssim, float* ws,
                            long ws_floats, int B, int h, int w, void* stream);

/* ---- Resize of the quantized output to the ground truth's size (measure.py:133-134, measure_SID_blur.py:91-92: im1 =
 * im1.resize(im2.size), Pillow's default filter on an 8-bit RGB image: antialiased bicubic, a = -0.5, fixed point).  src
 * (B,3,h_in,w_in) -> dst (B,3,h_out,w_out), planar uint8 on the device.  Per axis the caller supplies Pillow's tables for
 * (n_in, n_out) as int32 device arrays (hvi-cidnet_amd/metrics.py: resize_plan): bounds (n_out,2) = first tap, tap count;
 * coeffs (n_out,ksize) = the taps' coefficients scaled by 2^22, rows padded with zeros.  One pass writes
 *   out = clamp((2^21 + sum_{k < count} in[first + k] * coeffs[o, k]) >> 22, 0, 255)   (int32 accumulator, arithmetic shift).
 * The horizontal pass (bounds_x, coeffs_x, ksize_x: w_in -> w_out) runs first into tmp (B,3,h_in,w_out), then the vertical
 * one (bounds_y, coeffs_y, ksize_y: h_in -> h_out) into dst; each rounds to uint8, so the order is part of the contract.  A
 * pass whose axis keeps its size is skipped (its tables may be NULL, no rounding happens) and tmp is then unused (may be
 * NULL); with both sizes kept dst receives a copy of src.  tmp: cidnet_metric_resize_ws_bytes(...) bytes (host only, launches
 * nothing; 0 when at most one pass runs).  The tables live on the device and cannot be checked here without a copy: THEY MUST
 * HOLD n_out ROWS OF ksize COEFFICIENTS; the kernels hold first and count inside the source axis and the row whatever a
 * broken table says, so only bytes of src / tmp are ever read.  B * 3 * h * w >= 2^31 for src, dst or a needed tmp is
 * CIDNET_ERR_SHAPE.  No atomics, no reductions: a byte depends on its own taps alone, bit-identical from call to call and
 * independent of the rest of the batch. */
long cidnet_metric_resize_ws_bytes(int B, int h_in, int w_in, int h_out, int w_out);
int cidnet_metric_resize_u8(const uint8_t* src, uint8_t* dst, uint8_t* tmp, const int* bounds_x, const int* coeffs_x, int ksize_x,
                            const int* bounds_y, const int* coeffs_y, int ksize_y, int B, int h_in, int w_in, int h_out,
                            int w_out, void* stream);

/* ---- NIQE features (measure_niqe_bris.py -> loss/niqe_utils.py: calculate_niqe with its defaults): the no-reference
 * score of the unpaired sets, per image up to its (blocks, 36) feature matrix; the 36 x 36 tail (nanmean, covariance,
 * pinv) is the caller's, on the host.  Images are uint8 (B,3,h,w), h, w >= 96; hc = h / 96 * 96, wc = w / 96 * 96; blocks
 * are 96 x 96 (48 x 48 at the half-size scale), counted in column-major order (for w: for h), blocks = (hc / 96)(wc / 96).
 * window: the 7 x 7 `gaussian_window` of niqe_pris_params.npz, 49 fp64 values on the device.  tables: 4 x 9801 fp64 values
 * on the device over alpha[k] = np.arange(0.2, 10.001, 0.001)[k] (estimate_aggd_param): r_gam = gamma(2/a)^2 / (gamma(1/a)
 * gamma(3/a)) | sqrt(gamma(1/a) / gamma(3/a)) | gamma(2/a) / gamma(1/a) | alpha.  Every rounding of the reference is kept:
 * luma: y = (uint8) rint(fp32(fp32((24.966 R' + 128.553 G' + 65.481 B' + 16) / 255) * 255.0f)), R' = fp32(R) / 255.0f, the dot
 *   product in fp64, of the top-left hc x wc crop -- the reference passes RGB to a BGR routine (to_y_channel, bgr2ycbcr),
 *   and that effective rule is the contract.
 * half: out (B,h/2,w/2) = the antialiased bicubic imresize(img / 255, 0.5) * 255 of img (B,h,w; uint8, or fp32 when img_f32
 *   != 0; h, w even): taps [-3 -9 29 111 111 29 -9 -3] / 256 on inputs 2k-3 .. 2k+4, symmetric reflection, output rows
 *   first (into `rows`, (B,h/2,w) floats of scratch), then columns, fp64 sums rounded to fp32 once per pass (the reference
 *   sums the taps in fp32: up to 2 fp32 ulps apart).
 * moments: per block of img (B,h,w; uint8 or fp32; h, w multiples of block = 96 or 48) the MSCN values (img - mu) /
 *   (sigma + 1), mu = fp32(G * img), sigma = sqrt(|fp32(G * fp32(img^2)) - mu^2|) in fp32, the window sums in fp64 with a
 *   replicated border (niqe(): scipy's convolve on fp32 arrays), and from them moments (B,blocks,5,6) fp64: for the block
 *   and for the block times itself rolled inside the block by (0,1), (1,0), (1,1), (1,-1) (compute_feature; the product
 *   rounded to fp32) the count and sum of squares of the negatives, the same of the positives, sum |v| and sum v^2.
 *   mscn (optional, (B,h,w) fp32) receives the map; without it the map never leaves the compute unit.
 * fit: for each of n_blocks blocks (5 fits, 6 sums each) the 18 features of compute_feature at feat + block * feat_stride:
 *   alpha, (beta_l + beta_r) / 2, then per rolled map alpha, mean, beta_l, beta_r; alpha is the FIRST minimum of
 *   (r_gam - rhatnorm)^2, entry 0 when rhatnorm is NaN (numpy's argmin), and NaN propagates into the betas as in numpy.
 * features: all of the above for rgb (B,3,h,w): feat (B,blocks,36) fp64 = scale-1 features | half-size-scale features.
 *   ws: cidnet_metric_niqe_ws_floats(B, h, w) floats, 8-byte aligned.  h < 96 or w < 96 is CIDNET_ERR_SHAPE.
 * Fixed-order reductions: bit-identical results from call to call, independent of the rest of the batch. */
int cidnet_metric_niqe_luma(const uint8_t* rgb, uint8_t* y, int B, int h, int w, int hc, int wc, void* stream);
int cidnet_metric_niqe_half(const void* img, int img_f32, float* rows, float* out, int B, int h, int w, void* stream);
int cidnet_metric_niqe_moments(const void* img, int img_f32, const double* window, int block, float* mscn, double* moments,
                               int B, int h, int w, void* stream);
int cidnet_metric_niqe_fit(const double* moments, const double* tables, int block, double* feat, int feat_stride,
                           long n_blocks, void* stream);
long cidnet_metric_niqe_ws_floats(int B, int h, int w);
int cidnet_metric_niqe_features(const uint8_t* rgb, const double* window, const double* tables, double* feat, float* ws,
                                long ws_floats, int B, int h, int w, void* stream);

/* ---- LOE, the lightness order error (Wang et al. 2013, the paper of the NPE set): the second no-reference number of the
 * unpaired sets beside NIQE.  The reference has no LOE; the contract is this text.  low, out: planar uint8 (B,3,h,w) on the
 * device, the image as supplied and its enhancement.  Lightness L(p) = max(R, G, B) of a pixel, 0..255.  The sampling grid
 * is the caller's `step` (hvi-cidnet_amd/metrics.py: loe_grid): rows = h / step, cols = w / step (integer division), sample
 * (i, j) is pixel (i step, j step), m = rows cols; only those pixels are read.  With U(a, b) = 1 if a >= b else 0, L from low
 * and Le from out:
 *   num[b] = sum over all m x m ordered sample pairs (x, y), y = x included, of U(L(x), L(y)) xor U(Le(x), Le(y))   (int64)
 *   loe[b] = (double) num[b] / (double) m, the classic form, 0 .. m.  num is always exact; for m <= 2^26 it is below 2^53, so
 *   the division is the only rounding (beyond that, up to the 2^30 limit below, the conversion of num rounds as well).
 * Formed from the 256 x 256 joint histogram of (L, Le) (csrc/loe.hip: the identity and the two launches), so the cost is
 * O(m + 65536) per image.  ws: cidnet_metric_loe_ws_bytes(B) bytes, 16-byte aligned: B x 65536 32-bit bins, zeroed inside
 * the call.  low / out / num / loe / ws NULL, a misaligned ws, B, h, w or step < 1, or step > min(h, w) is CIDNET_ERR_ARG; a
 * short workspace CIDNET_ERR_WS; m > 2^30 or B > 65535 CIDNET_ERR_SHAPE.  Integer atomics only (no floating-point atomics, no
 * hand-off between blocks inside a launch): bit-identical from call to call, and an image's values do not depend on the rest
 * of the batch.
 * plan: host only, launches nothing; the function the launcher itself calls.  Writes out[0..5] = rows, cols, blocks per image
 *   of the histogram launch, samples per block (blocks x samples >= m), counter bits of a block's LDS sub-histogram (16: a
 *   block takes fewer than 2^16 samples, so a counter cannot carry into the one packed beside it), dynamic LDS bytes per block.
 *   out NULL or n < 6 is CIDNET_ERR_ARG and nothing is written; never writes past out[5]; the size errors are those above. */
long cidnet_metric_loe_ws_bytes(int B);
int cidnet_metric_loe_plan(int h, int w, int step, int* out, int n);
int cidnet_metric_loe_u8(const uint8_t* low, const uint8_t* out, int B, int h, int w, int step, long long* num, double* loe,
                         void* ws, long ws_bytes, void* stream);

/* ---- JPEG file round trip (eval.py saves a .jpg input's output under the input's name: Pillow writes a quality-75 4:2:0
 * baseline JPEG, and measure_niqe_bris.py scores what that file decodes to).  src (B,3,h,w) -> dst (B,3,h,w), planar uint8 on
 * the device: dst is what Image.open() returns for the file Image.save(f, 'JPEG', quality=q) writes of src, byte for byte,
 * without the file -- the entropy coder is lossless, so only the lossy stages run, all in libjpeg's 32-bit fixed point
 * (csrc/jpeg.hip): RGB -> YCbCr, h2v2 downsampling of the edge-replicated chroma (the DOWNSAMPLED rows are
 * replicated to whole blocks), jfdctint's forward DCT, c = sign(v) ((|v| + 4 t) / (8 t)) t per coefficient, jidctint's inverse
 * DCT, "fancy" h2v2 upsampling of the (ceil(h/2), ceil(w/2)) chroma planes, YCbCr -> RGB.
 * qtab: 256 int32 on the device (hvi-cidnet_amd/metrics.py: jpeg_quant_plan): for luma, then chroma, the 64 table entries t
 *   (1..255, natural row-major order) and then the 64 constants ceil(2^32 / (8 t)): the quotient is the high word of
 *   (|v| + 4 t) * constant, exact for every numerator below 2^16.  The table lives on the device and cannot be checked here
 *   without a copy; no address depends on it, so a broken table gives wrong bytes and nothing else.
 * ws: cidnet_metric_jpeg_ws_bytes(B, h, w) bytes (host only; 0 for sizes the launcher refuses), 16-byte aligned: per image the
 *   decoded luma plane and the two chroma planes over whole MCUs, 384 bytes per 16 x 16 MCU.
 * src / dst / ws / qtab NULL, a misaligned ws or qtab, B or h < 1, or w < 5 is CIDNET_ERR_ARG (libjpeg's decoder reads padded
 * columns of a chroma plane narrower than three samples: not reproduced); a short workspace CIDNET_ERR_WS; h or w > 65500
 * (no such file exists), more than 2^22 MCUs, or B > 65535 CIDNET_ERR_SHAPE.  Integer arithmetic only, no atomics, no
 * reductions: a byte depends on its own MCU and its chroma neighbours alone, bit-identical from call to call and independent of
 * the rest of the batch.  src and dst must not overlap.
 * plan: host only, launches nothing; the function the launcher itself calls.  Writes out[0..8] = MCU columns, MCU rows,
 *   whether the right MCUs are partial (w % 16 != 0), whether the bottom ones are (h % 16 != 0), rows and columns of a chroma
 *   plane, workgroups per MCU row of the first launch (8 MCUs each), its workgroups per image, workspace bytes per image.
 *   out NULL or n < 9 is CIDNET_ERR_ARG and nothing is written; never writes past out[8]; the size errors are those above. */
long cidnet_metric_jpeg_ws_bytes(int B, int h, int w);
int cidnet_metric_jpeg_plan(int h, int w, int* out, int n);
int cidnet_metric_jpeg_roundtrip_u8(const uint8_t* src, uint8_t* dst, void* ws, long ws_bytes, const int* qtab, int B, int h,
                                    int w, void* stream);

/* ---- Training batches from a resident uint8 set (data/data.py:6-12 transform1 + train.py:54-56 of the reference): random
 * crop, horizontal / vertical flip, ToTensor and the gamma power of one batch, low image and ground truth, in one launch.
 * arena: uint8 device memory holding every image of the set as planar (3,h,w).  plan: B rows of 8 int64 words on the device:
 *   byte offset of the low image in the arena | byte offset of its ground truth | h | w | y0 | x0 | flips (bit 0 horizontal,
 *   bit 1 vertical) | 0.  x, gt: (B,3,Sh,Sw) fp32.  With yy = y0 + (vflip ? Sh-1-i : i), xx = x0 + (hflip ? Sw-1-j : j):
 *   gt[s,c,i,j] = fp32(high[c,yy,xx]) / 255.0f, a correctly rounded division (ToTensor);
 *   x[s,c,i,j] = table[low[c,yy,xx]], table = 256 fp32 values on the device, pow(q / 255, gamma) per level as the caller
 *   rounded it (hvi-cidnet_amd/data.py: fp64 pow, rounded once); table == NULL: the quotient itself (gamma off).
 * Only bytes inside the crop windows are read.  The plan lives on the device and cannot be checked here without a copy:
 * EVERY ROW MUST HAVE BEEN RANGE-CHECKED ON THE HOST WHERE IT WAS MADE (0 <= y0 <= h-Sh, 0 <= x0 <= w-Sw, both images inside
 * the arena).  B * 3 > 65535 is CIDNET_ERR_SHAPE.  A value depends on its plan row alone: bit-identical from call to call
 * and independent of the rest of the batch. */
int cidnet_augment_crop_flip(const uint8_t* arena, const long* plan, const float* table, float* x, float* gt, int B, int Sh,
                             int Sw, void* stream);

/* ---- The same batch with the un-powered low image beside it (train_tnsm.py:55,68 of the reference: the network is fed
 * `im1 ** gamma`, the noise-consistency term of its loss is computed against the raw im1).  arena, plan, table, x, gt, the
 * window arithmetic and the limits are exactly those of cidnet_augment_crop_flip; in addition
 *   raw[s,c,i,j] = fp32(low[c,yy,xx]) / 255.0f, the same correctly rounded quotient as gt's, (B,3,Sh,Sw) fp32.
 * table == NULL is allowed: x and raw then both receive the quotient.  The low image's bytes are read once and looked up in
 * both tables: a launch moves B*3*Sh*Sw*(2 + 12) bytes, where two launches of the sibling (gamma on, gamma off) move
 * B*3*Sh*Sw*(4 + 16).  Only bytes inside the crop windows are read, nothing outside the three (B,3,Sh,Sw) tensors is
 * written; THE PLAN ROWS MUST HAVE BEEN RANGE-CHECKED ON THE HOST, as for the sibling.  B * 3 > 65535 is CIDNET_ERR_SHAPE.
 * A value depends on its plan row alone: bit-identical from call to call and to what the sibling writes for the same row. */
int cidnet_augment_crop_flip_raw(const uint8_t* arena, const long* plan, const float* table, float* x, float* raw, float* gt,
                                 int B, int Sh, int Sw, void* stream);

/* ---- Image files in and out (eval.py:60-75, eval_SID_blur.py, demo.py:40-60, app.py:33-53 of the reference: PIL image ->
 * ToTensor -> reflect pad to a multiple of 8 -> ** gamma -> model -> clamp -> crop -> ToPILImage -> save): the two conversions
 * between the interleaved (h,w,3) uint8 bytes of PIL / numpy / every file format and the planar fp32 (B,3,Hp,Wp) tensor of the
 * model, so that an image crosses the host link as 3 bytes per pixel in both directions.  The byte side holds B images, image
 * b at base + b * bs bytes (src_bs / dst_bs >= 3 h w; any byte alignment of base and bs); the fp32 side is contiguous.
 * ingest: for i < Hp, j < Wp, with ri = i < h ? i : 2(h-1) - i and rj = j < w ? j : 2(w-1) - j (F.pad(..., 'reflect') at the
 *   bottom and right: eval_sets.py:22-28, demo.py:47-52, app.py:35-40):  x[b,c,i,j] = T[src_b[ri,rj,c]].  table: 256 fp32
 *   values on the device, pow(q / 255, gamma) per level as the caller rounded it (hvi-cidnet_amd/data.py: gamma_table); table
 *   == NULL: T[q] = fp32(q) / 255.0f, a correctly rounded division (ToTensor).  Hp < h, Wp < w, Hp - h > h - 1 or Wp - w > w - 1
 *   is CIDNET_ERR_SHAPE (a reflection needs the pad to be smaller than the side); Hp and Wp need not be multiples of anything.
 * egress: for i < h, j < w:  dst_b[i,j,c] = (uint8) trunc(clamp(x[b,c,i,j], 0, 1) * 255.0f), NaN -> 0 (eval.py:69-73 with
 *   ToPILImage's pic.mul(255).byte()): value for value what cidnet_metric_to_uint8 writes, interleaved.  h > Hp or w > Wp is
 *   CIDNET_ERR_SHAPE.  Exactly the 3 h w bytes of each image are written: not one byte of the slack between images or after
 *   the last one is touched.
 * Both: only the 3 h w bytes of an image are ever read on the byte side.  bs < 3 h w, B > 65535 or more than 2^30 groups of
 * four pixels per image is CIDNET_ERR_SHAPE.  No atomics, no reductions: a value depends on its own image alone, bit-identical
 * from call to call and independent of the rest of the batch. */
int cidnet_image_ingest(const uint8_t* src, long src_bs, const float* table, float* x, int B, int h, int w, int Hp, int Wp,
                        void* stream);
int cidnet_image_egress(const float* x, uint8_t* dst, long dst_bs, int B, int Hp, int Wp, int h, int w, void* stream);

/* ---- PNG files written from the device (csrc/png.hip, csrc/png_codes.h; tests/png_ref.py restates the
 * stream in numpy and is the contract, byte for byte).  src: B interleaved (h,w,3) uint8 images, image b at src + b *
 * src_stride (>= 3 h w, any byte alignment) -> slot b at dst + b * dst_stride: the complete zlib stream of the image's one IDAT
 * chunk, sizes[b] bytes of it (int64), the rest of the slot's first `capacity` bytes zero.  The host adds the signature, IHDR,
 * the chunk lengths and CRC-32s.
 *   Rows: one type byte + 3 w filtered bytes, PNG's filters with bpp = 3 (left / up / up-left 0 outside the image, Avg =
 *   floor((left + up) / 2), Paeth ties left, up, up-left).  filter 0..4 forces None / Sub / Up / Avg / Paeth on every row; 5
 *   (adaptive) takes per row the type with the smallest sum of min(v, 256 - v) over its filtered bytes, ties to the lowest type;
 *   every candidate is computed from the RAW previous row, so rows are independent.
 *   Segments: R = max(1, segment_bytes / (1 + 3 w)) whole rows each, the last possibly fewer; one deflate block (BTYPE 2) per
 *   segment, BFINAL on the last, concatenated at bit granularity.  Literals only: HLIT = 0 (257 codes: the byte counts and the
 *   end of block with count 1), HDIST = 1 (two distance codes of length 1), HCLEN = 15, the 259 lengths sent as plain symbols
 *   0..15.  Code lengths: cidnet_png_code_lengths' procedure, limit 15, and limit 7 for the code-length code (one used symbol
 *   there: symbol 0, or 1 if 0 is the used one, also gets length 1).  Codes canonical (RFC 1951 3.2.2).
 *   Framing: 0x78 0x01, the blocks, zero bits to the next byte, Adler-32 of the filtered bytes, big-endian.
 * ws: B * plan[4] bytes, 16-byte aligned (filtered bytes and one record per segment).  dst 4-byte aligned, dst_stride a multiple
 * of 4 and >= the plan's capacity; sizes 8-byte aligned.  Nothing outside the first `capacity` bytes of the B slots, sizes[0..B)
 * and the workspace is written.  Integer arithmetic only; the only atomics are integer ORs and adds whose result does not depend
 * on their order: the bytes are identical from call to call and independent of the rest of the batch.  Three launches.
 * CIDNET_ERR_ARG, before any launch: a NULL pointer, B, h, w or segment_bytes < 1, filter outside 0..5, a slot below the
 *   capacity, a misaligned dst / dst_stride / ws / sizes, src_stride < 3 h w.  CIDNET_ERR_WS: a short workspace.
 *   CIDNET_ERR_SHAPE: a segment (or a single row) of more than 2^22 bytes -- a count must fit the sort key of the code-length
 *   procedure -- or B > 65535.
 * plan: host only, launches nothing; the function the launcher itself calls.  out[0..5] = rows per segment R, segments, whether
 *   the last segment is short, whether one row exceeds segment_bytes, workspace bytes per image, the capacity of one slot: a
 *   proven bound on the stream's size (per segment of n symbols 1887 header bits and 9 n bits where n < 2584, else 11 n; the
 *   proof is with png_plan in csrc/png.hip), a multiple of 4.  out NULL or n < 6 is CIDNET_ERR_ARG and nothing is written.
 * code_lengths: host only; the procedure the kernel runs, for the tests.  freq[0..n) counts (each < 2^23), n <= 257 -> lens[0..n):
 *   used symbols ascending by (count, symbol); two-queue merge, leaves in that order, internal nodes in creation order, the
 *   smaller head first and the leaf on equal weight; depth = length; while the deepest exceeds maxbits every used count becomes
 *   (count + 1) >> 1 and the tree is rebuilt; a single used symbol gets length 1; unused symbols 0.  maxbits outside 1..15 is
 *   CIDNET_ERR_ARG; more used symbols than 2^maxbits is CIDNET_ERR_SHAPE. */
#define CIDNET_PNG_FILTER_ADAPTIVE 5
int cidnet_png_plan(int h, int w, int segment_bytes, long* out, int n);
int cidnet_png_code_lengths(const unsigned* freq, int n, int maxbits, uint8_t* lens);
int cidnet_png_encode_u8(const uint8_t* src, long src_stride, uint8_t* dst, long dst_stride, long long* sizes, void* ws,
                         long ws_bytes, int B, int h, int w, int filter, int segment_bytes, void* stream);

/* ---- JPEG files written from the device (csrc/jpegenc.hip, csrc/jpeg_codes.h, csrc/jpeg_front.h, DESIGN.md 6.13;
 * tests/jpegenc_ref.py restates the scan and tests/test_jpegenc_cpu.py pins the restatement to Pillow).  src: B interleaved
 * (h,w,3) uint8 images, image b at src + b * src_stride (>= 3 h w, any byte alignment) -> slot b at dst + b * dst_stride: the
 * entropy-coded scan -- the bytes between the SOS segment and the EOI marker -- of the file Pillow's Image.save(f, 'JPEG',
 * quality=q) writes of the image at its defaults (baseline, 4:2:0, the Annex K Huffman tables, no restart markers), BYTE FOR
 * BYTE; sizes[b] bytes of it (int64), the rest of the slot's first `capacity` bytes zero.  The host adds the 623 bytes of
 * framing in front (SOI, APP0, two DQT, SOF0, four DHT, SOS) and the EOI behind (hvi-cidnet_amd/image_io.py: jpeg_file).
 *   Coefficients: those of cidnet_metric_jpeg_roundtrip_u8 before its dequantise step, sign(v) ((|v| + 4 t) / (8 t)): the same
 *   colour conversion, edge replication, h2v2 downsampling, forward DCT and exact division.  qtab: the 256 int32 of
 *   jpeg_quant_plan on the device, as there.
 *   Scan: one interleaved scan, MCUs in raster order over ceil(h/16) x ceil(w/16), in each the blocks Y(0,0) Y(0,1) Y(1,0)
 *   Y(1,1) Cb Cr.  A luma block outside ceil(h/8) x ceil(w/8) blocks is a DUMMY (libjpeg transforms none there): all AC zero,
 *   DC that of the block before it -- difference 0 and end of block, the six bits 00 1010, the predictor untouched.
 *   DC: one predictor per component, 0 at the start, through the whole image; diff = DC - pred, s = bit length of |diff|
 *   (0..11): the DC table's code of s, then the low s bits of diff, of diff - 1 when negative.  AC, zigzag 1..63: for v != 0
 *   after `run` zeros, run >> 4 ZRL codes (0xF0), the code of ((run & 15) << 4) | s, then s bits of v (v - 1 when negative);
 *   the end of block (0x00) when coefficient 63 is zero, nothing otherwise.  Bits MSB first; every 0xFF byte is followed by
 *   0x00; the last partial byte is filled with 1-bits (and stuffed if that makes 0xFF).
 * ws: B * plan[5] bytes, 16-byte aligned.  dst 4-byte aligned, dst_stride a multiple of 4 and >= the plan's capacity; sizes
 * 8-byte aligned; qtab 4-byte aligned.  Nothing outside the first `capacity` bytes of the B slots, sizes[0..B) and the workspace
 * is written.  Integer arithmetic only; the only atomics are integer ORs and adds whose result does not depend on their order:
 * the bytes are identical from call to call and independent of the rest of the batch.  No host synchronisation; six launches,
 * none of which waits for another workgroup (the bit offsets come from counts, a scan by one workgroup per image, then
 * emission at known offsets).  Widths below 5 are accepted: the round trip's limit belongs to the decoder.
 * CIDNET_ERR_ARG, before any launch: a NULL pointer, B, h or w < 1, a slot below the capacity, a misaligned dst / dst_stride /
 *   ws / sizes / qtab, src_stride < 3 h w.  CIDNET_ERR_WS: a short workspace.  CIDNET_ERR_SHAPE: h or w > 65500 (no such file
 *   exists), more than 2^22 MCUs, B > 65535.
 * plan: host only, launches nothing; the function the launcher itself calls.  out[0..8] = MCU columns, MCU rows, luma block
 *   columns ceil(w/8), luma block rows ceil(h/8), dummy blocks, workspace bytes per image, the capacity of one slot, the number
 *   of partial sums of the bit-offset scan (groups of 16 MCUs), workgroups of the first launch per image.  The capacity is a
 *   proven bound on the scan's size, a multiple of 4: a real block is at most 22 + 63 * 26 = 1660 bits, a dummy 6; the bytes
 *   of that many bits, doubled for stuffing, + 2 (the proof is with jpegenc_plan in csrc/jpegenc.hip).  out NULL or n < 9 is
 *   CIDNET_ERR_ARG and nothing is written; never writes past out[8]; the size errors are those above. */
int cidnet_jpeg_encode_plan(int h, int w, long* out, int n);
int cidnet_jpeg_encode_u8(const uint8_t* src, long src_stride, uint8_t* dst, long dst_stride, long long* sizes,
                          void* ws, long ws_bytes, const int* qtab, int B, int h, int w, void* stream);

/* ---- Tiled enhancement of one large image (hvi-cidnet_amd/image_io.py: tile_plan): the same two conversions seen through
 * overlapping windows of one fixed shape (th, tw), both multiples of 4.  The reference has no such mode; the contract is "the
 * model applied to each window of the reflect-padded image, blended by the plan's weights".
 * ingest_tiles: one (h,w,3) uint8 image (any byte alignment) -> x (n,3,th,tw) fp32.  origins: n rows of 2 int32 on the device,
 *   (y_t, x_t), the window's top-left corner in the padded image.  x[t,c,i,j] = T[src[ry,rx,c]] with ry = y_t + i, reflected
 *   as 2(h-1) - ry when ry >= h, and likewise rx = x_t + j against w: cidnet_image_ingest's arithmetic and table (NULL: fp32(q)
 *   / 255.0f) through a window.  The origins live on the device and cannot be checked here without a copy: EVERY WINDOW MUST
 *   LIE INSIDE THE PADDED IMAGE OF A PAD SMALLER THAN THE SIDE, CHECKED ON THE HOST WHERE THE PLAN WAS MADE (tile_plan does).
 *   The kernel clamps a coordinate that a broken plan would put outside the image, so that even then only the 3 h w bytes of
 *   the image are read.  n > 65535 or more than 2^30 groups of four pixels per tile is CIDNET_ERR_SHAPE.
 * egress_tiles: tiles (ny * nx,3,th,tw) fp32, tile (ky, kx) at index ky * nx + kx with its corner at (origins_y[ky],
 *   origins_x[kx]) (int32 on the device, ascending), and the weight tables wy (ny,th), wx (nx,tw) fp32 on the device ->
 *   dst (h,w,3) uint8.  A gather over the output pixels (y, x), y < h, x < w: for every tile that covers the pixel, ky
 *   ascending and kx ascending within it, with a = wy[ky, y - origins_y[ky]] * wx[kx, x - origins_x[kx]] (one fp32 product) and
 *   v = clamp(tile value, 0, 1), NaN -> 0:  acc += a * v, den += a, in fp32.  The value is acc / den (a correctly rounded
 *   fp32 division); A PIXEL COVERED BY EXACTLY ONE TILE TAKES v ITSELF, with no product and no division, so a plan of one tile
 *   writes what cidnet_image_egress writes; a pixel no tile covers is written as 0.  dst[y,x,c] = (uint8) trunc(value *
 *   255.0f).  Exactly the 3 h w bytes of dst are written, and only values inside the tiles and the tables are read, whatever
 *   the origin lists hold.  ny or nx > 1024, or more than 2^30 groups of four pixels, is CIDNET_ERR_SHAPE.
 * Both: th or tw not a multiple of 4 is CIDNET_ERR_SHAPE.  No atomics: a value depends on its own pixel's tiles alone, bit-
 * identical from call to call. */
int cidnet_image_ingest_tiles(const uint8_t* src, int h, int w, const float* table, const int* origins, float* x, int n, int th,
                              int tw, void* stream);
int cidnet_image_egress_tiles(const float* tiles, const int* origins_y, int ny, const int* origins_x, int nx, const float* wy,
                              const float* wx, uint8_t* dst, int h, int w, int th, int tw, void* stream);

/* ---- Geometric self-ensemble (hvi-cidnet_amd/image_io.py: ensemble_views / ensemble_merge): the 8 dihedral views of an image
 * in front of the model and the mean of the inverse-mapped results behind it.  The reference has no such mode; the contract is
 * "the model applied to each view, mapped back, summed in the fixed order below and divided by the number of views".
 * View k in 0..7 of a plane X of shape (H, W) is built in this order: if k & 1 reverse the columns; then if k & 2 reverse the
 * rows; then if k & 4 transpose.  With fr(i) = k & 2 ? H-1-i : i and fc(j) = k & 1 ? W-1-j : j:
 *   k = 0..3 ("group A", shape (H, W)):  V_k[i, j] = X[fr(i), fc(j)]        for i < H, j < W
 *   k = 4..7 ("group B", shape (W, H)):  V_k[p, q] = X[fr(q), fc(p)]        for p < W, q < H
 * C is a plain batch-like dimension: every (b, c) plane is mapped alike.  Any H, W >= 1.
 * views: x (B,C,H,W) -> y (B * count, C, Ho, Wo), (Ho, Wo) = (H, W) for group A and (W, H) for group B:
 *   y[b * count + v, c] = V_{first + v}(x[b, c]) for v < count.  A pure permutation: every output value is bit for bit one
 *   input value (NaN payloads and the sign of zero included), and exactly the B count C H W floats of y are written.  The views
 *   first .. first + count - 1 must lie wholly inside 0..3 or wholly inside 4..7, so that all outputs share one shape.
 *   CIDNET_ERR_SHAPE: count < 1; first < 0, first + count - 1 > 7, or a range that holds both 3 and 4; B * count > 65535; B, C,
 *   H or W <= 0; more than 2^31 - 1 tiles of 64 x 64 per image (C * ceil(H / 64) * ceil(W / 64)).
 * merge: ya (B * na, C, H, W) holds views 0 .. na - 1 of image b at index b * na + k; yb (B * nb, C, W, H) holds views 4 .. 4 +
 *   nb - 1 at index b * nb + (k - 4) -- the layout views writes, or the model's output for it -> out (B,C,H,W).  The inverse of a
 *   view undoes the transpose first and then the flips.  For every b, c, i < H, j < W, with fr / fc those of view k:
 *     acc = ya[b * na, c, i, j]                                      (the view-0 value itself)
 *     acc += ya[b * na + k, c, fr(i), fc(j)]        for k = 1 .. na - 1, ascending
 *     acc += yb[b * nb + k - 4, c, fc(j), fr(i)]    for k = 4 .. 4 + nb - 1, ascending
 *     out[b, c, i, j] = acc / (float)(na + nb)
 *   every sum one fp32 addition, the quotient one correctly rounded fp32 division.  No clamp: NaN and infinity propagate
 *   (cidnet_image_egress maps NaN to 0).  1 <= na <= 4 and 0 <= nb <= 4; yb is NULL exactly when nb == 0.
 *   CIDNET_ERR_SHAPE: na < 1, na > 4, nb < 0, nb > 4; yb == NULL with nb > 0 or yb != NULL with nb == 0; B > 65535; B, C, H or
 *   W <= 0; more than 2^31 - 1 tiles per image.
 * Both: x / y / ya / out == NULL is CIDNET_ERR_ARG; nothing is written on an error.  No atomics and no reduction across
 * lanes: a value depends on its own pixel's views alone, bit-identical from call to call and independent of the rest of the
 * batch.  The transposed side goes through 64 x 64 tiles in LDS, so that every global access on either side is a run of
 * consecutive floats (csrc/ensemble.hip). */
int cidnet_ensemble_views(const float* x, float* y, int B, int C, int H, int W, int first, int count, void* stream);
int cidnet_ensemble_merge(const float* ya, int na, const float* yb, int nb, float* out, int B, int C, int H, int W, void* stream);

/* ---- LPIPS, AlexNet variant (lpips.LPIPS(net='alex'), version 0.1, lpips=True, spatial=False, eval mode: measure.py:78,
 * 145-153 of the reference), the metric (csrc/lpips.hip; the training loss built on it follows below).  The definition, in the
 * order the entries are used:
 *  (1) ingest:  x = u / 127.5 - 1 formed in fp64 and rounded once to fp32, then the scaling layer in fp32,
 *      (x - shift_c) / scale_c with shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  u is the 8-bit value; with
 *      scale != NULL (GT mean) the fp64 value clip(u * scale[b], 0, 255), which is not re-quantized (measure.py:138-146).
 *  (2) features: five taps of torchvision's AlexNet `features`, each after its ReLU:
 *      conv(3->64, 11x11, stride 4, pad 2) | maxpool(3, 2), conv(64->192, 5x5, pad 2) | maxpool(3, 2), conv(192->384, 3x3,
 *      pad 1) | conv(384->256, 3x3, pad 1) | conv(256->256, 3x3, pad 1); every conv has a bias, sizes use floor, the pools
 *      have no padding and are not ceil mode.
 *  (3) per layer l: n(f) = f / (sqrt(sum_c f^2) + 1e-10) per pixel, d_l = mean over pixels of sum_c w_l[c] (n(f0) - n(f1))^2,
 *      w_l the layer's 1x1 head (C_l -> 1, no bias); C_l = 64, 192, 384, 256, 256.
 *  (4) score = sum_l d_l, one number per pair.
 *  (5) the smallest image is 31 x 31 (feature maps 7, 3, 1, 1, 1); anything smaller is CIDNET_ERR_SHAPE.
 * feature_sizes: host only.  sizes[2 l], sizes[2 l + 1] = height and width of tap l of an h x w image (step 2's floors);
 *   CIDNET_ERR_SHAPE under 31 in either axis.
 * ingest: step 1.  q uint8 (B,3,h,w) planar, scale NULL or B doubles on the device (what cidnet_metric_gt_mean_scale forms) -> x
 *   fp32 (B,3,h,w).
 * conv_relu: y = relu(conv(x) + bias), x (B,C,H,W), w (M,C,ksize,ksize) contiguous, y (B,M,Ho,Wo) with Ho = floor((H + 2 pad -
 *   ksize) / stride) + 1.  (ksize, stride, pad) is one of (11, 4, 2), (5, 1, 2), (3, 1, 1) and M a multiple of 64, else
 *   CIDNET_ERR_SHAPE; also when the padded input is smaller than the window, B > 65535 or a tensor of one image has more than
 *   2^31 - 1 elements.  An implicit GEMM on the fp32 matrix cores (fp32 products, fp32 accumulation: the accuracy of an fp32
 *   convolution); the padding and the remainder of K = C ksize^2 are zeros written by the staging, never a read outside x or
 *   w.  A block works on one image: an image's result does not depend on the rest of the batch.  All five layers of step 2.
 * maxpool3s2: y (planes, floor((H - 3) / 2) + 1, floor((W - 3) / 2) + 1) = the maximum of each 3 x 3 window at stride 2 of
 *   x (planes, H, W).  H < 3 or W < 3 is CIDNET_ERR_SHAPE.  A NaN in a window is skipped (fmaxf), where torch propagates it.
 * layer: step 3 for tap `layer` (0..4) of B pairs: f0, f1 fp32 (B,C,fh,fw), head C floats -> block partials in ws.  (C, fh,
 *   fw) must be what the layer has for an h x w image, else CIDNET_ERR_SHAPE.  fp64 from the fp32 features on: sums of
 *   squares, norms (as a reciprocal, one fp64 rounding away from the quotient), weighted squared differences.  No fused
 *   multiply-add: identical features give exactly 0.
 * finish: step 3's mean and step 4: layers (B,5) and score (B) doubles (either may be NULL) from the partials all five layer
 *   calls left in ws.  A fixed-order two-stage reduction (per-block partials in fixed slots, one wave per image sums them):
 *   no atomics, bit-identical from call to call, independent of the rest of the batch.
 *   ws: cidnet_metric_lpips_ws_floats(B, h, w) floats, 8-byte aligned, the same buffer for the five layer calls and finish;
 *   the query is host only and returns 0 for an image under 31 x 31. */
int cidnet_lpips_feature_sizes(int h, int w, int* sizes);
int cidnet_metric_lpips_ingest(const uint8_t* q, const double* scale, float* x, int B, int h, int w, void* stream);
int cidnet_lpips_conv_relu(const float* x, const float* w, const float* bias, float* y, int B, int M, int C, int H, int W, int ksize,
                           int stride, int pad, void* stream);
int cidnet_lpips_maxpool3s2(const float* x, float* y, long planes, int H, int W, void* stream);
long cidnet_metric_lpips_ws_floats(int B, int h, int w);
int cidnet_metric_lpips_layer(const float* f0, const float* f1, const float* head, float* ws, long ws_floats, int layer, int B, int C,
                              int fh, int fw, int h, int w, void* stream);
int cidnet_metric_lpips_finish(const float* ws, long ws_floats, double* layers, double* score, int B, int h, int w, void* stream);

/* ---- LPIPS training loss (AlexNet; lpips.LPIPS(net='alex')(x, gt, normalize=True).mean() times a weight), forward through the
 * entries above plus the three below, backward in csrc/lpips_loss.hip.  The contract:
 * x, gt: fp32 (B,3,h,w), h, w >= 31, any value range (nothing clamps).  gt is a constant: the only gradient is d/dx.
 *  (1) ingest (normalize=True): v = 2 x - 1 with one fp32 rounding (2 x is exact), then z = (v - shift_c) / scale_c in fp32, the
 *      constants of the metric's step 1.  Backward: gx = (g / scale_c) * 2.  Compiled without contraction: both directions are
 *      bit-identical to the same expression in fp32 torch.
 *  (2) features: the five post-ReLU taps of the metric's step 2, through cidnet_lpips_conv_relu and cidnet_lpips_maxpool3s2.
 *  (3) loss = weight * (1 / B) sum_b sum_l d_l(b), fp32, the d_l of the metric's step 3 from the same fixed-order fp64 partials.
 *  (4) gradient rules.
 *      ReLU: the gradient passes where the stored post-ReLU value is > 0.
 *      Pool 3/2: a window's gradient goes to its first maximum in scan order, row-major inside the window (a later value
 *        replaces the maximum only when strictly greater: ATen's rule, and cidnet_maxpool2_bwd's).  An input element sums the
 *        windows that chose it (up to four) in window scan order; rows and columns under no window get 0.  Gather form, no
 *        atomics.  A NaN never compares greater, so it is never chosen (torch would choose it).
 *      Distance: with n = f / (s + 1e-10), s = sqrt(sum_c f_c^2), P_l the pixels of layer l and w_c its head,
 *        dn_c = 2 w_c (n0_c - n1_c) weight / (B P_l),   df0_c = dn_c / (s + eps) - f0_c (sum_j dn_j f0_j) / (s (s + eps)^2).
 *        A pixel whose f0 is all zero gets df0 = 0 in every channel.  torch's autograd gives NaN there (sqrt'(0) * 0) and the
 *        formula's limit is dn / eps, about 1e10 times dn; but every channel of that pixel is 0, so the ReLU mask that follows
 *        lets nothing through: zero is the value on which the kernel, the mask and the limit agree.  A ground-truth pixel with
 *        s1 = 0 has n1 = 0, nothing special.  Per-pixel sums over channels in fp64 in a fixed order; the result is fp32.
 *      Convolution data gradient: dx[b][c][iy][ix] = sum_{m,ky,kx} w[m][c][ky][kx] dy[b][m][oy][ox] with iy = S oy - PAD + ky;
 *        fp32 products, fp32 accumulation, no dependence on the rest of the batch, no atomics, bit-identical from call to call.
 * ingest_f32 / ingest_f32_bwd: step 1 and its backward, (B,3,h,w) -> (B,3,h,w).
 * loss_finish: step 3 from the partials the five cidnet_metric_lpips_layer calls left in ws (cidnet_lpips_loss_ws_floats(B, h, w)
 *   floats, 8-byte aligned; host-only query, 0 under 31 x 31): one wave, images in order, layers in order, fp64, one rounding.
 * dgrad_weights: the frozen weights w (M,C,ksize,ksize) in the form a data gradient reads, written once per device.
 *   stride 1: wt (C,M,ksize,ksize), spatially flipped (the gradient as a convolution of dy).  stride 4 (ksize 11, C 3 only):
 *   wt (11,11,M,4) = the three channels of a (ky, kx, m) and a zero, read 16 bytes at a time: this wt must be 16-byte aligned
 *   (conv_dgrad returns CIDNET_ERR_ARG otherwise).  dgrad_weights_floats: its length; 0 = not taken.
 * conv_dgrad: dx (B,C,H,W) from dy (B,M,Ho,Wo) and wt = dgrad_weights of the layer (M,C,ksize,ksize), (ksize, stride, pad) one
 *   of (11, 4, 2) with C = 3, (5, 1, 2), (3, 1, 1) with C a multiple of 64; else CIDNET_ERR_SHAPE.  tap, addend: both NULL,
 *   or both (B,C,H,W) (stride 1 only): dx = tap > 0 ? dx + addend : 0 -- the ReLU mask of the tap dx is the gradient of and
 *   that tap's distance gradient.  Stride 1 runs the implicit GEMM of conv_relu on the fp32 matrix cores; stride 4 is a
 *   gather of the at most 3 x 3 windows that reach a pixel: pixels under no window get exactly 0.
 * maxpool3s2_bwd: gx (planes,H,W) from x (planes,H,W) and gy (planes,Ho,Wo) by the pool rule above; addend (planes,H,W) or
 *   NULL: with it, x is a post-ReLU tap and gx = x > 0 ? gx + addend : 0.  H < 3 or W < 3 is CIDNET_ERR_SHAPE.
 * layer_bwd: g (B,C,P) = df0 of the distance rule above for f0, f1 (B,C,P), head C floats, with `weight` the loss weight
 *   (the kernel divides by B P in fp64); relu_mask != 0 also zeroes g where f0 <= 0 (the deepest tap has no other mask).
 *   lpips_dist_kernel's layout: eight threads a pixel, meeting in LDS in group order. */
int cidnet_lpips_ingest_f32(const float* x, float* z, int B, int h, int w, void* stream);
int cidnet_lpips_ingest_f32_bwd(const float* g, float* gx, int B, int h, int w, void* stream);
long cidnet_lpips_loss_ws_floats(int B, int h, int w);
int cidnet_lpips_loss_finish(const float* ws, long ws_floats, float weight, float* loss, int B, int h, int w, void* stream);
long cidnet_lpips_dgrad_weights_floats(int M, int C, int ksize, int stride);
int cidnet_lpips_dgrad_weights(const float* w, float* wt, int M, int C, int ksize, int stride, void* stream);
int cidnet_lpips_conv_dgrad(const float* dy, const float* wt, const float* tap, const float* addend, float* dx, int B, int M, int C,
                            int H, int W, int ksize, int stride, int pad, void* stream);
int cidnet_lpips_maxpool3s2_bwd(const float* x, const float* gy, const float* addend, float* gx, long planes, int H, int W,
                                void* stream);
int cidnet_lpips_layer_bwd(const float* f0, const float* f1, const float* head, float* g, float weight, int relu_mask, int B, int C,
                           long P, void* stream);

/* ---- CIEDE2000 colour difference (csrc/ciede2000.hip): the mean dE00 between the restored image (colour 1) and its ground
 * truth (colour 2), the colour-fidelity number of the low-light literature, usually computed with scikit-image as
 * deltaE_ciede2000(rgb2lab(a), rgb2lab(b)).mean().  The reference has none; the contract is this text.  All arithmetic fp64.
 * sRGB -> Lab, scikit-image's constants: v = level / 255; lin = v > 0.04045 ? ((v + 0.055) / 1.055)^2.4 : v / 12.92;
 *   XYZ = M lin, each row summed left to right, M = [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169],
 *   [0.019334, 0.119193, 0.950227]]; divided by the D65 / 2 degree white (0.95047, 1.0, 1.08883); f(t) = t > 0.008856 ? cbrt(t)
 *   : 7.787 t + 16 / 116; L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z)).
 * dE00, Sharma, Wu and Dalal (2005), kL = kC = kH = 1: C = hypot(a, b); Cbar = (C1 + C2) / 2; G = 0.5 (1 - sqrt(Cbar^7 /
 *   (Cbar^7 + 25^7))); a' = (1 + G) a; C' = hypot(a', b); h' = atan2(b, a') in degrees, + 360 when negative (atan2(0, 0) = 0);
 *   dL' = L2 - L1; dC' = C2' - C1'; dh' = 0 if C1' C2' = 0, else h2' - h1' brought into (-180, 180] by -360 when > 180 and + 360
 *   when < -180; dH' = 2 sqrt(C1' C2') sin(dh' / 2); Lbar' = (L1 + L2) / 2; Cbar' = (C1' + C2') / 2; hbar' = h1' + h2' if C1' C2'
 *   = 0, else (h1' + h2') / 2 if |h1' - h2'| <= 180, else (h1' + h2' + 360) / 2 if h1' + h2' < 360, else (h1' + h2' - 360) / 2;
 *   T = 1 - 0.17 cos(hbar' - 30) + 0.24 cos(2 hbar') + 0.32 cos(3 hbar' + 6) - 0.20 cos(4 hbar' - 63) (degrees); dtheta = 30 exp(
 *   -((hbar' - 275) / 25)^2); R_C = 2 sqrt(Cbar'^7 / (Cbar'^7 + 25^7)); S_L = 1 + 0.015 (Lbar' - 50)^2 / sqrt(20 + (Lbar' - 50)^2);
 *   S_C = 1 + 0.045 Cbar'; S_H = 1 + 0.015 Cbar' T; R_T = -sin(2 dtheta) R_C; dE00 = sqrt(x^2 + y^2 + z^2 + R_T y z), x = dL' /
 *   S_L, y = dC' / S_C, z = dH' / S_H.  No fused multiply-add: two identical pixels give exactly 0.0.
 * u8: restored, gt planar uint8 (B,3,h,w), any h, w >= 1.  lin_table: 256 doubles on the device, the linear value of every
 *   level by the formula above, built by the host in fp64 (hvi-cidnet_amd/metrics.py: ciede2000_tables): no pow runs on the
 *   device for a level.  scale NULL: both sides are levels.  scale = B doubles on the device (GT mean; what
 *   cidnet_metric_gt_mean_scale forms): the restored pixel enters as v = clip(q scale[b], 0, 255) / 255, a real number that is not
 *   re-quantized (measure.py:138-141), through an fp64 pow; the ground truth still reads the table.  An image whose gray mean is
 *   0 has an infinite or NaN scale and gives whatever IEEE arithmetic gives.  map (B,h,w doubles) receives every pixel's dE00,
 *   mean (B doubles) the image values; either may be NULL, not both.  ws: cidnet_metric_ciede2000_ws_bytes(B, h, w) bytes,
 *   read and written only with mean.
 *   Reduction, no atomics: block x of an image takes pixels 1024 x .. 1024 x + 1023 of the flattened plane, thread t of its 256
 *   the pixels 1024 x + 4 t + 0..3, added in that order onto 0.0; the block tree -- in each wave of 64 the butterfly v +=
 *   v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1, then ((wave 0 + wave 1) + wave 2) + wave 3 -- gives slot x of the image in ws.  One
 *   block per image then adds slots t, t + 256, ... in that order onto 0.0 in thread t, sums the threads by the same tree and
 *   divides by h w.  The pixel -> block map depends on (h, w) only: bit-identical from call to call, and an image's value does
 *   not depend on the rest of the batch.
 *   restored / gt / lin_table NULL, map and mean both NULL, mean without ws, a pointer to doubles that is not 8-byte aligned, or
 *   B, h or w < 1 is CIDNET_ERR_ARG; a short workspace CIDNET_ERR_WS; h w > 2^31 - 1 or B > 65535 CIDNET_ERR_SHAPE.
 * ws_bytes: host only; 0 for sizes the launcher rejects.
 * plan: host only, launches nothing; the function the launcher itself calls.  Writes out[0..2] = blocks per image, pixels per
 *   block (blocks x pixels >= h w), static LDS bytes per block.  out NULL or n < 3 is CIDNET_ERR_ARG and nothing is written;
 *   never writes past out[2]; the size errors are those above.
 * lab: out[i] = dE00(lab1[i], lab2[i]) for n pairs of (L, a, b) doubles, (n,3) contiguous: the same core, so that it can be held
 *   against published Lab data.  A NULL or misaligned pointer or n < 1 is CIDNET_ERR_ARG. */
long cidnet_metric_ciede2000_ws_bytes(int B, int h, int w);
int cidnet_metric_ciede2000_plan(int h, int w, int* out, int n);
int cidnet_metric_ciede2000_u8(const uint8_t* restored, const uint8_t* gt, const double* scale, const double* lin_table, double* map,
                               double* mean, void* ws, long ws_bytes, int B, int h, int w, void* stream);
int cidnet_metric_ciede2000_lab(const double* lab1, const double* lab2, double* out, long n, void* stream);

/* ---- BRISQUE (csrc/brisque.hip): the second number measure_niqe_bris.py prints per unpaired set, imquality.brisque.score of
 * the saved output.  imquality, scikit-image, cv2 and libsvm are not at hand: the stages are restated from the description of
 * that package, and parity with it is NOT pinned; every stage is pinned to the scipy / scikit-learn routine named with it
 * (tests/brisque_ref.py).  All arithmetic fp64, no fused multiply-add, no atomics, fixed reduction order:
 * bit-identical from call to call, and an image's values do not depend on the rest of the batch.
 * gray: rgb planar uint8 (B,3,h,w) -> y (B,h,w) doubles, Y = ((0.2125 R + 0.7154 G) + 0.0721 B) / 255 (skimage's rgb2gray).
 * half: y (B,h,w) -> out (B,h2,w2), h2 = round(h / 2), w2 = round(w / 2) with numpy's rounding, half to even (17 x 23 -> 8 x 12):
 *   skimage.transform.rescale(y, 1/2) with its defaults -- the Gaussian of sigma 0.5 cut at radius 2 with a mirrored border
 *   (-1 -> 1), down the columns and then along the rows, each pass k0 x + k1 (x[-1] + x[+1]) + k2 (x[-2] + x[+2])
 *   (scipy.ndimage.gaussian_filter(y, 0.5, mode='mirror')), then order-1 resampling at (o + 0.5) n_in / n_out - 0.5 on both
 *   axes, the row pair first: (1 - ty) ((1 - tx) a00 + tx a01) + ty ((1 - tx) a10 + tx a11) (scipy.ndimage.zoom(order=1,
 *   mode='mirror', grid_mode=True)).  tmp: 2 B h w doubles of scratch.  A stage of its own so that another resampler is a
 *   local change.
 * moments: img is rgb (B,3,h,w) uint8 (img_f64 == 0: the gray value is formed while staging) or a gray plane (B,h,w) doubles
 *   (img_f64 != 0).  MSCN: mu = K * Y, s = K * Y^2, K[i][j] ~ exp(-((i-3)^2 + (j-3)^2) / (2 (7/6)^2)), 7 x 7, sum 1, ZERO outside
 *   the image, the 49 products added in row-major order (scipy.signal.convolve2d(.., 'same')); dev = sqrt(|mu^2 - s|);
 *   M = (Y - mu) / (dev + 1/255).  Five maps: M; H = M[r][c] M[r][c+1]; V = M[r][c] M[r+1][c]; D1 = M[r][c] M[r+1][c+1];
 *   D2 = M[r][c] M[r+1][c-1] -- slices, not rolls: a pair whose partner lies outside the image does not exist.  The plane is cut
 *   into 32 x 32 tiles in row-major order, tiles = ceil(h / 32) ceil(w / 32); a pair belongs to the tile of its M[r][c].
 *   moments (B,tiles,5,6) doubles, per tile and map: the count and the sum of squares of the elements < 0, the same of the
 *   elements >= 0 (zeros count there), sum |v|, sum v^2; counts are exact.  In a tile, thread t of 256 adds pixels t, t + 256,
 *   t + 512, t + 768 of the row-major tile in that order, then the butterfly of each wave and the four waves in order.
 *   mscn (optional, (B,h,w) doubles) receives M; without it the map never leaves the compute unit.
 * fit: moments (B,tiles,5,6) -> 18 features at feat + b feat_stride.  Per map the tile slots are added by lane l of 64 over
 *   tiles l, l + 64, ... in that order and then by the butterfly; with nl, Sl, nr, Sr, A, Q the six sums: sl = sqrt(Sl / nl),
 *   sr = sqrt(Sr / nr), g = sl / sr, n = nl + nr, r = (A / n)^2 / (Q / n), R = r (g^3 + 1)(g + 1) / (g^2 + 1)^2, alpha the root of
 *   phi(a) = exp(2 lgamma(2/a) - lgamma(1/a) - lgamma(3/a)) = R in [0.05, 100], bracketed 65 ways per round until the fp64
 *   bracket stops moving, alpha = (lo + hi) / 2 (oracle: scipy.optimize.brentq, xtol 1e-15); c = sqrt(Gamma(1/alpha) /
 *   Gamma(3/alpha)), mean = (sr - sl) c Gamma(2/alpha) / Gamma(1/alpha).  Features: M gives [alpha, (sl^2 + sr^2) / 2], each
 *   product map [alpha, mean, sl^2, sr^2], in the order M, H, V, D1, D2.  R outside (phi(0.05), phi(100)) or NaN (an empty side,
 *   no variance) makes all of that map's features NaN; nothing is raised.
 * svr: feat (B,36) -> score (B): z = -1 + 2 (f - fmin) / (fmax - fmin), score = sum_i coef[i] exp(-gamma |sv[i] - z|^2) - rho, the
 *   squared distance over the 36 features in order, the sum over the n_sv support vectors (sv (n_sv,36)) in order, by one
 *   thread.  rho_gamma: {rho, gamma}, two doubles on the device.
 * features: all of the above for rgb (B,3,h,w): feat (B,36) = the 18 features at full size | the 18 at half size.
 *   ws: cidnet_metric_brisque_ws_floats(B, h, w) floats, 8-byte aligned.
 * plan: host only, launches nothing; the function the launchers' sizes come from.  Writes out[0..8] = tile side, tile rows and
 *   tile columns at full size, h2, w2, tile rows and tile columns at half size, static LDS bytes of the tile kernel, workspace
 *   floats per image.  out NULL or n < 9 is CIDNET_ERR_ARG and nothing is written; never writes past out[8].
 * Errors: a NULL pointer (but mscn), a pointer to doubles that is not 8-byte aligned, B, h, w, tiles or n_sv < 1 is
 *   CIDNET_ERR_ARG; h or w < 16 (moments alone: < 8, the half-size plane of the smallest image), h w > 2^26, B > 65535 or
 *   feat_stride < 18 CIDNET_ERR_SHAPE; a short workspace CIDNET_ERR_WS.  ws_floats is 0 for sizes the launcher rejects. */
int cidnet_metric_brisque_plan(int h, int w, int* out, int n);
long cidnet_metric_brisque_ws_floats(int B, int h, int w);
int cidnet_metric_brisque_gray(const uint8_t* rgb, double* y, int B, int h, int w, void* stream);
int cidnet_metric_brisque_half(const double* y, double* tmp, double* out, int B, int h, int w, void* stream);
int cidnet_metric_brisque_moments(const void* img, int img_f64, double* mscn, double* moments, int B, int h, int w, void* stream);
int cidnet_metric_brisque_fit(const double* moments, int tiles, double* feat, int feat_stride, int B, void* stream);
int cidnet_metric_brisque_svr(const double* feat, const double* sv, const double* coef, const double* fmin, const double* fmax,
                              const double* rho_gamma, int n_sv, double* score, int B, void* stream);
int cidnet_metric_brisque_features(const uint8_t* rgb, double* feat, float* ws, long ws_floats, int B, int h, int w, void* stream);

/* ---- frequency-domain training loss (csrc/fft_loss.hip): an L1 distance between the half spectra of the
 * prediction a and the target b, fp32 (P,H,W) planes (P = B C), the term MIMO-UNet / DeepRFT add to a restoration objective.
 * The reference has none; the contract is this text, and torch.fft.rfft2 in fp64 is the oracle.  With d = a - b, Wh = W / 2 + 1:
 *   D[p,ky,kx] = sum_y sum_x d[p,y,x] exp(-2 pi i (ky y / H + kx x / W)),   ky < H, kx < Wh
 *   loss = weight s / (2 P H Wh) sum (|Re D| + |Im D|),   s = 1 (norm 0, "backward") or 1 / sqrt(H W) (norm 1, "ortho")
 *        = weight * l1_loss(view_as_real(rfft2(a, norm)), view_as_real(rfft2(b, norm)))
 *   dloss/da[p,y,x] = gloss weight s / (2 P H Wh) sum_{ky,kx} (sign(Re D) cos t - sign(Im D) sin t),  sign(0) = 0;  dloss/db = -dloss/da
 * -- the plain adjoint of the half spectrum, no Hermitian doubling: what autograd gives.
 * Each axis is a GEMM against a twiddle table on the fp32 matrix cores (fp32 products, fp32 accumulation over k in ascending
 * order), so every H x W up to 2048 a side is taken.  fp32 in every precision mode.  No atomics: bit-identical from call to
 * call; a plane's spectrum, signs and gradient do not depend on the other planes.
 * dft_table: table (N, Nk, 2) = (cos, -sin)(2 pi m / N), m = n k mod N reduced in integers, evaluated in fp64 and rounded once;
 *   exactly 0 / +-1 where 4 m is a multiple of N, so a purely real bin gets an imaginary part of exactly 0 and sign 0.
 *   N or Nk < 1 or a NULL / misaligned table is CIDNET_ERR_ARG; N > 2048 or Nk > N is CIDNET_ERR_SHAPE.
 * tab_h = dft_table(H, H), tab_w = dft_table(W, Wh) in all that follows; they are only read.
 * ws: cidnet_fft_loss_ws_floats(P, H, W) floats, 8-byte aligned, for every entry (host-only query; 0 for a refused shape).
 * loss_fwd: loss (1 float).  S NULL: nothing else is written -- the spectrum never goes to memory.  S (P,H,Wh,2): the signs of
 *   (Re D, Im D) as fp32 +-1 / 0, what loss_bwd reads.  a - b is formed while staging.  The sum of |.| is fp32 over the 16 values
 *   a lane holds, fp64 from there on: one fp64 partial per block in a fixed slot, one block adds the slots in a fixed order.
 *   Identical a and b give exactly 0.
 * loss_bwd: ga and / or gb = -ga (P,H,W), bit for bit each other's negation; either may be NULL (both: nothing is launched).
 *   gloss: the upstream gradient, one float on the device.  weight and norm as given to loss_fwd.
 * rfft2_fwd: D (P,H,Wh,2) = (Re, Im) of the unnormalised half spectrum of x.  rfft2_adj: g (P,H,W) = the adjoint of that map
 *   applied to Sin (P,H,Wh,2), g[y,x] = sum Sin_r cos t - Sin_i sin t.  The two linear maps on their own, for the tests.
 * plan: host only, launches nothing; the function the launchers' sizes come from.  Writes out[0..16] = the tile MT, NT, KC; the
 *   grids (x, y, z) of the row forward, the column forward, the column adjoint and the row adjoint; the number of fp64
 *   partials; the workspace floats.  out NULL or n < 17 is CIDNET_ERR_ARG; never writes past out[16].
 * Errors, before any launch and with nothing written: P, H or W < 1, a NULL (but S, ga, gb) or misaligned pointer (4 bytes; ws
 *   8), norm outside {0, 1}, a negative, NaN or infinite weight: CIDNET_ERR_ARG.  H or W > 2048, P > 65535, P H W or
 *   2 P H Wh > 2^31 - 1: CIDNET_ERR_SHAPE.  A short workspace: CIDNET_ERR_WS. */
int cidnet_dft_table(int N, int Nk, float* table, void* stream);
long cidnet_fft_loss_ws_floats(int P, int H, int W);
int cidnet_fft_loss_plan(int P, int H, int W, long* out, int n);
int cidnet_fft_loss_fwd(const float* a, const float* b, const float* tab_h, const float* tab_w, float weight, int norm, float* loss,
                        float* S, float* ws, long ws_floats, int P, int H, int W, void* stream);
int cidnet_fft_loss_bwd(const float* S, const float* tab_h, const float* tab_w, const float* gloss, float weight, int norm, float* ga,
                        float* gb, float* ws, long ws_floats, int P, int H, int W, void* stream);
int cidnet_rfft2_fwd(const float* x, const float* tab_h, const float* tab_w, float* D, float* ws, long ws_floats, int P, int H, int W,
                     void* stream);
int cidnet_rfft2_adj(const float* Sin, const float* tab_h, const float* tab_w, float* g, float* ws, long ws_floats, int P, int H, int W,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIDNET_HIP_H */
