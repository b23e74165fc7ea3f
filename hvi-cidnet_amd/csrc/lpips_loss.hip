// The backward pass of the LPIPS (AlexNet) training loss (include/cidnet_hip.h, "LPIPS training loss"); its forward is the
// metric's (csrc/lpips.hip).  The loss is weight / B * sum_b sum_l d_l(b); the chain from the five taps f_l of the image x
// back to x, with G_l the gradient at the (post-ReLU) tap l and Z_l = [f_l > 0] G_l the gradient at its convolution's output:
//   D_l  = d loss / d f_l of the layer's own distance term                                      lpips_layer_bwd_kernel
//   Z_4  = [f_4 > 0] D_4                                                                        (the same kernel, relu_mask)
//   Z_3  = [f_3 > 0] (dgrad5(Z_4) + D_3),  Z_2 = [f_2 > 0] (dgrad4(Z_3) + D_2)                  lpips_conv_kernel, kEpiMaskAdd
//   Z_1  = [f_1 > 0] (pool_bwd(f_1, dgrad3(Z_2)) + D_1)                                         kEpiPlain, lpips_maxpool_bwd_kernel
//   Z_0  = [f_0 > 0] (pool_bwd(f_0, dgrad2(Z_1)) + D_0)                                         the same pair
//   dz   = dgrad1(Z_0), the 11 x 11 stride-4 layer                                              lpips_conv1_dgrad_kernel
// and the ingest's backward (csrc/lpips.hip).  Every intermediate is written once; nothing is accumulated with atomics, so a
// result is bit-identical from call to call, and every kernel works on one image at a time, so an image's gradient does not
// depend on the rest of the batch (beyond the 1 / B of the mean).
// Stride-1 data gradients: the forward's implicit-GEMM template (csrc/lpips_conv.h) on dy with the flipped, transposed
// weights lpips_dgrad_weights_kernel writes once per device.
// Stride-4 data gradient (64 -> 3 channels, 11 x 11): a gather on the vector ALU, one thread per input pixel and all three
// channels.  With q = i + 2 the windows that reach row i are oy = floor(q / 4) - j, j = 0..2, at kernel row ky = q mod 4 + 4 j
// (< 11), so a pixel has at most 3 x 3 contributing output positions and 9 64 3 multiply-adds.  The weights are read from a
// phase-ordered copy [ky][kx][m][4] (the three channels of one (ky, kx, m) in one 16-byte load): the lanes of a wave differ in
// q mod 4 only, so a wave's load touches four addresses and the 93 KB of weights stay in the caches -- no block pays for
// staging them in LDS before its first product.
// Built with -ffp-contract=off (build.py), as lpips.hip: the distance derivative of two identical feature maps must be
// exactly 0 (n(f0) - n(f1) = 0 needs both products rounded alike), and the ingest pair is pinned bit for bit to fp32 torch.
#include "common.h"
#include "cidnet_hip.h"
#include "lpips_conv.h"

namespace cidnet {
namespace {

// mode 0: wt[c][m][k-1-ky][k-1-kx] = w[m][c][ky][kx] (the stride-1 data gradient as a convolution);
// mode 1: wt[ky][kx][m][4] = (w[m][0][ky][kx], w[m][1][ky][kx], w[m][2][ky][kx], 0) (the stride-4 gather, C = 3)
__global__ __launch_bounds__(256) void lpips_dgrad_weights_kernel(const float* __restrict__ w, float* __restrict__ wt, int M, int C,
                                                                  int k, int mode, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  if (mode == 0) {
    const int kx = (int)(i % k), ky = (int)((i / k) % k);
    const int c = (int)((i / ((long)k * k)) % C), m = (int)(i / ((long)k * k * C));
    wt[(((long)c * M + m) * k + (k - 1 - ky)) * k + (k - 1 - kx)] = w[i];
  } else {
    const int c = (int)(i % 4), m = (int)((i / 4) % M);
    const int kx = (int)((i / (4L * M)) % k), ky = (int)(i / (4L * M * k));
    wt[i] = c < 3 ? w[(((long)m * 3 + c) * k + ky) * k + kx] : 0.f;
  }
}

// dx[b][c][iy][ix] = sum_{m,ky,kx} w[m][c][ky][kx] dy[b][m][oy][ox] with iy = 4 oy - 2 + ky, ix = 4 ox - 2 + kx; the sum runs
// over window rows from the last (j = 0) to the first, columns likewise, m innermost: a fixed order.  fp32 products and sums.
__global__ __launch_bounds__(256) void lpips_conv1_dgrad_kernel(const float* __restrict__ dy, const float4* __restrict__ wp,
                                                                float* __restrict__ dx, int M, int H, int W, int Ho, int Wo) {
  const long hw = (long)H * W;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int b = blockIdx.y;
  const int iy = (int)(i / W), ix = (int)(i - (long)iy * W);
  const int qy = iy + 2, qx = ix + 2;
  const long P = (long)Ho * Wo;
  const float* dyb = dy + (long)b * M * P;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int jy = 0; jy < 3; ++jy) {
    const int oy = (qy >> 2) - jy, ky = (qy & 3) + 4 * jy;
    if (oy < 0 || oy >= Ho || ky > 10) continue;
    for (int jx = 0; jx < 3; ++jx) {
      const int ox = (qx >> 2) - jx, kx = (qx & 3) + 4 * jx;
      if (ox < 0 || ox >= Wo || kx > 10) continue;
      const float* g = dyb + (long)oy * Wo + ox;
      const float4* wq = wp + (long)(ky * 11 + kx) * M;
      for (int m = 0; m < M; ++m) {
        const float v = g[m * P];
        const float4 ww = wq[m];
        a0 += ww.x * v;
        a1 += ww.y * v;
        a2 += ww.z * v;
      }
    }
  }
  float* o = dx + (long)b * 3 * hw + i;
  o[0] = a0;
  o[hw] = a1;
  o[2 * hw] = a2;
}

// The backward of nn.MaxPool2d(3, 2), gather form: one thread per input element looks at the at most 2 x 2 windows that cover
// it, recomputes each window's first maximum in scan order (row-major inside the window, strictly greater replaces: ATen's
// rule) from x and adds the gradients of the windows that chose it, in window scan order.  Rows and columns under no window
// get 0.  With addend != NULL, x is a post-ReLU tap: gx = x > 0 ? sum + addend : 0.
__global__ __launch_bounds__(256) void lpips_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                const float* __restrict__ addend, float* __restrict__ gx, int H, int W,
                                                                int Ho, int Wo, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xi = (int)(i % W);
    const long t = i / W;
    const int yi = (int)(t % H);
    const long plane = t / H;
    const float* xp = x + plane * (long)H * W;
    const float* gp = gy + plane * (long)Ho * Wo;
    const int oy_lo = yi < 2 ? 0 : (yi - 1) >> 1, ox_lo = xi < 2 ? 0 : (xi - 1) >> 1;
    const int oy_hi = min(yi >> 1, Ho - 1), ox_hi = min(xi >> 1, Wo - 1);
    float s = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const float* p = xp + (long)(2 * oy) * W + 2 * ox;
        float m = p[0];
        int arg = 0;
#pragma unroll
        for (int k = 1; k < 9; ++k) {
          const float v = p[(k / 3) * W + (k % 3)];
          if (v > m) {
            m = v;
            arg = k;
          }
        }
        if (2 * oy + arg / 3 == yi && 2 * ox + arg % 3 == xi) s += gp[(long)oy * Wo + ox];
      }
    if (addend) s = x[i] > 0.f ? s + addend[i] : 0.f;
    gx[i] = s;
  }
}

// g[b][c][p] = d loss / d f0[b][c][p] of the layer's term  coef * sum_p sum_c head[c] (n0_c - n1_c)^2,  n = f / (s + 1e-10),
// s = sqrt(sum_c f_c^2):  dn_c = 2 head[c] (n0_c - n1_c) coef,  g_c = dn_c / (s + eps) - f0_c (sum_j dn_j f0_j) / (s (s + eps)^2),
// and g = 0 in every channel of a pixel whose f0 is all zero.  lpips_dist_kernel's layout: kDistPix pixels a block, the
// kDistGroups threads of a pixel take the channels g, g + kDistGroups, ... and meet in LDS, where each adds the groups' sums
// in group order.  fp64 from the fp32 features on, one rounding to fp32 at the store.  relu_mask: g_c = 0 where f0_c <= 0.
__global__ __launch_bounds__(kDistThreads) void lpips_layer_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                       const float* __restrict__ head, float* __restrict__ g, int C,
                                                                       long P, double coef, int relu_mask) {
  __shared__ double ss[2][kDistGroups][kDistPix];
  const long img = blockIdx.y;
  const int px = threadIdx.x % kDistPix, grp = threadIdx.x / kDistPix;
  const long p = (long)blockIdx.x * kDistPix + px;
  const bool in = p < P;
  const float* a = f0 + img * C * P + (in ? p : 0);
  const float* b = f1 + img * C * P + (in ? p : 0);
  float* o = g + img * C * P + (in ? p : 0);
  double sa = 0.0, sb = 0.0;
  if (in) {
    for (int c = grp; c < C; c += kDistGroups) {
      const double va = (double)a[c * P], vb = (double)b[c * P];
      sa += va * va;
      sb += vb * vb;
    }
  }
  ss[0][grp][px] = sa;
  ss[1][grp][px] = sb;
  __syncthreads();
  sa = 0.0;
  sb = 0.0;
#pragma unroll
  for (int k = 0; k < kDistGroups; ++k) {
    sa += ss[0][k][px];
    sb += ss[1][k][px];
  }
  __syncthreads();
  const double s = sqrt(sa);
  const double ra = 1.0 / (s + 1e-10), rb = 1.0 / (sqrt(sb) + 1e-10);
  double dot = 0.0;
  if (in) {
    for (int c = grp; c < C; c += kDistGroups) {
      const double va = (double)a[c * P];
      const double d = va * ra - (double)b[c * P] * rb;
      dot += ((2.0 * (double)head[c]) * d * coef) * va;
    }
  }
  ss[0][grp][px] = dot;
  __syncthreads();
  if (!in) return;
  dot = 0.0;
#pragma unroll
  for (int k = 0; k < kDistGroups; ++k) dot += ss[0][k][px];
  const bool dead = !(sa > 0.0);                                  // f0 all zero at this pixel
  const double back = dead ? 0.0 : dot / (s * ((s + 1e-10) * (s + 1e-10)));
  for (int c = grp; c < C; c += kDistGroups) {
    const float fa = a[c * P];
    const double va = (double)fa;
    const double d = va * ra - (double)b[c * P] * rb;
    const double dn = (2.0 * (double)head[c]) * d * coef;
    const double v = dn * ra - va * back;
    o[c * P] = (dead || (relu_mask && !(fa > 0.f))) ? 0.f : (float)v;
  }
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

long cidnet_lpips_dgrad_weights_floats(int M, int C, int ksize, int stride) {
  if (M <= 0 || C <= 0 || ksize <= 0) return 0;
  if (stride == 1) return (long)M * C * ksize * ksize;
  if (stride == 4 && ksize == 11 && C == 3) return (long)ksize * ksize * M * 4;
  return 0;
}

int cidnet_lpips_dgrad_weights(const float* w, float* wt, int M, int C, int ksize, int stride, void* stream) {
  CIDNET_CHECK_ARG(w && wt && M > 0 && C > 0 && ksize > 0);
  const long total = cidnet_lpips_dgrad_weights_floats(M, C, ksize, stride);
  if (total == 0 || (total + 255) / 256 > 2147483647L) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(lpips_dgrad_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, wt, M, C,
                     ksize, stride == 1 ? 0 : 1, total);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_lpips_conv_dgrad(const float* dy, const float* wt, const float* tap, const float* addend, float* dx, int B, int M, int C,
                            int H, int W, int ksize, int stride, int pad, void* stream) {
  CIDNET_CHECK_ARG(dy && wt && dx && B > 0 && M > 0 && C > 0 && H > 0 && W > 0);
  CIDNET_CHECK_ARG((tap == nullptr) == (addend == nullptr));
  if (B > 65535) return CIDNET_ERR_SHAPE;
  if (H + 2 * pad < ksize || W + 2 * pad < ksize) return CIDNET_ERR_SHAPE;
  if ((long)C * H * W > 2147483647L || (long)M * H * W > 2147483647L || (long)M * ksize * ksize > 2147483647L) return CIDNET_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (ksize == 11 && stride == 4 && pad == 2) {
    if (C != 3 || tap || M > 65535) return CIDNET_ERR_SHAPE;
    CIDNET_CHECK_ARG(reinterpret_cast<uintptr_t>(wt) % 16 == 0);       // read as float4
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const long nblk = ((long)H * W + 255) / 256;
    if (nblk > 2147483647L) return CIDNET_ERR_SHAPE;
    hipLaunchKernelGGL(lpips_conv1_dgrad_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, st, dy,
                       reinterpret_cast<const float4*>(wt), dx, M, H, W, Ho, Wo);
    CIDNET_LAUNCH_STATUS();
    return CIDNET_OK;
  }
  // stride 1: the output of the forward has the input's size; the GEMM's rows are the C input channels
  if (stride != 1 || C % kMT != 0 || C / kMT > 65535 || (long)H * W > 2147483647L - kNT) return CIDNET_ERR_SHAPE;
  if (ksize == 5 && pad == 2)
    return tap ? launch_conv<5, 1, 2, kEpiMaskAdd>(dy, wt, tap, addend, dx, B, C, M, H, W, H, W, st)
               : launch_conv<5, 1, 2, kEpiPlain>(dy, wt, nullptr, nullptr, dx, B, C, M, H, W, H, W, st);
  if (ksize == 3 && pad == 1)
    return tap ? launch_conv<3, 1, 1, kEpiMaskAdd>(dy, wt, tap, addend, dx, B, C, M, H, W, H, W, st)
               : launch_conv<3, 1, 1, kEpiPlain>(dy, wt, nullptr, nullptr, dx, B, C, M, H, W, H, W, st);
  return CIDNET_ERR_SHAPE;
}

int cidnet_lpips_maxpool3s2_bwd(const float* x, const float* gy, const float* addend, float* gx, long planes, int H, int W,
                                void* stream) {
  CIDNET_CHECK_ARG(x && gy && gx && planes > 0);
  if (H < 3 || W < 3) return CIDNET_ERR_SHAPE;
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long total = planes * H * W;
  hipLaunchKernelGGL(lpips_maxpool_bwd_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream, x, gy, addend, gx, H, W,
                     Ho, Wo, total);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_lpips_layer_bwd(const float* f0, const float* f1, const float* head, float* g, float weight, int relu_mask, int B, int C,
                           long P, void* stream) {
  CIDNET_CHECK_ARG(f0 && f1 && head && g && B > 0 && C > 0 && P > 0);
  const long nblk = (P + kDistPix - 1) / kDistPix;
  if (B > 65535 || nblk > 2147483647L) return CIDNET_ERR_SHAPE;
  const double coef = (double)weight / ((double)B * (double)P);
  hipLaunchKernelGGL(lpips_layer_bwd_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(kDistThreads), 0, (hipStream_t)stream, f0, f1, head,
                     g, C, P, coef, relu_mask);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
