// LPIPS (AlexNet, version 0.1, lpips=True, spatial=False, eval mode) on the device: the third number of the reference's
// measure.py (measure.py:78,145-153: loss_fn.forward(im2tensor(gt), im2tensor(restored))).  The forward pass, of the metric
// and of the training loss (whose backward kernels are csrc/lpips_loss.hip).
//   ingest:   x = u / 127.5 - 1 formed in fp64 and rounded once to fp32 (lpips.im2tensor: a numpy fp64 expression handed to
//             torch.Tensor), u the 8-bit value or, under GT mean, the float clip(u s, 0, 255) (measure.py:138-146: not
//             re-quantized); then the scaling layer in fp32, (x - shift_c) / scale_c.  The loss ingests a float image
//             (lpips' normalize=True): v = 2 x - 1 in fp32, then the same scaling layer; backward (g / scale_c) 2.
//   features: torchvision's AlexNet `features`, tapped after each of its five ReLUs:
//             conv 3->64 11x11 s4 p2 | pool 3/2, conv 64->192 5x5 p2 | pool 3/2, conv 192->384 3x3 p1 | conv 384->256 3x3 p1 |
//             conv 256->256 3x3 p1; every conv with bias, sizes by floor, pools unpadded.
//   distance: per layer, n(f) = f / (sqrt(sum_c f^2) + 1e-10) per pixel, d_l = mean over pixels of sum_c w_l[c] (n(f0) - n(f1))^2;
//             the score is sum_l d_l.
// Convolutions: the implicit-GEMM template of csrc/lpips_conv.h on the fp32 matrix cores (fp32 products, fp32 accumulation
// -- the accuracy of an fp32 convolution); K = 363 = 3 11 11 of the first layer is no multiple of the chunk, nor of the
// instruction's 2, and the stride sits in the staging's address arithmetic, so the 11x11 stride-4 layer, the 5x5 and the 3x3
// layers are instances of one template.  Bias and ReLU are the epilogue.
// Distance: fp64 from the fp32 features on (sums of squares, norms, weighted squared differences); eight threads per pixel,
// each with an eighth of the channels, block partials to fixed slots, one wave per image sums them in a fixed order: no
// atomics, bit-identical from call to call.
// Built with -ffp-contract=off (build.py): with a fused multiply-add, n(f0) - n(f1) of two identical features would keep the
// rounding residual of one product and identical images would not score exactly 0.
#include "common.h"
#include "cidnet_hip.h"
#include "gt_mean.h"
#include "lpips_conv.h"

namespace cidnet {
namespace {

struct LpipsSizes {
  int fh[5], fw[5];
};

// feature-map sizes of an h x w image; false below the 31 x 31 minimum (where the second pool would have no window)
inline bool lpips_sizes(int h, int w, LpipsSizes* s) {
  if (h < 31 || w < 31) return false;
  s->fh[0] = (h + 4 - 11) / 4 + 1;
  s->fw[0] = (w + 4 - 11) / 4 + 1;
  s->fh[1] = (s->fh[0] - 3) / 2 + 1;
  s->fw[1] = (s->fw[0] - 3) / 2 + 1;
  for (int l = 2; l < 5; ++l) {
    s->fh[l] = (s->fh[1] - 3) / 2 + 1;
    s->fw[l] = (s->fw[1] - 3) / 2 + 1;
  }
  return true;
}
inline int lpips_channels(int l) {
  const int c[5] = {64, 192, 384, 256, 256};
  return c[l];
}
inline long dist_blocks(long P) { return (P + kDistPix - 1) / kDistPix; }

// the scaling layer's constants (lpips.ScalingLayer)
__device__ __forceinline__ float lpips_shift(int c) { return c == 0 ? -.030f : (c == 1 ? -.088f : -.188f); }
__device__ __forceinline__ float lpips_scale(int c) { return c == 0 ? .458f : (c == 1 ? .448f : .450f); }

__global__ __launch_bounds__(256) void lpips_ingest_kernel(const uint8_t* __restrict__ q, const double* __restrict__ scale,
                                                           float* __restrict__ x, long hw, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long plane = i / hw;
  const int c = (int)(plane % 3);
  double u = (double)q[i];
  if (scale) u = gt_mean_value(q[i], scale[plane / 3]);
  const float v = (float)(u / 127.5 - 1.0);                      // fp64, rounded once
  x[i] = (v - lpips_shift(c)) / lpips_scale(c);                  // the scaling layer, fp32
}

// the loss's ingest of a float image in [0, 1] (any range is taken): BWD false, y = ((2 x - 1) - shift_c) / scale_c, 2 x exact
// and every other step one fp32 rounding; BWD true, y = (x / scale_c) 2 for the gradient x.  No contraction (build.py).
template <bool BWD>
__global__ __launch_bounds__(256) void lpips_ingest_f32_kernel(const float* __restrict__ x, float* __restrict__ y, long hw, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)((i / hw) % 3);
  if (BWD) {
    y[i] = (x[i] / lpips_scale(c)) * 2.f;
  } else {
    const float v = 2.f * x[i] - 1.f;
    y[i] = (v - lpips_shift(c)) / lpips_scale(c);
  }
}

// nn.MaxPool2d(kernel_size=3, stride=2): output floor((H - 3) / 2) + 1, no padding
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Ho,
                                                            int Wo, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const long t = i / Wo;
    const int yo = (int)(t % Ho);
    const long plane = t / Ho;
    const float* p = x + plane * (long)H * W + (long)(2 * yo) * W + 2 * xo;
    float m = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, p[dy * W + dx]);
    y[i] = m;
  }
}

// part[(img * 5 + layer) * stride + block] = sum over the block's pixels of sum_c head[c] (n(f0) - n(f1))^2.  A block has
// kDistPix pixels; the kDistGroups threads of a pixel take the channels g, g + kDistGroups, ... and meet in LDS, where each
// adds the groups' sums of squares in group order -- the same order in every thread, every call.
__global__ __launch_bounds__(kDistThreads) void lpips_dist_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                  const float* __restrict__ head, double* __restrict__ part, int C,
                                                                  long P, long stride, int layer) {
  __shared__ double red[kDistThreads / 64];
  __shared__ double ss[2][kDistGroups][kDistPix];
  const long img = blockIdx.y;
  const int px = threadIdx.x % kDistPix, grp = threadIdx.x / kDistPix;
  const long p = (long)blockIdx.x * kDistPix + px;
  const bool in = p < P;
  const float* a = f0 + img * C * P + (in ? p : 0);
  const float* b = f1 + img * C * P + (in ? p : 0);
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
  double acc = 0.0;
  if (in) {
    sa = 0.0;
    sb = 0.0;
#pragma unroll
    for (int k = 0; k < kDistGroups; ++k) {
      sa += ss[0][k][px];
      sb += ss[1][k][px];
    }
    const double ra = 1.0 / (sqrt(sa) + 1e-10), rb = 1.0 / (sqrt(sb) + 1e-10);
    for (int c = grp; c < C; c += kDistGroups) {
      const double d = (double)a[c * P] * ra - (double)b[c * P] * rb;
      acc += (double)head[c] * (d * d);
    }
  }
  acc = wave_sum_f64(acc);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < kDistThreads / 64; ++k) s += red[k];
    part[(img * 5 + layer) * stride + blockIdx.x] = s;
  }
}

struct DistPlan {
  int nblk[5];
  double n_pix[5];
};

// one wave per image: d_l = (sum of the layer's partials) / pixels in a fixed order, and their sum in layer order
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ part, long stride, DistPlan plan,
                                                          double* __restrict__ layers, double* __restrict__ total) {
  const long img = blockIdx.x;
  double sum = 0.0;
  for (int l = 0; l < 5; ++l) {
    const double* pp = part + (img * 5 + l) * stride;
    double a = 0.0;
    for (int t = threadIdx.x; t < plan.nblk[l]; t += 64) a += pp[t];
    a = wave_sum_f64(a);
    const double d = a / plan.n_pix[l];
    if (threadIdx.x == 0 && layers) layers[img * 5 + l] = d;
    sum += d;
  }
  if (threadIdx.x == 0 && total) total[img] = sum;
}

// one wave: loss = weight / B * sum_b sum_l d_l(b), the d_l formed from the partials exactly as lpips_finish_kernel forms them
// and added in image order, layer order inside an image; fp64 throughout, one rounding to fp32 at the end
__global__ __launch_bounds__(64) void lpips_loss_finish_kernel(const double* __restrict__ part, long stride, DistPlan plan, int B,
                                                               float weight, float* __restrict__ loss) {
  double total = 0.0;
  for (long img = 0; img < B; ++img) {
    double sum = 0.0;
    for (int l = 0; l < 5; ++l) {
      const double* pp = part + (img * 5 + l) * stride;
      double a = 0.0;
      for (int t = threadIdx.x; t < plan.nblk[l]; t += 64) a += pp[t];
      a = wave_sum_f64(a);
      sum += a / plan.n_pix[l];
    }
    total += sum;
  }
  if (threadIdx.x == 0) *loss = (float)((double)weight * (total / (double)B));
}

inline DistPlan dist_plan(const LpipsSizes& s) {
  DistPlan plan;
  for (int l = 0; l < 5; ++l) {
    const long P = (long)s.fh[l] * s.fw[l];
    plan.nblk[l] = (int)dist_blocks(P);
    plan.n_pix[l] = (double)P;
  }
  return plan;
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_lpips_feature_sizes(int h, int w, int* sizes) {
  CIDNET_CHECK_ARG(sizes && h > 0 && w > 0);
  LpipsSizes s;
  if (!lpips_sizes(h, w, &s)) return CIDNET_ERR_SHAPE;
  for (int l = 0; l < 5; ++l) {
    sizes[2 * l] = s.fh[l];
    sizes[2 * l + 1] = s.fw[l];
  }
  return CIDNET_OK;
}

int cidnet_metric_lpips_ingest(const uint8_t* q, const double* scale, float* x, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(q && x && B > 0 && h > 0 && w > 0);
  const long hw = (long)h * w;
  const long total = (long)B * 3 * hw;
  if ((total + 255) / 256 > 2147483647L) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(lpips_ingest_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, scale, x, hw,
                     total);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_lpips_conv_relu(const float* x, const float* w, const float* bias, float* y, int B, int M, int C, int H, int W, int ksize,
                           int stride, int pad, void* stream) {
  CIDNET_CHECK_ARG(x && w && bias && y && B > 0 && M > 0 && C > 0 && H > 0 && W > 0);
  if (M % kMT != 0 || B > 65535 || M / kMT > 65535) return CIDNET_ERR_SHAPE;
  if (H + 2 * pad < ksize || W + 2 * pad < ksize) return CIDNET_ERR_SHAPE;
  if ((long)C * H * W > 2147483647L || (long)C * ksize * ksize > 2147483647L) return CIDNET_ERR_SHAPE;
  const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
  if ((long)Ho * Wo > 2147483647L - kNT) return CIDNET_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (ksize == 11 && stride == 4 && pad == 2) return launch_conv<11, 4, 2, kEpiBiasRelu>(x, w, bias, nullptr, y, B, M, C, H, W, Ho, Wo, st);
  if (ksize == 5 && stride == 1 && pad == 2) return launch_conv<5, 1, 2, kEpiBiasRelu>(x, w, bias, nullptr, y, B, M, C, H, W, Ho, Wo, st);
  if (ksize == 3 && stride == 1 && pad == 1) return launch_conv<3, 1, 1, kEpiBiasRelu>(x, w, bias, nullptr, y, B, M, C, H, W, Ho, Wo, st);
  return CIDNET_ERR_SHAPE;
}

int cidnet_lpips_maxpool3s2(const float* x, float* y, long planes, int H, int W, void* stream) {
  CIDNET_CHECK_ARG(x && y && planes > 0);
  if (H < 3 || W < 3) return CIDNET_ERR_SHAPE;
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long total = planes * Ho * Wo;
  hipLaunchKernelGGL(lpips_maxpool_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, Ho, Wo, total);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

// layout (doubles): partials [B][5][blocks of layer 0]
long cidnet_metric_lpips_ws_floats(int B, int h, int w) {
  LpipsSizes s;
  if (B <= 0 || !lpips_sizes(h, w, &s)) return 0;
  return 2 * (long)B * 5 * dist_blocks((long)s.fh[0] * s.fw[0]);
}

int cidnet_metric_lpips_layer(const float* f0, const float* f1, const float* head, float* ws, long ws_floats, int layer, int B, int C,
                              int fh, int fw, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(f0 && f1 && head && ws && B > 0 && h > 0 && w > 0);
  LpipsSizes s;
  if (!lpips_sizes(h, w, &s) || layer < 0 || layer > 4 || B > 65535) return CIDNET_ERR_SHAPE;
  if (C != lpips_channels(layer) || fh != s.fh[layer] || fw != s.fw[layer]) return CIDNET_ERR_SHAPE;
  if (ws_floats < cidnet_metric_lpips_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  const long P = (long)fh * fw;
  const long stride = dist_blocks((long)s.fh[0] * s.fw[0]);
  hipLaunchKernelGGL(lpips_dist_kernel, dim3((unsigned)dist_blocks(P), (unsigned)B), dim3(kDistThreads), 0, (hipStream_t)stream, f0, f1,
                     head, reinterpret_cast<double*>(ws), C, P, stride, layer);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_metric_lpips_finish(const float* ws, long ws_floats, double* layers, double* score, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(ws && (layers || score) && B > 0 && h > 0 && w > 0);
  LpipsSizes s;
  if (!lpips_sizes(h, w, &s)) return CIDNET_ERR_SHAPE;
  if (ws_floats < cidnet_metric_lpips_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  const DistPlan plan = dist_plan(s);
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const double*>(ws),
                     dist_blocks((long)s.fh[0] * s.fw[0]), plan, layers, score);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

static int ingest_f32(const float* x, float* y, int B, int h, int w, bool bwd, hipStream_t st) {
  CIDNET_CHECK_ARG(x && y && B > 0 && h > 0 && w > 0);
  const long hw = (long)h * w;
  const long total = (long)B * 3 * hw;
  if ((total + 255) / 256 > 2147483647L) return CIDNET_ERR_SHAPE;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (bwd)
    hipLaunchKernelGGL(lpips_ingest_f32_kernel<true>, grid, dim3(256), 0, st, x, y, hw, total);
  else
    hipLaunchKernelGGL(lpips_ingest_f32_kernel<false>, grid, dim3(256), 0, st, x, y, hw, total);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_lpips_ingest_f32(const float* x, float* z, int B, int h, int w, void* stream) {
  return ingest_f32(x, z, B, h, w, false, (hipStream_t)stream);
}

int cidnet_lpips_ingest_f32_bwd(const float* g, float* gx, int B, int h, int w, void* stream) {
  return ingest_f32(g, gx, B, h, w, true, (hipStream_t)stream);
}

long cidnet_lpips_loss_ws_floats(int B, int h, int w) { return cidnet_metric_lpips_ws_floats(B, h, w); }

int cidnet_lpips_loss_finish(const float* ws, long ws_floats, float weight, float* loss, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(ws && loss && B > 0 && h > 0 && w > 0);
  LpipsSizes s;
  if (!lpips_sizes(h, w, &s)) return CIDNET_ERR_SHAPE;
  if (ws_floats < cidnet_lpips_loss_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  hipLaunchKernelGGL(lpips_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const double*>(ws),
                     dist_blocks((long)s.fh[0] * s.fw[0]), dist_plan(s), B, weight, loss);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
