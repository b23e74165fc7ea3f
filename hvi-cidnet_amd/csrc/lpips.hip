// LPIPS (AlexNet, version 0.1, lpips=True, spatial=False, eval mode) on the device: the third number of the reference's
// measure.py (measure.py:78,145-153: loss_fn.forward(im2tensor(gt), im2tensor(restored))).  Forward only.
//   ingest:   x = u / 127.5 - 1 formed in fp64 and rounded once to fp32 (lpips.im2tensor: a numpy fp64 expression handed to
//             torch.Tensor), u the 8-bit value or, under GT mean, the float clip(u s, 0, 255) (measure.py:138-146: not
//             re-quantized); then the scaling layer in fp32, (x - shift_c) / scale_c.
//   features: torchvision's AlexNet `features`, tapped after each of its five ReLUs:
//             conv 3->64 11x11 s4 p2 | pool 3/2, conv 64->192 5x5 p2 | pool 3/2, conv 192->384 3x3 p1 | conv 384->256 3x3 p1 |
//             conv 256->256 3x3 p1; every conv with bias, sizes by floor, pools unpadded.
//   distance: per layer, n(f) = f / (sqrt(sum_c f^2) + 1e-10) per pixel, d_l = mean over pixels of sum_c w_l[c] (n(f0) - n(f1))^2;
//             the score is sum_l d_l.
// Convolutions: one implicit-GEMM kernel, D[m][n] = sum_k W[m][k] X[k][n] with k = (c, ky, kx) and n a pixel of one image, on
// the fp32 matrix cores (v_mfma_f32_32x32x2f32: fp32 products, fp32 accumulation -- the accuracy of an fp32 convolution).
// A block of four waves owns 64 output channels x 64 pixels; K goes by in chunks of 64: the weight chunk and the im2col
// chunk are loaded into registers one chunk ahead and staged in LDS, zeros standing for the padding, for k >= K (363 =
// 3 11 11 is no multiple of the chunk, nor of the instruction's 2) and for pixels past the image's last -- no address
// outside the tensors is ever formed into a load.  The stride sits in the staging's address arithmetic (input row =
// S oy - PAD + ky), so the 11x11 stride-4 layer, the 5x5 and the 3x3 layers are instances of one template.  Bias and ReLU
// are the epilogue.  A block works on one image and its tiling is relative to that image, so an image's features do not
// depend on the rest of the batch.
// Distance: fp64 from the fp32 features on (sums of squares, norms, weighted squared differences); eight threads per pixel,
// each with an eighth of the channels, block partials to fixed slots, one wave per image sums them in a fixed order: no
// atomics, bit-identical from call to call.
// Built with -ffp-contract=off (build.py): with a fused multiply-add, n(f0) - n(f1) of two identical features would keep the
// rounding residual of one product and identical images would not score exactly 0.
#include "common.h"
#include "cidnet_hip.h"
#include "gt_mean.h"

namespace cidnet {
namespace {

constexpr int kMT = 64, kNT = 64, kKC = 64;                   // block tile: out channels x pixels; K chunk
constexpr int kLdA = kMT + 1, kLdB = kNT + 32;                 // LDS row strides (floats) of the [k][m] and [k][n] chunks
constexpr int kConvThreads = 256;
constexpr int kARows = kConvThreads / kKC;                     // weight rows one staging pass covers
constexpr int kAIter = kMT / kARows, kBIter = kKC / 4;         // staged values per thread and chunk: weights, im2col
constexpr int kDistThreads = 256, kDistPix = 32, kDistGroups = kDistThreads / kDistPix;

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

__global__ __launch_bounds__(256) void lpips_ingest_kernel(const uint8_t* __restrict__ q, const double* __restrict__ scale,
                                                           float* __restrict__ x, long hw, long total) {
  const float shift[3] = {-.030f, -.088f, -.188f}, scl[3] = {.458f, .448f, .450f};
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long plane = i / hw;
  const int c = (int)(plane % 3);
  double u = (double)q[i];
  if (scale) u = gt_mean_value(q[i], scale[plane / 3]);
  const float v = (float)(u / 127.5 - 1.0);                      // fp64, rounded once
  x[i] = (v - shift[c]) / scl[c];                                // the scaling layer, fp32
}

// y[b][m][oy][ox] = relu(bias[m] + sum_{c,ky,kx} w[m][c][ky][kx] x[b][c][S oy - PAD + ky][S ox - PAD + kx]), zeros outside x.
// grid: (pixel tiles, M / 64, B).  Waves 0..3 own the (32 m) x (32 n) quarters of the tile.
template <int KH, int S, int PAD>
__global__ __launch_bounds__(kConvThreads) void lpips_conv_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                                  const float* __restrict__ bias, float* __restrict__ y, int M, int C,
                                                                  int H, int W, int Ho, int Wo) {
  __shared__ float As[kKC * kLdA];
  __shared__ float Bs[kKC * kLdB];
  constexpr int KK = KH * KH;
  const int K = C * KK;
  const int P = Ho * Wo;
  const int b = blockIdx.z, m0 = blockIdx.y * kMT, p0 = blockIdx.x * kNT;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
  // im2col staging: this thread's pixel is fixed, its k runs over kb, kb + 4, ...
  const int n = t & 63, kb = t >> 6;
  const int p = p0 + n;
  const bool pin = p < P;
  const int oy = pin ? p / Wo : 0, ox = pin ? p - oy * Wo : 0;
  const int iy0 = oy * S - PAD, ix0 = ox * S - PAD;
  const float* xb = x + (long)b * C * H * W;
  // weight staging: consecutive lanes read consecutive k of one row
  const int ak = t % kKC, am = t / kKC;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // the chunk after the one in LDS waits in registers: its loads are in flight while the matrix cores work
  float ra[kAIter], rb[kBIter];
  auto fetch = [&](int k0) {
    const bool ak_in = k0 + ak < K;
#pragma unroll
    for (int i = 0; i < kAIter; ++i) ra[i] = ak_in ? wgt[(long)(m0 + am + kARows * i) * K + k0 + ak] : 0.f;
#pragma unroll
    for (int i = 0; i < kBIter; ++i) {
      const int kk = k0 + kb + 4 * i;
      const int c = kk / KK;
      const int r = kk - c * KK;
      const int ky = r / KH;
      const int kx = r - ky * KH;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = pin && kk < K && iy >= 0 && iy < H && ix >= 0 && ix < W;
      rb[i] = ok ? xb[((long)c * H + iy) * W + ix] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kKC) {
#pragma unroll
    for (int i = 0; i < kAIter; ++i) As[ak * kLdA + am + kARows * i] = ra[i];
#pragma unroll
    for (int i = 0; i < kBIter; ++i) Bs[(kb + 4 * i) * kLdB + n] = rb[i];
    __syncthreads();
    if (k0 + kKC < K) fetch(k0 + kKC);
    const float* ap = As + (lane >> 5) * kLdA + wm + (lane & 31);
    const float* bp = Bs + (lane >> 5) * kLdB + wn + (lane & 31);
#pragma unroll
    for (int k = 0; k < kKC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k * kLdA], bp[k * kLdB], acc, 0, 0, 0);
    __syncthreads();
  }
  // D[i][j]: j = lane % 32, i = 8 (r / 4) + 4 (lane / 32) + r % 4
  const int pj = p0 + wn + (lane & 31);
  if (pj < P) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
      const float v = acc[r] + bias[m];
      y[((long)b * M + m) * P + pj] = v > 0.f ? v : 0.f;
    }
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

inline int grid_for(long n, int cap) {
  long g = (n + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

template <int KH, int S, int PAD>
int launch_conv(const float* x, const float* w, const float* bias, float* y, int B, int M, int C, int H, int W, int Ho, int Wo,
                hipStream_t st) {
  const dim3 grid((unsigned)(((long)Ho * Wo + kNT - 1) / kNT), (unsigned)(M / kMT), (unsigned)B);
  hipLaunchKernelGGL((lpips_conv_kernel<KH, S, PAD>), grid, dim3(kConvThreads), 0, st, x, w, bias, y, M, C, H, W, Ho, Wo);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
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
  if (ksize == 11 && stride == 4 && pad == 2) return launch_conv<11, 4, 2>(x, w, bias, y, B, M, C, H, W, Ho, Wo, st);
  if (ksize == 5 && stride == 1 && pad == 2) return launch_conv<5, 1, 2>(x, w, bias, y, B, M, C, H, W, Ho, Wo, st);
  if (ksize == 3 && stride == 1 && pad == 1) return launch_conv<3, 1, 1>(x, w, bias, y, B, M, C, H, W, Ho, Wo, st);
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
  DistPlan plan;
  for (int l = 0; l < 5; ++l) {
    const long P = (long)s.fh[l] * s.fw[l];
    plan.nblk[l] = (int)dist_blocks(P);
    plan.n_pix[l] = (double)P;
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const double*>(ws),
                     dist_blocks((long)s.fh[0] * s.fw[0]), plan, layers, score);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
