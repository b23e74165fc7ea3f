// Evaluation metrics on the device: what the reference's eval.py + measure.py compute around a trained model.
//   to_uint8:  clamp(x, 0, 1) * 255.0f (fp32), truncated to uint8, top-left h x w crop      (eval.py:69-73, ToPILImage)
//   PSNR:      10 log10(255^2 / (mean((a - b)^2) + 1e-8)) over the 3 h w values of one image (measure.py:66-71)
//   SSIM:      per colour plane, 11 x 11 Gaussian window (sigma 1.5) over the valid region only, C1 = (0.01 255)^2,
//              C2 = (0.03 255)^2, mean of the map per plane, mean of the three planes           (measure.py:23-64)
//   GT mean:   s = mean(gray(gt)) / mean(gray(restored)), restored -> clip(restored * s, 0, 255) in fp64 (measure.py:138-141);
//              gray = the BT.601 fixed-point rule (4899 R + 9617 G + 1868 B + 8192) >> 14 on uint8, summed exactly.  The scale
//              is formed once (cidnet_metric_gt_mean_scale, below) and handed to every paired metric: PSNR/SSIM here,
//              csrc/lpips.hip and csrc/ciede2000.hip; gray and the clip are csrc/gt_mean.h.
// Arithmetic is fp64 as the reference's; the squared error sums are exact (integers, or products of fp32 values in fp64).
// Reductions: per-block partials written to fixed slots, summed by a per-image finishing kernel in a fixed order, so a
// result is bit-identical from call to call and does not depend on which other images share the batch.
//
// SSIM tile kernel: one wave owns 64 columns x kTH rows of one (image, plane); the uint8 tile + 5-pixel halo sits in LDS.
// Every lane walks its column down the tile: for each input row it forms the five horizontal window sums (x, y, x^2, y^2,
// x y; fp64) and scatters them into eleven rotating accumulators, one per pending output row -- the vertical pass runs in
// registers, and an output row is complete (and its SSIM formed) when the input row five below it has been added.
#include "common.h"
#include "cidnet_hip.h"
#include "gt_mean.h"

namespace cidnet {
namespace {

constexpr int kWin = 11, kR = 5;
constexpr int kTW = 64, kTH = 32;                              // output tile; one wave per tile
constexpr int kLH = kTH + 2 * kR, kLW = kTW + 2 * kR;          // 42 x 74 bytes per image in LDS
constexpr int kGrayChunk = 16384;                              // pixels per block of the gray-sum pass
constexpr int kGrayThreads = 256;

struct Gauss64 {
  double g[kWin];
};

inline Gauss64 make_gauss64() {                  // exp(-(i-5)^2 / (2 1.5^2)), normalised to sum 1, in double
  Gauss64 w;
  double s = 0.0;
  for (int i = 0; i < kWin; ++i) {
    const double d = (double)(i - kR);
    w.g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    s += w.g[i];
  }
  for (int i = 0; i < kWin; ++i) w.g[i] = w.g[i] / s;
  return w;
}

__global__ __launch_bounds__(256) void to_uint8_kernel(const float* __restrict__ x, uint8_t* __restrict__ q, long total, int Hp,
                                                      int Wp, int h, int w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % w);
  const long r = i / w;
  const int y = (int)(r % h);
  const long plane = r / h;
  const float v = x[(plane * Hp + y) * (long)Wp + c];
  const float cl = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;        // NaN -> 0
  q[i] = (uint8_t)(unsigned)(cl * 255.0f);                      // fp32 product, truncated (pic.mul(255).byte())
}

// gray sums of both images of each pair, per chunk of pixels (exact: integers)
__global__ __launch_bounds__(kGrayThreads) void gray_sum_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                unsigned long long* __restrict__ part, long hw, int n_chunk) {
  __shared__ unsigned red[2][kGrayThreads / 64];
  const long img = blockIdx.y;
  const uint8_t* pa = a + img * 3 * hw;
  const uint8_t* pb = b + img * 3 * hw;
  const long i0 = (long)blockIdx.x * kGrayChunk;
  const long i1 = i0 + kGrayChunk < hw ? i0 + kGrayChunk : hw;
  unsigned sa = 0, sb = 0;                                       // <= 16384 * 255 per block
  for (long i = i0 + threadIdx.x; i < i1; i += kGrayThreads) {
    sa += gray601(pa[i], pa[i + hw], pa[i + 2 * hw]);
    sb += gray601(pb[i], pb[i + hw], pb[i + 2 * hw]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sb += __shfl_xor(sb, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wv] = sa;
    red[1][wv] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long ta = 0, tb = 0;
    for (int k = 0; k < kGrayThreads / 64; ++k) {
      ta += red[0][k];
      tb += red[1][k];
    }
    part[((long)img * n_chunk + blockIdx.x) * 2 + 0] = ta;
    part[((long)img * n_chunk + blockIdx.x) * 2 + 1] = tb;
  }
}

// s = (sum_gt / N) / (sum_restored / N), one lane per image
__global__ void gt_mean_scale_kernel(const unsigned long long* __restrict__ part, int n_chunk, double n_pix, double* __restrict__ scale,
                                     int B) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= B) return;
  unsigned long long ta = 0, tb = 0;
  for (int k = 0; k < n_chunk; ++k) {
    ta += part[((long)img * n_chunk + k) * 2 + 0];
    tb += part[((long)img * n_chunk + k) * 2 + 1];
  }
  scale[img] = ((double)tb / n_pix) / ((double)ta / n_pix);
}

// One (image, plane) tile of 64 x kTH output pixels per block (one wave).  part[2 * tile] = sum of the SSIM map over the
// tile's pixels inside the valid region, part[2 * tile + 1] = sum of squared errors over the tile's pixels.
template <bool GTM, bool SSIM>
__global__ __launch_bounds__(64) void metric_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                         const double* __restrict__ scale, Gauss64 gw, double* __restrict__ part,
                                                         int h, int w) {
  __shared__ uint8_t ta[kLH * kLW], tb[kLH * kLW];
  const long plane = blockIdx.z;                                 // image * 3 + colour
  const double s = GTM ? scale[plane / 3] : 1.0;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const uint8_t* pa = a + plane * (long)h * w;
  const uint8_t* pb = b + plane * (long)h * w;
  for (int i = threadIdx.x; i < kLH * kLW; i += 64) {
    const int r = i / kLW, c = i - r * kLW;
    const int y = y0 - kR + r, x = x0 - kR + c;
    const bool in = y >= 0 && y < h && x >= 0 && x < w;
    ta[i] = in ? pa[(long)y * w + x] : 0;
    tb[i] = in ? pb[(long)y * w + x] : 0;
  }
  __syncthreads();
  const int c = threadIdx.x;
  const int x = x0 + c;
  const bool col_in = x < w;
  const bool col_valid = x >= kR && x <= w - 1 - kR;
  const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
  double se = 0.0, ssum = 0.0;
  double acc[kWin][5];
#pragma unroll
  for (int k = 0; k < kWin; ++k)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[k][m] = 0.0;
#pragma unroll 1
  for (int r0 = 0; r0 < kLH; r0 += kWin) {
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const int r = r0 + k;                                      // tile row of the input row (image row y0 - 5 + r)
      if (r >= kLH) continue;                                    // the last round of the 42-row tile has 9 rows
      const uint8_t* ra = ta + r * kLW + c;
      const uint8_t* rb = tb + r * kLW + c;
      // squared error of this lane's pixel of the input row, when the row is one of the tile's own rows
      if (r >= kR && r < kR + kTH && col_in && y0 - kR + r < h) {
        const unsigned av = ra[kR], bv = rb[kR];
        double d;
        if (GTM) d = (double)(float)gt_mean_value(av, s) - (double)bv;     // PSNR reads the fp32 cast (measure.py:67)
        else d = (double)((int)av - (int)bv);
        se += d * d;
      }
      if (SSIM) {
        double hs[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < kWin; ++i) {
          const double xv = GTM ? gt_mean_value(ra[i], s) : (double)ra[i];
          const double yv = (double)rb[i];
          const double g = gw.g[i];
          hs[0] += g * xv;
          hs[1] += g * yv;
          hs[2] += g * (xv * xv);
          hs[3] += g * (yv * yv);
          hs[4] += g * (xv * yv);
        }
        // input row r is tap j of output row r - j; that row's accumulator is slot (r - j) mod 11 = (k - j) mod 11
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
          const double g = gw.g[j];
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[(k - j + kWin) % kWin][m] += g * hs[m];
        }
        // output row r - 10 (image row y0 + r - 10) has all eleven taps now: slot (k + 1) mod 11
        double* o = acc[(k + 1) % kWin];
        const int y = y0 + r - 2 * kR;
        if (r >= 2 * kR && col_valid && y >= kR && y <= h - 1 - kR) {
          const double mu1 = o[0], mu2 = o[1];
          const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
          const double s1 = o[2] - mu1_sq, s2 = o[3] - mu2_sq, s12 = o[4] - mu1_mu2;
          ssum += ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        }
#pragma unroll
        for (int m = 0; m < 5; ++m) o[m] = 0.0;
      }
    }
  }
  se = wave_sum_f64(se);
  ssum = wave_sum_f64(ssum);
  if (threadIdx.x == 0) {
    const long tile = (plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[2 * tile] = ssum;
    part[2 * tile + 1] = se;
  }
}

// one wave per image: per-plane SSIM means, their mean, and the PSNR, from the tile partials in a fixed order
__global__ __launch_bounds__(64) void metric_finish_kernel(const double* __restrict__ part, int tiles_per_plane, double n_valid,
                                                           double n_values, double* __restrict__ psnr, double* __restrict__ ssim) {
  const long img = blockIdx.x;
  double se = 0.0, ssim_sum = 0.0;
  for (int p = 0; p < 3; ++p) {
    const double* pp = part + 2 * (img * 3 + p) * (long)tiles_per_plane;
    double a = 0.0, e = 0.0;
    for (int t = threadIdx.x; t < tiles_per_plane; t += 64) {
      a += pp[2 * t];
      e += pp[2 * t + 1];
    }
    a = wave_sum_f64(a);
    e = wave_sum_f64(e);
    ssim_sum += a / n_valid;
    se += e;
  }
  if (threadIdx.x == 0) {
    if (ssim) ssim[img] = ssim_sum / 3.0;
    if (psnr) psnr[img] = 10.0 * log10(255.0 * 255.0 / (se / n_values + 1e-8));
  }
}

inline long gray_chunks(long hw) { return (hw + kGrayChunk - 1) / kGrayChunk; }
inline long tiles_per_plane(int h, int w) { return (long)((w + kTW - 1) / kTW) * ((h + kTH - 1) / kTH); }

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_metric_to_uint8(const float* x, uint8_t* q, int B, int Hp, int Wp, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(x && q && B > 0 && Hp > 0 && Wp > 0 && h > 0 && w > 0);
  if (h > Hp || w > Wp) return CIDNET_ERR_SHAPE;
  const long total = (long)B * 3 * h * w;
  hipLaunchKernelGGL(to_uint8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, q, total, Hp, Wp,
                     h, w);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

// 8-byte words: gray partials [B][chunks][2]
long cidnet_metric_gt_mean_scale_ws_floats(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return 2 * (long)B * gray_chunks((long)h * w) * 2;
}

int cidnet_metric_gt_mean_scale(const uint8_t* restored, const uint8_t* gt, double* scale, float* ws, long ws_floats, int B, int h,
                                int w, void* stream) {
  CIDNET_CHECK_ARG(restored && gt && scale && ws && B > 0 && h > 0 && w > 0);
  if (B > 65535) return CIDNET_ERR_SHAPE;
  if (ws_floats < cidnet_metric_gt_mean_scale_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  const long hw = (long)h * w;
  const long n_chunk = gray_chunks(hw);
  unsigned long long* gpart = reinterpret_cast<unsigned long long*>(ws);
  hipLaunchKernelGGL(gray_sum_kernel, dim3((unsigned)n_chunk, (unsigned)B), dim3(kGrayThreads), 0, st, restored, gt, gpart, hw,
                     (int)n_chunk);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(gt_mean_scale_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, gpart, (int)n_chunk, (double)hw,
                     scale, B);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

// 8-byte words: tile partials [B][3][tiles][2]
long cidnet_metric_ws_floats(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return 2 * ((long)B * 3 * tiles_per_plane(h, w) * 2);
}

int cidnet_metric_psnr_ssim(const uint8_t* restored, const uint8_t* gt, const double* scale, double* psnr, double* ssim, float* ws,
                            long ws_floats, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(restored && gt && (psnr || ssim) && ws && B > 0 && h > 0 && w > 0);
  if (ssim && (h < kWin || w < kWin)) return CIDNET_ERR_SHAPE;     // the valid region would be empty
  if (ws_floats < cidnet_metric_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  const long hw = (long)h * w;
  double* tpart = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH), (unsigned)(B * 3));
  const Gauss64 g = make_gauss64();
  if (scale && ssim) hipLaunchKernelGGL((metric_tile_kernel<true, true>), grid, dim3(64), 0, st, restored, gt, scale, g, tpart, h, w);
  else if (scale) hipLaunchKernelGGL((metric_tile_kernel<true, false>), grid, dim3(64), 0, st, restored, gt, scale, g, tpart, h, w);
  else if (ssim) hipLaunchKernelGGL((metric_tile_kernel<false, true>), grid, dim3(64), 0, st, restored, gt, scale, g, tpart, h, w);
  else hipLaunchKernelGGL((metric_tile_kernel<false, false>), grid, dim3(64), 0, st, restored, gt, scale, g, tpart, h, w);
  CIDNET_LAUNCH_STATUS();
  const double n_valid = (double)(h - 2 * kR) * (double)(w - 2 * kR);
  hipLaunchKernelGGL(metric_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, tpart, (int)tiles_per_plane(h, w), n_valid,
                     3.0 * (double)hw, psnr, ssim);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
