// BRISQUE on the device: the second number of the reference's measure_niqe_bris.py (imquality.brisque.score), restated from
// the description of that package (include/cidnet_hip.h holds the contract, DESIGN.md 6.17 what is pinned to what).  All fp64.
//   gray      Y = ((0.2125 R + 0.7154 G) + 0.0721 B) / 255 of the uint8 planes;
//   MSCN      mu = K * Y, s = K * Y^2 with the 7 x 7 Gaussian K (sigma 7/6, sum 1), ZERO fill outside the image, the 49 taps
//             added in row-major order; dev = sqrt(|mu^2 - s|); M = (Y - mu) / (dev + 1/255);
//   products  H = M[r,c] M[r,c+1], V = M[r,c] M[r+1,c], D1 = M[r,c] M[r+1,c+1], D2 = M[r,c] M[r+1,c-1]: slices, no wrap -- a pair
//             whose partner lies outside the image does not exist, so the five maps have different element counts;
//   moments   per map six sums: count and sum of squares of the negatives, the same of the elements >= 0, sum |v|, sum v^2;
//   fit       the asymmetric generalised Gaussian: alpha is the root of phi(a) = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)) = R
//             in [0.05, 100], sectioned to a fixed point of the fp64 bracket;
//   half      Gaussian (sigma 0.5, radius 2, mirror) down the columns and then along the rows, then the 2-tap resampler at
//             (o + 0.5) in / out - 0.5 to (round(h / 2), round(w / 2)), half to even;
//   score     z = -1 + 2 (f - min) / (max - min), then sum_i coef_i exp(-gamma |sv_i - z|^2) - rho in file order.
// Compiled with -ffp-contract=off (build.py): the roundings are those of the text above.  No atomics, vector stores only,
// and every reduction has a fixed order (strided per-thread sums, xor-shuffle tree, waves in order; tile slots by lane and
// stride, then the same tree): results are bit-identical from call to call and do not depend on the rest of the batch.
//
// Tile kernel: one workgroup per (image, 32 x 32 tile).  The tile's gray values with a 4-pixel halo (3 for the window, 1 for
// the neighbours) are staged in LDS as fp64 (40 x 40 x 8 B = 12.5 KiB), the MSCN tile with one more column left and right and
// one more row below is formed beside it (33 x 34 x 8 B = 8.8 KiB), and the five maps' sums read it there.  A pair belongs to
// the tile that owns M[r,c].  32 keeps a 32-lane half-wave on one 256-byte LDS row (conflict-free 8-byte reads) and leaves
// the occupancy to the registers (125 VGPRs: four workgroups on a compute unit); see DESIGN.md 6.17 for the choice.
#include "common.h"
#include "cidnet_hip.h"

#include <cmath>

namespace cidnet {
namespace {

constexpr int kT = 32;                                          // tile side
constexpr int kHalo = 4, kR = 3, kWin = 7;
constexpr int kGW = kT + 2 * kHalo;                             // 40: staged gray rows / columns
constexpr int kMR = kT + 1, kMC = kT + 2;                       // MSCN tile: rows 0 .. T, columns -1 .. T
constexpr int kThreads = 256;
constexpr int kMaps = 5, kSums = 6;
constexpr int kFeat = 18;
constexpr int kMinSide = 16;
constexpr long kMaxPixels = 1L << 26;                           // keeps every per-image count inside an int
constexpr int kSvrChunk = 1024;

struct Window {
  double k[kWin * kWin];
};
struct Gauss5 {
  double k[3];                                                  // centre, +-1, +-2
};

inline Window make_window() {
  Window w;
  const double sigma = 7.0 / 6.0;
  double s = 0.0;
  for (int i = 0; i < kWin; ++i)
    for (int j = 0; j < kWin; ++j) {
      const double d = (double)((i - kR) * (i - kR) + (j - kR) * (j - kR));
      w.k[i * kWin + j] = std::exp(-d / (2.0 * sigma * sigma));
      s += w.k[i * kWin + j];
    }
  for (int i = 0; i < kWin * kWin; ++i) w.k[i] /= s;
  return w;
}

inline Gauss5 make_gauss5() {
  Gauss5 g;
  const double sigma = 0.5;
  double e[3], s = 0.0;
  for (int i = 0; i < 3; ++i) e[i] = std::exp(-0.5 / (sigma * sigma) * (double)(i * i));
  s = e[0] + 2.0 * e[1] + 2.0 * e[2];
  for (int i = 0; i < 3; ++i) g.k[i] = e[i] / s;
  return g;
}

inline int half_size(int n) {                                   // numpy's round(n / 2): half to even
  const int q = n / 2;
  return (n % 2 == 0 || q % 2 == 0) ? q : q + 1;
}

__device__ __forceinline__ double gray_of(const uint8_t* __restrict__ p, long hw, long i) {
  double v = 0.2125 * (double)p[i] + 0.7154 * (double)p[hw + i];
  v = v + 0.0721 * (double)p[2 * hw + i];
  return v / 255.0;
}

__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(256) void brisque_gray_kernel(const uint8_t* __restrict__ rgb, double* __restrict__ y, long hw,
                                                          long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long img = i / hw;
  y[i] = gray_of(rgb + img * 3 * hw, hw, i - img * hw);
}

// the 5-tap mirror Gaussian along one axis of (B,h,w): `step` = w down the columns (axis 0, n = h), 1 along the rows (n = w)
__global__ __launch_bounds__(256) void brisque_gauss_kernel(const double* __restrict__ in, double* __restrict__ out, Gauss5 g,
                                                           long total, int h, int w, int vertical) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % w);
  const long r = i / w;
  const int row = (int)(r % h);
  const long step = vertical ? (long)w : 1L;
  const int pos = vertical ? row : c, n = vertical ? h : w;
  const double* p = in + i - (long)pos * step;                   // element 0 of this pixel's line
  double acc = g.k[0] * p[(long)pos * step];
  acc += g.k[1] * (p[(long)mirror(pos - 1, n) * step] + p[(long)mirror(pos + 1, n) * step]);
  acc += g.k[2] * (p[(long)mirror(pos - 2, n) * step] + p[(long)mirror(pos + 2, n) * step]);
  out[i] = acc;
}

// (B,h,w) -> (B,oh,ow): order-1 resampling at (o + 0.5) in / out - 0.5 on both axes
__global__ __launch_bounds__(256) void brisque_resample_kernel(const double* __restrict__ in, double* __restrict__ out, long total,
                                                              int h, int w, int oh, int ow) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int oc = (int)(i % ow);
  const long r = i / ow;
  const int orow = (int)(r % oh);
  const long img = r / oh;
  const double cy = ((double)orow + 0.5) * ((double)h / (double)oh) - 0.5;
  const double cx = ((double)oc + 0.5) * ((double)w / (double)ow) - 0.5;
  const double fy = floor(cy), fx = floor(cx);
  const double ty = cy - fy, tx = cx - fx;
  int y0 = (int)fy, x0 = (int)fx;
  int y1 = y0 + 1, x1 = x0 + 1;
  y0 = mirror(y0, h);                                            // in / out is about 2: the taps stay inside; the fold and the
  x0 = mirror(x0, w);                                            // clamp below only keep a degenerate size in bounds
  y1 = mirror(y1, h);
  x1 = mirror(x1, w);
  y0 = min(max(y0, 0), h - 1);
  y1 = min(max(y1, 0), h - 1);
  x0 = min(max(x0, 0), w - 1);
  x1 = min(max(x1, 0), w - 1);
  const double* p = in + img * (long)h * w;
  const double a = (1.0 - tx) * p[(long)y0 * w + x0] + tx * p[(long)y0 * w + x1];
  const double b = (1.0 - tx) * p[(long)y1 * w + x0] + tx * p[(long)y1 * w + x1];
  out[i] = (1.0 - ty) * a + ty * b;
}

// One (image, tile) per workgroup; blockIdx.x = tile in row-major order, blockIdx.y = image.  RGB: the image is planar uint8
// (3,h,w) and the gray value is formed while staging; else it is an fp64 plane.
template <bool RGB>
__global__ __launch_bounds__(kThreads) void brisque_tile_kernel(const void* __restrict__ img, Window win, double* __restrict__ mscn_out,
                                                               double* __restrict__ moments, int h, int w, int ntx) {
  __shared__ double gy[kGW * kGW];                               // gray with its halo, zero outside the image
  __shared__ double ms[kMR * kMC];                               // MSCN: rows y0 .. y0 + T, columns x0 - 1 .. x0 + T
  __shared__ double gw[kWin * kWin];
  __shared__ double red[kThreads / 64][kMaps * kSums];
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int y0 = ty * kT, x0 = tx * kT;
  const long hw = (long)h * w;
  for (int i = threadIdx.x; i < kGW * kGW; i += kThreads) {
    const int r = i / kGW, c = i - r * kGW;
    const int y = y0 - kHalo + r, x = x0 - kHalo + c;
    double v = 0.0;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const long at = (long)y * w + x;
      if (RGB)
        v = gray_of(static_cast<const uint8_t*>(img) + (long)blockIdx.y * 3 * hw, hw, at);
      else
        v = static_cast<const double*>(img)[(long)blockIdx.y * hw + at];
    }
    gy[i] = v;
  }
  if (threadIdx.x < kWin * kWin) gw[threadIdx.x] = win.k[threadIdx.x];
  __syncthreads();
  for (int q = threadIdx.x; q < kMR * kMC; q += kThreads) {
    const int r = q / kMC, c = q - r * kMC;
    const int y = y0 + r, x = x0 - 1 + c;
    double m = 0.0;
    if (y < h && x >= 0 && x < w) {
      const double* t = gy + (r + kHalo - kR) * kGW + (c - 1 + kHalo - kR);      // top-left tap of this pixel's window
      double a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int dy = 0; dy < kWin; ++dy)
#pragma unroll
        for (int dx = 0; dx < kWin; ++dx) {
          const double v = t[dy * kGW + dx];
          const double g = gw[dy * kWin + dx];
          a1 += v * g;
          a2 += (v * v) * g;
        }
      const double v = t[kR * kGW + kR];
      const double dev = sqrt(fabs(a1 * a1 - a2));
      m = (v - a1) / (dev + 1.0 / 255.0);
      if (mscn_out && r < kT && c >= 1 && c <= kT) mscn_out[(long)blockIdx.y * hw + (long)y * w + x] = m;
    }
    ms[q] = m;
  }
  __syncthreads();
  double s[kMaps][4];                                            // sum of squares < 0, >= 0, sum |v|, sum v^2
  int n[kMaps][2];
#pragma unroll
  for (int a = 0; a < kMaps; ++a) {
    s[a][0] = s[a][1] = s[a][2] = s[a][3] = 0.0;
    n[a][0] = n[a][1] = 0;
  }
#pragma unroll 1
  for (int k = 0; k < kT * kT / kThreads; ++k) {
    const int q = threadIdx.x + k * kThreads;
    const int r = q / kT, c = q - r * kT;
    const int y = y0 + r, x = x0 + c;
    if (y >= h || x >= w) continue;
    const double* t = ms + r * kMC + c + 1;
    const double m = t[0];
    const bool below = y + 1 < h, right = x + 1 < w, left = x >= 1;
    const bool has[kMaps] = {true, right, below, below && right, below && left};
    const double v[kMaps] = {m, m * t[1], m * t[kMC], m * t[kMC + 1], m * t[kMC - 1]};
#pragma unroll
    for (int a = 0; a < kMaps; ++a) {
      if (!has[a]) continue;
      const double d2 = v[a] * v[a];
      if (v[a] < 0.0) {
        s[a][0] += d2;
        n[a][0] += 1;
      }
      if (v[a] >= 0.0) {                                         // zeros count on the right
        s[a][1] += d2;
        n[a][1] += 1;
      }
      s[a][2] += fabs(v[a]);
      s[a][3] += d2;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < kMaps; ++a) {
    const double o[kSums] = {wave_sum_f64((double)n[a][0]), wave_sum_f64(s[a][0]), wave_sum_f64((double)n[a][1]),
                             wave_sum_f64(s[a][1]),         wave_sum_f64(s[a][2]), wave_sum_f64(s[a][3])};
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kSums; ++j) red[wv][a * kSums + j] = o[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < kMaps * kSums) {
    double t = 0.0;
    for (int k = 0; k < kThreads / 64; ++k) t += red[k][threadIdx.x];
    moments[((long)blockIdx.y * gridDim.x + blockIdx.x) * (kMaps * kSums) + threadIdx.x] = t;
  }
}

__device__ __forceinline__ double phi(double a) {               // Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)), finite down to 0.05
  return exp(2.0 * lgamma(2.0 / a) - lgamma(1.0 / a) - lgamma(3.0 / a));
}

// One wave per (image, map): the tile slots are summed by lane and stride (lane l takes tiles l, l + 64, ... in that order),
// then by the xor tree; the root is bracketed by 64 points per round -- a bisection 65 ways -- until the bracket stops moving.
__global__ __launch_bounds__(64) void brisque_fit_kernel(const double* __restrict__ moments, int tiles, double* __restrict__ feat,
                                                        int feat_stride) {
  const int b = blockIdx.x / kMaps, map = blockIdx.x - b * kMaps;
  const int lane = threadIdx.x;
  const double* mo = moments + (long)b * tiles * (kMaps * kSums) + map * kSums;
  double s[kSums];
#pragma unroll
  for (int j = 0; j < kSums; ++j) s[j] = 0.0;
  for (int t = lane; t < tiles; t += 64) {
#pragma unroll
    for (int j = 0; j < kSums; ++j) s[j] += mo[(long)t * (kMaps * kSums) + j];
  }
#pragma unroll
  for (int j = 0; j < kSums; ++j) s[j] = wave_sum_f64(s[j]);
  const double sl = sqrt(s[1] / s[0]), sr = sqrt(s[3] / s[2]);
  const double gh = sl / sr;
  const double n = s[0] + s[2];
  const double mean_abs = s[4] / n;
  const double rhat = (mean_abs * mean_abs) / (s[5] / n);
  const double big_r = (rhat * (gh * gh * gh + 1.0) * (gh + 1.0)) / ((gh * gh + 1.0) * (gh * gh + 1.0));
  double lo = 0.05, hi = 100.0;
  const bool valid = big_r > phi(lo) && big_r < phi(hi);         // false for NaN: an empty side, or no variance
  double alpha = __builtin_nan("");
  if (valid) {
    for (int round = 0; round < 64; ++round) {
      const double p = lo + (hi - lo) * ((double)(lane + 1) / 65.0);
      const int below = __popcll(__ballot(phi(p) < big_r));       // phi increases: the lanes below the root come first
      const double plo = __shfl(p, below > 0 ? below - 1 : 0, 64), phi_ = __shfl(p, below < 64 ? below : 63, 64);
      const double nlo = below > 0 ? plo : lo, nhi = below < 64 ? phi_ : hi;
      if (nlo == lo && nhi == hi) break;
      lo = nlo;
      hi = nhi;
    }
    alpha = 0.5 * (lo + hi);
  }
  if (lane != 0) return;
  double* f = feat + (long)b * feat_stride;
  const double nan = __builtin_nan("");
  if (map == 0) {
    f[0] = alpha;
    f[1] = valid ? (sl * sl + sr * sr) / 2.0 : nan;
  } else {
    f += 2 + 4 * (map - 1);
    const double l1 = lgamma(1.0 / alpha), l2 = lgamma(2.0 / alpha), l3 = lgamma(3.0 / alpha);
    const double c = sqrt(exp(l1 - l3));
    f[0] = alpha;
    f[1] = valid ? (sr - sl) * c * exp(l2 - l1) : nan;
    f[2] = valid ? sl * sl : nan;
    f[3] = valid ? sr * sr : nan;
  }
}

// One workgroup per image: z in LDS, then the support vectors in chunks -- every thread one vector's term into LDS, thread 0
// adds the chunk's terms in file order.
__global__ __launch_bounds__(kThreads) void brisque_svr_kernel(const double* __restrict__ feat, const double* __restrict__ sv,
                                                              const double* __restrict__ coef, const double* __restrict__ fmin,
                                                              const double* __restrict__ fmax, const double* __restrict__ rho_gamma,
                                                              int n_sv, double* __restrict__ score) {
  __shared__ double z[2 * kFeat];
  __shared__ double term[kSvrChunk];
  const double* f = feat + (long)blockIdx.x * (2 * kFeat);
  if (threadIdx.x < 2 * kFeat) {
    const int j = threadIdx.x;
    z[j] = -1.0 + (2.0 * (f[j] - fmin[j])) / (fmax[j] - fmin[j]);
  }
  __syncthreads();
  const double gamma = rho_gamma[1];
  double acc = 0.0;
  for (int base = 0; base < n_sv; base += kSvrChunk) {
    const int cnt = min(kSvrChunk, n_sv - base);
    for (int i = threadIdx.x; i < cnt; i += kThreads) {
      const double* v = sv + (long)(base + i) * (2 * kFeat);
      double d2 = 0.0;
#pragma unroll 4
      for (int j = 0; j < 2 * kFeat; ++j) {
        const double d = v[j] - z[j];
        d2 += d * d;
      }
      term[i] = coef[base + i] * exp(-gamma * d2);
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < cnt; ++i) acc += term[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) score[blockIdx.x] = acc - rho_gamma[0];
}

struct Plan {
  int ty1, tx1, h2, w2, ty2, tx2;
  long tiles1, tiles2;
};

inline bool size_ok(int h, int w) { return h >= kMinSide && w >= kMinSide && (long)h * w <= kMaxPixels; }

inline Plan make_plan(int h, int w) {
  Plan p;
  p.ty1 = (h + kT - 1) / kT;
  p.tx1 = (w + kT - 1) / kT;
  p.h2 = half_size(h);
  p.w2 = half_size(w);
  p.ty2 = (p.h2 + kT - 1) / kT;
  p.tx2 = (p.w2 + kT - 1) / kT;
  p.tiles1 = (long)p.ty1 * p.tx1;
  p.tiles2 = (long)p.ty2 * p.tx2;
  return p;
}

// per image, in floats (every section a whole number of doubles): moments of both scales | gray | two filtered planes | half
inline long ws_floats_per_image(int h, int w) {
  const Plan p = make_plan(h, w);
  return 2 * ((p.tiles1 + p.tiles2) * kMaps * kSums + 3 * (long)h * w + (long)p.h2 * p.w2);
}

inline unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

int launch_gray(const uint8_t* rgb, double* y, int B, int h, int w, hipStream_t st) {
  const long hw = (long)h * w, total = (long)B * hw;
  hipLaunchKernelGGL(brisque_gray_kernel, dim3(blocks_of(total)), dim3(256), 0, st, rgb, y, hw, total);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int launch_half(const double* y, double* t1, double* t2, double* out, int B, int h, int w, hipStream_t st) {
  const Gauss5 g = make_gauss5();
  const int oh = half_size(h), ow = half_size(w);
  const long total = (long)B * h * w, total2 = (long)B * oh * ow;
  hipLaunchKernelGGL(brisque_gauss_kernel, dim3(blocks_of(total)), dim3(256), 0, st, y, t1, g, total, h, w, 1);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(brisque_gauss_kernel, dim3(blocks_of(total)), dim3(256), 0, st, (const double*)t1, t2, g, total, h, w, 0);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(brisque_resample_kernel, dim3(blocks_of(total2)), dim3(256), 0, st, (const double*)t2, out, total2, h, w, oh,
                     ow);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int launch_moments(const void* img, int img_f64, double* mscn, double* moments, int B, int h, int w, hipStream_t st) {
  const Window win = make_window();
  const int ntx = (w + kT - 1) / kT, nty = (h + kT - 1) / kT;
  const dim3 grid((unsigned)(ntx * nty), (unsigned)B);
  if (img_f64)
    hipLaunchKernelGGL(brisque_tile_kernel<false>, grid, dim3(kThreads), 0, st, img, win, mscn, moments, h, w, ntx);
  else
    hipLaunchKernelGGL(brisque_tile_kernel<true>, grid, dim3(kThreads), 0, st, img, win, mscn, moments, h, w, ntx);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int launch_fit(const double* moments, int tiles, double* feat, int feat_stride, int B, hipStream_t st) {
  hipLaunchKernelGGL(brisque_fit_kernel, dim3((unsigned)(B * kMaps)), dim3(64), 0, st, moments, tiles, feat, feat_stride);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_metric_brisque_plan(int h, int w, int* out, int n) {
  CIDNET_CHECK_ARG(out && n >= 9 && h > 0 && w > 0);
  if (!size_ok(h, w)) return CIDNET_ERR_SHAPE;
  const Plan p = make_plan(h, w);
  const int lds = (int)(sizeof(double) * (kGW * kGW + kMR * kMC + kWin * kWin + (kThreads / 64) * kMaps * kSums));
  const int v[9] = {kT, p.ty1, p.tx1, p.h2, p.w2, p.ty2, p.tx2, lds, (int)ws_floats_per_image(h, w)};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return CIDNET_OK;
}

long cidnet_metric_brisque_ws_floats(int B, int h, int w) {
  if (B <= 0 || B > 65535 || h <= 0 || w <= 0 || !size_ok(h, w)) return 0;
  return (long)B * ws_floats_per_image(h, w);
}

int cidnet_metric_brisque_gray(const uint8_t* rgb, double* y, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(rgb && y && aligned8(y) && B > 0 && h > 0 && w > 0);
  if (!size_ok(h, w) || B > 65535) return CIDNET_ERR_SHAPE;
  return launch_gray(rgb, y, B, h, w, (hipStream_t)stream);
}

int cidnet_metric_brisque_half(const double* y, double* tmp, double* out, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(y && tmp && out && aligned8(y) && aligned8(tmp) && aligned8(out) && B > 0 && h > 0 && w > 0);
  if (!size_ok(h, w) || B > 65535) return CIDNET_ERR_SHAPE;
  return launch_half(y, tmp, tmp + (long)B * h * w, out, B, h, w, (hipStream_t)stream);
}

int cidnet_metric_brisque_moments(const void* img, int img_f64, double* mscn, double* moments, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(img && moments && aligned8(moments) && aligned8(mscn) && (!img_f64 || aligned8(img)) && B > 0 && h > 0 && w > 0);
  if (h < kMinSide / 2 || w < kMinSide / 2 || (long)h * w > kMaxPixels || B > 65535) return CIDNET_ERR_SHAPE;
  return launch_moments(img, img_f64, mscn, moments, B, h, w, (hipStream_t)stream);
}

int cidnet_metric_brisque_fit(const double* moments, int tiles, double* feat, int feat_stride, int B, void* stream) {
  CIDNET_CHECK_ARG(moments && feat && aligned8(moments) && aligned8(feat) && tiles > 0 && B > 0);
  if (feat_stride < kFeat || (long)B * kMaps > 0x7fffffffL) return CIDNET_ERR_SHAPE;
  return launch_fit(moments, tiles, feat, feat_stride, B, (hipStream_t)stream);
}

int cidnet_metric_brisque_svr(const double* feat, const double* sv, const double* coef, const double* fmin, const double* fmax,
                              const double* rho_gamma, int n_sv, double* score, int B, void* stream) {
  CIDNET_CHECK_ARG(feat && sv && coef && fmin && fmax && rho_gamma && score && n_sv > 0 && B > 0);
  CIDNET_CHECK_ARG(aligned8(feat) && aligned8(sv) && aligned8(coef) && aligned8(fmin) && aligned8(fmax) && aligned8(rho_gamma) &&
                   aligned8(score));
  hipLaunchKernelGGL(brisque_svr_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, feat, sv, coef, fmin, fmax,
                     rho_gamma, n_sv, score);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_metric_brisque_features(const uint8_t* rgb, double* feat, float* ws, long ws_floats, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(rgb && feat && ws && aligned8(feat) && aligned8(ws) && B > 0 && h > 0 && w > 0);
  if (!size_ok(h, w) || B > 65535) return CIDNET_ERR_SHAPE;
  if (ws_floats < cidnet_metric_brisque_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  const Plan p = make_plan(h, w);
  const long hw = (long)h * w;
  double* mom1 = reinterpret_cast<double*>(ws);
  double* mom2 = mom1 + B * p.tiles1 * kMaps * kSums;
  double* gray = mom2 + B * p.tiles2 * kMaps * kSums;
  double* t1 = gray + B * hw;
  double* t2 = t1 + B * hw;
  double* half = t2 + B * hw;
  int rc = launch_moments(rgb, 0, nullptr, mom1, B, h, w, st);
  if (rc) return rc;
  if ((rc = launch_gray(rgb, gray, B, h, w, st))) return rc;
  if ((rc = launch_half(gray, t1, t2, half, B, h, w, st))) return rc;
  if ((rc = launch_moments(half, 1, nullptr, mom2, B, p.h2, p.w2, st))) return rc;
  if ((rc = launch_fit(mom1, (int)p.tiles1, feat, 2 * kFeat, B, st))) return rc;
  return launch_fit(mom2, (int)p.tiles2, feat + kFeat, 2 * kFeat, B, st);
}

}  // extern "C"
