// NIQE features on the device: what the reference's measure_niqe_bris.py -> loss/niqe_utils.py (calculate_niqe with its
// defaults) computes per image, up to the (blocks, 36) feature matrix; the 36 x 36 tail runs on the host (metrics.py).
//   luma      Y = rint(fp32(fp32((24.966 R' + 128.553 G' + 65.481 B' + 16) / 255) * 255.0f)), R' = fp32(R) / 255.0f, the dot
//             product in fp64: the reference hands its RGB array to a BGR routine, and that effective rule is the contract
//             (niqe_utils.py: to_y_channel -> bgr2ycbcr, then .round());  cropped to (h / 96 * 96, w / 96 * 96), top-left;
//   MSCN      mu = fp32(G * x), s2 = fp32(G * fp32(x x)), sigma = sqrtf(|s2 - mu mu|), (x - mu) / (sigma + 1) in fp32; G the
//             7 x 7 window (fp64, from the parameter file), taps accumulated in fp64 in row-major order, border replicated
//             (niqe_utils.py: niqe(), scipy.ndimage.convolve on fp32 arrays);
//   half size x / 255.0f, 8 taps [-3 -9 29 111 111 29 -9 -3] / 256 on inputs 2k-3 .. 2k+4, symmetric reflection, output rows
//             first, then columns, fp64 accumulation and one fp32 rounding per pass, then * 255.0f (imresize(img / 255, 0.5));
//   moments   per 96 x 96 block (48 x 48 at the second scale) and per map -- the block, and the block times itself rolled
//             inside the block by (0,1), (1,0), (1,1), (1,-1), the product rounded to fp32 -- six sums: count and sum of
//             squares of the negatives, the same of the positives, sum |v|, sum v^2 (fp64);
//   fit       gammahat, rhatnorm, first minimum of (r_gam - rhatnorm)^2 over the 9801-entry table, beta_l, beta_r, mean
//             (estimate_aggd_param, compute_feature); a NaN rhatnorm selects entry 0 as numpy's argmin does.
// This file is compiled with -ffp-contract=off (build.py): every rounding above is explicit, none is fused away.
// Reductions have a fixed order (strided per-thread sums, xor-shuffle tree, waves in order): results are bit-identical
// from call to call and an image's values do not depend on the rest of the batch.  No atomics, vector stores only.
//
// Block kernel: one workgroup per (image, block).  The block plus its 3-pixel halo is staged in LDS in its storage type
// (102 x 102 uint8 for the Y plane, fp32 for the half-size image), the MSCN block is formed beside it in LDS (96 x 96 fp32 =
// 36 KiB) and the five maps' sums read it there with the in-block wrap.  The map goes to HBM only when the caller passes a
// buffer.
#include "common.h"
#include "cidnet_hip.h"

namespace cidnet {
namespace {

constexpr int kR = 3, kWin = 7;
constexpr int kThreads = 256;
constexpr int kGrid = 9801;                                     // alpha = 0.2, 0.201, ..., 10.0
constexpr int kMaps = 5, kSums = 6;

__global__ __launch_bounds__(256) void niqe_luma_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ y, long total,
                                                       int h, int w, int hc, int wc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % wc);
  const long r = i / wc;
  const int row = (int)(r % hc);
  const long img = r / hc;
  const long hw = (long)h * w;
  const uint8_t* p = rgb + img * 3 * hw + (long)row * w + c;
  const float rf = (float)p[0] / 255.0f, gf = (float)p[hw] / 255.0f, bf = (float)p[2 * hw] / 255.0f;
  double v = (double)rf * 24.966 + (double)gf * 128.553;
  v = v + (double)bf * 65.481;
  v = v + 16.0;
  const float f = (float)(v / 255.0) * 255.0f;
  y[i] = (uint8_t)(int)rintf(f);                                 // half to even; 16 <= f <= 235
}

template <typename T>
__device__ __forceinline__ float load_px(const T* p, long i) { return (float)p[i]; }

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i); }

struct Taps {
  double t[8];
};
inline Taps make_taps() {
  const int k[8] = {-3, -9, 29, 111, 111, 29, -9, -3};
  Taps t;
  for (int i = 0; i < 8; ++i) t.t[i] = (double)k[i] / 256.0;
  return t;
}

// (B,h,w) -> (B,h/2,w): output row i from input rows 2i-3 .. 2i+4 of x / 255
template <typename T>
__global__ __launch_bounds__(256) void niqe_half_rows_kernel(const T* __restrict__ in, float* __restrict__ out, Taps tp, long total,
                                                            int h, int w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % w);
  const long r = i / w;
  const int row = (int)(r % (h / 2));
  const long img = r / (h / 2);
  const T* p = in + img * (long)h * w + c;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = load_px(p, (long)reflect(2 * row - 3 + k, h) * w) / 255.0f;
    acc += (double)v * tp.t[k];
  }
  out[i] = (float)acc;
}

// (B,h2,w) -> (B,h2,w/2), * 255
__global__ __launch_bounds__(256) void niqe_half_cols_kernel(const float* __restrict__ in, float* __restrict__ out, Taps tp,
                                                            long total, int w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (w / 2));
  const long r = i / (w / 2);
  const float* p = in + r * (long)w;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc += (double)p[reflect(2 * c - 3 + k, w)] * tp.t[k];
  out[i] = (float)acc * 255.0f;
}

// One (image, block) per workgroup; blockIdx.x = block in column-major order (bw * nh + bh), blockIdx.y = image.
template <typename T, int BS>
__global__ __launch_bounds__(kThreads) void niqe_block_kernel(const T* __restrict__ img, const double* __restrict__ window,
                                                             float* __restrict__ mscn_out, double* __restrict__ moments, int h,
                                                             int w) {
  constexpr int LW = BS + 2 * kR;
  constexpr int NPT = BS * BS / kThreads;                        // 36 or 9 pixels per thread
  static_assert(BS * BS % kThreads == 0, "block size");
  __shared__ T tile[LW * LW];                                    // the input with its halo (uint8 or fp32)
  __shared__ float ms[BS * BS];                                  // the MSCN block
  __shared__ double gw[kWin * kWin];
  __shared__ double red[kThreads / 64][kMaps * kSums];
  const int nh = h / BS;
  const int bw = blockIdx.x / nh, bh = blockIdx.x - bw * nh;
  const int y0 = bh * BS, x0 = bw * BS;
  const T* p = img + (long)blockIdx.y * h * w;
  for (int i = threadIdx.x; i < LW * LW; i += kThreads) {
    const int r = i / LW, c = i - r * LW;
    int y = y0 - kR + r, x = x0 - kR + c;
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);                     // border: nearest
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    tile[i] = p[(long)y * w + x];
  }
  if (threadIdx.x < kWin * kWin) gw[threadIdx.x] = window[threadIdx.x];
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < NPT; ++k) {
    const int q = threadIdx.x + k * kThreads;
    const int r = q / BS, c = q - r * BS;
    const T* t = tile + r * LW + c;
    double a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int dy = 0; dy < kWin; ++dy)
#pragma unroll
      for (int dx = 0; dx < kWin; ++dx) {
        const float v = (float)t[dy * LW + dx];
        const float v2 = v * v;
        const double g = gw[dy * kWin + dx];
        a1 += (double)v * g;
        a2 += (double)v2 * g;
      }
    const float mu = (float)a1, s2 = (float)a2;
    const float x = (float)t[kR * LW + kR];
    const float sigma = sqrtf(fabsf(s2 - mu * mu));
    const float m = (x - mu) / (sigma + 1.0f);
    ms[q] = m;
    if (mscn_out) mscn_out[((long)blockIdx.y * h + y0 + r) * w + x0 + c] = m;
  }
  __syncthreads();
  double s[kMaps][4];                                            // sum of squares < 0, > 0, sum |v|, sum v^2
  int n[kMaps][2];
#pragma unroll
  for (int a = 0; a < kMaps; ++a) {
    s[a][0] = s[a][1] = s[a][2] = s[a][3] = 0.0;
    n[a][0] = n[a][1] = 0;
  }
#pragma unroll 1
  for (int k = 0; k < NPT; ++k) {
    const int q = threadIdx.x + k * kThreads;
    const int r = q / BS, c = q - r * BS;
    const int ru = r == 0 ? BS - 1 : r - 1;                       // np.roll wraps inside the block
    const int cl = c == 0 ? BS - 1 : c - 1, cr = c == BS - 1 ? 0 : c + 1;
    const float x = ms[q];
    const float v[kMaps] = {x, x * ms[r * BS + cl], x * ms[ru * BS + c], x * ms[ru * BS + cl], x * ms[ru * BS + cr]};
#pragma unroll
    for (int a = 0; a < kMaps; ++a) {
      const double d = (double)v[a];
      const double d2 = d * d;
      if (v[a] < 0.f) {
        s[a][0] += d2;
        n[a][0] += 1;
      }
      if (v[a] > 0.f) {
        s[a][1] += d2;
        n[a][1] += 1;
      }
      s[a][2] += fabs(d);
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

// One wave per fit (workgroup = one block's five fits would idle four waves on the scan; one wave each keeps it simple).
// tables: r_gam[kGrid] | sqrt(gamma(1/a) / gamma(3/a))[kGrid] | gamma(2/a) / gamma(1/a)[kGrid] | a[kGrid]
__global__ __launch_bounds__(64) void niqe_fit_kernel(const double* __restrict__ moments, const double* __restrict__ tables,
                                                     double n_px, double* __restrict__ feat, int feat_stride) {
  const long blk = blockIdx.x / kMaps;
  const int map = blockIdx.x - (int)(blk * kMaps);
  const double* mo = moments + (long)blockIdx.x * kSums;
  const double left = sqrt(mo[1] / mo[0]), right = sqrt(mo[3] / mo[2]);
  const double gh = left / right;
  const double mean_abs = mo[4] / n_px;
  const double rhat = mean_abs * mean_abs / (mo[5] / n_px);
  const double rhn = (rhat * (gh * gh * gh + 1.0) * (gh + 1.0)) / ((gh * gh + 1.0) * (gh * gh + 1.0));
  double best = __builtin_inf();
  int idx = kGrid;
  for (int k = threadIdx.x; k < kGrid; k += 64) {
    const double d = tables[k] - rhn;
    const double d2 = d * d;
    if (d2 < best) {                                             // strict: the first minimum of this lane's entries
      best = d2;
      idx = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ob < best || (ob == best && oi < idx)) {
      best = ob;
      idx = oi;
    }
  }
  if (threadIdx.x != 0) return;
  if (idx >= kGrid) idx = 0;                                     // NaN (or infinite) distances everywhere: numpy's argmin gives 0
  const double alpha = tables[3 * kGrid + idx];
  const double bl = left * tables[kGrid + idx], br = right * tables[kGrid + idx];
  double* f = feat + blk * feat_stride;
  if (map == 0) {
    f[0] = alpha;
    f[1] = (bl + br) / 2.0;
  } else {
    f += 2 + 4 * (map - 1);
    f[0] = alpha;
    f[1] = (br - bl) * tables[2 * kGrid + idx];
    f[2] = bl;
    f[3] = br;
  }
}

inline long align2(long floats) { return (floats + 1) & ~1L; }

int launch_luma(const uint8_t* rgb, uint8_t* y, int B, int h, int w, int hc, int wc, hipStream_t st) {
  const long total = (long)B * hc * wc;
  hipLaunchKernelGGL(niqe_luma_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, rgb, y, total, h, w, hc, wc);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int launch_half(const void* img, int img_f32, float* rows, float* out, int B, int h, int w, hipStream_t st) {
  const Taps tp = make_taps();
  const long t1 = (long)B * (h / 2) * w, t2 = (long)B * (h / 2) * (w / 2);
  if (img_f32)
    hipLaunchKernelGGL(niqe_half_rows_kernel<float>, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, (const float*)img, rows, tp,
                       t1, h, w);
  else
    hipLaunchKernelGGL(niqe_half_rows_kernel<uint8_t>, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, (const uint8_t*)img,
                       rows, tp, t1, h, w);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(niqe_half_cols_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, st, rows, out, tp, t2, w);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int launch_moments(const void* img, int img_f32, const double* window, int block, float* mscn, double* moments, int B, int h,
                   int w, hipStream_t st) {
  const dim3 grid((unsigned)((h / block) * (w / block)), (unsigned)B);
  if (block == 96 && !img_f32)
    hipLaunchKernelGGL((niqe_block_kernel<uint8_t, 96>), grid, dim3(kThreads), 0, st, (const uint8_t*)img, window, mscn, moments, h, w);
  else if (block == 96)
    hipLaunchKernelGGL((niqe_block_kernel<float, 96>), grid, dim3(kThreads), 0, st, (const float*)img, window, mscn, moments, h, w);
  else if (!img_f32)
    hipLaunchKernelGGL((niqe_block_kernel<uint8_t, 48>), grid, dim3(kThreads), 0, st, (const uint8_t*)img, window, mscn, moments, h, w);
  else
    hipLaunchKernelGGL((niqe_block_kernel<float, 48>), grid, dim3(kThreads), 0, st, (const float*)img, window, mscn, moments, h, w);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int launch_fit(const double* moments, const double* tables, int block, double* feat, int feat_stride, long n_blocks,
               hipStream_t st) {
  hipLaunchKernelGGL(niqe_fit_kernel, dim3((unsigned)(n_blocks * kMaps)), dim3(64), 0, st, moments, tables,
                     (double)block * (double)block, feat, feat_stride);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_metric_niqe_luma(const uint8_t* rgb, uint8_t* y, int B, int h, int w, int hc, int wc, void* stream) {
  CIDNET_CHECK_ARG(rgb && y && B > 0 && h > 0 && w > 0 && hc > 0 && wc > 0);
  if (hc > h || wc > w) return CIDNET_ERR_SHAPE;
  return launch_luma(rgb, y, B, h, w, hc, wc, (hipStream_t)stream);
}

int cidnet_metric_niqe_half(const void* img, int img_f32, float* rows, float* out, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(img && rows && out && B > 0 && h > 0 && w > 0);
  if (h % 2 || w % 2 || h < 4 || w < 4) return CIDNET_ERR_SHAPE;  // the reflection reaches 3 samples inward
  return launch_half(img, img_f32, rows, out, B, h, w, (hipStream_t)stream);
}

int cidnet_metric_niqe_moments(const void* img, int img_f32, const double* window, int block, float* mscn, double* moments,
                               int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(img && window && moments && B > 0 && h > 0 && w > 0);
  if ((block != 96 && block != 48) || h % block || w % block) return CIDNET_ERR_SHAPE;
  return launch_moments(img, img_f32, window, block, mscn, moments, B, h, w, (hipStream_t)stream);
}

int cidnet_metric_niqe_fit(const double* moments, const double* tables, int block, double* feat, int feat_stride,
                           long n_blocks, void* stream) {
  CIDNET_CHECK_ARG(moments && tables && feat && n_blocks > 0 && block > 0);
  if (feat_stride < 18 || n_blocks * kMaps > 0x7fffffffL) return CIDNET_ERR_SHAPE;
  return launch_fit(moments, tables, block, feat, feat_stride, n_blocks, (hipStream_t)stream);
}

// layout (floats): moments [2][B][blocks][5][6] fp64 | half-size rows [B][hc/2][wc] | half-size image [B][hc/2][wc/2] |
// Y [B][hc][wc] uint8
long cidnet_metric_niqe_ws_floats(int B, int h, int w) {
  if (B <= 0 || h < 96 || w < 96) return 0;
  const long hc = h / 96 * 96, wc = w / 96 * 96;
  const long nblk = (hc / 96) * (wc / 96);
  return 2 * (2 * B * nblk * kMaps * kSums) + align2(B * (hc / 2) * wc) + align2(B * (hc / 2) * (wc / 2)) +
         align2((B * hc * wc + 3) / 4);
}

int cidnet_metric_niqe_features(const uint8_t* rgb, const double* window, const double* tables, double* feat, float* ws,
                                long ws_floats, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(rgb && window && tables && feat && ws && B > 0);
  if (h < 96 || w < 96) return CIDNET_ERR_SHAPE;
  if (ws_floats < cidnet_metric_niqe_ws_floats(B, h, w)) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  const int hc = h / 96 * 96, wc = w / 96 * 96;
  const long nblk = (long)(hc / 96) * (wc / 96);
  double* mom1 = reinterpret_cast<double*>(ws);
  double* mom2 = mom1 + B * nblk * kMaps * kSums;
  float* rows = reinterpret_cast<float*>(mom2 + B * nblk * kMaps * kSums);
  float* half = rows + align2((long)B * (hc / 2) * wc);
  uint8_t* y = reinterpret_cast<uint8_t*>(half + align2((long)B * (hc / 2) * (wc / 2)));
  int rc = launch_luma(rgb, y, B, h, w, hc, wc, st);
  if (rc) return rc;
  if ((rc = launch_moments(y, 0, window, 96, nullptr, mom1, B, hc, wc, st))) return rc;
  if ((rc = launch_half(y, 0, rows, half, B, hc, wc, st))) return rc;
  if ((rc = launch_moments(half, 1, window, 48, nullptr, mom2, B, hc / 2, wc / 2, st))) return rc;
  if ((rc = launch_fit(mom1, tables, 96, feat, 36, B * nblk, st))) return rc;
  return launch_fit(mom2, tables, 48, feat + 18, 36, B * nblk, st);
}

}  // extern "C"
