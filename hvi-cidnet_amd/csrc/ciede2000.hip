// CIEDE2000 colour difference of image pairs (include/cidnet_hip.h: cidnet_metric_ciede2000_*): the mean over an image's pixels
// of dE00(Lab(restored), Lab(gt)), restored as colour 1 and the ground truth as colour 2.  All arithmetic is fp64; the file is
// built with -ffp-contract=off, so the two inlined sRGB -> Lab conversions of a pixel round alike and two identical pixels give
// exactly 0.0.
//
// sRGB -> Lab (scikit-image's constants): v = level / 255; lin = v > 0.04045 ? ((v + 0.055) / 1.055)^2.4 : v / 12.92;
// X = (m00 R + m01 G) + m02 B (that order) with M = [[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169],
// [0.019334, 0.119193, 0.950227]]; divided by the D65 / 2 degree white (0.95047, 1.0, 1.08883); f(t) = t > 0.008856 ? cbrt(t) :
// 7.787 t + 16 / 116; L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z)).  The linear value of an 8-bit level is
// read from a 256-entry table the host built with the formula above (staged in LDS): no device pow runs for a level.  Only the
// GT-mean variant's restored side, the real number clip(q s, 0, 255) / 255, goes through the fp64 pow.
//
// dE00: Sharma, Wu and Dalal (2005) with kL = kC = kH = 1, the cases of h', dh' and the mean hue exactly as the header lists them.
//
// Reduction (no atomics): block x of image b takes pixels 1024 x .. 1024 x + 1023 of the flattened h w plane, thread t the four
// pixels 1024 x + 4 t + 0..3 (4-byte loads of the planes; a group that reaches past the image is read byte by byte, lane by
// lane).  A thread adds its values in pixel order onto 0.0, block_tree() sums the 256 threads, and the result goes to slot
// ws[b * blocks + x].  The finish kernel, one block per image: thread t adds slots t, t + 256, ... in that order onto 0.0, the
// same block_tree() sums the threads, and the total is divided by h w.  block_tree(): inside each wave of 64 the butterfly
// v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; then ((wave 0 + wave 1) + wave 2) + wave 3.  The pixel -> block map depends on
// (h, w) only, so a call repeats bit for bit and an image's value does not depend on its batch.
#include <math.h>

#include "cidnet_hip.h"
#include "common.h"
#include "gt_mean.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kPerBlock = kThreads * kPerThread;       // pixels of one image per block
constexpr int kLds = 256 * 8 + (kThreads / 64) * 8;    // the level table and the waves' sums
constexpr double kDeg = 57.29577951308232;             // 180 / pi
constexpr double kRad = 0.017453292519943295;          // pi / 180
constexpr double k25p7 = 6103515625.0;                 // 25^7

struct __attribute__((packed, aligned(1))) u8x4 {
  uint32_t v;
};

struct Lab {
  double L, a, b;
};

__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }

__device__ __forceinline__ Lab lab_of_linear(double r, double g, double b) {
  const double x = ((0.412453 * r + 0.357580 * g) + 0.180423 * b) / 0.95047;
  const double y = (0.212671 * r + 0.715160 * g) + 0.072169 * b;                  // white Y = 1.0
  const double z = ((0.019334 * r + 0.119193 * g) + 0.950227 * b) / 1.08883;
  const double fx = lab_f(x), fy = lab_f(y), fz = lab_f(z);
  return Lab{116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)};
}

// v in [0, 1], any real number: the GT-mean variant's restored side
__device__ __forceinline__ double linear_of(double v) { return v > 0.04045 ? pow((v + 0.055) / 1.055, 2.4) : v / 12.92; }

__device__ __forceinline__ double pow7(double c) {
  const double c2 = c * c, c4 = c2 * c2;
  return c4 * c2 * c;
}

__device__ __forceinline__ double hue_deg(double b, double ap) {
  const double h = atan2(b, ap) * kDeg;                                           // atan2(0, 0) = 0
  return h < 0.0 ? h + 360.0 : h;
}

__device__ __forceinline__ double cos_deg(double d) { return cos(d * kRad); }

// colour 1 = p, colour 2 = q
__device__ __forceinline__ double delta_e00(const Lab p, const Lab q) {
  const double C1 = hypot(p.a, p.b), C2 = hypot(q.a, q.b);
  const double cb7 = pow7((C1 + C2) / 2.0);
  const double G = 0.5 * (1.0 - sqrt(cb7 / (cb7 + k25p7)));
  const double a1 = (1.0 + G) * p.a, a2 = (1.0 + G) * q.a;
  const double Cp1 = hypot(a1, p.b), Cp2 = hypot(a2, q.b);
  const double h1 = hue_deg(p.b, a1), h2 = hue_deg(q.b, a2);
  const bool grey = Cp1 * Cp2 == 0.0;
  const double dL = q.L - p.L, dC = Cp2 - Cp1;
  double dh = h2 - h1;
  dh = dh > 180.0 ? dh - 360.0 : (dh < -180.0 ? dh + 360.0 : dh);
  dh = grey ? 0.0 : dh;
  const double dH = 2.0 * sqrt(Cp1 * Cp2) * sin(dh / 2.0 * kRad);
  const double Lb = (p.L + q.L) / 2.0, Cb = (Cp1 + Cp2) / 2.0;
  const double hs = h1 + h2;
  const double hb = grey ? hs : (fabs(h1 - h2) <= 180.0 ? hs / 2.0 : (hs < 360.0 ? (hs + 360.0) / 2.0 : (hs - 360.0) / 2.0));
  const double T = 1.0 - 0.17 * cos_deg(hb - 30.0) + 0.24 * cos_deg(2.0 * hb) + 0.32 * cos_deg(3.0 * hb + 6.0) -
                   0.20 * cos_deg(4.0 * hb - 63.0);
  const double u = (hb - 275.0) / 25.0;
  const double dtheta = 30.0 * exp(-(u * u));
  const double cp7 = pow7(Cb);
  const double RC = 2.0 * sqrt(cp7 / (cp7 + k25p7));
  const double l50 = (Lb - 50.0) * (Lb - 50.0);
  const double SL = 1.0 + 0.015 * l50 / sqrt(20.0 + l50);
  const double SC = 1.0 + 0.045 * Cb;
  const double SH = 1.0 + 0.015 * Cb * T;
  const double RT = -sin(2.0 * dtheta * kRad) * RC;
  const double x = dL / SL, y = dC / SC, z = dH / SH;
  return sqrt(x * x + y * y + z * z + RT * y * z);
}

// the fixed tree of the header comment; the total is valid in thread 0.  red: one double per wave.
__device__ __forceinline__ double block_tree(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    t = red[0];
    for (int i = 1; i < kThreads / 64; ++i) t += red[i];
  }
  return t;
}

// grid (blocks per image, B).  n = h w < 2^31.  SCALED: the restored side is clip(q scale[b], 0, 255) / 255.
template <bool SCALED>
__global__ __launch_bounds__(kThreads) void ciede_u8_kernel(const uint8_t* __restrict__ restored, const uint8_t* __restrict__ gt,
                                                            const double* __restrict__ scale, const double* __restrict__ lin_table,
                                                            double* __restrict__ map, double* __restrict__ partial, long n) {
  __shared__ double lin[256];
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x;
  lin[tid] = lin_table[tid];
  __syncthreads();
  const long img = blockIdx.y;
  const uint8_t* rp = restored + img * 3 * n;
  const uint8_t* gp = gt + img * 3 * n;
  const long p0 = (long)blockIdx.x * kPerBlock + (long)kPerThread * tid;
  uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};                                       // R, G, B of restored, then of gt: 4 pixels each
  int cnt = 0;
  if (p0 + kPerThread <= n) {
    cnt = kPerThread;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      w[c] = reinterpret_cast<const u8x4*>(rp + c * n + p0)->v;
      w[3 + c] = reinterpret_cast<const u8x4*>(gp + c * n + p0)->v;
    }
  } else if (p0 < n) {                                                            // the image's last group: p0 + k < n per byte
    cnt = (int)(n - p0);
    for (int k = 0; k < cnt; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        w[c] |= (uint32_t)rp[c * n + p0 + k] << (8 * k);
        w[3 + c] |= (uint32_t)gp[c * n + p0 + k] << (8 * k);
      }
    }
  }
  const double s = SCALED ? scale[img] : 1.0;
  double acc = 0.0;
#pragma unroll 1
  for (int k = 0; k < cnt; ++k) {
    const int sh = 8 * k;
    const Lab q = lab_of_linear(lin[(w[3] >> sh) & 255u], lin[(w[4] >> sh) & 255u], lin[(w[5] >> sh) & 255u]);
    Lab p;
    if (SCALED) {
      double v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = linear_of(gt_mean_value((w[c] >> sh) & 255u, s) / 255.0);
      p = lab_of_linear(v[0], v[1], v[2]);
    } else {
      p = lab_of_linear(lin[(w[0] >> sh) & 255u], lin[(w[1] >> sh) & 255u], lin[(w[2] >> sh) & 255u]);
    }
    const double d = delta_e00(p, q);
    if (map) map[img * n + p0 + k] = d;
    acc += d;
  }
  if (!partial) return;                                                           // uniform: the map alone was asked for
  const double t = block_tree(acc, red);
  if (tid == 0) partial[img * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void ciede_finish_kernel(const double* __restrict__ partial, int blocks, double n,
                                                                double* __restrict__ mean) {
  __shared__ double red[kThreads / 64];
  const double* slot = partial + (long)blockIdx.x * blocks;
  double acc = 0.0;
  for (int i = threadIdx.x; i < blocks; i += kThreads) acc += slot[i];
  const double t = block_tree(acc, red);
  if (threadIdx.x == 0) mean[blockIdx.x] = t / n;
}

__global__ __launch_bounds__(kThreads) void ciede_lab_kernel(const double* __restrict__ lab1, const double* __restrict__ lab2,
                                                             double* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  out[i] = delta_e00(Lab{lab1[3 * i], lab1[3 * i + 1], lab1[3 * i + 2]}, Lab{lab2[3 * i], lab2[3 * i + 1], lab2[3 * i + 2]});
}

// The one place the block split is decided: the launcher, the workspace query and cidnet_metric_ciede2000_plan call it.
int ciede_plan(int h, int w, long* blocks) {
  if (h < 1 || w < 1) return CIDNET_ERR_ARG;
  const long n = (long)h * w;
  if (n > 2147483647L) return CIDNET_ERR_SHAPE;
  *blocks = (n + kPerBlock - 1) / kPerBlock;
  return CIDNET_OK;
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

long cidnet_metric_ciede2000_ws_bytes(int B, int h, int w) {
  long blocks;
  if (B < 1 || ciede_plan(h, w, &blocks) != CIDNET_OK) return 0;
  return (long)B * blocks * 8;
}

int cidnet_metric_ciede2000_plan(int h, int w, int* out, int n) {
  if (!out || n < 3) return CIDNET_ERR_ARG;
  long blocks;
  const int rc = ciede_plan(h, w, &blocks);
  if (rc != CIDNET_OK) return rc;
  out[0] = (int)blocks; out[1] = kPerBlock; out[2] = kLds;
  return CIDNET_OK;
}

int cidnet_metric_ciede2000_u8(const uint8_t* restored, const uint8_t* gt, const double* scale, const double* lin_table, double* map,
                               double* mean, void* ws, long ws_bytes, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(restored && gt && lin_table && (map || mean) && B >= 1);
  CIDNET_CHECK_ARG(aligned8(scale) && aligned8(lin_table) && aligned8(map) && aligned8(mean) && aligned8(ws));
  long blocks;
  const int rc = ciede_plan(h, w, &blocks);
  if (rc != CIDNET_OK) return rc;
  if (B > 65535) return CIDNET_ERR_SHAPE;
  if (mean) {
    CIDNET_CHECK_ARG(ws);
    if (ws_bytes < (long)B * blocks * 8) return CIDNET_ERR_WS;
  }
  const long n = (long)h * w;
  double* partial = mean ? reinterpret_cast<double*>(ws) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks, (unsigned)B);
  if (scale)
    hipLaunchKernelGGL(ciede_u8_kernel<true>, grid, dim3(kThreads), 0, st, restored, gt, scale, lin_table, map, partial, n);
  else
    hipLaunchKernelGGL(ciede_u8_kernel<false>, grid, dim3(kThreads), 0, st, restored, gt, scale, lin_table, map, partial, n);
  CIDNET_LAUNCH_STATUS();
  if (mean) {
    hipLaunchKernelGGL(ciede_finish_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, partial, (int)blocks, (double)n, mean);
    CIDNET_LAUNCH_STATUS();
  }
  return CIDNET_OK;
}

int cidnet_metric_ciede2000_lab(const double* lab1, const double* lab2, double* out, long n, void* stream) {
  CIDNET_CHECK_ARG(lab1 && lab2 && out && n >= 1 && aligned8(lab1) && aligned8(lab2) && aligned8(out));
  const long blocks = (n + kThreads - 1) / kThreads;
  if (blocks > 2147483647L) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(ciede_lab_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, lab1, lab2, out, n);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
