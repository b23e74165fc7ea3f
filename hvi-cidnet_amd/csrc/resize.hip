// Pillow's 8-bit bicubic resize on the device: what measure.py:133-134 does to the enhanced image before it is scored against
// a ground truth of another size (im1.resize(im2.size): antialiased bicubic, fixed-point arithmetic).
//   Each pass is  out = clamp((2^21 + sum_k src[first + k] * coeff[k]) >> 22, 0, 255)  with an int32 accumulator, the taps
//   and their 22-bit coefficients per output position coming from the caller's tables (hvi-cidnet_amd/metrics.py: resize_plan,
//   a restatement of Pillow's coefficient routine).  The horizontal pass runs first and rounds to uint8, then the vertical
//   one: the order is part of the result.  A pass whose axis keeps its size is skipped, not run as an identity.
// Integer arithmetic only: every output byte depends on its own taps alone, bit-identical from call to call.
//
// Both kernels walk the output bytes in memory order, one lane per byte, so the stores of a wave are 64 consecutive bytes.
//   horizontal: a lane's taps are consecutive bytes of one source row and its own row of the coefficient table; neighbouring
//     lanes read overlapping spans of the same row, which the vector L1 serves after the first touch.
//   vertical: consecutive lanes are consecutive columns of one output row, so every tap is one coalesced read of a source row
//     and the coefficient is the same for the whole row.
// The tap count is a loop bound read from the table (an 83:1 reduction has 172 taps); nothing is kept in a per-lane array.
#include "common.h"
#include "cidnet_hip.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kBits = 22;                                      // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr long kMaxBytes = 1L << 31;

__device__ __forceinline__ uint8_t clip8(int acc) {
  const int v = acc >> kBits;                                  // arithmetic shift
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// taps of output position `o`: first source index and count, held inside [0, n_in] and the table's row whatever the table says
__device__ __forceinline__ void taps_of(const int* __restrict__ bounds, int o, int n_in, int ksize, int& first, int& count) {
  int f = bounds[2 * o], n = bounds[2 * o + 1];
  f = f < 0 ? 0 : (f > n_in ? n_in : f);
  const int room = n_in - f < ksize ? n_in - f : ksize;
  first = f;
  count = n < 0 ? 0 : (n > room ? room : n);
}

// src (rows, w_in) -> dst (rows, w_out), rows = B * 3 * h
__global__ __launch_bounds__(kThreads) void resize_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                                              int ksize, long total, int w_in, int w_out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int xx = (int)(i % w_out);
  const long row = i / w_out;
  int first, count;
  taps_of(bounds, xx, w_in, ksize, first, count);
  const uint8_t* s = src + row * w_in + first;
  const int* k = coeffs + (long)xx * ksize;
  int acc = 1 << (kBits - 1);
  for (int t = 0; t < count; ++t) acc += (int)s[t] * k[t];
  dst[i] = clip8(acc);
}

// src (planes, h_in, w) -> dst (planes, h_out, w), planes = B * 3
__global__ __launch_bounds__(kThreads) void resize_cols_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                                              int ksize, long total, int h_in, int h_out, int w) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const long r = i / w;
  const int yy = (int)(r % h_out);
  const long plane = r / h_out;
  int first, count;
  taps_of(bounds, yy, h_in, ksize, first, count);
  const uint8_t* s = src + (plane * h_in + first) * (long)w + x;
  const int* k = coeffs + (long)yy * ksize;
  int acc = 1 << (kBits - 1);
  for (int t = 0; t < count; ++t) acc += (int)s[(long)t * w] * k[t];
  dst[i] = clip8(acc);
}

inline unsigned blocks_for(long total) { return (unsigned)((total + kThreads - 1) / kThreads); }

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

long cidnet_metric_resize_ws_bytes(int B, int h_in, int w_in, int h_out, int w_out) {
  if (B <= 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0) return 0;
  return (h_in != h_out && w_in != w_out) ? (long)B * 3 * h_in * w_out : 0;
}

int cidnet_metric_resize_u8(const uint8_t* src, uint8_t* dst, uint8_t* tmp, const int* bounds_x, const int* coeffs_x, int ksize_x,
                            const int* bounds_y, const int* coeffs_y, int ksize_y, int B, int h_in, int w_in, int h_out,
                            int w_out, void* stream) {
  CIDNET_CHECK_ARG(src && dst && B > 0 && h_in > 0 && w_in > 0 && h_out > 0 && w_out > 0);
  const bool horiz = w_in != w_out, vert = h_in != h_out;
  CIDNET_CHECK_ARG(!horiz || (bounds_x && coeffs_x && ksize_x > 0));
  CIDNET_CHECK_ARG(!vert || (bounds_y && coeffs_y && ksize_y > 0));
  CIDNET_CHECK_ARG(!(horiz && vert) || tmp);
  const long n_in = (long)B * 3 * h_in * w_in, n_out = (long)B * 3 * h_out * w_out, n_tmp = (long)B * 3 * h_in * w_out;
  if (n_in >= kMaxBytes || n_out >= kMaxBytes || (horiz && vert && n_tmp >= kMaxBytes)) return CIDNET_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (!horiz && !vert) {
    if (src != dst) {
      hipError_t e = hipMemcpyAsync(dst, src, (size_t)n_in, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return (int)e;
    }
    return CIDNET_OK;
  }
  const uint8_t* rows = src;                                   // what the vertical pass reads
  if (horiz) {
    uint8_t* out = vert ? tmp : dst;
    hipLaunchKernelGGL(resize_rows_kernel, dim3(blocks_for(n_tmp)), dim3(kThreads), 0, st, src, out, bounds_x, coeffs_x, ksize_x,
                       n_tmp, w_in, w_out);
    CIDNET_LAUNCH_STATUS();
    rows = out;
  }
  if (vert) {
    hipLaunchKernelGGL(resize_cols_kernel, dim3(blocks_for(n_out)), dim3(kThreads), 0, st, rows, dst, bounds_y, coeffs_y, ksize_y,
                       n_out, h_in, h_out, w_out);
    CIDNET_LAUNCH_STATUS();
  }
  return CIDNET_OK;
}

}  // extern "C"
