// Elementwise passes over slices of the trainer's flat fp32 buffers (include/cidnet_hip.h: cidnet_grad_accumulate,
// cidnet_ema_update, cidnet_swap): the gradient sum of an accumulated update, the exponential moving average of the
// weights behind the Adam kernel, and the exchange that puts the averaged weights under the model's Parameters and back.
//
// The buffers are slices of one arena (bucket starts; n_live is no multiple of 4), so only 4-byte alignment is promised and
// any n >= 1 must work: block 0 handles a scalar head of 0..3 elements (up to the first 16-byte boundary of the buffer that
// is written, `dst` / `ema` / `a`) and a scalar tail of 0..3; the grid-stride body moves 16 bytes per lane and buffer.
// Nothing outside [0, n) is read or written.  No atomics; every element is owned by exactly one lane.
// Every fp32 operation is rounded on its own (__fadd_rn / __fsub_rn / __fmul_rn are never contracted into an fma, and the
// file is built with -ffp-contract=off besides), so a numpy fp32 restatement is bit-exact.
#include <stdint.h>

#include "common.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;

// elements in front of the first 16-byte boundary of `p`, at most n
__device__ __forceinline__ long head_of(const float* p, long n) {
  const long h = (long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  return h < n ? h : n;
}

__global__ __launch_bounds__(kThreads) void grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long n,
                                                                   int first) {
  const long head = head_of(dst, n);
  const long n4 = (n - head) >> 2;
  float* d = dst + head;
  const float* s = src + head;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 v = load4u(s + 4 * i);
    if (!first) {
      const f32x4 a = load4u(d + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(a[e], v[e]);
    }
    store4u(d + 4 * i, v);
  }
  if (blockIdx.x == 0) {
    const long tail0 = head + (n4 << 2);
    const long t = threadIdx.x;
    long i = -1;
    if (t < head) i = t;
    else if (t - head < n - tail0) i = tail0 + (t - head);
    if (i >= 0) dst[i] = first ? src[i] : __fadd_rn(dst[i], src[i]);
  }
}

__device__ __forceinline__ float ema_one(float e, float p, float w) { return __fadd_rn(e, __fmul_rn(w, __fsub_rn(p, e))); }

__global__ __launch_bounds__(kThreads) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float w,
                                                              const float* __restrict__ record) {
  if (record && record[0] == 0.f) return;      // grid-uniform: the guard skipped this step, the average stays where it is
  const long head = head_of(ema, n);
  const long n4 = (n - head) >> 2;
  float* eb = ema + head;
  const float* pb = p + head;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 e = load4u(eb + 4 * i);
    const f32x4 q = load4u(pb + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = ema_one(e[k], q[k], w);
    store4u(eb + 4 * i, e);
  }
  if (blockIdx.x == 0) {
    const long tail0 = head + (n4 << 2);
    const long t = threadIdx.x;
    long i = -1;
    if (t < head) i = t;
    else if (t - head < n - tail0) i = tail0 + (t - head);
    if (i >= 0) ema[i] = ema_one(ema[i], p[i], w);
  }
}

// a and b do not overlap (checked by the entry point); a lane loads both values, then stores both
__global__ __launch_bounds__(kThreads) void swap_kernel(float* a, float* b, long n) {
  const long head = head_of(a, n);
  const long n4 = (n - head) >> 2;
  float* ab = a + head;
  float* bb = b + head;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 va = load4u(ab + 4 * i);
    const f32x4 vb = load4u(bb + 4 * i);
    store4u(ab + 4 * i, vb);
    store4u(bb + 4 * i, va);
  }
  if (blockIdx.x == 0) {
    const long tail0 = head + (n4 << 2);
    const long t = threadIdx.x;
    long i = -1;
    if (t < head) i = t;
    else if (t - head < n - tail0) i = tail0 + (t - head);
    if (i >= 0) {
      const float va = a[i], vb = b[i];
      a[i] = vb;
      b[i] = va;
    }
  }
}

int grid_for(long n) {
  const long g = ((n + 3) / 4 + kThreads - 1) / kThreads;
  return (int)(g > kMaxBlocks ? kMaxBlocks : (g < 1 ? 1 : g));
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_grad_accumulate(float* dst, const float* src, long n, int first, void* stream) {
  CIDNET_CHECK_ARG(dst && src && n > 0 && aligned4(dst) && aligned4(src));
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, dst, src, n, first);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_ema_update(float* ema, const float* p, long n, float w, const float* record, void* stream) {
  CIDNET_CHECK_ARG(ema && p && n > 0 && aligned4(ema) && aligned4(p));
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, ema, p, n, w, record);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_swap(float* a, float* b, long n, void* stream) {
  CIDNET_CHECK_ARG(a && b && n > 0 && aligned4(a) && aligned4(b));
  CIDNET_CHECK_ARG(a + n <= b || b + n <= a);
  hipLaunchKernelGGL(swap_kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, a, b, n);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
