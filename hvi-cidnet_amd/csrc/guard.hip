// The guard in front of the fused Adam (include/cidnet_hip.h: cidnet_grad_guard, cidnet_adam_step_dev): the 2-norm of the
// flat gradient in fp64, the clipping coefficient of torch.nn.utils.clip_grad_norm_, the decision to apply or skip the
// step, Adam's step count and bias corrections -- all formed on the device, so the host, which runs steps ahead of the
// device, never waits for a norm.  The reference's own clip (train.py:68-69) runs before zero_grad() / backward() and so
// clips the previous step's gradients; this one sits between the backward (after the all-reduce) and the update.
//
// Two launches for the norm: per-block fp64 partials in fixed slots, then one block that adds the slots in a fixed order.
// The square of an fp32 value is exact in fp64, so only the additions round; no atomics, no hand-off between blocks inside
// a launch, repeated calls are bit-identical.
#include "common.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPartials = 256;          // at most this many blocks / slots: 7.9 MB are latency-sized, not bandwidth-sized

// Sum over the block in a fixed order; result valid in thread 0.  `red`: LDS scratch of kWaves doubles.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < kWaves; ++i) t += red[i];
  }
  return t;
}

__global__ __launch_bounds__(kThreads) void sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
  __shared__ double red[kWaves];
  double acc = 0.0;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 v = load4u(g + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)v[e];
      acc += d * d;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double d = (double)g[(n4 << 2) + threadIdx.x];
    acc += d * d;
  }
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One block: adds the partials, decides, and writes state, record and log row from thread 0.
__global__ __launch_bounds__(kThreads) void guard_finish_kernel(const double* __restrict__ part, int nparts, float grad_scale,
                                                                float max_norm, int skip_nonfinite, float beta1, float beta2,
                                                                const float* __restrict__ loss, long long* __restrict__ state,
                                                                float* __restrict__ record, double* __restrict__ log_row) {
  __shared__ double red[kWaves];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) a += part[i];
  const double ss = block_sum_f64(a, red);
  if (threadIdx.x != 0) return;
  const bool finite = isfinite(ss);
  const bool apply = finite || !skip_nonfinite;
  const double norm = sqrt(ss) * (double)grad_scale;
  const bool clip = max_norm > 0.f && isfinite(max_norm);
  double coef = 1.0;
  if (clip) {
    coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;                // torch's clamp(max=1): a NaN norm stays NaN, an infinite one gives 0
  }
  long long applied = state[0], skipped = state[1];
  if (apply) ++applied; else ++skipped;
  state[0] = applied;
  state[1] = skipped;
  const double t = (double)(applied > 0 ? applied : 1);
  record[0] = apply ? 1.f : 0.f;
  record[1] = (float)((double)grad_scale * coef);
  record[2] = (float)(1.0 - pow((double)beta1, t));
  record[3] = (float)sqrt(1.0 - pow((double)beta2, t));
  if (log_row) {
    log_row[0] = loss ? (double)loss[0] : __builtin_nan("");
    log_row[1] = norm;
    log_row[2] = coef;
    log_row[3] = apply ? (double)applied : -(double)(applied + 1);
  }
}

// adam_kernel of train.hip with the gradient scale and the bias corrections read from the decision record
__global__ __launch_bounds__(kThreads) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                            float wd, const float* __restrict__ record) {
  __shared__ float rec[4];                     // the record is read once per block, by its first four lanes
  if (threadIdx.x < 4) rec[threadIdx.x] = record[threadIdx.x];
  __syncthreads();
  if (rec[0] == 0.f) return;                   // block-uniform, after the barrier: the whole grid leaves p, m, v alone
  const float gscale = rec[1], bc1 = rec[2], bc2_sqrt = rec[3];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float gi = g[i] * gscale;
    const float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - (lr / bc1) * (mi / denom);
  }
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

long cidnet_grad_guard_ws_doubles(void) { return kPartials; }

int cidnet_grad_guard(const float* g, long n, float grad_scale, float max_norm, int skip_nonfinite, float beta1, float beta2,
                      const float* loss, double* ws, long ws_doubles, long* state, float* record, double* log_row,
                      void* stream) {
  CIDNET_CHECK_ARG(g && ws && state && record && n > 0);
  if (ws_doubles < kPartials) return CIDNET_ERR_WS;
  long b = ((n + 3) / 4 + kThreads - 1) / kThreads;
  const int grid = (int)(b > kPartials ? kPartials : (b < 1 ? 1 : b));
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g, n, ws);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, ws, grid, grad_scale, max_norm,
                     skip_nonfinite, beta1, beta2, loss, reinterpret_cast<long long*>(state), record, log_row);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_adam_step_dev(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, const float* record, void* stream) {
  CIDNET_CHECK_ARG(p && g && m && v && record && n > 0);
  long gsz = (n + kThreads - 1) / kThreads;
  const int grid = (int)(gsz > 4096 ? 4096 : gsz);
  hipLaunchKernelGGL(adam_dev_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, record);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
