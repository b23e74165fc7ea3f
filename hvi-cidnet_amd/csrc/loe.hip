// LOE, the lightness order error of Wang et al. 2013 (include/cidnet_hip.h: cidnet_metric_loe_*): how many ordered pairs of
// sampled pixels change their lightness order between the low input and the enhanced output.  L = max(R, G, B) is a byte,
// so the pair count depends on the samples only through the 256 x 256 joint histogram H[a][b] = #{x : L(x) = a, Le(x) = b}:
// with A[a] = #{L <= a}, B[b] = #{Le <= b} and C[a][b] = #{L <= a and Le <= b} (the 2-D inclusive prefix of H)
//   num = sum_{x,y} [L(x) >= L(y)] xor [Le(x) >= Le(y)] = sum_{a,b} H[a][b] (A[a] + B[b] - 2 C[a][b]),
// because for a sample x in bin (a, b) the y with L(y) <= a number A[a], those with Le(y) <= b number B[b], and the y that
// satisfy both are counted in both.  O(m + 65536) per image instead of O(m^2).
//
// Two launches on one stream, no hand-off between blocks inside a launch:
//   1. loe_hist_kernel: a block takes at most kMaxSamples consecutive samples of one image into a sub-histogram in LDS, 65536
//      counters of 16 bits, two per dword, bumped by a 32-bit LDS integer add of 1 << 16 (bin & 1).  A block's samples number
//      fewer than 2^16, so no counter can carry into its neighbour.  Natural images put most samples into a few bins near the
//      diagonal: the contention stays inside the compute unit, and a block sends one global integer add per non-zero bin.
//   2. loe_finish_kernel: one block per image walks H in 32-row chunks -- a row prefix per wave into LDS, then one thread per
//      column carries the column prefix down the rows -- and sums the weighted terms in 64-bit integers.
// Integer adds only, so the order in which blocks and lanes arrive does not matter: repeated calls are bit-identical.
#include "cidnet_hip.h"
#include "common.h"

namespace cidnet {
namespace {

constexpr int kBins = 65536;
constexpr int kHistThreads = 1024;
constexpr int kHistDwords = kBins / 2;                 // 16-bit counters, two per dword: 128 KiB of the CU's 160 KiB
constexpr int kHistLds = kHistDwords * 4;
constexpr int kCounterBits = 16;
constexpr int kMaxSamples = 16384;                     // per block; must stay below 2^kCounterBits
static_assert(kMaxSamples < (1 << kCounterBits), "a block's samples must fit a 16-bit counter");
constexpr int kFinThreads = 256;
constexpr int kFinRows = 32;                           // rows of H per chunk: 32 KiB of LDS

struct LoePlan {
  int rows, cols, blocks, per_block, counter_bits, lds_bytes;
};

// The one place the sampling grid and the block split are decided: the launcher and cidnet_metric_loe_plan both call it.
int loe_plan(int h, int w, int step, LoePlan* p) {
  if (h < 1 || w < 1 || step < 1 || step > (h < w ? h : w)) return CIDNET_ERR_ARG;
  const long rows = h / step, cols = w / step, m = rows * cols;
  if (m > (1L << 30)) return CIDNET_ERR_SHAPE;         // 32-bit bins and sample indices, with room for a loop's last stride
  const long blocks = (m + kMaxSamples - 1) / kMaxSamples;
  p->rows = (int)rows;
  p->cols = (int)cols;
  p->blocks = (int)blocks;
  p->per_block = (int)((m + blocks - 1) / blocks);
  p->counter_bits = kCounterBits;
  p->lds_bytes = kHistLds;
  return CIDNET_OK;
}

struct __attribute__((packed, aligned(1))) u8x4 {
  uint32_t v;
};

__device__ __forceinline__ uint32_t max3u(uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t t = a > b ? a : b;
  return t > c ? t : c;
}

__device__ __forceinline__ void bump(uint32_t* lds, uint32_t l, uint32_t e) {
  const uint32_t bin = (l << 8) | e;
  atomicAdd(&lds[bin >> 1], 1u << ((bin & 1u) * 16u));
}

// grid (blocks per image, B).  Samples s0 .. s1 - 1 of image blockIdx.y, s = i * cols + j at pixel (i * step, j * step).
__global__ __launch_bounds__(kHistThreads) void loe_hist_kernel(const uint8_t* __restrict__ low, const uint8_t* __restrict__ out,
                                                                long plane, int w, int step, int cols, int m, int per_block,
                                                                uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t lds[];
  const int tid = threadIdx.x;
  for (int i = tid; i < kHistDwords; i += kHistThreads) lds[i] = 0u;
  __syncthreads();
  const long base = (long)blockIdx.y * 3 * plane;
  const uint8_t* lp = low + base;
  const uint8_t* op = out + base;
  const int s0 = (int)((long)blockIdx.x * per_block);            // blocks * per_block < m + blocks: no overflow of long
  const int s1 = (m - s0 < per_block) ? m : s0 + per_block;      // s0 < m: blocks = ceil(m / per_block) at most
  if (step == 1) {                                               // cols == w: sample s is pixel s, four per lane and load
    const int groups = (s1 - s0) >> 2;
    for (int g = tid; g < groups; g += kHistThreads) {
      const long o = s0 + 4 * g;
      const uint32_t lr = reinterpret_cast<const u8x4*>(lp + o)->v, lg = reinterpret_cast<const u8x4*>(lp + plane + o)->v,
                     lb = reinterpret_cast<const u8x4*>(lp + 2 * plane + o)->v;
      const uint32_t er = reinterpret_cast<const u8x4*>(op + o)->v, eg = reinterpret_cast<const u8x4*>(op + plane + o)->v,
                     eb = reinterpret_cast<const u8x4*>(op + 2 * plane + o)->v;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sh = 8 * k;
        bump(lds, max3u((lr >> sh) & 255u, (lg >> sh) & 255u, (lb >> sh) & 255u),
             max3u((er >> sh) & 255u, (eg >> sh) & 255u, (eb >> sh) & 255u));
      }
    }
    for (int s = s0 + 4 * groups + tid; s < s1; s += kHistThreads)
      bump(lds, max3u(lp[s], lp[plane + s], lp[2 * plane + s]), max3u(op[s], op[plane + s], op[2 * plane + s]));
  } else {
    for (int s = s0 + tid; s < s1; s += kHistThreads) {
      const int i = s / cols, j = s - i * cols;
      const long o = (long)i * step * w + (long)j * step;        // i * step < h, j * step < w
      bump(lds, max3u(lp[o], lp[plane + o], lp[2 * plane + o]), max3u(op[o], op[plane + o], op[2 * plane + o]));
    }
  }
  __syncthreads();
  uint32_t* H = hist + (long)blockIdx.y * kBins;
  for (int i = tid; i < kHistDwords; i += kHistThreads) {
    const uint32_t v = lds[i];
    if (v & 0xffffu) atomicAdd(&H[2 * i], v & 0xffffu);
    if (v >> 16) atomicAdd(&H[2 * i + 1], v >> 16);
  }
}

// One block per image.  All 64-bit arithmetic is modulo 2^64 (unsigned); num <= m^2 <= 2^60, so the count is exact.  (double)num
// is exact too while m <= 2^26 (num < 2^53): the division is then the only rounding of loe.
__global__ __launch_bounds__(kFinThreads) void loe_finish_kernel(const uint32_t* __restrict__ hist, int m,
                                                                 long long* __restrict__ num, double* __restrict__ loe) {
  __shared__ __attribute__((aligned(16))) uint32_t P[kFinRows][256];        // P[r][b] = sum_{b' <= b} H[a0 + r][b']
  __shared__ unsigned long long red[kFinThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t* H = hist + (long)blockIdx.x * kBins;
  uint32_t C = 0, colsum = 0, A = 0;                   // C[a][t], sum_{a' <= a} H[a'][t], A[a]: all <= m < 2^31
  unsigned long long acc = 0;
  for (int a0 = 0; a0 < 256; a0 += kFinRows) {
    for (int r = wv; r < kFinRows; r += kFinThreads / 64) {
      uint4 v = *reinterpret_cast<const uint4*>(H + (a0 + r) * 256 + 4 * lane);
      v.y += v.x; v.z += v.y; v.w += v.z;
      uint32_t s = v.w;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t n = __shfl_up(s, o, 64);
        if (lane >= o) s += n;
      }
      const uint32_t ex = s - v.w;
      v.x += ex; v.y += ex; v.z += ex; v.w += ex;
      *reinterpret_cast<uint4*>(&P[r][4 * lane]) = v;
    }
    __syncthreads();
    for (int r = 0; r < kFinRows; ++r) {
      const uint32_t p = P[r][t], pl = t ? P[r][t - 1] : 0u, hv = p - pl;
      A += P[r][255];
      C += p;
      colsum += hv;
      acc += (unsigned long long)hv * ((unsigned long long)A - 2ull * (unsigned long long)C);
    }
    __syncthreads();
  }
  acc += (unsigned long long)colsum * (unsigned long long)C;     // B[t] = C[255][t]
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (t == 0) {
    unsigned long long n = 0;
    for (int i = 0; i < kFinThreads / 64; ++i) n += red[i];
    num[blockIdx.x] = (long long)n;
    loe[blockIdx.x] = (double)n / (double)m;
  }
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

long cidnet_metric_loe_ws_bytes(int B) { return B < 1 ? 0 : (long)B * kBins * 4; }

int cidnet_metric_loe_plan(int h, int w, int step, int* out, int n) {
  if (!out || n < 6) return CIDNET_ERR_ARG;
  LoePlan p;
  const int rc = loe_plan(h, w, step, &p);
  if (rc != CIDNET_OK) return rc;
  out[0] = p.rows; out[1] = p.cols; out[2] = p.blocks; out[3] = p.per_block; out[4] = p.counter_bits; out[5] = p.lds_bytes;
  return CIDNET_OK;
}

int cidnet_metric_loe_u8(const uint8_t* low, const uint8_t* out, int B, int h, int w, int step, long long* num, double* loe,
                         void* ws, long ws_bytes, void* stream) {
  CIDNET_CHECK_ARG(low && out && num && loe && ws && B >= 1 && ((uintptr_t)ws & 15) == 0);
  LoePlan p;
  const int rc = loe_plan(h, w, step, &p);
  if (rc != CIDNET_OK) return rc;
  if (B > 65535) return CIDNET_ERR_SHAPE;
  if (ws_bytes < cidnet_metric_loe_ws_bytes(B)) return CIDNET_ERR_WS;
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)B * kBins * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  static LdsLimit lds;                                 // once per device: the kernel's dynamic-LDS limit
  e = lds.raise(reinterpret_cast<const void*>(&loe_hist_kernel), kHistLds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(loe_hist_kernel, dim3(p.blocks, B), dim3(kHistThreads), kHistLds, (hipStream_t)stream, low, out,
                     (long)h * w, w, step, p.cols, p.rows * p.cols, p.per_block, reinterpret_cast<uint32_t*>(ws));
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(loe_finish_kernel, dim3(B), dim3(kFinThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(ws), p.rows * p.cols, num, loe);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
