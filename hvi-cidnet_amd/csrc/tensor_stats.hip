// Per-tensor statistics of a flat fp32 buffer (include/cidnet_hip.h: cidnet_tensor_stats, cidnet_tensor_stats_plan): for every
// segment of the trainer's gradient or weight arena the 2-norm and the largest magnitude of its finite elements, the number
// of non-finite ones and the index of the first.  The guard (guard.hip) says THAT a step went non-finite; this says WHERE,
// without the host waiting: the rows land in a device ring (dp.TensorLog) that is read once per epoch.
//
// Shaped like the guard: two launches, fp64 partials in fixed slots, a fixed order of additions, no atomics and no hand-off
// between blocks inside a launch, so repeated calls are bit-identical.  A tile belongs to one segment and a segment's row is
// formed from its own slots alone, so it does not depend on what else is in the call.
#include "common.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 4096;                    // elements per tile: 16 per thread, four 16-byte loads
constexpr int kPerPass = kThreads * 4;
constexpr long kMaxTiles = 1L << 30;           // tile numbers are int32, with room for a grid and for T + 2 tiles
constexpr int kNoFirst = 0x7fffffff;

struct Slot {                                  // one tile's partial, 32 bytes
  double sum;
  double max;
  long long count;
  long long first;                             // index inside the SEGMENT, -1: none
};
static_assert(sizeof(Slot) == 32, "the workspace is 32 bytes per tile");

struct StatsPlan {
  long tiles, ws_bytes, table_ints;
};

// The one place the tiling is decided: the launcher and cidnet_tensor_stats_plan both call it.  seg_tiles and table may be
// NULL; nothing is written unless every check has passed.
int stats_plan(const long* off, const long* len, long T, long n, StatsPlan* p, int* seg_tiles, int* table, long table_ints) {
  if (!off || !len || T < 1 || n < 1) return CIDNET_ERR_ARG;
  if (T > kMaxTiles) return CIDNET_ERR_SHAPE;
  long tiles = 0;
  for (long t = 0; t < T; ++t) {
    if (len[t] < 1 || off[t] < 0 || off[t] > n || len[t] > n - off[t]) return CIDNET_ERR_ARG;
    tiles += (len[t] - 1) / kTile + 1;
    if (tiles > kMaxTiles) return CIDNET_ERR_SHAPE;
  }
  if (table && table_ints < T + 2 * tiles) return CIDNET_ERR_ARG;
  p->tiles = tiles;
  p->ws_bytes = tiles * (long)sizeof(Slot);
  p->table_ints = T + 2 * tiles;
  long j = 0;
  for (long t = 0; t < T; ++t) {
    const long k = (len[t] - 1) / kTile + 1;
    if (seg_tiles) seg_tiles[t] = (int)k;
    if (table) {
      table[t] = (int)j;
      for (long i = 0; i < k; ++i) {
        table[T + 2 * (j + i)] = (int)t;
        table[T + 2 * (j + i) + 1] = (int)i;
      }
    }
    j += k;
  }
  return CIDNET_OK;
}

struct Acc {
  double sum;
  float max;
  int count, first;                            // first: index inside the tile, kNoFirst: none
};

// classify by the exponent bits, then either add or count: no comparison and no fmax ever sees a NaN
__device__ __forceinline__ void take(Acc& a, float x, int i) {
  const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const float m = finite ? fabsf(x) : 0.f;
  const double d = finite ? (double)x : 0.0;
  a.sum += d * d;
  a.max = m > a.max ? m : a.max;
  a.count += finite ? 0 : 1;
  a.first = (!finite && i < a.first) ? i : a.first;
}

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_min_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

// grid: tiles.  Tile j = tile k of segment t (table); elements [k * 4096, min(len[t], (k + 1) * 4096)) of the segment.
__global__ __launch_bounds__(kThreads) void stats_tile_kernel(const float* __restrict__ buf, const long* __restrict__ off,
                                                              const long* __restrict__ len, const int* __restrict__ tile,
                                                              Slot* __restrict__ slots) {
  __shared__ double rsum[kWaves];
  __shared__ float rmax[kWaves];
  __shared__ int rcnt[kWaves], rfirst[kWaves];
  const int t = tile[2 * blockIdx.x], k = tile[2 * blockIdx.x + 1];
  const long start = (long)k * kTile;
  const long left = len[t] - start;
  const int cnt = left < kTile ? (int)left : kTile;
  const float* x = buf + off[t] + start;
  Acc a = {0.0, 0.f, 0, kNoFirst};
#pragma unroll
  for (int q = 0; q < kTile / kPerPass; ++q) {
    const int i = q * kPerPass + 4 * (int)threadIdx.x;
    if (i + 4 <= cnt) {
      const f32x4 v = load4u(x + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) take(a, v[e], i + e);
    } else {
      for (int e = i; e < cnt; ++e) take(a, x[e], e);        // the tile's last 1..3 elements, one thread
    }
  }
  a.sum = wave_sum_f64(a.sum);
  a.max = wave_max_f32(a.max);
  a.count = wave_sum_i32(a.count);
  a.first = wave_min_i32(a.first);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    rsum[w] = a.sum; rmax[w] = a.max; rcnt[w] = a.count; rfirst[w] = a.first;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  Acc r = {0.0, 0.f, 0, kNoFirst};
  for (int i = 0; i < kWaves; ++i) {
    r.sum += rsum[i];
    r.max = rmax[i] > r.max ? rmax[i] : r.max;
    r.count += rcnt[i];
    r.first = rfirst[i] < r.first ? rfirst[i] : r.first;
  }
  Slot s;
  s.sum = r.sum;
  s.max = (double)r.max;
  s.count = r.count;
  s.first = r.first == kNoFirst ? -1 : start + r.first;
  slots[blockIdx.x] = s;
}

// grid: T, one wave each.  Adds segment t's slots first[t] .. first[t] + ceil(len[t] / 4096) - 1.
__global__ __launch_bounds__(64) void stats_finish_kernel(const Slot* __restrict__ slots, const long* __restrict__ len,
                                                          const int* __restrict__ first_tile, float scale,
                                                          double* __restrict__ out) {
  const int t = blockIdx.x;
  const long k = (len[t] - 1) / kTile + 1;
  const Slot* s = slots + first_tile[t];
  double sum = 0.0, mx = 0.0;
  long long count = 0, first = 0x7fffffffffffffffLL;
  for (long i = threadIdx.x; i < k; i += 64) {
    const Slot v = s[i];
    sum += v.sum;
    mx = v.max > mx ? v.max : mx;
    count += v.count;
    first = (v.first >= 0 && v.first < first) ? v.first : first;
  }
  sum = wave_sum_f64(sum);
  mx = wave_max_f64(mx);
  count = wave_sum_i64(count);
  first = wave_min_i64(first);
  if (threadIdx.x != 0) return;
  double* row = out + 4 * (long)t;
  row[0] = sqrt(sum) * (double)scale;
  row[1] = mx * (double)scale;
  row[2] = (double)count;
  row[3] = count > 0 ? (double)first : -1.0;
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_tensor_stats_plan(const long* off, const long* len, long T, long n, long* out, int n_out, int* seg_tiles, int* table,
                             long table_ints) {
  if (!out || n_out < 3) return CIDNET_ERR_ARG;
  StatsPlan p;
  const int rc = stats_plan(off, len, T, n, &p, seg_tiles, table, table_ints);
  if (rc != CIDNET_OK) return rc;
  out[0] = p.tiles; out[1] = p.ws_bytes; out[2] = p.table_ints;
  return CIDNET_OK;
}

int cidnet_tensor_stats(const float* buf, long n, const long* off, const long* len, long T, const long* off_dev,
                        const long* len_dev, const int* table_dev, float scale, double* out, void* ws, long ws_bytes,
                        void* stream) {
  CIDNET_CHECK_ARG(buf && off_dev && len_dev && table_dev && out && ws);
  CIDNET_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 7) == 0);
  CIDNET_CHECK_ARG(scale >= 0.f && scale <= 3.402823466e38f);          // false for a NaN as well
  StatsPlan p;
  const int rc = stats_plan(off, len, T, n, &p, nullptr, nullptr, 0);
  if (rc != CIDNET_OK) return rc;
  if (ws_bytes < p.ws_bytes) return CIDNET_ERR_WS;
  Slot* slots = reinterpret_cast<Slot*>(ws);
  hipLaunchKernelGGL(stats_tile_kernel, dim3((unsigned)p.tiles), dim3(kThreads), 0, (hipStream_t)stream, buf, off_dev, len_dev,
                     table_dev + T, slots);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, slots, len_dev, table_dev, scale,
                     out);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
