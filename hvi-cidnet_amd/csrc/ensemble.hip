// Geometric self-ensemble: the 8 dihedral views of an image in front of the model, and their inverse-mapped mean behind it.
//   view k of a plane X (H, W), k in 0..7:   k & 1: reverse the columns;  then k & 2: reverse the rows;  then k & 4: transpose.
//            fr(i) = k & 2 ? H-1-i : i,   fc(j) = k & 1 ? W-1-j : j   (both their own inverses)
//            k < 4 ("group A", shape (H, W)):   V_k[i, j] = X[fr(i), fc(j)]
//            k >= 4 ("group B", shape (W, H)):  V_k[p, q] = X[fr(q), fc(p)]
//   views:   y[b * count + v, c] = V_{first + v}(x[b, c]): a pure permutation, every output value is bit for bit one input value.
//   merge:   the inverse undoes the transpose first and then the flips, which is the same index map read the other way:
//            out[b,c,i,j] = (ya[b*na+0, c, i, j] + ya[b*na+1, c, i, W-1-j] + ya[b*na+2, c, H-1-i, j] + ya[b*na+3, c, H-1-i, W-1-j]
//                            + yb[b*nb+0, c, j, i] + yb[b*nb+1, c, W-1-j, i] + yb[b*nb+2, c, j, H-1-i] + yb[b*nb+3, c, W-1-j, H-1-i])
//                           / (float)(na + nb)
//            cut off after na terms of the first line and nb of the second, summed in fp32 from left to right starting from the
//            view-0 value itself (acc = v0; acc += v1; ...), then one correctly rounded fp32 division.  No clamp: NaN and
//            infinity propagate.
//
// Both kernels stream: they are bound by memory.  A block of 256 threads owns a 64 x 64 tile of one (b, c) plane of the
// (H, W) side: thread t owns, in each of 4 passes, the 4 consecutive pixels 4 (t % 16) .. + 3 of tile row t / 16 + 16 pass:
// one 16-byte access per lane at dword alignment (gfx950 runs global memory in unaligned access mode), 16 lanes on the 256
// contiguous bytes of a tile row, so a wave moves four whole row segments per instruction.  A reversed row is the same
// segment with the lane order and the four values of a lane reversed: still one 16-byte access per lane on contiguous bytes.
// A group of four that crosses the plane's right edge goes value by value.
// The transposed side cannot be walked that way: a row of the (H, W) tile is a column of the (W, H) one, a row stride apart.
// The tile goes through LDS instead, tile[64][65] floats -- views: filled from x in rows, read in columns; merge: filled
// from yb in columns, read in rows -- so that on the (W, H) side, too, a lane moves 4 consecutive floats of one row and 16
// lanes a contiguous 256-byte segment.  The LDS accesses are single dwords (bank = dword address mod 32): a row access
// tile[r][4 c4 + m] puts the 16 lanes of a row on banks r + m + 4 c4, a column access tile[4 i4 + m][c] on 65 (4 i4 + m) + c =
// 4 i4 + m + c mod 32: either way 8 banks taken twice by the 16 lanes, and the second row / column of the 32-lane half on the
// 8 banks next to them -- 2-way, where the unpadded [64][64] tile would put a whole column on ONE bank (32-way).  Two cycles
// per LDS instruction where one would do is far below what the global side costs per tile, so no swizzle is spent on it.
// views reads x once and writes every requested view of the group from the same registers / the same LDS tile.  merge keeps
// the 16 running sums of a thread in registers, takes group A straight from memory and group B view by view through two
// LDS tiles used in turn (one barrier per view: a tile is written again only after the barrier that follows its successor's
// writes, which every thread reaches after its reads of it).  No atomics, no reductions across lanes: a value depends on
// its own pixel's views alone, in a fixed order.
#include "common.h"
#include "cidnet_hip.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;                                        // tile side: 16 lanes x 4 floats per row
constexpr int kPad = kTile + 1;                                  // LDS row stride in floats
constexpr int kPasses = kTile * kTile / (4 * kThreads);          // 4: rows t / 16 + 16 pass

__device__ __forceinline__ f32x4 rev4(f32x4 v) { return f32x4{v[3], v[2], v[1], v[0]}; }

// 4 values at row[j0 .. j0 + 3] of a row of n floats (flip: at row[n-1-j0 .. n-4-j0], in that order); lanes past n are 0
__device__ __forceinline__ f32x4 load_seg(const float* row, int j0, int n, bool flip) {
  if (j0 + 4 <= n) {
    const f32x4 v = load4u(row + (flip ? n - 4 - j0 : j0));
    return flip ? rev4(v) : v;
  }
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 3; ++m)
    if (j0 + m < n) v[m] = row[flip ? n - 1 - (j0 + m) : j0 + m];
  return v;
}

// the inverse: v[m] -> row[j0 + m] (flip: row[n-1-(j0+m)]) for j0 + m < n
__device__ __forceinline__ void store_seg(float* row, int j0, int n, bool flip, f32x4 v) {
  if (j0 + 4 <= n) {
    store4u(row + (flip ? n - 4 - j0 : j0), flip ? rev4(v) : v);
    return;
  }
#pragma unroll
  for (int m = 0; m < 3; ++m)
    if (j0 + m < n) row[flip ? n - 1 - (j0 + m) : j0 + m] = v[m];
}

// blockIdx.x = (c * tiles_y + ty) * tiles_x + tx, blockIdx.y = b.  kTrans: views first .. first+count-1 lie in 4..7, else in 0..3.
template <bool kTrans>
__global__ __launch_bounds__(kThreads) void ensemble_views_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H,
                                                                  int W, int first, int count, int tiles_x, int tiles_y) {
  __shared__ float tile[kTrans ? kTile * kPad : 1];
  const int tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y, c = rest / tiles_y;
  const long b = blockIdx.y;
  const long plane = (long)H * W;
  const float* xp = x + (b * C + c) * plane;
  const int i0 = ty * kTile, j0 = tx * kTile;
  const int r = threadIdx.x >> 4, q4 = 4 * (threadIdx.x & 15);

  f32x4 v[kPasses];
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int i = i0 + r + 16 * p;
    v[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < H && j0 + q4 < W) v[p] = load_seg(xp + (long)i * W, j0 + q4, W, false);
  }
  if (kTrans) {
#pragma unroll
    for (int p = 0; p < kPasses; ++p)
#pragma unroll
      for (int m = 0; m < 4; ++m) tile[(r + 16 * p) * kPad + q4 + m] = v[p][m];
    __syncthreads();
  }
  for (int s = 0; s < count; ++s) {
    const int k = first + s;
    const bool fc = k & 1, fr = k & 2;
    float* yp = y + ((b * count + s) * C + c) * plane;
    if (!kTrans) {                                               // V[fr(i), fc(j)] = X[i, j]
#pragma unroll
      for (int p = 0; p < kPasses; ++p) {
        const int i = i0 + r + 16 * p;
        if (i < H && j0 + q4 < W) store_seg(yp + (long)(fr ? H - 1 - i : i) * W, j0 + q4, W, fc, v[p]);
      }
    } else {                                                     // V[fc(j), fr(i)] = X[i, j]: row fc(j) of (W, H), 4 consecutive i
#pragma unroll
      for (int p = 0; p < kPasses; ++p) {
        const int jl = r + 16 * p, j = j0 + jl;                  // this thread's column of the tile, its 4 rows q4 .. q4 + 3
        if (j >= W || i0 + q4 >= H) continue;
        const f32x4 t = {tile[q4 * kPad + jl], tile[(q4 + 1) * kPad + jl], tile[(q4 + 2) * kPad + jl], tile[(q4 + 3) * kPad + jl]};
        store_seg(yp + (long)(fc ? W - 1 - j : j) * H, i0 + q4, H, fr, t);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void ensemble_merge_kernel(const float* __restrict__ ya, int na, const float* __restrict__ yb,
                                                                  int nb, float* __restrict__ out, int C, int H, int W, int tiles_x,
                                                                  int tiles_y) {
  __shared__ float tile[2][kTile * kPad];
  const int tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y, c = rest / tiles_y;
  const long b = blockIdx.y;
  const long plane = (long)H * W;
  const int i0 = ty * kTile, j0 = tx * kTile;
  const int r = threadIdx.x >> 4, q4 = 4 * (threadIdx.x & 15);

  f32x4 acc[kPasses];
  for (int k = 0; k < na; ++k) {                                 // group A: out[i, j] += ya_k[fr(i), fc(j)]
    const bool fc = k & 1, fr = k & 2;
    const float* yp = ya + ((b * na + k) * C + c) * plane;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int i = i0 + r + 16 * p;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < H && j0 + q4 < W) v = load_seg(yp + (long)(fr ? H - 1 - i : i) * W, j0 + q4, W, fc);
      if (k == 0) {
        acc[p] = v;                                              // the view-0 value itself: no 0 + v (which would turn -0 into +0)
      } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[p][m] += v[m];
      }
    }
  }
  for (int s = 0; s < nb; ++s) {                                 // group B: out[i, j] += yb_s[fc(j), fr(i)], through LDS
    const bool fc = s & 1, fr = s & 2;
    const float* yp = yb + ((b * nb + s) * C + c) * plane;
    float* tl = tile[s & 1];
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int jl = r + 16 * p, j = j0 + jl;                    // row fc(j) of (W, H), its 4 consecutive values fr(i0 + q4 ..)
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (j < W && i0 + q4 < H) v = load_seg(yp + (long)(fc ? W - 1 - j : j) * H, i0 + q4, H, fr);
#pragma unroll
      for (int m = 0; m < 4; ++m) tl[(q4 + m) * kPad + jl] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < kPasses; ++p)
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[p][m] += tl[(r + 16 * p) * kPad + q4 + m];
  }
  const float n = (float)(na + nb);
  float* op = out + (b * C + c) * plane;
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int i = i0 + r + 16 * p;
    if (i >= H || j0 + q4 >= W) continue;
    const f32x4 o = {acc[p][0] / n, acc[p][1] / n, acc[p][2] / n, acc[p][3] / n};
    store_seg(op + (long)i * W, j0 + q4, W, false, o);
  }
}

// blocks per image, or 0 when the launch would not fit
inline long tiles_of(int C, int H, int W, int* tiles_x, int* tiles_y) {
  *tiles_x = (W + kTile - 1) / kTile;
  *tiles_y = (H + kTile - 1) / kTile;
  const long n = (long)C * *tiles_x * *tiles_y;
  return n > 0x7fffffffL ? 0 : n;
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_ensemble_views(const float* x, float* y, int B, int C, int H, int W, int first, int count, void* stream) {
  CIDNET_CHECK_ARG(x && y);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || count < 1 || first < 0 || first > 7 || count > 4) return CIDNET_ERR_SHAPE;
  if (first + count - 1 > 7 || (first < 4 && first + count - 1 >= 4)) return CIDNET_ERR_SHAPE;       // one group, inside 0..7
  if ((long)B * count > 65535) return CIDNET_ERR_SHAPE;
  int tiles_x, tiles_y;
  const long gx = tiles_of(C, H, W, &tiles_x, &tiles_y);
  if (gx == 0) return CIDNET_ERR_SHAPE;
  if (first < 4)
    hipLaunchKernelGGL(ensemble_views_kernel<false>, dim3((unsigned)gx, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, x, y, C,
                       H, W, first, count, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(ensemble_views_kernel<true>, dim3((unsigned)gx, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, x, y, C,
                       H, W, first, count, tiles_x, tiles_y);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_ensemble_merge(const float* ya, int na, const float* yb, int nb, float* out, int B, int C, int H, int W, void* stream) {
  CIDNET_CHECK_ARG(ya && out);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || na < 1 || na > 4 || nb < 0 || nb > 4) return CIDNET_ERR_SHAPE;
  if ((yb == nullptr) != (nb == 0)) return CIDNET_ERR_SHAPE;
  if (B > 65535) return CIDNET_ERR_SHAPE;
  int tiles_x, tiles_y;
  const long gx = tiles_of(C, H, W, &tiles_x, &tiles_y);
  if (gx == 0) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(ensemble_merge_kernel, dim3((unsigned)gx, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, ya, na, yb, nb,
                     out, C, H, W, tiles_x, tiles_y);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
