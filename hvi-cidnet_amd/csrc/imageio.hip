// Image files in and out: the two ends of the reference's eval.py / eval_SID_blur.py / demo.py / app.py around the model, between
// the interleaved (h,w,3) bytes that PIL and every file format hold and the planar fp32 tensor the network takes.
//   ingest:  ri = i < h ? i : 2(h-1) - i,  rj = j < w ? j : 2(w-1) - j            (F.pad(..., 'reflect') at the bottom and right:
//            x[b,c,i,j] = T[src_b[ri,rj,c]]   for i < Hp, j < Wp                   eval_sets.py:22-28, demo.py:47-52, app.py:35-40)
//            T = the caller's 256-entry table (pow(q / 255, gamma), data.gamma_table), or fp32(q) / 255.0f when table == NULL
//            (a correctly rounded fp32 division: ToTensor's .div(255)).
//   egress:  dst_b[i,j,c] = (uint8) trunc(clamp(x[b,c,i,j], 0, 1) * 255.0f)   for i < h, j < w; NaN -> 0
//            (eval.py:69-73 with ToPILImage's pic.mul(255).byte(): value for value what cidnet_metric_to_uint8 writes, interleaved).
// Image b of the byte side starts at base + b * bs (bs >= 3 h w, any byte alignment); the fp32 side is (B,3,Hp,Wp) contiguous.
//
// Both kernels are byte shuffles bound by memory.  blockIdx.y is the image, a lane owns 4 consecutive pixels of one row of
// the fp32 side: 12 consecutive bytes of the byte side (three dword accesses at an arbitrary byte address; gfx950 runs global
// memory in unaligned access mode) against one 16-byte access per colour plane, consecutive lanes on consecutive groups, so a
// wave moves 1 KiB of contiguous memory per plane and instruction.  The 256 quotients / powers sit in LDS, filled once per
// block (csrc/augment.hip has the same layout).  The exceptions go one pixel at a time: a row tail of 1-3 pixels, and in ingest a
// group that touches the reflected columns (at most two groups per row when the pad is below 8).  Nothing outside the 3 h w bytes
// of an image is read or written, whatever follows them.  No atomics, no reductions: a value depends on its own image alone.
//
// The tiled forms (one large image as n overlapping windows of one shape (th, tw), multiples of 4; image_io.py: tile_plan):
//   ingest_tiles:  x[t,c,i,j] = T[src[ry,rx,c]], ry = y_t + i reflected as 2(h-1) - ry when ry >= h, rx likewise: ingest seen
//                  through a window whose corner (y_t, x_t) is read from device memory; blockIdx.y is the tile.
//   egress_tiles:  a gather over the output pixels: for every tile that covers (y, x), rows outer, both ascending,
//                  acc += (wy wx) clamp(v), den += wy wx in fp32; the pixel is acc / den, or clamp(v) itself where one tile
//                  covers it (no product, no division: a plan of one tile writes what egress writes); then quantised and
//                  interleaved as in egress.  No atomics.
// Same lane layout.  Bytes per pixel, from shapes:
//   ingest_tiles  3 read + 12 written per TILE pixel, so 15 per image pixel in the interior and 15 c where c tiles cover it
//                 (the bytes of an overlap are read once per covering window; they sit in L2 between two neighbouring tiles);
//   egress_tiles  12 read + 3 written = 15 in the interior; 12 c + 3 where c tiles cover the pixel (c = 2 along an edge
//                 between two tiles, 4 at a corner, at most 9 where a flush last tile makes a triple cover on both axes),
//                 plus 4 bytes of wx per cover and one broadcast wy per row, from tables that stay in L2: (ny th + nx tw)
//                 floats in all.
// The origin lists sit in LDS (a binary search finds a pixel's first covering tile on each axis).  The weights are read from
// the tables in place: with one row segment per lane group every wx entry is used once per block, so a copy to LDS has no
// reuse to pay for it.  A group of four pixels that straddles a tile's edge (origins that are no multiples of 4) is read pixel
// by pixel; a group at the image's right edge that lies inside the tile is read whole (the pad's columns are tile pixels too)
// and only its 1-3 pixels inside the image are written, byte by byte.  Every index into a tile or a table is checked against
// (th, tw) itself, so nothing outside the tiles, the tables and the 3 h w output bytes is touched whatever the origin lists hold.
#include "common.h"
#include "cidnet_hip.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kGroups = 2;                                       // 4-pixel groups per thread: all loads fly before the first store

struct __attribute__((packed, aligned(1))) u32u {
  uint32_t v;
};

__device__ __forceinline__ uint32_t ld32u(const uint8_t* p) { return reinterpret_cast<const u32u*>(p)->v; }
__device__ __forceinline__ void st32u(uint8_t* p, uint32_t v) { reinterpret_cast<u32u*>(p)->v = v; }

__device__ __forceinline__ uint32_t byte_at(uint32_t d0, uint32_t d1, uint32_t d2, int idx) {      // byte idx of the 12
  const uint32_t word = idx < 4 ? d0 : (idx < 8 ? d1 : d2);
  return (word >> (8 * (idx & 3))) & 255u;
}

__device__ __forceinline__ uint32_t quant(float v) {
  const float cl = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;          // NaN -> 0
  return (uint32_t)(cl * 255.0f);                                // fp32 product, truncated (pic.mul(255).byte())
}

__global__ __launch_bounds__(kThreads) void image_ingest_kernel(const uint8_t* __restrict__ src, long src_bs,
                                                                const float* __restrict__ table, float* __restrict__ x, int h,
                                                                int w, int Hp, int Wp, int G) {
  __shared__ float tab[256];
  tab[threadIdx.x] = table ? table[threadIdx.x] : (float)threadIdx.x / 255.0f;
  const long b = blockIdx.y;
  const uint8_t* img = src + b * src_bs;
  const long plane = (long)Hp * Wp;
  float* xb = x + b * 3 * plane;
  __syncthreads();

  const int items = Hp * G;
  const int first = blockIdx.x * (kThreads * kGroups) + threadIdx.x;
  uint32_t d[kGroups][3];                                        // the group's bytes, pixel-interleaved: r0 g0 b0 r1 | g1 b1 r2 g2 | ...
  int n[kGroups];
  long dst[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const int it = first + k * kThreads;
    n[k] = 0;
    if (it >= items) continue;
    const int i = it / G, j = 4 * (it - i * G);
    n[k] = Wp - j < 4 ? Wp - j : 4;
    const int ri = i < h ? i : 2 * (h - 1) - i;
    const uint8_t* row = img + (long)ri * w * 3;
    dst[k] = (long)i * Wp + j;
    if (n[k] == 4 && j + 4 <= w) {                               // 12 consecutive bytes inside the row
      const uint8_t* p = row + 3L * j;
      d[k][0] = ld32u(p);
      d[k][1] = ld32u(p + 4);
      d[k][2] = ld32u(p + 8);
    } else {                                                     // tail or reflected columns: pixel by pixel, byte by byte
      uint32_t by[12];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int jj = j + m;
        const int rj = jj < w ? jj : 2 * (w - 1) - jj;
        const bool on = m < n[k];
        const uint8_t* p = row + 3L * (on ? rj : 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) by[3 * m + c] = on ? (uint32_t)p[c] : 0u;
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) d[k][q] = by[4 * q] | (by[4 * q + 1] << 8) | (by[4 * q + 2] << 16) | (by[4 * q + 3] << 24);
    }
  }
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    if (n[k] == 0) continue;
    const uint32_t d0 = d[k][0], d1 = d[k][1], d2 = d[k][2];
    // byte 3 m + c of the 12 is pixel m, colour c
    const uint32_t px[3][4] = {{d0 & 255u, d0 >> 24, (d1 >> 16) & 255u, (d2 >> 8) & 255u},
                               {(d0 >> 8) & 255u, d1 & 255u, d1 >> 24, (d2 >> 16) & 255u},
                               {(d0 >> 16) & 255u, (d1 >> 8) & 255u, d2 & 255u, d2 >> 24}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = xb + c * plane + dst[k];
      if (n[k] == 4) {
        const f32x4 r = {tab[px[c][0]], tab[px[c][1]], tab[px[c][2]], tab[px[c][3]]};
        store4u(o, r);
      } else {
#pragma nounroll
        for (int m = 0; m < n[k]; ++m) o[m] = tab[byte_at(d0, d1, d2, 3 * m + c)];     // a loop: keeps the 16-byte store whole
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void image_egress_kernel(const float* __restrict__ x, uint8_t* __restrict__ dst, long dst_bs,
                                                                int Hp, int Wp, int h, int w, int G) {
  const long b = blockIdx.y;
  const long plane = (long)Hp * Wp;
  const float* xb = x + b * 3 * plane;
  uint8_t* img = dst + b * dst_bs;

  const int items = h * G;
  const int first = blockIdx.x * (kThreads * kGroups) + threadIdx.x;
  f32x4 v[kGroups][3];
  int n[kGroups];
  long out[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const int it = first + k * kThreads;
    n[k] = 0;
    if (it >= items) continue;
    const int i = it / G, j = 4 * (it - i * G);
    n[k] = w - j < 4 ? w - j : 4;
    out[k] = ((long)i * w + j) * 3;
    const float* p = xb + (long)i * Wp + j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (n[k] == 4) {
        v[k][c] = load4u(p + c * plane);
      } else {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 3; ++m)
          if (m < n[k]) t[m] = p[c * plane + m];
        v[k][c] = t;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    if (n[k] == 0) continue;
    uint32_t by[12];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int c = 0; c < 3; ++c) by[3 * m + c] = quant(v[k][c][m]);
    uint8_t* o = img + out[k];
    if (n[k] == 4) {
#pragma unroll
      for (int q = 0; q < 3; ++q) st32u(o + 4 * q, by[4 * q] | (by[4 * q + 1] << 8) | (by[4 * q + 2] << 16) | (by[4 * q + 3] << 24));
    } else {
#pragma unroll
      for (int m = 0; m < 9; ++m)
        if (m < 3 * n[k]) o[m] = (uint8_t)by[m];
    }
  }
}

constexpr int kMaxOrigins = 1024;                                // per axis, in LDS

__device__ __forceinline__ int reflect_in(int r, int n) {        // r >= 0 expected; the clamp only holds a broken plan inside
  const int m = r < n ? r : 2 * (n - 1) - r;
  return m < 0 ? 0 : (m < n ? m : n - 1);
}

__global__ __launch_bounds__(kThreads) void image_ingest_tiles_kernel(const uint8_t* __restrict__ img, const float* __restrict__ table,
                                                                      const int* __restrict__ origins, float* __restrict__ x, int h,
                                                                      int w, int th, int tw, int G) {
  __shared__ float tab[256];
  tab[threadIdx.x] = table ? table[threadIdx.x] : (float)threadIdx.x / 255.0f;
  const long t = blockIdx.y;
  const int y0 = max(origins[2 * t], 0), x0 = max(origins[2 * t + 1], 0);
  const long plane = (long)th * tw;
  float* xt = x + t * 3 * plane;
  __syncthreads();

  const int items = th * G;
  const int first = blockIdx.x * (kThreads * kGroups) + threadIdx.x;
  uint32_t d[kGroups][3];                                        // as in image_ingest_kernel
  bool on[kGroups];
  long dst[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const int it = first + k * kThreads;
    on[k] = it < items;
    if (!on[k]) continue;
    const int i = it / G, j = 4 * (it - i * G);
    const uint8_t* row = img + (long)reflect_in(y0 + i, h) * w * 3;
    const int gj = x0 + j;
    dst[k] = (long)i * tw + j;
    if (gj + 4 <= w) {                                           // 12 consecutive bytes inside the row
      const uint8_t* p = row + 3L * gj;
      d[k][0] = ld32u(p);
      d[k][1] = ld32u(p + 4);
      d[k][2] = ld32u(p + 8);
    } else {                                                     // the reflected columns: pixel by pixel, byte by byte
      uint32_t by[12];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint8_t* p = row + 3L * reflect_in(gj + m, w);
#pragma unroll
        for (int c = 0; c < 3; ++c) by[3 * m + c] = (uint32_t)p[c];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) d[k][q] = by[4 * q] | (by[4 * q + 1] << 8) | (by[4 * q + 2] << 16) | (by[4 * q + 3] << 24);
    }
  }
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    if (!on[k]) continue;
    const uint32_t d0 = d[k][0], d1 = d[k][1], d2 = d[k][2];
    const uint32_t px[3][4] = {{d0 & 255u, d0 >> 24, (d1 >> 16) & 255u, (d2 >> 8) & 255u},
                               {(d0 >> 8) & 255u, d1 & 255u, d1 >> 24, (d2 >> 16) & 255u},
                               {(d0 >> 16) & 255u, (d1 >> 8) & 255u, d2 & 255u, d2 >> 24}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 r = {tab[px[c][0]], tab[px[c][1]], tab[px[c][2]], tab[px[c][3]]};
      store4u(xt + c * plane + dst[k], r);
    }
  }
}

// first k in [0, n) with o[k] + t > p (o ascending); n when there is none
__device__ __forceinline__ int first_cover(const int* o, int n, int t, int p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (o[mid] + t > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ float clamp01(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }      // NaN -> 0, as quant

__global__ __launch_bounds__(kThreads) void image_egress_tiles_kernel(const float* __restrict__ tiles, const int* __restrict__ origins_y,
                                                                      int ny, const int* __restrict__ origins_x, int nx,
                                                                      const float* __restrict__ wy, const float* __restrict__ wx,
                                                                      uint8_t* __restrict__ dst, int h, int w, int th, int tw, int G) {
  __shared__ int oy[kMaxOrigins], ox[kMaxOrigins];
  for (int k = threadIdx.x; k < ny; k += kThreads) oy[k] = origins_y[k];
  for (int k = threadIdx.x; k < nx; k += kThreads) ox[k] = origins_x[k];
  __syncthreads();
  const int it = blockIdx.x * kThreads + threadIdx.x;
  if (it >= h * G) return;
  const int y = it / G, x = 4 * (it - y * G);
  const int n = w - x < 4 ? w - x : 4;
  const long plane = (long)th * tw;

  float acc[3][4], one[3][4], den[4];
  int cnt[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    den[m] = 0.f;
    cnt[m] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c][m] = one[c][m] = 0.f;
  }
  const int kx0 = first_cover(ox, nx, tw, x);
  for (int ky = first_cover(oy, ny, th, y); ky < ny && oy[ky] <= y; ++ky) {
    const int ty = y - oy[ky];
    if ((unsigned)ty >= (unsigned)th) continue;
    const float a = wy[(long)ky * th + ty];
    for (int kx = kx0; kx < nx && ox[kx] <= x + 3; ++kx) {
      const int tx = x - ox[kx];                                 // of the group's first pixel; -3 .. tw - 1
      const float* p = tiles + ((long)ky * nx + kx) * 3 * plane + (long)ty * tw + tx;
      const float* b = wx + (long)kx * tw + tx;
      f32x4 v[3], bw;
      bool in[4];
      if (tx >= 0 && tx + 4 <= tw) {                             // the whole group inside the tile: 16 bytes per plane
        bw = load4u(b);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = load4u(p + c * plane);
#pragma unroll
        for (int m = 0; m < 4; ++m) in[m] = true;
      } else {                                                   // the group straddles the tile's edge: pixel by pixel
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          in[m] = (unsigned)(tx + m) < (unsigned)tw && m < n;
          bw[m] = in[m] ? b[m] : 0.f;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][m] = in[m] ? p[c * plane + m] : 0.f;
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (!in[m]) continue;
        const float g = a * bw[m];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float cl = clamp01(v[c][m]);
          if (cnt[m] == 0) one[c][m] = cl;
          acc[c][m] += g * cl;
        }
        den[m] += g;
        ++cnt[m];
      }
    }
  }
  uint32_t by[12];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int c = 0; c < 3; ++c) by[3 * m + c] = quant(cnt[m] == 1 ? one[c][m] : (cnt[m] ? acc[c][m] / den[m] : 0.f));
  uint8_t* o = dst + ((long)y * w + x) * 3;
  if (n == 4) {
#pragma unroll
    for (int q = 0; q < 3; ++q) st32u(o + 4 * q, by[4 * q] | (by[4 * q + 1] << 8) | (by[4 * q + 2] << 16) | (by[4 * q + 3] << 24));
  } else {
#pragma unroll
    for (int m = 0; m < 9; ++m)
      if (m < 3 * n) o[m] = (uint8_t)by[m];
  }
}

// grid.x blocks for `rows` rows of G groups; 0 when the launch would not fit
inline long grid_x(long rows, long G) {
  const long items = rows * G;
  return items > (1L << 30) ? 0 : (items + kThreads * kGroups - 1) / (kThreads * kGroups);
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_image_ingest(const uint8_t* src, long src_bs, const float* table, float* x, int B, int h, int w, int Hp, int Wp,
                        void* stream) {
  CIDNET_CHECK_ARG(src && x && B > 0 && h > 0 && w > 0 && Hp > 0 && Wp > 0);
  if (Hp < h || Wp < w || Hp - h > h - 1 || Wp - w > w - 1) return CIDNET_ERR_SHAPE;     // reflection: pad < side
  if (src_bs < 3L * h * w || B > 65535) return CIDNET_ERR_SHAPE;
  const long G = ((long)Wp + 3) / 4;
  const long gx = grid_x(Hp, G);
  if (gx == 0) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(image_ingest_kernel, dim3((unsigned)gx, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, src, src_bs,
                     table, x, h, w, Hp, Wp, (int)G);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_image_egress(const float* x, uint8_t* dst, long dst_bs, int B, int Hp, int Wp, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(x && dst && B > 0 && h > 0 && w > 0 && Hp > 0 && Wp > 0);
  if (h > Hp || w > Wp) return CIDNET_ERR_SHAPE;
  if (dst_bs < 3L * h * w || B > 65535) return CIDNET_ERR_SHAPE;
  const long G = ((long)w + 3) / 4;
  const long gx = grid_x(h, G);
  if (gx == 0) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(image_egress_kernel, dim3((unsigned)gx, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, x, dst, dst_bs,
                     Hp, Wp, h, w, (int)G);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_image_ingest_tiles(const uint8_t* src, int h, int w, const float* table, const int* origins, float* x, int n, int th,
                              int tw, void* stream) {
  CIDNET_CHECK_ARG(src && origins && x && h > 0 && w > 0 && n > 0 && th > 0 && tw > 0);
  if (th % 4 || tw % 4 || n > 65535) return CIDNET_ERR_SHAPE;
  const long G = tw / 4;
  const long gx = grid_x(th, G);
  if (gx == 0) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(image_ingest_tiles_kernel, dim3((unsigned)gx, (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, src, table,
                     origins, x, h, w, th, tw, (int)G);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_image_egress_tiles(const float* tiles, const int* origins_y, int ny, const int* origins_x, int nx, const float* wy,
                              const float* wx, uint8_t* dst, int h, int w, int th, int tw, void* stream) {
  CIDNET_CHECK_ARG(tiles && origins_y && origins_x && wy && wx && dst && ny > 0 && nx > 0 && h > 0 && w > 0 && th > 0 && tw > 0);
  if (th % 4 || tw % 4 || ny > kMaxOrigins || nx > kMaxOrigins) return CIDNET_ERR_SHAPE;
  const long G = ((long)w + 3) / 4;
  const long items = (long)h * G;
  if (items > (1L << 30)) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(image_egress_tiles_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, tiles, origins_y, ny, origins_x, nx, wy, wx, dst, h, w, th, tw, (int)G);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
