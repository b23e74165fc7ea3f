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

}  // extern "C"
