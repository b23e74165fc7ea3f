// Training batches from a resident uint8 set: what the reference's data/data.py transform1 (RandomCrop, RandomHorizontalFlip,
// RandomVerticalFlip, ToTensor) and train.py:54-56 (im1 ** gamma) do per sample on the host, as one launch per batch.
//   yy = y0 + (vflip ? S_h-1-i : i)        xx = x0 + (hflip ? S_w-1-j : j)
//   gt[s,c,i,j] = fp32(high[c,yy,xx]) / 255.0f                 (a correctly rounded fp32 division: ToTensor's .div(255))
//   x [s,c,i,j] = table[low[c,yy,xx]]                          (table = pow(q / 255, gamma) per level, built by the caller in
//                                                               fp64 and rounded once; NULL: the quotient itself)
// The set is one uint8 arena of planar (3,h,w) images; sample s reads plan row s (8 x int64: byte offset of the low image,
// byte offset of its ground truth, h, w, y0, x0, flips (bit 0 horizontal, bit 1 vertical), 0).  The row is wave-uniform
// (blockIdx.y = s * 3 + c), so it arrives through scalar loads.
//
// A pixel has 256 possible values, so both conversions are 256-entry tables in LDS: the quotients are formed once per block
// (one division per thread), the gamma table is copied from the caller's 1 KiB.  A lane owns 4 consecutive output pixels of
// one row: one 4-byte load per image at an arbitrary byte address (the crop window starts anywhere; gfx950 runs global
// memory in unaligned access mode), a byte swap under hflip, 8 LDS lookups, two 16-byte stores.  Consecutive lanes own
// consecutive groups, so a wave writes 1 KiB of contiguous output per store.  The last group of a row whose width is not a
// multiple of 4 reads and writes its 1-3 pixels one by one: no byte outside the crop window is ever touched, so a window that
// ends at the arena's last byte (or starts at its first, mirrored) is safe.  No atomics, no reductions: a value depends on its
// plan row alone.
//
// crop_flip_kernel<true> (cidnet_augment_crop_flip_raw) also writes the low image WITHOUT the power, raw = low / 255, which
// the reference's train_tnsm.py:55,68 keeps beside `im1 ** gamma` for its noise-consistency term: the low image's bytes are
// still loaded once per group, each byte is looked up in both tables, and a group issues three 16-byte stores --
// 2 + 12 bytes per output pixel where two launches of the plain kernel move 2 * (2 + 8).  crop_flip_kernel<false> is the
// plain kernel, instruction for instruction what it was before the template.
#include "common.h"
#include "cidnet_hip.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kGroups = 2;                                       // 4-pixel groups per thread: both loads fly before the first store
constexpr int kPlanWords = 8;

struct __attribute__((packed, aligned(1))) u32u {
  uint32_t v;
};

__device__ __forceinline__ uint32_t load4b(const uint8_t* p, int n) {      // bytes p[0..n-1], little-endian, upper bytes 0
  if (n == 4) return reinterpret_cast<const u32u*>(p)->v;
  uint32_t v = 0;
  for (int m = 0; m < n; ++m) v |= (uint32_t)p[m] << (8 * m);
  return v;
}

__device__ __forceinline__ void lookup_store(float* o, const float* tab, uint32_t v, int n) {
  if (n == 4) {
    const f32x4 r = {tab[v & 255u], tab[(v >> 8) & 255u], tab[(v >> 16) & 255u], tab[v >> 24]};
    store4u(o, r);
  } else {
    for (int m = 0; m < n; ++m) o[m] = tab[(v >> (8 * m)) & 255u];
  }
}

template <bool kRaw>
__global__ __launch_bounds__(kThreads) void crop_flip_kernel(const uint8_t* __restrict__ arena, const long* __restrict__ plan,
                                                             const float* __restrict__ table, float* __restrict__ x,
                                                             float* __restrict__ gt, int Sh, int Sw, int G,
                                                             float* __restrict__ raw) {
  __shared__ float tq[256], tx[256];
  {
    const float q = (float)threadIdx.x / 255.0f;
    tq[threadIdx.x] = q;
    tx[threadIdx.x] = table ? table[threadIdx.x] : q;
  }
  const int plane = blockIdx.y;                                  // s * 3 + c
  const int s = plane / 3, c = plane - 3 * s;
  const long* row = plan + (long)s * kPlanWords;
  const long lo = row[0], hi = row[1];
  const int h = (int)row[2], w = (int)row[3], y0 = (int)row[4], x0 = (int)row[5], flips = (int)row[6];
  const bool hflip = (flips & 1) != 0, vflip = (flips & 2) != 0;
  const long chan = (long)c * h * w;
  const uint8_t* plo = arena + lo + chan;
  const uint8_t* phi = arena + hi + chan;
  float* ox = x + (long)plane * Sh * Sw;
  float* og = gt + (long)plane * Sh * Sw;
  __syncthreads();

  const int items = Sh * G;
  const int first = blockIdx.x * (kThreads * kGroups) + threadIdx.x;
  uint32_t a[kGroups], b[kGroups];
  int n[kGroups];
  long dst[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const int it = first + k * kThreads;
    n[k] = 0;
    if (it >= items) continue;
    const int i = it / G, j = 4 * (it - i * G);
    n[k] = Sw - j < 4 ? Sw - j : 4;
    const int yy = y0 + (vflip ? Sh - 1 - i : i);
    const int xs = x0 + (hflip ? Sw - j - n[k] : j);             // first source byte of the group's n pixels
    const long src = (long)yy * w + xs;
    dst[k] = (long)i * Sw + j;
    a[k] = load4b(plo + src, n[k]);
    b[k] = load4b(phi + src, n[k]);
  }
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    if (n[k] == 0) continue;
    if (hflip) {                                                 // output pixel m of the group is source byte n-1-m
      a[k] = __builtin_bswap32(a[k]) >> (8 * (4 - n[k]));
      b[k] = __builtin_bswap32(b[k]) >> (8 * (4 - n[k]));
    }
    lookup_store(ox + dst[k], tx, a[k], n[k]);
    if constexpr (kRaw) lookup_store(raw + (long)plane * Sh * Sw + dst[k], tq, a[k], n[k]);
    lookup_store(og + dst[k], tq, b[k], n[k]);
  }
}

template <bool kRaw>
int launch_crop_flip(const uint8_t* arena, const long* plan, const float* table, float* x, float* raw, float* gt, int B, int Sh,
                     int Sw, void* stream) {
  const long G = ((long)Sw + 3) / 4;
  const long items = (long)Sh * G;
  if ((long)B * 3 > 65535 || items > (1L << 30)) return CIDNET_ERR_SHAPE;
  const dim3 grid((unsigned)((items + kThreads * kGroups - 1) / (kThreads * kGroups)), (unsigned)(B * 3));
  hipLaunchKernelGGL(crop_flip_kernel<kRaw>, grid, dim3(kThreads), 0, (hipStream_t)stream, arena, plan, table, x, gt, Sh, Sw,
                     (int)G, raw);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_augment_crop_flip(const uint8_t* arena, const long* plan, const float* table, float* x, float* gt, int B, int Sh,
                             int Sw, void* stream) {
  CIDNET_CHECK_ARG(arena && plan && x && gt && B > 0 && Sh > 0 && Sw > 0);
  return launch_crop_flip<false>(arena, plan, table, x, nullptr, gt, B, Sh, Sw, stream);
}

int cidnet_augment_crop_flip_raw(const uint8_t* arena, const long* plan, const float* table, float* x, float* raw, float* gt,
                                 int B, int Sh, int Sw, void* stream) {
  CIDNET_CHECK_ARG(arena && plan && x && raw && gt && B > 0 && Sh > 0 && Sw > 0);
  return launch_crop_flip<true>(arena, plan, table, x, raw, gt, B, Sh, Sw, stream);
}

}  // extern "C"
