// The front end of a baseline JPEG in libjpeg's own 32-bit fixed point, shared by the file round trip (csrc/jpeg.hip) and the
// encoder (csrc/jpegenc.hip): colour conversion (jccolor.c), the "islow" forward DCT (jfdctint.c) and the exact-division
// quantiser.  Integer arithmetic only; tests/jpeg_ref.py restates every line.
#pragma once
#include "common.h"

namespace cidnet {
namespace jpegfe {

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// RGB -> Y and the UNROUNDED-to-plane Cb, Cr of one pixel (each 0..255)
__device__ __forceinline__ void ycc(int r, int g, int b, int* y, int* cb, int* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// libjpeg jfdctint.c, one pass over d[0..7]: kFirst -- the row pass (scaled up by 2^2), else the column pass
template <bool kFirst>
__device__ __forceinline__ void fdct8(int* d) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = kFirst ? 11 : 15;
  d[0] = kFirst ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4] = kFirst ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  const int e = (t12 + t13) * 4433;
  d[2] = descale(e + t13 * 6270, n);
  d[6] = descale(e - t12 * 15137, n);
  const int z5 = (t4 + t6 + t5 + t7) * 9633;
  const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
  d[7] = descale(t4 * 2446 + z1 + z3, n);
  d[5] = descale(t5 * 16819 + z2 + z4, n);
  d[3] = descale(t6 * 25172 + z2 + z3, n);
  d[1] = descale(t7 * 12299 + z1 + z4, n);
}

// sign(v) ((|v| + 4 t) / (8 t)), m = ceil(2^32 / (8 t)).  |v| + 4 t < 2^16 (an 8 x 8 DCT of bytes, scaled by 8, stays below
// 2^15), and for a numerator below 2^16 and a divisor below 2^11 the high word of n * ceil(2^32 / d) is n / d exactly (n d < 2^32).
__device__ __forceinline__ int quantise(int v, int t, unsigned m) {
  const int q = (int)__umulhi((unsigned)((v < 0 ? -v : v) + 4 * t), m);
  return v < 0 ? -q : q;
}

}  // namespace jpegfe
}  // namespace cidnet
