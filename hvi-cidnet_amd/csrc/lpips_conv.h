// What the LPIPS forward (csrc/lpips.hip) and the backward of its training loss (csrc/lpips_loss.hip) share: the distance
// kernels' thread layout, the streaming kernels' grid rule, and the implicit-GEMM convolution of the extractor, which the
// forward and the stride-1 data gradients both run: D[m][n] = sum_k W[m][k] X[k][n] with k = (c, ky, kx) and n a
// pixel of one image, on the fp32 matrix cores (v_mfma_f32_32x32x2f32: fp32 products, fp32 accumulation).  A block of four
// waves owns 64 output channels x 64 pixels; K goes by in chunks of 64: the weight chunk and the im2col chunk are loaded
// into registers one chunk ahead and staged in LDS, zeros standing for the padding, for k >= K and for pixels past the
// image's last -- no address outside the tensors is ever formed into a load.  The stride sits in the staging's address
// arithmetic (input row = S oy - PAD + ky).  A block works on one image and its tiling is relative to that image, so an
// image's result does not depend on the rest of the batch.  Only the epilogue differs between the users:
//   kEpiBiasRelu: y = relu(acc + e0[m])                       e0 = the bias (M); the forward
//   kEpiPlain:    y = acc                                     a data gradient whose consumer is a pool backward
//   kEpiMaskAdd:  y = e0 > 0 ? acc + e1 : 0                   e0 = the post-ReLU tap y is the gradient of (its ReLU mask),
//                                                             e1 = that tap's distance gradient; both shaped like y
// A stride-1 data gradient is this convolution of dy with the spatially flipped weights, M and C exchanged, same padding.
#pragma once
#include "common.h"

namespace cidnet {
namespace {

constexpr int kMT = 64, kNT = 64, kKC = 64;                   // block tile: out channels x pixels; K chunk
constexpr int kLdA = kMT + 1, kLdB = kNT + 32;                 // LDS row strides (floats) of the [k][m] and [k][n] chunks
constexpr int kConvThreads = 256;
constexpr int kARows = kConvThreads / kKC;                     // weight rows one staging pass covers
constexpr int kAIter = kMT / kARows, kBIter = kKC / 4;         // staged values per thread and chunk: weights, im2col
constexpr int kEpiBiasRelu = 0, kEpiPlain = 1, kEpiMaskAdd = 2;
// the distance kernels' layout, forward and backward: kDistPix pixels a block, kDistGroups threads a pixel
constexpr int kDistThreads = 256, kDistPix = 32, kDistGroups = kDistThreads / kDistPix;

inline int grid_for(long n, int cap) {
  long g = (n + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// y[b][m][oy][ox] = epilogue(sum_{c,ky,kx} w[m][c][ky][kx] x[b][c][S oy - PAD + ky][S ox - PAD + kx]), zeros outside x.
// grid: (pixel tiles, M / 64, B).  Waves 0..3 own the (32 m) x (32 n) quarters of the tile.
template <int KH, int S, int PAD, int EPI>
__global__ __launch_bounds__(kConvThreads) void lpips_conv_kernel(const float* __restrict__ x, const float* __restrict__ wgt,
                                                                  const float* __restrict__ e0, const float* __restrict__ e1,
                                                                  float* __restrict__ y, int M, int C, int H, int W, int Ho, int Wo) {
  __shared__ float As[kKC * kLdA];
  __shared__ float Bs[kKC * kLdB];
  constexpr int KK = KH * KH;
  const int K = C * KK;
  const int P = Ho * Wo;
  const int b = blockIdx.z, m0 = blockIdx.y * kMT, p0 = blockIdx.x * kNT;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
  // im2col staging: this thread's pixel is fixed, its k runs over kb, kb + 4, ...
  const int n = t & 63, kb = t >> 6;
  const int p = p0 + n;
  const bool pin = p < P;
  const int oy = pin ? p / Wo : 0, ox = pin ? p - oy * Wo : 0;
  const int iy0 = oy * S - PAD, ix0 = ox * S - PAD;
  const float* xb = x + (long)b * C * H * W;
  // weight staging: consecutive lanes read consecutive k of one row
  const int ak = t % kKC, am = t / kKC;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // the chunk after the one in LDS waits in registers: its loads are in flight while the matrix cores work
  float ra[kAIter], rb[kBIter];
  auto fetch = [&](int k0) {
    const bool ak_in = k0 + ak < K;
#pragma unroll
    for (int i = 0; i < kAIter; ++i) ra[i] = ak_in ? wgt[(long)(m0 + am + kARows * i) * K + k0 + ak] : 0.f;
#pragma unroll
    for (int i = 0; i < kBIter; ++i) {
      const int kk = k0 + kb + 4 * i;
      const int c = kk / KK;
      const int r = kk - c * KK;
      const int ky = r / KH;
      const int kx = r - ky * KH;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = pin && kk < K && iy >= 0 && iy < H && ix >= 0 && ix < W;
      rb[i] = ok ? xb[((long)c * H + iy) * W + ix] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kKC) {
#pragma unroll
    for (int i = 0; i < kAIter; ++i) As[ak * kLdA + am + kARows * i] = ra[i];
#pragma unroll
    for (int i = 0; i < kBIter; ++i) Bs[(kb + 4 * i) * kLdB + n] = rb[i];
    __syncthreads();
    if (k0 + kKC < K) fetch(k0 + kKC);
    const float* ap = As + (lane >> 5) * kLdA + wm + (lane & 31);
    const float* bp = Bs + (lane >> 5) * kLdB + wn + (lane & 31);
#pragma unroll
    for (int k = 0; k < kKC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k * kLdA], bp[k * kLdB], acc, 0, 0, 0);
    __syncthreads();
  }
  // D[i][j]: j = lane % 32, i = 8 (r / 4) + 4 (lane / 32) + r % 4
  const int pj = p0 + wn + (lane & 31);
  if (pj < P) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
      const long o = ((long)b * M + m) * P + pj;
      if (EPI == kEpiBiasRelu) {
        const float v = acc[r] + e0[m];
        y[o] = v > 0.f ? v : 0.f;
      } else if (EPI == kEpiPlain) {
        y[o] = acc[r];
      } else {
        y[o] = e0[o] > 0.f ? acc[r] + e1[o] : 0.f;
      }
    }
  }
}

template <int KH, int S, int PAD, int EPI>
int launch_conv(const float* x, const float* w, const float* e0, const float* e1, float* y, int B, int M, int C, int H, int W, int Ho,
                int Wo, hipStream_t st) {
  const dim3 grid((unsigned)(((long)Ho * Wo + kNT - 1) / kNT), (unsigned)(M / kMT), (unsigned)B);
  hipLaunchKernelGGL((lpips_conv_kernel<KH, S, PAD, EPI>), grid, dim3(kConvThreads), 0, st, x, w, e0, e1, y, M, C, H, W, Ho, Wo);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // namespace
}  // namespace cidnet
