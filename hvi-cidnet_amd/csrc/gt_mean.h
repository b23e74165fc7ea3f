// The "GT mean" rescale of the paired metrics (measure.py:138-141): what csrc/metrics.hip, csrc/lpips.hip and
// csrc/ciede2000.hip share.  The scale itself, s = mean(gray(gt)) / mean(gray(restored)), is formed once per pair by
// cidnet_metric_gt_mean_scale (csrc/metrics.hip); every user reads it from the caller's B doubles.
#pragma once
#include <hip/hip_runtime.h>

namespace cidnet {

// the BT.601 fixed-point gray of an 8-bit pixel
__device__ __forceinline__ unsigned gray601(unsigned r, unsigned g, unsigned b) {
  return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}

// clip(a * s, 0, 255) in fp64 (a NaN scale -- an all-black restored image -- propagates as np.clip does).  One multiply and
// two compares: nothing a compiler could contract, so the same bits with and without -ffp-contract=off.
__device__ __forceinline__ double gt_mean_value(unsigned a, double s) {
  const double v = (double)a * s;
  return v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
}

}  // namespace cidnet
