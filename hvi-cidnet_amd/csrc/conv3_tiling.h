// Host-side launch plans of the 3x3 convolution family, shared by the launchers and by the tiling query
// cidnet_conv3x3_tiling (conv3.hip): each plan is computed once, by the function its launcher calls.
#pragma once

namespace cidnet {

// conv3_thin.hip: the streaming forward kernels (M <= 4: the "m" kernel, else K <= 4: the "k" kernel)
struct C3ThinPlan {
  int kside;          // 0: c3_thin_m_kernel, 1: c3_thin_k_kernel
  int rows;           // strip height
  int nx4, nstrips;
  long lds_bytes;     // dynamic LDS of the launch
};
C3ThinPlan c3_thin_plan(int M, int K, int H, int W);
// the weight-gradient kernels' strips (16 rows) of a plane
void c3_thin_wgrad_strips(int H, int W, int* rows, int* nstrips);

// conv3x.hip: the persistent bf16x3 forward / data-gradient kernel with x_levels activation levels
struct C3xPlan {
  int tiles_x, tiles_y, mchunks, kchunks;
  long nwork, nblk;
};
C3xPlan c3x_plan(int B, int M, int K, int H, int W, int x_levels);

// conv3xw.hip: the persistent bf16x3 weight-gradient kernel
struct C3xwPlan {
  int pairs, nblk, tiles_x, tiles_y;
  long ntiles;
};
C3xwPlan c3xw_plan(int B, int M, int N, int H, int W);

}  // namespace cidnet
