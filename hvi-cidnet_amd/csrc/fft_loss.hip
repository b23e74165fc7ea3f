// Frequency-domain training loss (include/cidnet_hip.h, "frequency-domain training loss"):
//   loss = weight s / (2 P H Wh) sum (|Re D| + |Im D|),  D = rfft2(a - b),  Wh = W / 2 + 1,  s = 1 or 1 / sqrt(H W),
// with the transform of each axis as a GEMM against a twiddle table on the fp32 matrix cores (v_mfma_f32_32x32x2f32: fp32
// products, fp32 accumulation), so any H x W goes through the same code: no radix, no size restriction up to 2048 a side.
//
// The tables (dft_table_kernel) hold e^{-2 pi i n k / N} = (c, s') = (cos, -sin) as fp32 pairs, (N, Nk, 2), from an fp64 sincospi
// of the integer-reduced angle.  With them, for one plane d (H x W) and j = 2 kx + part the interleaved (re, im) column:
//   (a) row forward     R  (P H x 2 Wh) = d (P H x W)       . Tw (W x 2 Wh)        Tw = tab_w read as a row-major matrix
//   (b) column forward  D  (H x 2 Wh)   = Th (H x 2 H)      . rot+(R) (2 H x 2 Wh) Th = tab_h read as a row-major matrix (it is
//   (c) column adjoint  G  (H x 2 Wh)   = Th (H x 2 H)      . rot-(S) (2 H x 2 Wh)      symmetric in (y, ky)); per plane
//   (d) row adjoint     g  (P H x W)    = G (P H x 2 Wh)    . Tw^T (2 Wh x W)
// rot+(X)[2 y + 0][j] = X[y][j];  rot+(X)[2 y + 1][(kx, 0)] = -X[y][kx][1],  rot+(X)[2 y + 1][(kx, 1)] = X[y][kx][0]: the real form
// of (c + i s')(Xr + i Xi).  rot- has the signs of its odd rows exchanged: the real form of the transposed map, which is (c) because
// loss = sum sr Dr + si Di locally and Dr = c Rr - s' Ri, Di = c Ri + s' Rr.
//
// One kernel template runs all four, built like lpips_conv_kernel (csrc/lpips_conv.h): a block of four waves owns a 64 x 64
// tile, K goes by in chunks of 64, the next chunk waits in registers while the matrix cores work on the one in LDS, zeros
// stand for everything past an edge, and no address outside a tensor is ever formed into a load.  A thread accumulates its
// tile entries over k = 0, 1, 2, ... in order, two k a matrix instruction.  No atomics anywhere: (b) leaves one fp64 partial per
// block in a fixed slot and one block sums the slots in a fixed order, so two calls on the same input are bit-identical.
#include "cidnet_hip.h"
#include "common.h"

#include <cmath>

namespace cidnet {
namespace {

constexpr int kMT = 64, kNT = 64, kKC = 64;                    // block tile (rows x columns of the product) and K chunk
constexpr int kLdA = kMT + 1;                                  // LDS row stride (floats) of the [k][m] chunk
constexpr int kLdB = kNT + 32, kLdBT = kNT + 1;                // of the [k][n] chunk: staged along n / along k (kBTabT)
constexpr int kThreads = 256;
constexpr int kIter = kMT * kKC / kThreads;                    // staged values per thread, chunk and operand
constexpr int kMaxSide = 2048;

// how B[k][n] is read: a row-major (K x N) table, the same table transposed, rot+ / rot- of a (planes, K / 2, N) tensor
constexpr int kBTab = 0, kBTabT = 1, kBRotFwd = 2, kBRotAdj = 3;
// what happens to the tile: stored; |.| summed into the block's partial (and its signs stored when wanted); scaled into ga / -gb
constexpr int kEpiStore = 0, kEpiAbs = 1, kEpiGrad = 2;

struct GemmArgs {
  const float* a;      // A[m][k] = a[z a_zs + m K + k] - (a2 ? a2[the same] : 0)
  const float* a2;
  long a_zs;
  const float* b;      // see kB*; the rot forms add z b_zs
  long b_zs;
  float* out;          // kEpiStore / kEpiAbs (may be NULL there) / kEpiGrad (ga, may be NULL): out[z o_zs + m N + n]
  float* out2;         // kEpiGrad: gb = -ga, may be NULL
  long o_zs;
  double* part;        // kEpiAbs: one slot per block, (z, y, x) order
  const float* gup;    // kEpiGrad: device scalar or NULL (= 1)
  float scale;         // kEpiGrad: the host constant
  int M, N, K;
};

// grid: (M tiles, N tiles, planes).  Waves 0..3 own the (32 m) x (32 n) quarters of the tile.
template <int BMODE, int EPI>
__global__ __launch_bounds__(kThreads) void dft_gemm_kernel(GemmArgs g) {
  __shared__ float As[kKC * kLdA];
  __shared__ float Bs[kKC * kLdB];
  __shared__ double red[kThreads / 64];
  constexpr int ldb = BMODE == kBTabT ? kLdBT : kLdB;
  const int M = g.M, N = g.N, K = g.K;
  const int z = blockIdx.z, m0 = blockIdx.x * kMT, n0 = blockIdx.y * kNT;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
  const int lo = t & 63, hi = t >> 6;                          // staging: lo runs along the contiguous index of the source
  const float* ap = g.a + (long)z * g.a_zs;
  const float* ap2 = g.a2 ? g.a2 + (long)z * g.a_zs : nullptr;
  const float* bp0 = (BMODE == kBRotFwd || BMODE == kBRotAdj) ? g.b + (long)z * g.b_zs : g.b;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // the chunk after the one in LDS waits in registers: its loads are in flight while the matrix cores work
  float ra[kIter], rb[kIter];
  auto fetch = [&](int k0) {
    {
      const int k = k0 + lo;                                   // consecutive lanes read consecutive k of one row of A
#pragma unroll
      for (int i = 0; i < kIter; ++i) {
        const int m = m0 + hi + 4 * i;
        float v = 0.f;
        if (k < K && m < M) {
          const long o = (long)m * K + k;
          v = ap[o];
          if (ap2) v -= ap2[o];
        }
        ra[i] = v;
      }
    }
    if (BMODE == kBTabT) {
      const int k = k0 + lo;                                   // B[k][n] = b[n K + k]: consecutive lanes, consecutive k
#pragma unroll
      for (int i = 0; i < kIter; ++i) {
        const int n = n0 + hi + 4 * i;
        rb[i] = (k < K && n < N) ? bp0[(long)n * K + k] : 0.f;
      }
    } else {
      const int n = n0 + lo;                                   // consecutive lanes, consecutive n
#pragma unroll
      for (int i = 0; i < kIter; ++i) {
        const int k = k0 + hi + 4 * i;
        float v = 0.f;
        if (k < K && n < N) {
          if (BMODE == kBTab) {
            v = bp0[(long)k * N + n];
          } else if (!(k & 1)) {
            v = bp0[(long)(k >> 1) * N + n];
          } else {                                             // N is even: n ^ 1 < N with n
            v = bp0[(long)(k >> 1) * N + (n ^ 1)];
            if (((n & 1) == 0) == (BMODE == kBRotFwd)) v = -v;
          }
        }
        rb[i] = v;
      }
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kKC) {
#pragma unroll
    for (int i = 0; i < kIter; ++i) As[lo * kLdA + hi + 4 * i] = ra[i];
    if (BMODE == kBTabT) {
#pragma unroll
      for (int i = 0; i < kIter; ++i) Bs[lo * ldb + hi + 4 * i] = rb[i];
    } else {
#pragma unroll
      for (int i = 0; i < kIter; ++i) Bs[(hi + 4 * i) * ldb + lo] = rb[i];
    }
    __syncthreads();
    if (k0 + kKC < K) fetch(k0 + kKC);
    const float* fa = As + (lane >> 5) * kLdA + wm + (lane & 31);
    const float* fb = Bs + (lane >> 5) * ldb + wn + (lane & 31);
#pragma unroll
    for (int k = 0; k < kKC; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[k * kLdA], fb[k * ldb], acc, 0, 0, 0);
    __syncthreads();
  }
  // D[i][j]: j = lane % 32, i = 8 (r / 4) + 4 (lane / 32) + r % 4
  const int n = n0 + wn + (lane & 31);
  const int mb = m0 + wm + (lane >> 5) * 4;
  float* o1 = g.out ? g.out + (long)z * g.o_zs : nullptr;
  if (EPI == kEpiStore) {
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r >> 2) * 8 + (r & 3);
        if (m < M) o1[(long)m * N + n] = acc[r];
      }
    }
  } else if (EPI == kEpiAbs) {
    float s = 0.f;                                             // fp32 within the lane, fp64 from here on
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mb + (r >> 2) * 8 + (r & 3);
      if (n < N && m < M) {
        const float v = acc[r];
        s += fabsf(v);
        if (o1) o1[(long)m * N + n] = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
      }
    }
    const double ws = wave_sum_f64((double)s);
    if (lane == 0) red[wv] = ws;
    __syncthreads();
    if (t == 0) g.part[((long)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  } else {
    float* o2 = g.out2 ? g.out2 + (long)z * g.o_zs : nullptr;
    const float f = g.gup ? g.scale * g.gup[0] : g.scale;
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r >> 2) * 8 + (r & 3);
        if (m < M) {
          const float v = acc[r] * f;
          if (o1) o1[(long)m * N + n] = v;
          if (o2) o2[(long)m * N + n] = -v;
        }
      }
    }
  }
}

// table[(n Nk + k) 2 + {0, 1}] = (cos, -sin)(2 pi m / N), m = n k mod N reduced in integers; fp64, rounded once.  2 m / N is a
// multiple of 1/2 exactly where 4 m is a multiple of N, and sincospi is exact there: 0 and +-1 come out as such.
__global__ __launch_bounds__(256) void dft_table_kernel(int N, int Nk, float* __restrict__ table) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * Nk) return;
  const int n = (int)(i / Nk), k = (int)(i - (long)n * Nk);
  const long m = ((long)n * k) % N;
  double s, c;
  sincospi(2.0 * (double)m / (double)N, &s, &c);
  table[2 * i] = (float)c;
  table[2 * i + 1] = (float)(-s);
}

// one block: thread t adds slots t, t + 256, ... in that order onto 0.0, then the butterfly of each wave and the four waves in order
__global__ __launch_bounds__(256) void fft_loss_finish_kernel(const double* __restrict__ part, long n, double scale, float* __restrict__ loss) {
  __shared__ double red[4];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) * scale);
}

struct Plan {
  int Wh, N2;            // W / 2 + 1 and the interleaved width 2 Wh
  int ga[3], gb[3], gc[3], gd[3];
  long parts, scratch;   // fp64 partials of (b); floats of R (forward) or G (backward) behind them
  long ws_floats;
};

inline int tiles(long n, int t) { return (int)((n + t - 1) / t); }

// CIDNET_OK and the plan, or the error the entry points return for the shape
int make_plan(int P, int H, int W, Plan& p) {
  if (P < 1 || H < 1 || W < 1) return CIDNET_ERR_ARG;
  if (H > kMaxSide || W > kMaxSide || P > 65535) return CIDNET_ERR_SHAPE;
  p.Wh = W / 2 + 1;
  p.N2 = 2 * p.Wh;
  const long rows = (long)P * H;
  if (rows * p.N2 > 0x7fffffffL || rows * W > 0x7fffffffL) return CIDNET_ERR_SHAPE;
  const int a[3] = {tiles(rows, kMT), tiles(p.N2, kNT), 1}, b[3] = {tiles(H, kMT), tiles(p.N2, kNT), P},
            d[3] = {tiles(rows, kMT), tiles(W, kNT), 1};
  for (int i = 0; i < 3; ++i) p.ga[i] = a[i], p.gb[i] = b[i], p.gc[i] = b[i], p.gd[i] = d[i];
  p.parts = (long)b[0] * b[1] * b[2];
  p.scratch = rows * p.N2;
  p.ws_floats = 2 * p.parts + p.scratch;
  return CIDNET_OK;
}

inline bool aligned(const void* p, unsigned a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

inline dim3 grid_of(const int* g) { return dim3((unsigned)g[0], (unsigned)g[1], (unsigned)g[2]); }

template <int BMODE, int EPI>
int launch(const int* grid, const GemmArgs& g, hipStream_t st) {
  hipLaunchKernelGGL((dft_gemm_kernel<BMODE, EPI>), grid_of(grid), dim3(kThreads), 0, st, g);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

// (a): R = (a - b) Tw
int row_forward(const Plan& p, const float* a, const float* b, const float* tab_w, float* R, int P, int H, int W, hipStream_t st) {
  GemmArgs g = {};
  g.a = a, g.a2 = b, g.b = tab_w, g.out = R, g.M = P * H, g.N = p.N2, g.K = W;
  return launch<kBTab, kEpiStore>(p.ga, g, st);
}

// (b) / (c): out = Th rot(X) per plane; EPI kEpiAbs sums |.| into part and stores the signs when out != NULL
template <int BMODE, int EPI>
int column_pass(const Plan& p, const float* tab_h, const float* X, float* out, double* part, int H, hipStream_t st) {
  GemmArgs g = {};
  g.a = tab_h, g.b = X, g.b_zs = (long)H * p.N2, g.out = out, g.o_zs = (long)H * p.N2, g.part = part;
  g.M = H, g.N = p.N2, g.K = 2 * H;
  return launch<BMODE, EPI>(p.gb, g, st);
}

// (d): ga = scale gup G Tw^T, gb = -ga
int row_adjoint(const Plan& p, const float* G, const float* tab_w, const float* gup, float scale, float* ga, float* gb, int P, int H,
                int W, hipStream_t st) {
  GemmArgs g = {};
  g.a = G, g.b = tab_w, g.out = ga, g.out2 = gb, g.gup = gup, g.scale = scale, g.M = P * H, g.N = W, g.K = p.N2;
  return launch<kBTabT, kEpiGrad>(p.gd, g, st);
}

// weight s / (2 P H Wh) in fp64
inline double loss_scale(const Plan& p, float weight, int norm, int P, int H, int W) {
  const double s = norm ? 1.0 / std::sqrt((double)H * (double)W) : 1.0;
  return (double)weight * s / (2.0 * (double)P * (double)H * (double)p.Wh);
}

inline bool weight_ok(float w) { return w >= 0.f && std::isfinite(w); }

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_dft_table(int N, int Nk, float* table, void* stream) {
  CIDNET_CHECK_ARG(N >= 1 && Nk >= 1 && aligned(table, 4));
  if (N > kMaxSide || Nk > N) return CIDNET_ERR_SHAPE;
  hipLaunchKernelGGL(dft_table_kernel, dim3((unsigned)(((long)N * Nk + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, Nk, table);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

long cidnet_fft_loss_ws_floats(int P, int H, int W) {
  Plan p;
  return make_plan(P, H, W, p) == CIDNET_OK ? p.ws_floats : 0;
}

int cidnet_fft_loss_plan(int P, int H, int W, long* out, int n) {
  constexpr int kFields = 17;
  CIDNET_CHECK_ARG(out && n >= kFields);
  Plan p;
  const int rc = make_plan(P, H, W, p);
  if (rc != CIDNET_OK) return rc;
  const long f[kFields] = {kMT, kNT, kKC, p.ga[0], p.ga[1], p.ga[2], p.gb[0], p.gb[1], p.gb[2], p.gc[0], p.gc[1], p.gc[2],
                           p.gd[0], p.gd[1], p.gd[2], p.parts, p.ws_floats};
  for (int i = 0; i < kFields; ++i) out[i] = f[i];
  return CIDNET_OK;
}

int cidnet_fft_loss_fwd(const float* a, const float* b, const float* tab_h, const float* tab_w, float weight, int norm, float* loss,
                        float* S, float* ws, long ws_floats, int P, int H, int W, void* stream) {
  Plan p;
  const int rc = make_plan(P, H, W, p);
  if (rc != CIDNET_OK) return rc;
  CIDNET_CHECK_ARG(aligned(a, 4) && aligned(b, 4) && aligned(tab_h, 4) && aligned(tab_w, 4) && aligned(loss, 4) && aligned(ws, 8));
  CIDNET_CHECK_ARG((!S || aligned(S, 4)) && (norm == 0 || norm == 1) && weight_ok(weight));
  if (ws_floats < p.ws_floats) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  float* R = ws + 2 * p.parts;
  int e = row_forward(p, a, b, tab_w, R, P, H, W, st);
  if (e) return e;
  e = column_pass<kBRotFwd, kEpiAbs>(p, tab_h, R, S, part, H, st);
  if (e) return e;
  hipLaunchKernelGGL(fft_loss_finish_kernel, dim3(1), dim3(256), 0, st, part, p.parts, loss_scale(p, weight, norm, P, H, W), loss);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

int cidnet_fft_loss_bwd(const float* S, const float* tab_h, const float* tab_w, const float* gloss, float weight, int norm, float* ga,
                        float* gb, float* ws, long ws_floats, int P, int H, int W, void* stream) {
  Plan p;
  const int rc = make_plan(P, H, W, p);
  if (rc != CIDNET_OK) return rc;
  CIDNET_CHECK_ARG(aligned(S, 4) && aligned(tab_h, 4) && aligned(tab_w, 4) && aligned(gloss, 4) && aligned(ws, 8));
  CIDNET_CHECK_ARG((!ga || aligned(ga, 4)) && (!gb || aligned(gb, 4)) && (norm == 0 || norm == 1) && weight_ok(weight));
  if (ws_floats < p.ws_floats) return CIDNET_ERR_WS;
  if (!ga && !gb) return CIDNET_OK;
  hipStream_t st = (hipStream_t)stream;
  float* G = ws + 2 * p.parts;
  const int e = column_pass<kBRotAdj, kEpiStore>(p, tab_h, S, G, nullptr, H, st);
  if (e) return e;
  return row_adjoint(p, G, tab_w, gloss, (float)loss_scale(p, weight, norm, P, H, W), ga, gb, P, H, W, st);
}

int cidnet_rfft2_fwd(const float* x, const float* tab_h, const float* tab_w, float* D, float* ws, long ws_floats, int P, int H, int W,
                     void* stream) {
  Plan p;
  const int rc = make_plan(P, H, W, p);
  if (rc != CIDNET_OK) return rc;
  CIDNET_CHECK_ARG(aligned(x, 4) && aligned(tab_h, 4) && aligned(tab_w, 4) && aligned(D, 4) && aligned(ws, 8));
  if (ws_floats < p.ws_floats) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  float* R = ws + 2 * p.parts;
  const int e = row_forward(p, x, nullptr, tab_w, R, P, H, W, st);
  if (e) return e;
  return column_pass<kBRotFwd, kEpiStore>(p, tab_h, R, D, nullptr, H, st);
}

int cidnet_rfft2_adj(const float* Sin, const float* tab_h, const float* tab_w, float* g, float* ws, long ws_floats, int P, int H, int W,
                     void* stream) {
  Plan p;
  const int rc = make_plan(P, H, W, p);
  if (rc != CIDNET_OK) return rc;
  CIDNET_CHECK_ARG(aligned(Sin, 4) && aligned(tab_h, 4) && aligned(tab_w, 4) && aligned(g, 4) && aligned(ws, 8));
  if (ws_floats < p.ws_floats) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  float* G = ws + 2 * p.parts;
  const int e = column_pass<kBRotAdj, kEpiStore>(p, tab_h, Sin, G, nullptr, H, st);
  if (e) return e;
  return row_adjoint(p, G, tab_w, nullptr, 1.0f, g, nullptr, P, H, W, st);
}

}  // extern "C"
