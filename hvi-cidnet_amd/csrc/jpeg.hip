// The JPEG file round trip of an 8-bit RGB image without the file (include/cidnet_hip.h: cidnet_metric_jpeg_*): what Pillow's
// Image.save(f, 'JPEG', quality=q) followed by Image.open(f) returns, byte for byte.  The entropy coder is lossless, so the
// decoded file equals the lossy stages alone, all of them libjpeg's 32-bit fixed-point arithmetic: RGB ->
// YCbCr, h2v2 chroma downsampling, the "islow" forward DCT, quantise / dequantise, the islow inverse DCT, "fancy" h2v2
// upsampling, YCbCr -> RGB.  No floating point anywhere, no atomics, no reductions.
//
// Two launches on one stream:
//   A. jpeg_codec_kernel: a block of 384 threads takes a tile of 8 MCUs (128 x 16 pixels): 32 luma and 2 x 8 chroma blocks of
//      8 x 8, kept in LDS as int32 with a row pitch of 9 dwords and a block stride of 72.  Eight lanes own a block, lane j its
//      row j or its column j: with that pitch the 32 lanes of a half-wave (4 blocks x 8 lanes) touch 32 different banks
//      whether they walk rows (8 (b + r) + r + k mod 32) or columns (8 b + c + 9 k mod 32), so both directions are free of
//      conflicts and no transpose is ever written.  Forward rows -> forward columns, quantise, dequantise and the inverse
//      column pass in registers (libjpeg's decoder runs columns first) -> inverse rows, clamp, 8 bytes per lane into the
//      workspace.  Nothing but those bytes goes to memory in between.
//   B. jpeg_finish_kernel: a thread takes four pixels of a row: their luma, the 4 x 2 chroma neighbours of each plane,
//      triangle upsampling (it reads across tile borders, hence the second launch), colour conversion, store.
// Workspace per image: luma (H16, W16), then Cb and Cr (H16 / 2, W16 / 2), H16 and W16 the sizes rounded up to whole MCUs, so
// that every store of launch A is an aligned 8-byte store and needs no mask inside the MCU grid.
#include "cidnet_hip.h"
#include "common.h"
#include "jpeg_front.h"

namespace cidnet {
namespace {

constexpr int kTileMcus = 8;                           // MCUs (16 x 16 pixels) per block of launch A, side by side
constexpr int kTileBlocks = kTileMcus * 6;             // 8 x 8 blocks: 4 luma per MCU, then 8 Cb, then 8 Cr
constexpr int kCodecThreads = kTileBlocks * 8;         // 384: eight lanes per 8 x 8 block
constexpr int kPitch = 9;                              // dwords per block row in LDS
constexpr int kBlockStride = 8 * kPitch;               // 72
constexpr int kTileQuads = kTileMcus * 64;             // 2 x 2 pixel groups per tile
constexpr int kFinishThreads = 256;
constexpr int kMaxSide = 65500;                        // libjpeg's JPEG_MAX_DIMENSION: a larger image has no file

struct JpegPlan {
  int mcu_cols, mcu_rows, partial_right, partial_bottom, ch, cw, tiles_x, blocks, ws_image;
};

// The one place the MCU grid, the launch grid and the workspace are decided: both launchers' host code and the query call it.
int jpeg_plan(int h, int w, JpegPlan* p) {
  if (h < 1 || w < 5) return CIDNET_ERR_ARG;           // w < 5: the decoder's edge columns read padding (not reproduced)
  if (h > kMaxSide || w > kMaxSide) return CIDNET_ERR_SHAPE;
  const long mc = (w + 15) / 16, mr = (h + 15) / 16;
  if (mc * mr * 256 > (1L << 30)) return CIDNET_ERR_SHAPE;       // 32-bit offsets inside one image's workspace
  p->mcu_cols = (int)mc;
  p->mcu_rows = (int)mr;
  p->partial_right = (w & 15) != 0;
  p->partial_bottom = (h & 15) != 0;
  p->ch = (h + 1) / 2;
  p->cw = (w + 1) / 2;
  p->tiles_x = (int)((mc + kTileMcus - 1) / kTileMcus);
  p->blocks = p->tiles_x * (int)mr;
  p->ws_image = (int)(mc * mr * 384);                  // 256 luma + 2 x 64 chroma bytes per MCU
  return CIDNET_OK;
}

using jpegfe::descale;
using jpegfe::fdct8;

// libjpeg jidctint.c, one pass over c[0..7], descaled by kShift (11: the column pass, 18: the row pass)
template <int kShift>
__device__ __forceinline__ void idct8(int* c) {
  const int e = (c[2] + c[6]) * 4433;
  const int e2 = e - c[6] * 15137, e3 = e + c[2] * 6270;
  const int e0 = (c[0] + c[4]) * 8192, e1 = (c[0] - c[4]) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  const int z5 = (c[7] + c[3] + c[5] + c[1]) * 9633;
  const int z1 = (c[7] + c[1]) * -7373, z2 = (c[5] + c[3]) * -20995, z3 = (c[7] + c[3]) * -16069 + z5, z4 = (c[5] + c[1]) * -3196 + z5;
  const int o0 = c[7] * 2446 + z1 + z3, o1 = c[5] * 16819 + z2 + z4, o2 = c[3] * 25172 + z2 + z3, o3 = c[1] * 12299 + z1 + z4;
  c[0] = descale(t10 + o3, kShift);
  c[7] = descale(t10 - o3, kShift);
  c[1] = descale(t11 + o2, kShift);
  c[6] = descale(t11 - o2, kShift);
  c[2] = descale(t12 + o1, kShift);
  c[5] = descale(t12 - o1, kShift);
  c[3] = descale(t13 + o0, kShift);
  c[4] = descale(t13 - o0, kShift);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The 2 x 2 pixels (y0 | y1, x0 | x1) of one image: their luma, and the sums of their Cb and of their Cr
__device__ __forceinline__ void quad(const uint8_t* __restrict__ img, long plane, int w, int y0, int y1, int x0, int x1, int* yv,
                                     int* cb, int* cr) {
  const long o[4] = {(long)y0 * w + x0, (long)y0 * w + x1, (long)y1 * w + x0, (long)y1 * w + x1};
  int sb = 0, sr = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int pb, pr;
    jpegfe::ycc(img[o[i]], img[plane + o[i]], img[2 * plane + o[i]], &yv[i], &pb, &pr);
    sb += pb;
    sr += pr;
  }
  *cb = sb;
  *cr = sr;
}

// grid (tiles_x, mcu_rows, B).  qtab: int32 [2][2][64], luma then chroma: the table t in natural order, then ceil(2^32 / (8 t)).
__global__ __launch_bounds__(kCodecThreads) void jpeg_codec_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ ws,
                                                                   const int* __restrict__ qtab, int h, int w, int mcu_cols,
                                                                   int mcu_rows, int ch, long ws_image) {
  __shared__ int lds[kTileBlocks * kBlockStride];
  const int tid = threadIdx.x;
  const int X0 = blockIdx.x * (16 * kTileMcus);
  const long plane = (long)h * w;
  const uint8_t* img = src + (long)blockIdx.z * 3 * plane;
  // colour conversion and chroma downsampling.  Every coordinate is held inside the image: that IS the edge replication.
  for (int qi = tid; qi < kTileQuads; qi += kCodecThreads) {
    const int qx = qi & (kTileQuads / 8 - 1), qy = qi / (kTileQuads / 8);
    const int R = blockIdx.y * 8 + qy;                 // row of the downsampled planes; luma rows 2 R, 2 R + 1
    const int x0 = min(X0 + 2 * qx, w - 1), x1 = min(X0 + 2 * qx + 1, w - 1);
    int yv[4], cb, cr;
    quad(img, plane, w, min(2 * R, h - 1), min(2 * R + 1, h - 1), x0, x1, yv, &cb, &cr);
    if (R >= ch) {                                     // below the image the DOWNSAMPLED row ch - 1 is repeated, not the pixels
      int unused[4];
      quad(img, plane, w, 2 * (ch - 1), min(2 * ch - 1, h - 1), x0, x1, unused, &cb, &cr);
    }
    const int lx = 2 * qx, ly = 2 * qy;
    int* yb = lds + ((lx >> 4) * 4 + ((ly >> 3) << 1) + ((lx >> 3) & 1)) * kBlockStride + (ly & 7) * kPitch + (lx & 7);
    yb[0] = yv[0] - 128;
    yb[1] = yv[1] - 128;
    yb[kPitch] = yv[2] - 128;
    yb[kPitch + 1] = yv[3] - 128;
    const int bias = 1 + (qx & 1);                     // 1, 2, 1, 2, ... by output column; a tile starts on an even one
    int* cp = lds + (4 * kTileMcus + (qx >> 3)) * kBlockStride + qy * kPitch + (qx & 7);
    cp[0] = ((cb + bias) >> 2) - 128;
    cp[kTileMcus * kBlockStride] = ((cr + bias) >> 2) - 128;
  }
  __syncthreads();
  const int b = tid >> 3, j = tid & 7;
  int* blk = lds + b * kBlockStride;
  int d[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = blk[j * kPitch + k];
  fdct8<true>(d);
#pragma unroll
  for (int k = 0; k < 8; ++k) blk[j * kPitch + k] = d[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = blk[k * kPitch + j];
  fdct8<false>(d);
  const int* qt = qtab + (b >= 4 * kTileMcus ? 128 : 0);         // uniform per wave: waves 0-3 luma, 4 Cb, 5 Cr
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // c = sign(v) ((|v| + 4 t) / (8 t)) t: jpeg_front.h has the quotient and why it is exact
    const int t = qt[k * 8 + j];
    d[k] = jpegfe::quantise(d[k], t, (unsigned)qt[64 + k * 8 + j]) * t;
  }
  idct8<11>(d);
#pragma unroll
  for (int k = 0; k < 8; ++k) blk[k * kPitch + j] = d[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = blk[j * kPitch + k];
  idct8<18>(d);
  uint2 out = {0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    out.x |= (unsigned)clamp255(d[k] + 128) << (8 * k);
    out.y |= (unsigned)clamp255(d[k + 4] + 128) << (8 * k);
  }
  uint8_t* wi = ws + (long)blockIdx.z * ws_image;
  const int W16 = mcu_cols * 16;
  if (b < 4 * kTileMcus) {
    const int m = b >> 2, sub = b & 3;
    if (blockIdx.x * kTileMcus + m < mcu_cols) {       // the last tile of a row may hold fewer than 8 MCUs
      const long o = (long)(blockIdx.y * 16 + (sub >> 1) * 8 + j) * W16 + X0 + m * 16 + (sub & 1) * 8;
      *reinterpret_cast<uint2*>(wi + o) = out;
    }
  } else {
    const int comp = (b - 4 * kTileMcus) >> 3, m = b & 7;
    if (blockIdx.x * kTileMcus + m < mcu_cols) {
      const long cplane = (long)mcu_rows * mcu_cols * 64;
      const long o = 4 * cplane + comp * cplane + (long)(blockIdx.y * 8 + j) * (W16 >> 1) + (X0 >> 1) + m * 8;
      *reinterpret_cast<uint2*>(wi + o) = out;
    }
  }
}

// grid (ceil(ceil(w / 4) / 256), h, B): pixels 4 k .. 4 k + 3 of row blockIdx.y.  The chroma columns and rows are held inside
// the cropped (ch, cw) planes, which turns libjpeg's first- and last-column cases (4 s) and its replicated neighbour rows into
// the general formula: 3 s + s.
__global__ __launch_bounds__(kFinishThreads) void jpeg_finish_kernel(const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst,
                                                                     int h, int w, int mcu_cols, int mcu_rows, int ch, int cw,
                                                                     long ws_image, int dword_stores) {
  const int x0 = 4 * (blockIdx.x * kFinishThreads + threadIdx.x);
  if (x0 >= w) return;
  const int y = blockIdx.y, W16 = mcu_cols * 16, C2 = W16 >> 1;
  const long cplane = (long)mcu_rows * mcu_cols * 64;
  const uint8_t* wi = ws + (long)blockIdx.z * ws_image;
  const unsigned y4 = *reinterpret_cast<const unsigned*>(wi + (long)y * W16 + x0);
  const int cur = y >> 1, nb = (y & 1) ? min(cur + 1, ch - 1) : max(cur - 1, 0);
  const int c0 = x0 >> 1;                              // <= cw - 1, since x0 < w
  const int col[4] = {max(c0 - 1, 0), c0, min(c0 + 1, cw - 1), min(c0 + 2, cw - 1)};
  int up[2][4];
#pragma unroll
  for (int comp = 0; comp < 2; ++comp) {
    const uint8_t* cp = wi + 4 * cplane + comp * cplane;
    int s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = 3 * cp[(long)cur * C2 + col[i]] + cp[(long)nb * C2 + col[i]];
    up[comp][0] = (3 * s[1] + s[0] + 8) >> 4;
    up[comp][1] = (3 * s[1] + s[2] + 7) >> 4;
    up[comp][2] = (3 * s[2] + s[1] + 8) >> 4;
    up[comp][3] = (3 * s[2] + s[3] + 7) >> 4;
  }
  unsigned r4 = 0, g4 = 0, b4 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int yy = (y4 >> (8 * i)) & 255, cb = up[0][i] - 128, cr = up[1][i] - 128;
    r4 |= (unsigned)clamp255(yy + ((91881 * cr + 32768) >> 16)) << (8 * i);
    g4 |= (unsigned)clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)) << (8 * i);
    b4 |= (unsigned)clamp255(yy + ((116130 * cb + 32768) >> 16)) << (8 * i);
  }
  const long plane = (long)h * w;
  uint8_t* o = dst + (long)blockIdx.z * 3 * plane + (long)y * w + x0;
  if (dword_stores) {                                  // w a multiple of 4 and dst aligned: decided on the host
    *reinterpret_cast<unsigned*>(o) = r4;
    *reinterpret_cast<unsigned*>(o + plane) = g4;
    *reinterpret_cast<unsigned*>(o + 2 * plane) = b4;
  } else {
    const int n = min(4, w - x0);
    for (int i = 0; i < n; ++i) {
      o[i] = (uint8_t)(r4 >> (8 * i));
      o[plane + i] = (uint8_t)(g4 >> (8 * i));
      o[2 * plane + i] = (uint8_t)(b4 >> (8 * i));
    }
  }
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

long cidnet_metric_jpeg_ws_bytes(int B, int h, int w) {
  JpegPlan p;
  if (B < 1 || jpeg_plan(h, w, &p) != CIDNET_OK) return 0;
  return (long)B * p.ws_image;
}

int cidnet_metric_jpeg_plan(int h, int w, int* out, int n) {
  if (!out || n < 9) return CIDNET_ERR_ARG;
  JpegPlan p;
  const int rc = jpeg_plan(h, w, &p);
  if (rc != CIDNET_OK) return rc;
  out[0] = p.mcu_cols; out[1] = p.mcu_rows; out[2] = p.partial_right; out[3] = p.partial_bottom; out[4] = p.ch; out[5] = p.cw;
  out[6] = p.tiles_x; out[7] = p.blocks; out[8] = p.ws_image;
  return CIDNET_OK;
}

int cidnet_metric_jpeg_roundtrip_u8(const uint8_t* src, uint8_t* dst, void* ws, long ws_bytes, const int* qtab, int B, int h,
                                    int w, void* stream) {
  CIDNET_CHECK_ARG(src && dst && ws && qtab && B >= 1 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)qtab & 3) == 0);
  JpegPlan p;
  const int rc = jpeg_plan(h, w, &p);
  if (rc != CIDNET_OK) return rc;
  if (B > 65535) return CIDNET_ERR_SHAPE;
  if (ws_bytes < (long)B * p.ws_image) return CIDNET_ERR_WS;
  hipLaunchKernelGGL(jpeg_codec_kernel, dim3(p.tiles_x, p.mcu_rows, B), dim3(kCodecThreads), 0, (hipStream_t)stream, src,
                     reinterpret_cast<uint8_t*>(ws), qtab, h, w, p.mcu_cols, p.mcu_rows, p.ch, (long)p.ws_image);
  CIDNET_LAUNCH_STATUS();
  const int dword_stores = (w & 3) == 0 && ((uintptr_t)dst & 3) == 0;
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3(ceil_div((w + 3) / 4, kFinishThreads), h, B), dim3(kFinishThreads), 0,
                     (hipStream_t)stream, reinterpret_cast<const uint8_t*>(ws), dst, h, w, p.mcu_cols, p.mcu_rows, p.ch, p.cw,
                     (long)p.ws_image, dword_stores);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
