// The entropy-coded scan of a baseline JPEG on the device (include/cidnet_hip.h: cidnet_jpeg_encode_*; DESIGN.md 6.13;
// tests/jpegenc_ref.py restates it and tests/test_jpegenc_cpu.py pins the restatement to Pillow): interleaved uint8 (B,h,w,3)
// -> per image the bytes between SOS and EOI of the file Image.save(f, 'JPEG', quality=q) writes, byte for byte.  The host
// keeps the 623 bytes of framing.  Integer arithmetic only.  The file has no restart markers, so the DC chain and the bit
// offsets run through the whole image: counts first, an exclusive scan, then emission at known offsets.  No workgroup ever
// waits for another one: every dependency is a kernel boundary.
//
// Six launches on one stream; a "group" is kGroupMcus = 16 consecutive MCUs of the scan, a wave takes an 8 x 8 block with lane
// k holding zigzag coefficient k:
//   1. jpegenc_transform_kernel  grid (ceil(MCU columns / 8), MCU rows, B), 384 threads: the front end of csrc/jpeg.hip
//      (jpeg_front.h) up to the quantiser, on interleaved bytes; the coefficients go to the workspace as int16 in zigzag order,
//      768 bytes per MCU in scan order (Y00 Y01 Y10 Y11 Cb Cr), one 16-byte store per thread.
//   2. jpegenc_count_kernel      grid (groups, B), 256 threads: a block's bits -- a ballot of v != 0 gives a lane its run, the
//      run its ZRL count and code -- summed per MCU and per group.  A luma block past ceil(h/8) x ceil(w/8) is a dummy: it is
//      coded as difference 0 + end of block and leaves the predictor alone, whatever the transform wrote for it.
//   3. jpegenc_offsets_kernel    grid (B): ONE workgroup per image scans the group sums (64-bit offsets) and zeroes the one
//      dword of the unstuffed stream that each group shares with the group before it.
//   4. jpegenc_emit_kernel       grid (groups, B): the same codes again, a wave prefix sum of their lengths, ds_or into a zeroed
//      LDS window of the group's bits, whole dwords stored; only the group's first and last dword go out as atomic ORs.
//      Counts the 0xFF among the bytes that lie wholly inside the group.
//   5. jpegenc_stuff_scan_kernel grid (B): adds the byte each group shares with the next (now complete), scans the counts:
//      every group's offset in the slot, and sizes[b].
//   6. jpegenc_copy_kernel       grid (groups, B): copies the group's bytes with a 0x00 behind every 0xFF, fills the tail bits
//      with ones, and zeroes its share of the slot behind the stream.
// Workspace per image: coefficients | bits per MCU | one record per group (+ one for the totals) | the unstuffed stream.
#include "cidnet_hip.h"
#include "common.h"
#include "jpeg_codes.h"
#include "jpeg_front.h"

namespace cidnet {
namespace {

constexpr int kTileMcus = 8;                           // launch 1: MCUs per workgroup, side by side (as csrc/jpeg.hip)
constexpr int kTileBlocks = kTileMcus * 6;
constexpr int kTransformThreads = kTileBlocks * 8;     // 384: eight lanes per 8 x 8 block
constexpr int kPitch = 9;
constexpr int kBlockStride = 8 * kPitch;
constexpr int kTileQuads = kTileMcus * 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroupMcus = 16;                         // MCUs per partial sum of the scan: four per wave
constexpr int kMaxSide = 65500;                        // libjpeg's JPEG_MAX_DIMENSION
constexpr long kMaxMcus = 1L << 22;
constexpr int kRealBits = 22 + 63 * 26;                // see jpegenc_plan
constexpr int kDummyBits = 6;
constexpr int kWinDwords = (31 + kGroupMcus * 6 * kRealBits + 31) / 32 + 3;
constexpr int kTab = jpegcodes::kTabEntries;

__constant__ jpegcodes::Tables kCodes = jpegcodes::kTables;

struct Record {                                        // one per group, and one more whose off / out are the image's totals
  unsigned long long off;                              // bits in front of the group
  unsigned long long out;                              // bytes of the slot in front of the group's bytes
  unsigned bits, ff;                                   // the group's bits; 0xFF bytes among the bytes that START in it
  unsigned pad[2];
};
static_assert(sizeof(Record) == 32, "Record");

struct EncPlan {
  int mcu_cols, mcu_rows, bw, bh, tiles_x;
  long mcus, dummies, groups, bits_off, rec_off, stream_off, stream_bytes, ws_image, capacity;
};

// The one place the grids, the workspace and the slot are decided: the launcher and the query call it.
// The slot bound: a real block costs at most 22 + 63 * 26 = 1660 bits.  DC: the longest code (9 bits luma, 11 chroma: asserted
// in jpeg_codes.h) and 11 value bits.  AC: charge every zigzag position 1..63 -- a non-zero coefficient at most 16 code + 10
// value bits; a ZRL (11 bits at most) stands for 16 zero positions in front of a later non-zero one, under one bit each; the
// end of block (4 bits at most) is sent only when position 63 is zero, and no ZRL covers that position.  A dummy block is the
// six bits 00 1010.  The padded byte count doubles if every byte is stuffed; + 2 as slack, rounded up to whole dwords.
int jpegenc_plan(int h, int w, EncPlan* p) {
  if (h < 1 || w < 1) return CIDNET_ERR_ARG;
  if (h > kMaxSide || w > kMaxSide) return CIDNET_ERR_SHAPE;
  const long mc = (w + 15) / 16, mr = (h + 15) / 16, bw = (w + 7) / 8, bh = (h + 7) / 8;
  if (mc * mr > kMaxMcus) return CIDNET_ERR_SHAPE;
  p->mcu_cols = (int)mc;
  p->mcu_rows = (int)mr;
  p->bw = (int)bw;
  p->bh = (int)bh;
  p->tiles_x = (int)((mc + kTileMcus - 1) / kTileMcus);
  p->mcus = mc * mr;
  p->dummies = 4 * p->mcus - bw * bh;
  p->groups = (p->mcus + kGroupMcus - 1) / kGroupMcus;
  const long bits = (bw * bh + 2 * p->mcus) * kRealBits + p->dummies * kDummyBits;
  const long bytes = (bits + 7) / 8;
  p->capacity = (2 * bytes + 2 + 3) / 4 * 4;
  p->bits_off = p->mcus * 768;                                       // a multiple of 16
  p->rec_off = p->bits_off + (p->mcus * 4 + 15) / 16 * 16;
  p->stream_off = p->rec_off + (p->groups + 1) * (long)sizeof(Record);
  p->stream_bytes = (bytes + 4 + 15) / 16 * 16;                      // whole dwords, and the dword behind the last bit
  p->ws_image = p->stream_off + p->stream_bytes;
  return CIDNET_OK;
}

struct Geo {
  int mcu_cols, bw, bh;
  long mcus, groups, bits_off, rec_off, stream_off, stream_bytes, ws_image;
};

__device__ __forceinline__ const int16_t* coef_of(const uint8_t* wi) { return reinterpret_cast<const int16_t*>(wi); }
__device__ __forceinline__ unsigned* mcu_bits_of(uint8_t* wi, const Geo& g) { return reinterpret_cast<unsigned*>(wi + g.bits_off); }
__device__ __forceinline__ Record* records_of(uint8_t* wi, const Geo& g) { return reinterpret_cast<Record*>(wi + g.rec_off); }

// grid (tiles_x, mcu_rows, B).  qtab: int32 [2][2][64], luma then chroma: the table t in natural order, then ceil(2^32 / (8 t)).
__global__ __launch_bounds__(kTransformThreads) void jpegenc_transform_kernel(const uint8_t* __restrict__ src, long src_stride,
                                                                              uint8_t* __restrict__ ws, long ws_image,
                                                                              const int* __restrict__ qtab, int h, int w,
                                                                              int mcu_cols, int ch) {
  __shared__ int lds[kTileBlocks * kBlockStride];
  const int tid = threadIdx.x;
  const int X0 = blockIdx.x * (16 * kTileMcus);
  const uint8_t* img = src + (long)blockIdx.z * src_stride;
  // colour conversion and chroma downsampling.  Every coordinate is held inside the image: that IS the edge replication.
  for (int qi = tid; qi < kTileQuads; qi += kTransformThreads) {
    const int qx = qi & (kTileQuads / 8 - 1), qy = qi / (kTileQuads / 8);
    const int R = blockIdx.y * 8 + qy;                 // row of the downsampled planes; luma rows 2 R, 2 R + 1
    const int x0 = min(X0 + 2 * qx, w - 1), x1 = min(X0 + 2 * qx + 1, w - 1);
    const int yl0 = min(2 * R, h - 1), yl1 = min(2 * R + 1, h - 1);
    // below the image the DOWNSAMPLED row ch - 1 is repeated, not the pixels
    const int yc0 = R >= ch ? 2 * (ch - 1) : yl0, yc1 = R >= ch ? min(2 * ch - 1, h - 1) : yl1;
    const int ys[4] = {yl0, yl0, yl1, yl1}, yc[4] = {yc0, yc0, yc1, yc1}, xs[4] = {x0, x1, x0, x1};
    int yv[4], cb = 0, cr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* p = img + ((long)ys[i] * w + xs[i]) * 3;
      int pb, pr;
      jpegfe::ycc(p[0], p[1], p[2], &yv[i], &pb, &pr);
      if (yc[i] != ys[i]) {                            // only in MCU rows below the image
        const uint8_t* c = img + ((long)yc[i] * w + xs[i]) * 3;
        int unused;
        jpegfe::ycc(c[0], c[1], c[2], &unused, &pb, &pr);
      }
      cb += pb;
      cr += pr;
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
  jpegfe::fdct8<true>(d);
#pragma unroll
  for (int k = 0; k < 8; ++k) blk[j * kPitch + k] = d[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = blk[k * kPitch + j];
  jpegfe::fdct8<false>(d);
  const int* qt = qtab + (b >= 4 * kTileMcus ? 128 : 0);         // uniform per wave: waves 0-3 luma, 4 Cb, 5 Cr
#pragma unroll
  for (int k = 0; k < 8; ++k) blk[k * kPitch + j] = jpegfe::quantise(d[k], qt[k * 8 + j], (unsigned)qt[64 + k * 8 + j]);
  __syncthreads();
  // thread t: zigzag coefficients k0 .. k0 + 7 of block b6 of the tile's MCU m, 16 bytes
  const int m = tid / 48, b6 = (tid % 48) >> 3, k0 = (tid & 7) * 8;
  if (blockIdx.x * kTileMcus + m < mcu_cols) {         // the last tile of a row may hold fewer than 8 MCUs
    const int* sb = lds + (b6 < 4 ? m * 4 + b6 : 4 * kTileMcus + (b6 - 4) * kTileMcus + m) * kBlockStride;
    unsigned o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n0 = kCodes.natural[k0 + 2 * i], n1 = kCodes.natural[k0 + 2 * i + 1];
      const int v0 = sb[(n0 >> 3) * kPitch + (n0 & 7)], v1 = sb[(n1 >> 3) * kPitch + (n1 & 7)];
      o[i] = ((unsigned)v0 & 0xffffu) | ((unsigned)v1 << 16);
    }
    const long mcu = (long)blockIdx.y * mcu_cols + blockIdx.x * kTileMcus + m;
    uint8_t* wi = ws + (long)blockIdx.z * ws_image;
    *reinterpret_cast<uint4*>(wi + ((mcu * 6 + b6) * 64 + k0) * 2) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

__device__ __forceinline__ bool luma_real(const Geo& g, long mcu, int k) {
  const int mx = (int)(mcu % g.mcu_cols), my = (int)(mcu / g.mcu_cols);
  return 2 * mx + (k & 1) < g.bw && 2 * my + (k >> 1) < g.bh;
}

// The DC predictor of block b6 of MCU mcu: the DC of the component's block before it in scan order, dummies passed over (a
// dummy repeats the DC in front of it); 0 for the first.  Block 0 of every MCU is real, so the walk ends within four steps.
__device__ __forceinline__ int dc_pred(const int16_t* __restrict__ coef, const Geo& g, long mcu, int b6) {
  if (b6 >= 4) return mcu ? coef[((mcu - 1) * 6 + b6) * 64] : 0;
  long j = mcu * 4 + b6 - 1;
  for (int step = 0; step < 4 && j >= 0; ++step, --j)
    if (luma_real(g, j >> 2, (int)(j & 3))) return coef[((j >> 2) * 6 + (j & 3)) * 64];
  return 0;
}

__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }           // of a >= 0; 0 for 0

// Lane k's share of one block's code: `nb` bits (59 at most: three ZRL of 11, a code of 16, 10 value bits), the first of them
// the most significant of `bits`.  v: the lane's zigzag coefficient, in lane 0 the DC DIFFERENCE.  tab: the component's packed
// table in LDS.  Every lane of the wave is here.
__device__ __forceinline__ void lane_code(const unsigned* tab, int v, int lane, unsigned long long* bits, int* nb) {
  const unsigned long long nz = __ballot(lane > 0 && v != 0);
  const int a = v < 0 ? -v : v, s = bit_length(a);
  const unsigned vb = (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
  unsigned long long out = 0;
  int n = 0;
  if (lane == 0) {
    const unsigned e = tab[jpegcodes::kDcBase + min(s, 15)];
    out = ((unsigned long long)(e & 0xffffu) << s) | vb;
    n = (int)(e >> 16) + s;
  } else if (v != 0) {
    const unsigned long long below = nz & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;     // the non-zero coefficient in front, or the DC
    const int run = lane - prev - 1;
    const unsigned z = tab[0xF0], e = tab[(((unsigned)run & 15u) << 4) | (unsigned)min(s, 15)];
    for (int i = 0; i < (run >> 4); ++i) out = (out << (z >> 16)) | (z & 0xffffu);
    out = (out << (e >> 16)) | (e & 0xffffu);
    out = (out << s) | vb;
    n = (run >> 4) * (int)(z >> 16) + (int)(e >> 16) + s;
  } else if (lane == 63) {
    const unsigned e = tab[0x00];                      // the end of block: coefficient 63 is zero
    out = e & 0xffffu;
    n = (int)(e >> 16);
  }
  *bits = out;
  *nb = n;
}

// the lane's coefficient of block b6 of MCU mcu as lane_code takes it
__device__ __forceinline__ int lane_value(const int16_t* __restrict__ coef, const Geo& g, long mcu, int b6, int lane) {
  if (b6 < 4 && !luma_real(g, mcu, b6)) return 0;      // a dummy: difference 0, no AC
  int v = coef[(mcu * 6 + b6) * 64 + lane];
  if (lane == 0) v -= dc_pred(coef, g, mcu, b6);
  return v;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned wave_scan_u32(unsigned v, int lane) {             // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// inclusive scan over the block's kThreads values and their total, in every thread.  red: kWaves words of LDS
__device__ __forceinline__ unsigned block_scan_u32(unsigned v, unsigned* red, unsigned* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned incl = wave_scan_u32(v, lane);
  __syncthreads();                                     // red may still be read from the call before
  if (lane == 63) red[wv] = incl;
  __syncthreads();
  unsigned t = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    if (i < wv) incl += red[i];
    t += red[i];
  }
  *total = t;
  return incl;
}

__device__ __forceinline__ void load_tables(unsigned* tab) {
  for (int i = threadIdx.x; i < 2 * kTab; i += kThreads) tab[i] = kCodes.e[i];
}

// grid (groups, B)
__global__ __launch_bounds__(kThreads) void jpegenc_count_kernel(uint8_t* __restrict__ ws, Geo g) {
  __shared__ unsigned tab[2 * kTab];
  __shared__ unsigned gsum;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint8_t* wi = ws + (long)blockIdx.y * g.ws_image;
  const int16_t* coef = coef_of(wi);
  load_tables(tab);
  if (tid == 0) gsum = 0u;
  __syncthreads();
  unsigned mine = 0;
  for (int i = 0; i < kGroupMcus / kWaves; ++i) {
    const long mcu = (long)blockIdx.x * kGroupMcus + wv * (kGroupMcus / kWaves) + i;
    if (mcu >= g.mcus) break;                          // uniform per wave
    unsigned bits_mcu = 0;
    for (int b6 = 0; b6 < 6; ++b6) {
      unsigned long long bits;
      int nb;
      lane_code(tab + (b6 >= 4 ? kTab : 0), lane_value(coef, g, mcu, b6, lane), lane, &bits, &nb);
      bits_mcu += wave_sum_u32((unsigned)nb);
    }
    if (lane == 0) mcu_bits_of(wi, g)[mcu] = bits_mcu;
    mine += bits_mcu;
  }
  if (lane == 0) atomicAdd(&gsum, mine);
  __syncthreads();
  if (tid == 0) records_of(wi, g)[blockIdx.x].bits = gsum;
}

// grid (B): one workgroup per image
__global__ __launch_bounds__(kThreads) void jpegenc_offsets_kernel(uint8_t* __restrict__ ws, Geo g) {
  __shared__ unsigned red[kWaves];
  uint8_t* wi = ws + (long)blockIdx.x * g.ws_image;
  Record* rec = records_of(wi, g);
  unsigned* stream = reinterpret_cast<unsigned*>(wi + g.stream_off);
  const long stream_dw = g.stream_bytes / 4;
  unsigned long long carry = 0;
  for (long base = 0; base < g.groups; base += kThreads) {
    const long i = base + threadIdx.x;
    const unsigned v = i < g.groups ? rec[i].bits : 0u;      // 256 groups hold under 2^26 bits
    unsigned total;
    const unsigned incl = block_scan_u32(v, red, &total);
    if (i < g.groups) {
      const unsigned long long off = carry + (incl - v);
      rec[i].off = off;
      if ((long)(off >> 5) < stream_dw) stream[off >> 5] = 0u;       // the dword shared with the group in front
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    rec[g.groups].off = carry;
    if ((long)(carry >> 5) < stream_dw) stream[carry >> 5] = 0u;
  }
}

// grid (groups, B)
__global__ __launch_bounds__(kThreads) void jpegenc_emit_kernel(uint8_t* __restrict__ ws, Geo g) {
  __shared__ unsigned win[kWinDwords];                 // word i: bits 32 i .. 32 i + 31 behind the group's first dword, MSB first
  __shared__ unsigned tab[2 * kTab];
  __shared__ unsigned nff;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint8_t* wi = ws + (long)blockIdx.y * g.ws_image;
  const int16_t* coef = coef_of(wi);
  Record* rec = records_of(wi, g);
  unsigned* stream = reinterpret_cast<unsigned*>(wi + g.stream_off);
  const long stream_dw = g.stream_bytes / 4;
  const unsigned long long goff = rec[blockIdx.x].off;
  const unsigned gbits = rec[blockIdx.x].bits;
  const long gw0 = (long)(goff >> 5);
  const unsigned rel = (unsigned)(goff & 31);
  for (int i = tid; i < kWinDwords; i += kThreads) win[i] = 0u;
  load_tables(tab);
  if (tid == 0) nff = 0u;
  __syncthreads();

  const long m0 = (long)blockIdx.x * kGroupMcus;
  const unsigned mb = (lane < kGroupMcus && m0 + lane < g.mcus) ? mcu_bits_of(wi, g)[m0 + lane] : 0u;
  const unsigned before = wave_scan_u32(mb, lane) - mb;          // bits of the group in front of its MCU `lane`
  for (int i = 0; i < kGroupMcus / kWaves; ++i) {
    const int m = wv * (kGroupMcus / kWaves) + i;
    const long mcu = m0 + m;
    if (mcu >= g.mcus) break;                          // uniform per wave
    unsigned pos = rel + __shfl(before, m, 64);
    for (int b6 = 0; b6 < 6; ++b6) {
      unsigned long long bits;
      int nb;
      lane_code(tab + (b6 >= 4 ? kTab : 0), lane_value(coef, g, mcu, b6, lane), lane, &bits, &nb);
      const unsigned incl = wave_scan_u32((unsigned)nb, lane);
      if (nb) {
        const unsigned p = pos + incl - (unsigned)nb, wd = p >> 5, sh = p & 31;
        const unsigned long long x = bits << (64 - nb);
        const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
        const unsigned o0 = hi >> sh, o1 = (sh ? hi << (32 - sh) : 0u) | (lo >> sh), o2 = sh ? lo << (32 - sh) : 0u;
        if (o0 && wd < (unsigned)kWinDwords) atomicOr(&win[wd], o0);
        if (o1 && wd + 1 < (unsigned)kWinDwords) atomicOr(&win[wd + 1], o1);
        if (o2 && wd + 2 < (unsigned)kWinDwords) atomicOr(&win[wd + 2], o2);
      }
      pos += __shfl(incl, 63, 64);
    }
  }
  __syncthreads();
  const unsigned endbit = rel + gbits;
  const unsigned ndw = min((endbit + 31u) >> 5, (unsigned)kWinDwords);
  // bytes that lie wholly inside the group: first_byte <= byte < end_byte
  const long first_byte = (long)((goff + 7) >> 3), end_byte = (long)((goff + gbits) >> 3);
  unsigned cnt = 0;
  for (unsigned t = tid; t < ndw; t += kThreads) {
    const unsigned v = win[t];
    const long idx = gw0 + t;
    if (idx < stream_dw) {
      const unsigned mem = __builtin_bswap32(v);       // the stream's first bit is the top bit of its first BYTE
      const bool shared = t == 0 || (t == ndw - 1 && (endbit & 31u));
      if (shared) atomicOr(&stream[idx], mem);         // zeroed by launch 3; the neighbour group ORs its own bits
      else stream[idx] = mem;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long byte = 4 * idx + c;
      cnt += (byte >= first_byte && byte < end_byte && ((v >> (24 - 8 * c)) & 255u) == 255u) ? 1u : 0u;
    }
  }
  cnt = wave_sum_u32(cnt);
  if (lane == 0 && cnt) atomicAdd(&nff, cnt);
  __syncthreads();
  if (tid == 0) rec[blockIdx.x].ff = nff;
}

// grid (B): one workgroup per image.  A group spans at least 32 bits (an MCU is at least 4 x 6 + 2 x 4), so the byte that holds
// a group's last bit, when the next group shares it, STARTS in this group and is counted with it here.
__global__ __launch_bounds__(kThreads) void jpegenc_stuff_scan_kernel(uint8_t* __restrict__ ws, Geo g, long long* __restrict__ sizes) {
  __shared__ unsigned red[kWaves];
  uint8_t* wi = ws + (long)blockIdx.x * g.ws_image;
  Record* rec = records_of(wi, g);
  const uint8_t* stream = wi + g.stream_off;
  unsigned long long carry = 0;
  for (long base = 0; base < g.groups; base += kThreads) {
    const long i = base + threadIdx.x;
    unsigned v = 0;
    if (i < g.groups) {
      const unsigned long long e = rec[i].off + rec[i].bits;
      v = rec[i].ff;
      if ((e & 7) && (long)(e >> 3) < g.stream_bytes) {
        unsigned byte = stream[e >> 3];
        if (i == g.groups - 1) byte |= (1u << (8 - (unsigned)(e & 7))) - 1u;        // the tail is filled with ones
        v += byte == 255u ? 1u : 0u;
      }
      rec[i].ff = v;
    }
    unsigned total;
    const unsigned incl = block_scan_u32(v, red, &total);
    if (i < g.groups) rec[i].out = ((rec[i].off + 7) >> 3) + carry + (incl - v);
    carry += total;
  }
  if (threadIdx.x == 0) {
    const unsigned long long size = ((rec[g.groups].off + 7) >> 3) + carry;
    rec[g.groups].out = size;
    sizes[blockIdx.x] = (long long)size;
  }
}

// grid (groups, B)
__global__ __launch_bounds__(kThreads) void jpegenc_copy_kernel(uint8_t* __restrict__ ws, Geo g, uint8_t* __restrict__ dst,
                                                                long dst_stride, long capacity) {
  __shared__ unsigned red[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint8_t* wi = ws + (long)blockIdx.y * g.ws_image;
  const Record* rec = records_of(wi, g);
  const uint8_t* stream = wi + g.stream_off;
  uint8_t* slot = dst + (long)blockIdx.y * dst_stride;
  const unsigned long long total = rec[g.groups].off;
  const long size = (long)rec[g.groups].out, nbytes = (long)((total + 7) >> 3);
  const Record r = rec[blockIdx.x];
  const long b0 = (long)((r.off + 7) >> 3), b1 = (long)((r.off + r.bits + 7) >> 3);
  long o = (long)r.out;
  for (long base = b0; base < b1; base += kThreads) {
    const long i = base + tid;
    const bool valid = i < b1 && i < g.stream_bytes;
    unsigned v = valid ? stream[i] : 0u;
    if (i == nbytes - 1 && (total & 7)) v |= (1u << (8 - (unsigned)(total & 7))) - 1u;
    const bool ff = valid && v == 255u;
    const unsigned long long m = __ballot(ff);
    __syncthreads();                                   // red may still be read from the pass before
    if (lane == 0) red[wv] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = (unsigned)__popcll(m & ((1ull << lane) - 1ull)), pass = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      if (k < wv) before += red[k];
      pass += red[k];
    }
    if (valid) {
      const long p = o + (i - base) + before;
      if (p < capacity) slot[p] = (uint8_t)v;          // the plan's capacity is a proven bound; never store past the slot
      if (ff && p + 1 < capacity) slot[p + 1] = 0;
    }
    o += kThreads + pass;
  }
  // the slot behind the stream becomes zero: whole dwords shared out over the groups, the odd bytes by the last group
  const long cap_dw = capacity / 4, z0 = (size + 3) / 4;
  const long per = (cap_dw + g.groups - 1) / g.groups;
  const long lo = max(z0, (long)blockIdx.x * per), hi = min(cap_dw, ((long)blockIdx.x + 1) * per);
  unsigned* slot32 = reinterpret_cast<unsigned*>(slot);
  for (long i = lo + tid; i < hi; i += kThreads) slot32[i] = 0u;
  if (blockIdx.x == g.groups - 1 && tid == 0)
    for (long i = size; i < 4 * z0 && i < capacity; ++i) slot[i] = 0;
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_jpeg_encode_plan(int h, int w, long* out, int n) {
  if (!out || n < 9) return CIDNET_ERR_ARG;
  EncPlan p;
  const int rc = jpegenc_plan(h, w, &p);
  if (rc != CIDNET_OK) return rc;
  out[0] = p.mcu_cols; out[1] = p.mcu_rows; out[2] = p.bw; out[3] = p.bh; out[4] = p.dummies; out[5] = p.ws_image;
  out[6] = p.capacity; out[7] = p.groups; out[8] = (long)p.tiles_x * p.mcu_rows;
  return CIDNET_OK;
}

int cidnet_jpeg_encode_u8(const uint8_t* src, long src_stride, uint8_t* dst, long dst_stride, long long* sizes, void* ws,
                          long ws_bytes, const int* qtab, int B, int h, int w, void* stream) {
  CIDNET_CHECK_ARG(src && dst && sizes && ws && qtab && B >= 1);
  EncPlan p;
  const int rc = jpegenc_plan(h, w, &p);
  if (rc != CIDNET_OK) return rc;
  CIDNET_CHECK_ARG(dst_stride >= p.capacity && (dst_stride & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)ws & 15) == 0 &&
                   ((uintptr_t)sizes & 7) == 0 && ((uintptr_t)qtab & 3) == 0 && src_stride >= 3L * h * w);
  if (B > 65535) return CIDNET_ERR_SHAPE;
  if (ws_bytes < (long)B * p.ws_image) return CIDNET_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* wsb = reinterpret_cast<uint8_t*>(ws);
  Geo g;
  g.mcu_cols = p.mcu_cols; g.bw = p.bw; g.bh = p.bh; g.mcus = p.mcus; g.groups = p.groups; g.bits_off = p.bits_off;
  g.rec_off = p.rec_off; g.stream_off = p.stream_off; g.stream_bytes = p.stream_bytes; g.ws_image = p.ws_image;
  const dim3 per_group((unsigned)p.groups, B), per_image(B);
  hipLaunchKernelGGL(jpegenc_transform_kernel, dim3(p.tiles_x, p.mcu_rows, B), dim3(kTransformThreads), 0, st, src, src_stride, wsb,
                     p.ws_image, qtab, h, w, p.mcu_cols, (h + 1) / 2);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(jpegenc_count_kernel, per_group, dim3(kThreads), 0, st, wsb, g);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(jpegenc_offsets_kernel, per_image, dim3(kThreads), 0, st, wsb, g);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(jpegenc_emit_kernel, per_group, dim3(kThreads), 0, st, wsb, g);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(jpegenc_stuff_scan_kernel, per_image, dim3(kThreads), 0, st, wsb, g, sizes);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(jpegenc_copy_kernel, per_group, dim3(kThreads), 0, st, wsb, g, dst, dst_stride, p.capacity);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
