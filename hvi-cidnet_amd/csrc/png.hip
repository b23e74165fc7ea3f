// The PNG writer's IDAT payload on the device (include/cidnet_hip.h: cidnet_png_*; tests/png_ref.py is the
// contract, byte for byte): interleaved uint8 (B,h,w,3) -> per image one complete zlib stream -- per-row PNG filters, then one
// dynamic-Huffman deflate block per segment of whole rows, literals only (no LZ77 search: on photographs it buys nothing and
// it is what costs zlib its time).  Integer arithmetic only.  The host keeps the chunk framing and the CRC-32.
//
// Three launches on one stream, grid (segments, B) for the two that work:
//   0. png_zero_kernel: the B output slots become zero (the packer ORs into the two dwords a block shares with its neighbours).
//   A. png_filter_kernel: a wave takes a row, a lane four consecutive bytes of it (four unaligned dword loads: the bytes, their
//      left, up and up-left neighbours): the five candidate filters' scores sum |v| (v as a signed byte) in one pass, a
//      wave-wide reduction picks the type, a second pass writes the filtered bytes into the workspace and counts them into the
//      wave's own LDS histogram (lanes that hold lane 0's value are added as one: a constant image would otherwise put 64
//      lanes on one counter).  Then the block ranks the used (count, symbol) keys in parallel and ONE lane runs the code-length
//      procedure of png_codes.h on the sorted keys, for the literal code (limit 15) and for the code-length code (limit 7), and
//      assembles the block header's bits.  The segment's record -- code table, header bits, bit count, Adler partial sums --
//      goes to the workspace.
//   B. png_pack_kernel: the block sums the bit counts of the segments before it (its bit offset), then takes 2048 bytes at a
//      time: eight symbols per thread concatenated in two 64-bit registers, a block scan of the bit lengths, ds_or into a
//      zeroed LDS window, whole dwords stored.  Only the block's first and last dword can be shared with a neighbour: those two
//      are ORed into the zeroed slot, so the bytes do not depend on the order in which blocks arrive.  The image's last block
//      adds the end of block, the pad to a byte, the Adler-32 (combined from the segments' partial sums) and sizes[b].
// Workspace per image: the filtered bytes h (1 + 3 w), rounded up to 16, then one record of kRecBytes per segment.
#include "cidnet_hip.h"
#include "common.h"
#include "png_codes.h"

namespace cidnet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 8;                          // symbols a thread of the packer encodes per chunk
constexpr int kChunk = kThreads * kPerThread;          // 2048
constexpr int kHdrDwords = 64;                         // a block header takes at most 17 + 57 + 259 * 7 = 1887 bits
constexpr int kHdrBitsMax = 17 + 19 * 3 + 259 * 7;
constexpr int kTabDwords = 260;                        // 257 code-table entries, padded
constexpr int kRecBytes = (kTabDwords + kHdrDwords) * 4 + 32;    // + bit count, header bits, Adler sum, Adler weighted sum
constexpr int kBufDwords = (31 + kChunk * 15 + 15 + 7 + 32) / 32 + 2;
constexpr long kMaxSegmentBytes = 1L << 22;            // a count must fit a sort key (png_codes.h) with room to spare
constexpr unsigned kAdlerMod = 65521u;
constexpr int kAdaptive = 5;

struct PngPlan {
  long rows, segments, last_short, row_exceeds, ws_image, capacity, row_bytes, filt_bytes;
};

// The one place the segments, the workspace and the slot are decided: the launcher and the query call it.
// The slot bound: a block's header is at most 1887 bits.  Its n symbols (the bytes and the end of block) cost
// at most 9 n bits where the limiter cannot run -- a Huffman code is no dearer than the flat 9-bit code, and a tree deeper than
// 15 needs a total count of at least F(18) = 2584 -- and at most 11 n bits where it can: after k halvings the code is optimal
// for counts c' with c <= 2^k c' and sum c' < n / 2^k + 257, so it costs less than 9 n + 9 * 257 * 2^k, and the k-th halving
// needs 2584 <= n / 2^(k-1) + 257, i.e. 2^k <= 2 n / 2327.
int png_plan(int h, int w, int segment_bytes, PngPlan* p) {
  if (h < 1 || w < 1 || segment_bytes < 1) return CIDNET_ERR_ARG;
  const long row = 1 + 3L * w;
  long rows = segment_bytes / row;
  if (rows < 1) rows = 1;
  if (rows > h) rows = h;
  if (rows * row > kMaxSegmentBytes) return CIDNET_ERR_SHAPE;
  rows = segment_bytes / row < 1 ? 1 : segment_bytes / row;      // reported as the contract states it: not clipped to h
  const long per = rows < h ? rows : h;
  p->rows = rows;
  p->segments = (h + per - 1) / per;
  p->last_short = h % per != 0;
  p->row_exceeds = row > segment_bytes;
  p->row_bytes = row;
  p->filt_bytes = (h * row + 15) / 16 * 16;
  p->ws_image = p->filt_bytes + p->segments * kRecBytes;
  long bits = 0;
  for (long s = 0; s < p->segments; ++s) {
    const long left = h - s * per, n = (left < per ? left : per) * row + 1;
    bits += kHdrBitsMax + (n < 2584 ? 9 : 11) * n;
  }
  p->capacity = (2 + (bits + 7) / 8 + 4 + 3) / 4 * 4;
  return CIDNET_OK;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// the sum over the block, in every thread.  red: kWaves words of LDS, free to be reused after the call's last barrier
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
  v = wave_sum_u64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) t += red[i];
  return t;
}

// the five filtered values of byte x with left a, up b, up-left c (PNG specification 9.2, 9.4), each mod 256
__device__ __forceinline__ void candidates(int x, int a, int b, int c, int* f) {
  const int p = a + b - c;
  int pa = p - a, pb = p - b, pc = p - c;
  pa = pa < 0 ? -pa : pa;
  pb = pb < 0 ? -pb : pb;
  pc = pc < 0 ? -pc : pc;
  const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  f[0] = x;
  f[1] = (x - a) & 255;
  f[2] = (x - b) & 255;
  f[3] = (x - ((a + b) >> 1)) & 255;
  f[4] = (x - pred) & 255;
}

// four bytes at any address as one dword access (gfx950 takes unaligned global dwords)
__device__ __forceinline__ unsigned ld4(const uint8_t* p) {
  unsigned v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ void st4(uint8_t* p, unsigned v) { __builtin_memcpy(p, &v, 4); }

// bytes i .. i + 3 of a row of n bytes with their left, up and up-left neighbours; positions at or past n read as 0.
// Inside the row (3 <= i, i + 4 <= n) four dword loads, at the row's two ends byte loads.
__device__ __forceinline__ void load_group(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, bool up, long i,
                                           long n, int* x, int* a, int* b, int* c) {
  if (i >= 3 && i + 4 <= n) {
    const unsigned xw = ld4(cur + i), aw = ld4(cur + i - 3), bw = up ? ld4(prev + i) : 0u, cw = up ? ld4(prev + i - 3) : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = (xw >> (8 * k)) & 255;
      a[k] = (aw >> (8 * k)) & 255;
      b[k] = (bw >> (8 * k)) & 255;
      c[k] = (cw >> (8 * k)) & 255;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long j = i + k;
      const bool in = j < n;
      x[k] = in ? cur[j] : 0;
      a[k] = (in && j >= 3) ? cur[j - 3] : 0;
      b[k] = (in && up) ? prev[j] : 0;
      c[k] = (in && up && j >= 3) ? prev[j - 3] : 0;
    }
  }
}

// one value per lane into the wave's histogram; every lane of the wave is here.  The active lanes that hold lane 0's value
// (whether lane 0 itself is active or not) are added as one, by the lowest of them
__device__ __forceinline__ void hist_add(unsigned* hist, int v, bool active, int lane) {
  const int v0 = __builtin_amdgcn_readfirstlane(v);
  const unsigned long long same = __ballot(active && v == v0);
  if (active) {
    if (v == v0) {
      if (lane == __ffsll((long long)same) - 1) atomicAdd(&hist[v0], (unsigned)__popcll(same));
    } else {
      atomicAdd(&hist[v], 1u);
    }
  }
}

__device__ __forceinline__ void put_bits(unsigned* words, unsigned* pos, unsigned value, unsigned n) {
  const unsigned at = *pos, wd = at >> 5, sh = at & 31;
  words[wd] |= value << sh;
  if (sh + n > 32) words[wd + 1] |= value >> (32 - sh);
  *pos = at + n;
}

struct Record {
  unsigned* table;
  unsigned* hdr;
  unsigned long long* meta;                            // total bits | header bits | sum d | sum (L - i) d_i
};

__device__ __forceinline__ Record record(uint8_t* ws_image, long filt_bytes, long s) {
  uint8_t* r = ws_image + filt_bytes + s * kRecBytes;
  Record rec;
  rec.table = reinterpret_cast<unsigned*>(r);
  rec.hdr = rec.table + kTabDwords;
  rec.meta = reinterpret_cast<unsigned long long*>(rec.hdr + kHdrDwords);
  return rec;
}

__global__ __launch_bounds__(kThreads) void png_zero_kernel(unsigned* __restrict__ dst, long stride_dw, long cap_dw) {
  unsigned* slot = dst + (long)blockIdx.y * stride_dw;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < cap_dw; i += (long)gridDim.x * kThreads) slot[i] = 0u;
}

// grid (segments, B).  filter: 0..4 forces a type, kAdaptive chooses per row
__global__ __launch_bounds__(kThreads) void png_filter_kernel(const uint8_t* __restrict__ src, long src_stride,
                                                              uint8_t* __restrict__ ws, long ws_image, long filt_bytes, int h,
                                                              int w, long rows, int filter) {
  __shared__ unsigned hist[kWaves][kTabDwords];
  __shared__ unsigned freq[kTabDwords];
  __shared__ unsigned keys[png::kSymbols];
  __shared__ unsigned wt[2 * png::kSymbols];
  __shared__ uint16_t par[2 * png::kSymbols];
  __shared__ uint8_t lens[kTabDwords];
  __shared__ unsigned codes[kTabDwords];
  __shared__ unsigned hdr[kHdrDwords];
  __shared__ unsigned clfreq[20], clkeys[20], clcodes[20];
  __shared__ uint8_t cllens[20];
  __shared__ unsigned long long sums[3];               // Adler sum, Adler weighted sum, bit count
  __shared__ unsigned long long red[kWaves];
  __shared__ unsigned used, hdr_bits;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long seg = blockIdx.x, row = 1 + 3L * w, n = 3L * w;
  const long r0 = seg * rows, r1 = r0 + rows < h ? r0 + rows : h;
  const long L = (r1 - r0) * row;
  const uint8_t* img = src + (long)blockIdx.y * src_stride;
  uint8_t* wi = ws + (long)blockIdx.y * ws_image;

  for (int i = tid; i < kWaves * kTabDwords; i += kThreads) (&hist[0][0])[i] = 0u;
  for (int i = tid; i < kTabDwords; i += kThreads) lens[i] = 0;
  if (tid < kHdrDwords) hdr[tid] = 0u;
  if (tid < 3) sums[tid] = 0ull;
  if (tid == 0) used = 0u;
  __syncthreads();

  unsigned long long asum = 0, wsum = 0;
  for (long r = r0 + wv; r < r1; r += kWaves) {
    const uint8_t* cur = img + r * n;
    const uint8_t* prev = cur - n;                     // read only where r > 0
    const bool up = r > 0;
    int type = filter;
    if (filter == kAdaptive) {
      unsigned score[5] = {0u, 0u, 0u, 0u, 0u};
      for (long i = 4L * lane; i < n; i += 256) {        // a lane takes four consecutive bytes
        int x[4], a[4], b[4], c[4];
        load_group(cur, prev, up, i, n, x, a, b, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (i + k < n) {
            int f[5];
            candidates(x[k], a[k], b[k], c[k], f);
#pragma unroll
            for (int t = 0; t < 5; ++t) score[t] += (unsigned)(f[t] < 256 - f[t] ? f[t] : 256 - f[t]);
          }
        }
      }
      unsigned best = 0;
      type = 0;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const unsigned sc = wave_sum_u32(score[t]);
        if (t == 0 || sc < best) {                     // ties go to the lowest type
          best = sc;
          type = t;
        }
      }
    }
    uint8_t* out = wi + r * row;
    const long p0 = (r - r0) * row;                    // position of the type byte inside the segment
    if (lane == 0) {
      out[0] = (uint8_t)type;
      asum += (unsigned)type;
      wsum += (unsigned long long)(L - p0) * (unsigned)type;
    }
    hist_add(hist[wv], type, lane == 0, lane);
    for (long base = 0; base < n; base += 256) {
      const long i = base + 4L * lane;
      int v[4] = {0, 0, 0, 0};
      if (i < n) {
        int x[4], a[4], b[4], c[4];
        load_group(cur, prev, up, i, n, x, a, b, c);
        unsigned packed = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (i + k < n) {
            int f[5];
            candidates(x[k], a[k], b[k], c[k], f);
            v[k] = type == 0 ? f[0] : type == 1 ? f[1] : type == 2 ? f[2] : type == 3 ? f[3] : f[4];
            packed |= (unsigned)v[k] << (8 * k);
            asum += (unsigned)v[k];
            wsum += (unsigned long long)(L - (p0 + 1 + i + k)) * (unsigned)v[k];
          }
        }
        if (i + 4 <= n) {
          st4(out + 1 + i, packed);
        } else {
          for (int k = 0; i + k < n; ++k) out[1 + i + k] = (uint8_t)v[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) hist_add(hist[wv], v[k], i + k < n, lane);
    }
  }
  asum = wave_sum_u64(asum);
  wsum = wave_sum_u64(wsum);
  if (lane == 0) {
    atomicAdd(&sums[0], asum);
    atomicAdd(&sums[1], wsum);
  }
  __syncthreads();
  for (int s = tid; s < png::kSymbols; s += kThreads) {
    unsigned f = 1u;                                   // the end of block
    if (s < 256) f = hist[0][s] + hist[1][s] + hist[2][s] + hist[3][s];
    freq[s] = f;
  }
  __syncthreads();
  // the used keys in ascending order: a key's rank is the number of smaller used keys (keys are distinct)
  for (int s = tid; s < png::kSymbols; s += kThreads) {
    const unsigned f = freq[s];
    if (f) {
      const unsigned key = (f << png::kKeyShift) | (unsigned)s;
      int rank = 0;
      for (int j = 0; j < png::kSymbols; ++j) {
        const unsigned fj = freq[j];
        rank += (fj != 0u && ((fj << png::kKeyShift) | (unsigned)j) < key) ? 1 : 0;
      }
      keys[rank] = key;
      atomicAdd(&used, 1u);
    }
  }
  __syncthreads();
  if (tid == 0) {
    png::lengths_from_keys(keys, (int)used, 15, lens, wt, par);
    png::canonical_codes(lens, png::kSymbols, codes);
    // the code-length code over the 257 + 2 lengths sent as plain symbols 0..15 (the two distance codes have length 1)
    for (int i = 0; i < 19; ++i) {
      clfreq[i] = 0u;
      cllens[i] = 0;
    }
    for (int s = 0; s < png::kSymbols; ++s) ++clfreq[lens[s]];
    clfreq[1] += 2u;
    int cm = 0;
    for (int i = 0; i < 19; ++i)
      if (clfreq[i]) clkeys[cm++] = (clfreq[i] << png::kKeyShift) | (unsigned)i;
    png::lengths_from_keys(clkeys, cm, 7, cllens, wt, par);
    if (cm == 1) cllens[cllens[0] ? 1 : 0] = 1;
    png::canonical_codes(cllens, 19, clcodes);
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    unsigned pos = 0;
    put_bits(hdr, &pos, seg == (long)gridDim.x - 1 ? 1u : 0u, 1);           // BFINAL
    put_bits(hdr, &pos, 2u, 2);                                            // BTYPE: dynamic Huffman
    put_bits(hdr, &pos, 0u, 5);                                            // HLIT: 257 codes
    put_bits(hdr, &pos, 1u, 5);                                            // HDIST: 2 codes
    put_bits(hdr, &pos, 15u, 4);                                           // HCLEN: 19 entries
    for (int i = 0; i < 19; ++i) put_bits(hdr, &pos, cllens[order[i]], 3);
    for (int s = 0; s < png::kSymbols; ++s) put_bits(hdr, &pos, clcodes[lens[s]] & 0xffffu, clcodes[lens[s]] >> 16);
    put_bits(hdr, &pos, clcodes[1] & 0xffffu, clcodes[1] >> 16);
    put_bits(hdr, &pos, clcodes[1] & 0xffffu, clcodes[1] >> 16);
    hdr_bits = pos;
  }
  __syncthreads();
  unsigned long long bits = 0;
  Record rec = record(wi, filt_bytes, seg);
  for (int s = tid; s < kTabDwords; s += kThreads) {
    const unsigned e = s < png::kSymbols ? codes[s] : 0u;
    rec.table[s] = e;
    if (s < png::kSymbols) bits += (unsigned long long)freq[s] * (e >> 16);
  }
  if (tid < kHdrDwords) rec.hdr[tid] = hdr[tid];
  bits = block_sum_u64(bits, red);
  if (tid == 0) {
    rec.meta[0] = bits + hdr_bits;
    rec.meta[1] = hdr_bits;
    rec.meta[2] = sums[0];
    rec.meta[3] = sums[1];
  }
}

// OR the low `nb` bits of hi:lo into the window at bit `pos`
__device__ __forceinline__ void or_bits(unsigned* buf, unsigned pos, unsigned long long lo, unsigned long long hi, int nb) {
  const unsigned wd = pos >> 5, sh = pos & 31;
  const unsigned v[4] = {(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
  unsigned carry = 0u;
  int p = 0;
#pragma unroll
  for (; p < 4; ++p) {
    if (p * 32 >= nb) break;
    const unsigned o = (v[p] << sh) | carry;
    carry = sh ? v[p] >> (32 - sh) : 0u;
    if (o) atomicOr(&buf[wd + p], o);
  }
  if (carry) atomicOr(&buf[wd + p], carry);
}

// grid (segments, B)
__global__ __launch_bounds__(kThreads) void png_pack_kernel(uint8_t* __restrict__ ws, long ws_image, long filt_bytes,
                                                            uint8_t* __restrict__ dst, long dst_stride, long cap_dw,
                                                            long long* __restrict__ sizes, int h, int w, long rows) {
  __shared__ unsigned buf[kBufDwords];
  __shared__ unsigned tab[kTabDwords];
  __shared__ unsigned long long red[kWaves];
  __shared__ unsigned wtot[kWaves];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long seg = blockIdx.x, nseg = gridDim.x, row = 1 + 3L * w;
  const long r0 = seg * rows, r1 = r0 + rows < h ? r0 + rows : h;
  const long L = (r1 - r0) * row;
  const bool last = seg == nseg - 1;
  uint8_t* wi = ws + (long)blockIdx.y * ws_image;
  const uint8_t* f = wi + r0 * row;
  unsigned* outw = reinterpret_cast<unsigned*>(dst + (long)blockIdx.y * dst_stride);
  Record rec = record(wi, filt_bytes, seg);

  unsigned long long before = 0;
  for (long j = tid; j < seg; j += kThreads) before += record(wi, filt_bytes, j).meta[0];
  before = block_sum_u64(before, red);
  unsigned adler = 0u;
  if (last) {                                          // uniform per block
    const unsigned long long total = (unsigned long long)h * row;
    unsigned long long sa = 0, sb = 0;
    for (long j = tid; j < nseg; j += kThreads) {
      const Record rj = record(wi, filt_bytes, j);
      const long j0 = j * rows, j1 = j0 + rows < h ? j0 + rows : h;
      const unsigned long long after = total - (unsigned long long)j1 * row;     // bytes behind segment j
      const unsigned long long a = rj.meta[2] % kAdlerMod;
      sa += a;
      sb += (rj.meta[3] % kAdlerMod + (after % kAdlerMod) * a) % kAdlerMod;
    }
    sa = block_sum_u64(sa, red);
    sb = block_sum_u64(sb, red);
    const unsigned a = (unsigned)((1u + sa) % kAdlerMod), b = (unsigned)((total % kAdlerMod + sb) % kAdlerMod);
    adler = (b << 16) | a;
  }
  for (int i = tid; i < kBufDwords; i += kThreads) buf[i] = 0u;
  for (int i = tid; i < kTabDwords; i += kThreads) tab[i] = rec.table[i];
  const unsigned hdr_bits = (unsigned)rec.meta[1];
  __syncthreads();

  const unsigned long long P0 = 16ull + before;        // behind the two bytes 0x78 0x01
  long gword = (long)(P0 >> 5);
  unsigned rel = (unsigned)(P0 & 31);
  bool first = true;
  if (seg == 0 && tid == 0) atomicOr(&outw[0], 0x0178u);

  // header, then chunks: each pass ORs `nbits` bits into the window behind `rel` and then flushes the whole dwords
  long c0 = -1;                                        // -1: the header pass
  for (;;) {
    unsigned nbits;
    bool final_pass;
    if (c0 < 0) {
      if (tid < kHdrDwords && tid * 32 < (int)hdr_bits) or_bits(buf, rel + 32u * tid, rec.hdr[tid], 0ull, 32);
      nbits = hdr_bits;                                // bits of the last word past hdr_bits are zero
      final_pass = false;
    } else {
      unsigned long long lo = 0, hi = 0;
      int nb = 0;
      const long idx = c0 + (long)tid * kPerThread;
      unsigned long long sym = 0;
      if (idx + kPerThread <= L) {
        sym = ld4(f + idx) | ((unsigned long long)ld4(f + idx + 4) << 32);
      } else {
        for (int k = 0; idx + k < L; ++k) sym |= (unsigned long long)f[idx + k] << (8 * k);
      }
#pragma unroll
      for (int k = 0; k < kPerThread; ++k) {
        if (idx + k < L) {
          const unsigned e = tab[(sym >> (8 * k)) & 255];
          const unsigned long long code = e & 0xffffu;
          const int len = (int)(e >> 16);
          if (nb < 64) {
            lo |= code << nb;
            if (nb + len > 64) hi |= code >> (64 - nb);
          } else {
            hi |= code << (nb - 64);
          }
          nb += len;
        }
      }
      unsigned incl = (unsigned)nb;                    // inclusive scan over the wave, then over the waves
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      if (lane == 63) wtot[wv] = incl;
      __syncthreads();
      unsigned off = incl - (unsigned)nb, total = 0u;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) {
        if (i < wv) off += wtot[i];
        total += wtot[i];
      }
      if (nb) or_bits(buf, rel + off, lo, hi, nb);
      nbits = total;
      final_pass = c0 + kChunk >= L;
      if (final_pass) {                                // the end of block; behind the last block the pad and the Adler-32
        const unsigned e = tab[256];
        if (tid == 0) or_bits(buf, rel + nbits, e & 0xffffu, 0ull, (int)(e >> 16));
        nbits += e >> 16;
        if (last) {
          nbits += (8u - ((rel + nbits) & 7u)) & 7u;   // gword * 32 is a multiple of 8
          if (tid == 0) or_bits(buf, rel + nbits, __builtin_bswap32(adler), 0ull, 32);
          nbits += 32u;
        }
      }
    }
    __syncthreads();
    const unsigned endbit = rel + nbits, nfull = endbit >> 5;
    const unsigned carry = buf[nfull];
    for (unsigned t = tid; t < nfull; t += kThreads) {
      const long g = gword + t;
      if (g < cap_dw) {                                // the plan's capacity is a proven bound; never store past the slot
        if (first && t == 0) atomicOr(&outw[g], buf[t]);
        else outw[g] = buf[t];
      }
    }
    __syncthreads();
    for (unsigned t = tid; t <= nfull; t += kThreads) buf[t] = t == 0 ? carry : 0u;
    __syncthreads();
    gword += nfull;
    rel = endbit & 31;
    first = false;
    if (final_pass) break;
    c0 = c0 < 0 ? 0 : c0 + kChunk;
  }
  if (tid == 0) {
    if (rel && gword < cap_dw) atomicOr(&outw[gword], buf[0]);
    if (last) sizes[blockIdx.y] = (long long)((((unsigned long long)gword << 5) + rel) >> 3);
  }
}

}  // namespace
}  // namespace cidnet

using namespace cidnet;

extern "C" {

int cidnet_png_plan(int h, int w, int segment_bytes, long* out, int n) {
  if (!out || n < 6) return CIDNET_ERR_ARG;
  PngPlan p;
  const int rc = png_plan(h, w, segment_bytes, &p);
  if (rc != CIDNET_OK) return rc;
  out[0] = p.rows; out[1] = p.segments; out[2] = p.last_short; out[3] = p.row_exceeds; out[4] = p.ws_image; out[5] = p.capacity;
  return CIDNET_OK;
}

int cidnet_png_code_lengths(const unsigned* freq, int n, int maxbits, uint8_t* lens) {
  if (!freq || !lens || n < 1 || n > png::kSymbols || maxbits < 1 || maxbits > 15) return CIDNET_ERR_ARG;
  unsigned keys[png::kSymbols], wt[2 * png::kSymbols];
  uint16_t par[2 * png::kSymbols];
  int m = 0;
  for (int s = 0; s < n; ++s) {
    lens[s] = 0;
    if (freq[s] > png::kMaxCount) return CIDNET_ERR_SHAPE;
    if (freq[s]) keys[m++] = (freq[s] << png::kKeyShift) | (unsigned)s;
  }
  if (m > 1 && (1 << maxbits) < m) return CIDNET_ERR_SHAPE;      // no code of that depth holds m symbols
  if (m) png::lengths_from_keys(keys, m, maxbits, lens, wt, par);
  return CIDNET_OK;
}

int cidnet_png_encode_u8(const uint8_t* src, long src_stride, uint8_t* dst, long dst_stride, long long* sizes, void* ws,
                         long ws_bytes, int B, int h, int w, int filter, int segment_bytes, void* stream) {
  CIDNET_CHECK_ARG(src && dst && sizes && ws && B >= 1 && filter >= 0 && filter <= kAdaptive);
  PngPlan p;
  const int rc = png_plan(h, w, segment_bytes, &p);
  if (rc != CIDNET_OK) return rc;
  CIDNET_CHECK_ARG(dst_stride >= p.capacity && (dst_stride & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)ws & 15) == 0 &&
                   ((uintptr_t)sizes & 7) == 0 && src_stride >= 3L * h * w);
  if (B > 65535 || p.segments > 0x7fffffffL) return CIDNET_ERR_SHAPE;
  if (ws_bytes < (long)B * p.ws_image) return CIDNET_ERR_WS;
  const long cap_dw = p.capacity / 4;
  hipStream_t st = (hipStream_t)stream;
  const int zb = (int)(cap_dw / (kThreads * 16) < 1 ? 1 : (cap_dw / (kThreads * 16) > 1024 ? 1024 : cap_dw / (kThreads * 16)));
  hipLaunchKernelGGL(png_zero_kernel, dim3(zb, B), dim3(kThreads), 0, st, reinterpret_cast<unsigned*>(dst), dst_stride / 4, cap_dw);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)p.segments, B), dim3(kThreads), 0, st, src, src_stride,
                     reinterpret_cast<uint8_t*>(ws), p.ws_image, p.filt_bytes, h, w, p.rows, filter);
  CIDNET_LAUNCH_STATUS();
  hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)p.segments, B), dim3(kThreads), 0, st, reinterpret_cast<uint8_t*>(ws),
                     p.ws_image, p.filt_bytes, dst, dst_stride, cap_dw, sizes, h, w, p.rows);
  CIDNET_LAUNCH_STATUS();
  return CIDNET_OK;
}

}  // extern "C"
