// The code-length procedure of the PNG writer (tests/png_ref.py: code_lengths) as plain C++, one function for
// the kernel (one lane runs it, on arrays in LDS) and for the host (cidnet_png_code_lengths, which the CPU suite pins to the
// numpy restatement).  No recursion, no allocation, no floating point.
//   1. the used symbols ascending by (count, symbol);  2. the two-queue merge: leaves in that order, internal nodes in the
//   order they were made, the smaller head first and the leaf on equal weight;  3. a symbol's depth is its length;  4. where
//   the deepest exceeds the limit every count becomes (count + 1) >> 1 and the tree is built again;  5. a single used symbol
//   gets length 1.
// A key is count << 9 | symbol in one 32-bit word, so a count must stay below 2^23 (png_plan refuses longer segments).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CIDNET_PNG_HD __host__ __device__ inline
#else
#define CIDNET_PNG_HD inline
#endif

namespace cidnet {
namespace png {

constexpr int kSymbols = 257;                          // literal / length code: the byte values and the end of block
constexpr int kKeyShift = 9;
constexpr unsigned kMaxCount = (1u << 23) - 1;

// insertion sort: linear on keys that are already ascending (the kernel ranks them in parallel before, and the limiter's
// halving keeps them nearly sorted)
CIDNET_PNG_HD void sort_keys(unsigned* keys, int m) {
  for (int i = 1; i < m; ++i) {
    const unsigned k = keys[i];
    int j = i - 1;
    while (j >= 0 && keys[j] > k) {
      keys[j + 1] = keys[j];
      --j;
    }
    keys[j + 1] = k;
  }
}

// keys: the m >= 1 used symbols as count << 9 | symbol, in any order (sorted on return; the counts are the limiter's last).
// wt: 2 m - 1 words, par: 2 m - 1 half-words of scratch.  lens[symbol] is written for the used symbols only.
CIDNET_PNG_HD void lengths_from_keys(unsigned* keys, int m, int maxbits, uint8_t* lens, unsigned* wt, uint16_t* par) {
  if (m == 1) {
    lens[keys[0] & ((1u << kKeyShift) - 1)] = 1;
    return;
  }
  for (;;) {
    sort_keys(keys, m);
    for (int i = 0; i < m; ++i) wt[i] = keys[i] >> kKeyShift;
    int li = 0, ni = m;
    for (int nn = m; nn < 2 * m - 1; ++nn) {
      unsigned sum = 0;
      for (int t = 0; t < 2; ++t) {
        int pick;
        if (li < m && (ni >= nn || wt[li] <= wt[ni])) pick = li++;
        else pick = ni++;
        sum += wt[pick];
        par[pick] = (uint16_t)nn;
      }
      wt[nn] = sum;
    }
    wt[2 * m - 2] = 0;                                 // from here on wt holds depths: a parent is made after its children
    unsigned deepest = 0;
    for (int i = 2 * m - 3; i >= 0; --i) {
      wt[i] = wt[par[i]] + 1;
      if (i < m && wt[i] > deepest) deepest = wt[i];
    }
    if (deepest <= (unsigned)maxbits) break;
    for (int i = 0; i < m; ++i) {
      const unsigned c = keys[i] >> kKeyShift, s = keys[i] & ((1u << kKeyShift) - 1);
      keys[i] = (((c + 1) >> 1) << kKeyShift) | s;
    }
  }
  for (int i = 0; i < m; ++i) lens[keys[i] & ((1u << kKeyShift) - 1)] = (uint8_t)wt[i];
}

// RFC 1951 3.2.2 over lens[0..n), lengths <= 15 -> codes[symbol] = the code bit-reversed (deflate packs Huffman codes MSB
// first into an LSB-first stream) | length << 16; 0 for an unused symbol
CIDNET_PNG_HD void canonical_codes(const uint8_t* lens, int n, unsigned* codes) {
  unsigned count[17], next[17];
  for (int b = 0; b < 17; ++b) count[b] = 0;
  for (int s = 0; s < n; ++s) ++count[lens[s]];
  count[0] = 0;
  unsigned code = 0;
  next[0] = 0;
  for (int b = 1; b < 17; ++b) {
    code = (code + count[b - 1]) << 1;
    next[b] = code;
  }
  for (int s = 0; s < n; ++s) {
    const unsigned l = lens[s];
    if (!l) {
      codes[s] = 0;
      continue;
    }
    unsigned c = next[l]++, r = 0;
    for (unsigned b = 0; b < l; ++b) {
      r = (r << 1) | (c & 1);
      c >>= 1;
    }
    codes[s] = r | (l << 16);
  }
}

}  // namespace png
}  // namespace cidnet
