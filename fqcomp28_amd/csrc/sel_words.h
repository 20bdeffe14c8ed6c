// What select.hip (the selection and the probe) and pair.hip (the calls on two chunks) share: the result words, "a line of a
// record of this chunk" and the packed byte compares on the words of a line.
#pragma once
#include "fqgpu_internal.h"

// the result words on the device: the report (include/fqgpu.h; word 0 is filled in by the host) and the two flags.  Every
// driver of both files frames its work with SelectScratch::begin and SelectScratch::finish (fqgpu_internal.h).
static_assert(FQGPU_FILTER_REPORT_WORDS == FQGPU_TRIM_REPORT_WORDS, "one result struct serves both reports");
struct SelectResult {
  unsigned long long w[FQGPU_TAIL_REPORT_WORDS];
  unsigned int bad;       // a byte that cannot be judged, a record outside the chunk or without symbols
  unsigned int not_bare;  // k_crc_check's verdict: text behind a '+', or the last '\n' outside the chunk
};

namespace {

constexpr unsigned SW_GROUP_LANES = 8;  // lanes that read one record's lines together: select.hip's SEL_GROUP_LANES, asserted equal there

// a line of a record of this chunk: it has symbols, no more than a readlen_t counts, and lies inside the chunk
__device__ __forceinline__ bool sel_line_inside(unsigned off, unsigned len, unsigned long long raw_len) {
  return len != 0 && len <= 65535u && (unsigned long long)off + len <= raw_len;
}

constexpr unsigned SW_H = 0x80808080u, SW_L = 0x01010101u;
// per byte of x (every byte < 128), 0 <= k <= 128: bit 7 set where the byte is >= k
__device__ __forceinline__ unsigned sw_ge(unsigned x, unsigned k) { return ((x | SW_H) - k * SW_L) & SW_H; }
// ... set where the byte equals c
__device__ __forceinline__ unsigned sw_eq(unsigned x, unsigned c) { return ~sw_ge(x ^ (c * SW_L), 1u) & SW_H; }
// 0xFF in the bytes [lo, hi) of a word, 0 <= lo, hi <= 4
__device__ __forceinline__ unsigned sw_mask(int lo, int hi) {
  lo = max(lo, 0);
  hi = min(hi, 4);
  if (lo >= hi) return 0u;
  return (0xFFFFFFFFu >> (8 * (4 - hi))) & (0xFFFFFFFFu << (8 * lo));
}
// bit j set for the bytes lo <= j < hi of a 16-byte word (any lo, hi)
__device__ __forceinline__ unsigned sel_bits(int lo, int hi) {
  lo = min(max(lo, 0), 16);
  hi = min(max(hi, 0), 16);
  return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

constexpr unsigned CLIP_GATHER = 0x00204081u;  // x * this: the bits 7, 15, 23, 31 of x side by side in the bits 28 .. 31
struct __attribute__((packed)) SelU128 { uint32_t a, b, c, d; };  // sixteen bytes at any address

// the record that holds byte o of the output: the last r in [lo, hi] with koff[r] <= o (a dropped record has no byte, so
// koff[r] == koff[r + 1] there and the search steps over it); the caller knows koff[lo] <= o
__device__ __forceinline__ unsigned sel_find(const unsigned long long *__restrict__ koff, unsigned lo, unsigned hi, unsigned long long o) {
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1) >> 1);
    if (koff[mid] <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace
