// Read summary of a chunk that lies in HBM (include/fqgpu.h: fqgpu_chunk_stats, fqgpu_dblock_stats): counts of bases and
// qualities by position in the read, histograms of read length, mean quality and GC content.  Extension: nothing in the
// reference.
//
// One pass over the sequence and quality lines by the chunk's device record table.  A wave takes a span of 16 consecutive
// records at a time -- their table entries with one load, a span ahead -- and counts them one after the other while the
// first bytes of the next four are on their way.  Within a record lane = position: every wave-load is 64 consecutive bytes
// of one line, and the 64 lanes of a count land in 64 different rows of the table.  The table of a workgroup lives in LDS
// as u32 -- a chunk is shorter than 2^32 bytes, so no cell can overflow --: STATS_WINDOW_ROWS rows of 64 quality + 5 base
// columns.  69 words is odd, so the rows a wave touches in one column (constant data) lie on different banks.  One more
// row stands for row P ("every position >= P") when P is beyond the window; positions between the window and P -- long
// reads at a large P -- are added to the result in global memory directly (correct, slow, rare).  The per-read values
// (Phred sum, G + C, N) travel packed in one u64 per lane and are summed over the wave by shuffles; lane 0 files the read.
// Reads shorter than 64 leave lanes idle for their one step; the four records in flight per wave keep the loads coming.
//
// The grid is persistent, one workgroup per compute unit (the table fills most of a CU's LDS), spans dealt out wave by
// wave.  At the end every workgroup stores its table to a slab of its own, and k_stats_reduce adds the slabs -- sixteen to
// a thread, zero sums skipped -- into the u64 result.  Integer sums: the result does not depend on the order.
#include "fqgpu_internal.h"

namespace {

constexpr unsigned STATS_THREADS = 1024;      // threads of a workgroup: 16 waves, one span each at a time
constexpr unsigned STATS_WINDOW_ROWS = 320;   // positions 0 .. 319 are counted in LDS
constexpr unsigned STATS_ROW_WORDS = 69;      // 64 quality columns, 5 base columns
constexpr unsigned STATS_UNROLL = 4;          // 64-position steps of a record whose loads are in flight together
constexpr unsigned STATS_SPAN_RECORDS = 16;   // consecutive records a wave takes at a time: its span of the record table
constexpr unsigned STATS_STAGES = 4;          // records of a span whose first bytes are in flight while one is counted
constexpr unsigned STATS_REDUCE_SLABS = 16;   // slabs a thread of k_stats_reduce adds
constexpr unsigned STATS_HEAD = 176;          // the result's fixed words (include/fqgpu.h), at the same places in a slab
constexpr unsigned W_BASES = 1, W_MINLEN = 2, W_MAXLEN = 3, W_WITH_N = 4, W_MEANQ = 8, W_GC = 72;
// a slab (and the LDS of a workgroup), u32 words: head | len_hist[WINDOW + 1] | cells[WINDOW + 1][ROW_WORDS];
// entry WINDOW of both tables is row P when P >= WINDOW.  The head's W_MINLEN holds ~min_len, so that zero is neutral.
constexpr unsigned SLAB_LEN = STATS_HEAD, SLAB_CELLS = SLAB_LEN + STATS_WINDOW_ROWS + 1;
constexpr unsigned SLAB_WORDS = SLAB_CELLS + (STATS_WINDOW_ROWS + 1) * STATS_ROW_WORDS;
constexpr unsigned NO_ROW = 0xFFFFFFFFu;
static_assert(SLAB_WORDS * 4 <= 160 * 1024, "a slab is one workgroup's LDS");
static_assert(STATS_SPAN_RECORDS <= 64 && STATS_STAGES <= STATS_SPAN_RECORDS, "a span's entries sit in the lanes of one wave");
static_assert(STATS_ROW_WORDS % 2 == 1 && STATS_ROW_WORDS == FQGPU_QUAL_ALPHA + 5, "odd row: 64 rows, 64 banks");

__host__ __device__ inline unsigned long long stats_len_word(unsigned row) { return STATS_HEAD + row; }
__host__ __device__ inline unsigned long long stats_base_word(unsigned P, unsigned row, unsigned b) {
  return STATS_HEAD + (P + 1ull) + 5ull * row + b;
}
__host__ __device__ inline unsigned long long stats_qual_word(unsigned P, unsigned row, unsigned q) {
  return STATS_HEAD + 6ull * (P + 1ull) + 64ull * row + q;
}

// where row (<= P) is counted in LDS: its own place inside the window, the spare place for row P, or nowhere
__device__ __forceinline__ unsigned stats_lds_row(unsigned row, unsigned P) {
  return row < STATS_WINDOW_ROWS ? row : (row == P ? STATS_WINDOW_ROWS : NO_ROW);
}

__device__ __forceinline__ unsigned stats_base_code(unsigned c) {
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? 4u : 5u;
}

// per-read values of a lane, packed: Phred sum [0, 24), G + C [24, 41), N [41, 58) -- a read has at most 65535 symbols
constexpr unsigned PK_GC = 24, PK_N = 41;

// what a wave keeps of one record on its way through the pipeline: the table entry (uniform) and the bytes of its first
// 64 * STATS_UNROLL positions, lane = position
struct StatsStage {
  fqgpu_rec rec;
  bool ok;  // a record of this chunk: its bytes were asked for
  unsigned s[STATS_UNROLL], q[STATS_UNROLL];
};

__device__ __forceinline__ void stats_load(unsigned (&s)[STATS_UNROLL], unsigned (&q)[STATS_UNROLL], const uint8_t *sp, const uint8_t *qp,
                                           unsigned p0, unsigned len, unsigned lane) {
#pragma unroll
  for (unsigned k = 0; k < STATS_UNROLL; k++) {
    const unsigned p = p0 + 64 * k + lane;
    s[k] = p < len ? sp[p] : 0u;
    q[k] = p < len ? qp[p] : 0u;
  }
}

__global__ void __launch_bounds__(STATS_THREADS)
k_stats_count(const uint8_t *__restrict__ raw, unsigned long long raw_len, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
              unsigned P, uint32_t *__restrict__ slabs, unsigned long long *__restrict__ out, unsigned *__restrict__ bad) {
  extern __shared__ uint32_t lds[];
  for (unsigned i = threadIdx.x; i < SLAB_WORDS; i += STATS_THREADS) lds[i] = 0;
  __syncthreads();
  uint32_t *const len_hist = lds + SLAB_LEN, *const cells = lds + SLAB_CELLS;
  const unsigned lane = fq_lane(), waves = gridDim.x * (STATS_THREADS / 64);
  const unsigned n_spans = (n_recs + STATS_SPAN_RECORDS - 1) / STATS_SPAN_RECORDS;
  unsigned w_bases = 0, w_min = 0xFFFFFFFFu, w_max = 0, w_with_n = 0;  // of the wave's records (the same in every lane)
  bool w_bad = false;

  // lane k < STATS_SPAN_RECORDS: entry k of a span's part of the record table (len 0 behind the table's end)
  const auto span_table = [&](unsigned span) {
    const unsigned long long r = (unsigned long long)span * STATS_SPAN_RECORDS + lane;
    fqgpu_rec e = {0u, 0u, 0u};
    if (lane < STATS_SPAN_RECORDS && r < n_recs) e = recs[r];
    return e;
  };
  // record k of the span in hand: its entry to every lane, and the loads of its first bytes
  const auto fetch = [&](StatsStage &st, const fqgpu_rec &mine, unsigned k) {
    st.rec.seq_off = __builtin_amdgcn_readlane(mine.seq_off, k);
    st.rec.qual_off = __builtin_amdgcn_readlane(mine.qual_off, k);
    st.rec.len = __builtin_amdgcn_readlane(mine.len, k);
    st.ok = st.rec.len != 0 && st.rec.len <= 65535u && (unsigned long long)st.rec.seq_off + st.rec.len <= raw_len &&
            (unsigned long long)st.rec.qual_off + st.rec.len <= raw_len;
    if (st.ok) stats_load(st.s, st.q, raw + st.rec.seq_off, raw + st.rec.qual_off, 0, st.rec.len, lane);  // (uniform)
  };
  const auto count = [&](const StatsStage &st) {
    const fqgpu_rec rec = st.rec;
    if (!st.ok) {  // (uniform) not a record of this chunk: nothing of it was read
      w_bad = true;
      return;
    }
    unsigned long long acc = 0;
    for (unsigned p0 = 0; p0 < rec.len; p0 += 64 * STATS_UNROLL) {
      unsigned s[STATS_UNROLL], q[STATS_UNROLL];
      if (p0 == 0) {
#pragma unroll
        for (unsigned k = 0; k < STATS_UNROLL; k++) { s[k] = st.s[k]; q[k] = st.q[k]; }
      } else {  // a long read: the rest of it is not loaded ahead
        stats_load(s, q, raw + rec.seq_off, raw + rec.qual_off, p0, rec.len, lane);
      }
#pragma unroll
      for (unsigned k = 0; k < STATS_UNROLL; k++) {
        const unsigned p = p0 + 64 * k + lane;
        if (p >= rec.len) continue;
        const unsigned row = p < P ? p : P, at = stats_lds_row(row, P);
        const unsigned b = stats_base_code(s[k]), ph = q[k] - 33u;
        if (b > 4u || ph > 63u) w_bad = true;
        if (b <= 4u) {
          if (at != NO_ROW) atomicAdd(&cells[at * STATS_ROW_WORDS + 64 + b], 1u);
          else atomicAdd(&out[stats_base_word(P, row, b)], 1ull);
          acc += (unsigned long long)(b == 1u || b == 2u) << PK_GC | (unsigned long long)(b == 4u) << PK_N;
        }
        if (ph <= 63u) {
          if (at != NO_ROW) atomicAdd(&cells[at * STATS_ROW_WORDS + ph], 1u);
          else atomicAdd(&out[stats_qual_word(P, row, ph)], 1ull);
          acc += ph;
        }
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    const unsigned q_sum = (unsigned)(acc & ((1u << PK_GC) - 1u)), gc = (unsigned)(acc >> PK_GC) & 0x1FFFFu, n = (unsigned)(acc >> PK_N);
    w_bases += rec.len;
    w_min = min(w_min, rec.len);
    w_max = max(w_max, rec.len);
    w_with_n += n != 0;
    if (lane == 0) {
      atomicAdd(&lds[W_MEANQ + q_sum / rec.len], 1u);
      atomicAdd(&lds[W_GC + 100u * gc / rec.len], 1u);
      const unsigned row = rec.len < P ? rec.len : P, at = stats_lds_row(row, P);
      if (at != NO_ROW) atomicAdd(&len_hist[at], 1u);
      else atomicAdd(&out[stats_len_word(row)], 1ull);
    }
  };

  // A wave takes spans of STATS_SPAN_RECORDS consecutive records.  The span's table entries arrive with ONE load, a span
  // ahead; the bytes of STATS_STAGES records are in flight while the record in front of them is counted.
  unsigned span = blockIdx.x * (STATS_THREADS / 64) + (threadIdx.x >> 6);
  fqgpu_rec next = span < n_spans ? span_table(span) : fqgpu_rec{0u, 0u, 0u};
  for (; span < n_spans; span += waves) {
    const fqgpu_rec mine = next;
    if (span + waves < n_spans) next = span_table(span + waves);
    const unsigned here = min(STATS_SPAN_RECORDS, n_recs - span * STATS_SPAN_RECORDS);  // records of this span
    StatsStage st[STATS_STAGES];
#pragma unroll
    for (unsigned d = 0; d < STATS_STAGES; d++)
      if (d < here) fetch(st[d], mine, d);
    for (unsigned g = 0; g < here; g += STATS_STAGES) {
#pragma unroll
      for (unsigned d = 0; d < STATS_STAGES; d++) {
        if (g + d >= here) break;
        count(st[d]);
        if (g + d + STATS_STAGES < here) fetch(st[d], mine, g + d + STATS_STAGES);
      }
    }
  }
  if (__any(w_bad) && lane == 0) *bad = 1u;  // (every writer stores the same value)
  if (lane == 0 && w_max) {
    atomicAdd(&lds[W_BASES], w_bases);
    atomicMax(&lds[W_MINLEN], ~w_min);
    atomicMax(&lds[W_MAXLEN], w_max);
    atomicAdd(&lds[W_WITH_N], w_with_n);
  }
  __syncthreads();
  uint32_t *const slab = slabs + (size_t)blockIdx.x * SLAB_WORDS;
  for (unsigned i = threadIdx.x; i < SLAB_WORDS; i += STATS_THREADS) slab[i] = lds[i];
}

// out += the slabs: thread x of row y takes word x of the slabs [16 y, 16 y + 16)
__global__ void __launch_bounds__(256)
k_stats_reduce(const uint32_t *__restrict__ slabs, unsigned n_slabs, unsigned P, unsigned long long *__restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= SLAB_WORDS) return;
  const unsigned s0 = blockIdx.y * STATS_REDUCE_SLABS, s1 = min(n_slabs, s0 + STATS_REDUCE_SLABS);
  const bool is_max = i == W_MINLEN || i == W_MAXLEN;
  unsigned long long v = 0;
  for (unsigned s = s0; s < s1; s++) {
    const uint32_t x = slabs[(size_t)s * SLAB_WORDS + i];
    v = is_max ? max(v, (unsigned long long)x) : v + x;
  }
  if (!v) return;
  if (i < STATS_HEAD) {
    if (is_max) atomicMax(&out[i], v);
    else atomicAdd(&out[i], v);
    return;
  }
  // a place of the window is its own row; the spare place is row P (in use only when P lies beyond the window)
  const bool cell = i >= SLAB_CELLS;
  const unsigned j = cell ? i - SLAB_CELLS : i - SLAB_LEN, at = cell ? j / STATS_ROW_WORDS : j, c = cell ? j % STATS_ROW_WORDS : 0u;
  const unsigned row = at < STATS_WINDOW_ROWS ? at : P;
  atomicAdd(&out[!cell ? stats_len_word(row) : c < 64u ? stats_qual_word(P, row, c) : stats_base_word(P, row, c - 64u)], v);
}

}  // namespace

void StatsScratch::release_host() {
  if (host_bad) (void)hipHostFree(host_bad);
  host_bad = nullptr;
  attr_set = false;
}

// The summary of the chunk v (raw_dev[0, raw_len) with the record table recs_dev), on st, waited for: out[0, fqgpu_stats_words(P)).
// FQGPU_E_ARG with out zeroed: a byte that cannot be counted, or a record that is not inside the chunk or has no symbol
// (len 0: no parser of this project makes one, and a read without symbols has no mean quality and no GC content).
int fq_stats_chunk(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, unsigned P, uint64_t *out) {
  const uint8_t *const raw_dev = v.raw;
  const fqgpu_rec *const recs_dev = v.recs;
  const size_t raw_len = v.raw_len, n_recs = v.n_recs;
  const size_t words = fqgpu_stats_words(P);
  if (!words || n_recs >= ((size_t)1 << 32) || raw_len >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  StatsScratch &ss = ctx->stats;
  constexpr unsigned wg_waves = STATS_THREADS / 64;
  const size_t n_spans = (n_recs + STATS_SPAN_RECORDS - 1) / STATS_SPAN_RECORDS;
  const unsigned n_wgs = (unsigned)min((size_t)ctx->n_cus, (n_spans + wg_waves - 1) / wg_waves);
  int rc;
  if ((rc = ss.out.reserve(words * 8)) || (rc = ss.slabs.reserve((size_t)max(n_wgs, 1u) * SLAB_WORDS * 4)) || (rc = ss.bad.reserve(4))) return rc;
  if (!ss.host_bad) FQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&ss.host_bad), 4, hipHostMallocPortable));
  if (!ss.attr_set) {
    FQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_stats_count), hipFuncAttributeMaxDynamicSharedMemorySize, SLAB_WORDS * 4));
    ss.attr_set = true;
  }
  unsigned long long *const out_dev = ss.out.as<unsigned long long>();
  FQ_HIP(hipMemsetAsync(out_dev, 0, words * 8, st));
  FQ_HIP(hipMemsetAsync(ss.bad.p, 0, 4, st));
  if (n_wgs) {
    fq_timer_span_begin(ctx, "stats", st);
    hipLaunchKernelGGL(k_stats_count, dim3(n_wgs), dim3(STATS_THREADS), SLAB_WORDS * 4, st, raw_dev, (unsigned long long)raw_len, recs_dev,
                       (unsigned)n_recs, P, ss.slabs.as<uint32_t>(), out_dev, ss.bad.as<unsigned>());
    hipLaunchKernelGGL(k_stats_reduce, dim3((SLAB_WORDS + 255) / 256, (n_wgs + STATS_REDUCE_SLABS - 1) / STATS_REDUCE_SLABS), dim3(256), 0, st,
                       ss.slabs.as<uint32_t>(), n_wgs, P, out_dev);
    fq_timer_span_end(ctx, st);
    FQ_HIP(hipGetLastError());
  }
  FQ_HIP(hipMemcpyAsync(ss.host_bad, ss.bad.p, 4, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipMemcpyAsync(out, out_dev, words * 8, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  if (*ss.host_bad) {
    for (size_t i = 0; i < words; i++) out[i] = 0;
    return FQGPU_E_ARG;
  }
  out[0] = n_recs;
  out[W_MINLEN] = n_recs ? 0xFFFFFFFFull - out[W_MINLEN] : 0;  // (the slabs hold ~min_len)
  out[5] = P;
  return FQGPU_OK;
}
