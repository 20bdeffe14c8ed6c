// The reads of a chunk that lies in HBM which pass a filter (include/fqgpu.h: fqgpu_chunk_filter, fqgpu_dblock_filter), gathered
// on the device so that only the kept bytes come down.  Extension: nothing in the reference.
//
// Three steps on the caller's stream.
//
// k_filter_judge -- one pass over the lines the criteria need, by the chunk's device record table.  A wave takes 64
// consecutive records: their table entries with ONE load, lane = record.  The bytes are then read by parts of the wave: eight
// lanes to a record, eight records at a time, every lane an ALIGNED 16-byte word of a line per load (a line starts anywhere:
// the bytes in front of it and behind it are masked off, and the 64 spare bytes every raw block has behind its chunk let the
// chunk's last word be read whole), the words of the NEXT eight records on their way while those of the
// eight in hand are judged -- so a wait is for the lines of eight records, not for one, and the kernel holds no LDS table, so
// a CU holds many such waves.  The words are judged four bytes at a time (a byte >= 128 is refused first, which makes the
// packed compares exact): the sum of a line's quality bytes by v_sad_u8, "N", "not a base", "Phred below the level", "not a
// quality" by packed compares and a population count.  A record's eight lanes add up by shuffles and hand the three counts back
// to the record's own lane, which gives the verdict, the kept size (the canonical length, or 0), the start of the record's
// header line and -- by one ballot per wave -- the keep bits.  The sequence lines are not loaded at all when max_n is off, the
// quality lines not when min_mean_q and low_q are off: a length-only filter reads the record table alone.  THE BYTES OF A LINE
// THAT IS NOT LOADED ARE NOT JUDGED: a sequence byte outside ACGTN / a quality byte outside 33 .. 96 refuses the chunk only
// when a criterion reads that line.  The report's counters are summed over the wave by shuffles, over the workgroup in LDS,
// and reach global memory as one 64-bit atomic per counter and workgroup.
//
// fq_scan_u32_to_u64 -- the kept sizes become the records' places in the output.
//
// k_filter_gather -- the compacting copy, for a chunk whose '+' lines are bare (k_crc_check's test, made by the judge on the
// way): there a record's canonical bytes are one span of the chunk and a run of consecutive kept records is one longer span,
// so the output is a sequence of runs, each a copy of the chunk shifted by one constant.  The kernel is driven by the
// DESTINATION: a workgroup owns an aligned tile of the output, every lane aligned 16-byte words of it, every store a full
// aligned 16-byte store.  The workgroup finds the records of its tile's first and last byte (two uniform binary searches
// in the offsets); when both lie in one run -- every tile of a filter that keeps everything, most tiles behind long runs --
// the tile is one shifted copy, 16 bytes a lane from wherever the source lies.  Otherwise every lane searches among the
// tile's records: a word inside one run is copied the same way, a word across a seam is put together byte by byte.
// k_filter_gather_records is the form for chunks with text behind a '+' (one wave per kept record, as k_crc_canon_write):
// a correctness path.
//
// All global stores are ordinary vector stores from plain C++.
#include "fqgpu_internal.h"

#include <string.h>

namespace {

constexpr unsigned FILT_THREADS = 256;        // threads of a judge workgroup: four waves
constexpr unsigned FILT_WAVE_RECORDS = 64;    // consecutive records a wave takes: lane = record
constexpr unsigned FILT_GROUP_LANES = 8;      // lanes that read one record's lines together
constexpr unsigned FILT_UNROLL = 2;           // 16-byte words of a line a lane has in flight
constexpr unsigned FILT_GATHER_THREADS = 256; // threads of a gather workgroup
constexpr unsigned FILT_GATHER_WORDS = 4;     // 16-byte words of the output a gather lane writes
constexpr unsigned FILT_ROUND_RECORDS = FILT_WAVE_RECORDS / FILT_GROUP_LANES;  // records a wave reads at a time
constexpr unsigned FILT_STEP_BYTES = FILT_GROUP_LANES * 16 * FILT_UNROLL;      // bytes of a line a record's lanes ask for in one go
constexpr unsigned FILT_TILE_BYTES = FILT_GATHER_THREADS * 16 * FILT_GATHER_WORDS;  // output bytes of a gather workgroup
static_assert(FILT_WAVE_RECORDS == 64 && FILT_GROUP_LANES * FILT_ROUND_RECORDS == 64, "a wave's records sit in its lanes");

// the result words on the device: the report (include/fqgpu.h; word 0 is filled in by the host) and the two flags
struct FilterResult {
  unsigned long long w[FQGPU_FILTER_REPORT_WORDS];
  unsigned int bad;       // a byte that cannot be judged, a record outside the chunk or without symbols
  unsigned int not_bare;  // k_crc_check's verdict: text behind a '+', or the last '\n' outside the chunk
};
constexpr unsigned R_KEPT = 1, R_BASES_IN = 2, R_BASES_KEPT = 3, R_BYTES_KEPT = 4, R_DROPPED = 5, R_COUNTERS = 10;

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

// the aligned 16 bytes at raw + a, a inside the chunk: every raw block has 64 spare bytes behind the chunk (api.hip), so the
// word that holds the chunk's last byte can be read whole; what it holds behind the chunk is masked off by the callers
__device__ __forceinline__ uint4 filt_load16(const uint8_t *__restrict__ raw, unsigned long long a) {
  return *reinterpret_cast<const uint4 *>(raw + a);
}

// what a lane keeps of the record its group reads: the lines' places and the first words of both
struct FiltStage {
  unsigned seq_off, qual_off, len;  // len 0: nothing to read (behind the table's end, or not a record of this chunk)
  uint4 s[FILT_UNROLL], q[FILT_UNROLL];
};

// the lane's words of one line: word k of the lane is the aligned word 8 k + sub of the line, counted from the word that
// holds the line's first byte; p0: bytes of the line (from that word on) asked for before
__device__ __forceinline__ void filt_load_line(uint4 (&v)[FILT_UNROLL], const uint8_t *__restrict__ raw, unsigned off, unsigned len, unsigned p0, unsigned sub) {
  const unsigned lead = off & 15u, span = len ? lead + len : 0u;
  const uint8_t *const line = raw + (off - lead);
#pragma unroll
  for (unsigned k = 0; k < FILT_UNROLL; k++) {
    const unsigned rel = p0 + 16u * (FILT_GROUP_LANES * k + sub);
    v[k] = rel < span ? filt_load16(line, rel) : make_uint4(0, 0, 0, 0);
  }
}

struct FiltCounts {
  unsigned n, qsum, low;  // N of the sequence line; sum of the quality BYTES; quality bytes below the level
  bool bad;
};

// one word of a sequence line: [first, last) are its bytes inside the line
__device__ __forceinline__ void filt_judge_seq(FiltCounts &c, const uint4 v, int first, int last) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned m = sw_mask(first - 4 * i, last - 4 * i), x = w[i] & m;
    if (x & SW_H) c.bad = true;
    const unsigned y = x & ~SW_H, is_n = sw_eq(y, 'N');
    const unsigned base = sw_eq(y, 'A') | sw_eq(y, 'C') | sw_eq(y, 'G') | sw_eq(y, 'T') | is_n;
    if ((base & m) != (SW_H & m)) c.bad = true;
    c.n += __popc(is_n & m);
  }
}

// one word of a quality line; level: the first byte value that is not "low" (33 + low_q)
__device__ __forceinline__ void filt_judge_qual(FiltCounts &c, const uint4 v, int first, int last, unsigned level) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned m = sw_mask(first - 4 * i, last - 4 * i), x = w[i] & m;
    if (x & SW_H) c.bad = true;
    const unsigned y = x & ~SW_H;
    if ((sw_ge(y, 33u) & m) != (SW_H & m) || (sw_ge(y, 97u) & m)) c.bad = true;
    c.qsum = __builtin_amdgcn_sad_u8(x, 0u, c.qsum);
    c.low += __popc(~sw_ge(y, level) & SW_H & m);
  }
}

__global__ void __launch_bounds__(FILT_THREADS)
k_filter_judge(const uint8_t *__restrict__ raw, unsigned long long raw_len, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
               const fqgpu_filter f, uint32_t *__restrict__ ksize, uint32_t *__restrict__ hstart,
               unsigned long long *__restrict__ keep, FilterResult *__restrict__ res) {
  __shared__ unsigned wg[R_COUNTERS];
  if (threadIdx.x < R_COUNTERS) wg[threadIdx.x] = 0;
  __syncthreads();
  const unsigned lane = fq_lane(), sub = lane & (FILT_GROUP_LANES - 1), group = lane / FILT_GROUP_LANES;
  const bool need_seq = f.max_n != FQGPU_FILTER_NONE, need_qual = f.min_mean_q != 0 || f.low_q != 0;
  const unsigned level = 33u + f.low_q;
  const unsigned long long r0 = ((unsigned long long)blockIdx.x * (FILT_THREADS / 64) + (threadIdx.x >> 6)) * FILT_WAVE_RECORDS;
  const unsigned long long r = r0 + lane;
  const bool have = r < n_recs;
  fqgpu_rec mine = {0u, 0u, 0u};
  if (have) mine = recs[r];
  // the start of the record's header line: behind the record in front (its entry sits in the lane in front)
  unsigned h0 = __shfl_up(mine.qual_off + mine.len + 1u, 1);
  if (lane == 0) h0 = have && r ? recs[r - 1].qual_off + recs[r - 1].len + 1u : 0u;
  const bool ok = have && mine.len != 0 && mine.len <= 65535u && (unsigned long long)mine.seq_off + mine.len <= raw_len &&
                  (unsigned long long)mine.qual_off + mine.len <= raw_len;
  bool bad = have && !ok;
  const unsigned read_len = ok ? mine.len : 0u;  // (nothing of a record outside the chunk is read)

  unsigned n_count = 0, q_bytes = 0, low_count = 0;
  if (need_seq || need_qual) {  // (uniform)
    // record j of the wave's 64, for the lanes of the group that reads it
    const auto fetch = [&](FiltStage &st, unsigned j) {
      st.seq_off = __shfl(mine.seq_off, j);
      st.qual_off = __shfl(mine.qual_off, j);
      st.len = __shfl(read_len, j);
      if (need_seq) filt_load_line(st.s, raw, st.seq_off, st.len, 0, sub);
      if (need_qual) filt_load_line(st.q, raw, st.qual_off, st.len, 0, sub);
    };
    const auto judge_words = [&](FiltCounts &c, const uint4 (&v)[FILT_UNROLL], unsigned off, unsigned len, unsigned p0, bool is_seq) {
      const int lead = (int)(off & 15u), span = lead + (int)len;
#pragma unroll
      for (unsigned k = 0; k < FILT_UNROLL; k++) {
        const int rel = (int)(p0 + 16u * (FILT_GROUP_LANES * k + sub));
        if (rel >= span) continue;
        const int first = max(lead - rel, 0), last = min(span - rel, 16);
        if (is_seq) filt_judge_seq(c, v[k], first, last);
        else filt_judge_qual(c, v[k], first, last, level);
      }
    };
    const auto consume = [&](const FiltStage &st) {
      FiltCounts c = {0u, 0u, 0u, false};
      // the words a line can touch, counted from the aligned word of its first byte: the two lines start at different places
      const unsigned span_s = need_seq && st.len ? (st.seq_off & 15u) + st.len : 0u, span_q = need_qual && st.len ? (st.qual_off & 15u) + st.len : 0u;
      if (span_s) judge_words(c, st.s, st.seq_off, st.len, 0, true);
      if (span_q) judge_words(c, st.q, st.qual_off, st.len, 0, false);
      for (unsigned p0 = FILT_STEP_BYTES; p0 < max(span_s, span_q); p0 += FILT_STEP_BYTES) {  // a long read: the rest, not loaded ahead
        uint4 s[FILT_UNROLL], q[FILT_UNROLL];
        if (p0 < span_s) filt_load_line(s, raw, st.seq_off, st.len, p0, sub);
        if (p0 < span_q) filt_load_line(q, raw, st.qual_off, st.len, p0, sub);
        if (p0 < span_s) judge_words(c, s, st.seq_off, st.len, p0, true);
        if (p0 < span_q) judge_words(c, q, st.qual_off, st.len, p0, false);
      }
      // over the record's eight lanes; packed: N and low counts are at most 65535 each, the byte sum below 2^23
      unsigned a = c.n | c.low << 16, b = c.qsum | (c.bad ? 0x80000000u : 0u);
#pragma unroll
      for (unsigned d = 1; d < FILT_GROUP_LANES; d <<= 1) {
        a += __shfl_xor(a, d);
        const unsigned o = __shfl_xor(b, d);
        b = ((b & 0x7FFFFFFFu) + (o & 0x7FFFFFFFu)) | ((b | o) & 0x80000000u);
      }
      return make_uint2(a, b);
    };
    FiltStage cur, nxt;
    fetch(cur, group);
#pragma unroll 1
    for (unsigned k = 0; k < FILT_GROUP_LANES; k++) {  // round k: group g reads record 8 k + g
      if (k + 1 < FILT_GROUP_LANES) fetch(nxt, FILT_ROUND_RECORDS * (k + 1) + group);
      const uint2 got = consume(cur);
      // back to the record's own lane: lane 8 k + g takes what group g's lanes hold
      const unsigned a = __shfl(got.x, (lane & (FILT_ROUND_RECORDS - 1)) * FILT_GROUP_LANES);
      const unsigned b = __shfl(got.y, (lane & (FILT_ROUND_RECORDS - 1)) * FILT_GROUP_LANES);
      if (lane / FILT_ROUND_RECORDS == k) {
        n_count = a & 0xFFFFu;
        low_count = a >> 16;
        q_bytes = b & 0x7FFFFFFFu;
        bad = bad || (b >> 31);
      }
      if (k + 1 < FILT_GROUP_LANES) cur = nxt;
    }
  }

  // the verdict: 0 kept, 1 .. 5 the first criterion that fails
  unsigned verdict = 0;
  if (ok) {
    const unsigned long long phred = need_qual ? q_bytes - 33ull * mine.len : 0ull;
    if (mine.len < f.min_len) verdict = 1;
    else if (mine.len > f.max_len) verdict = 2;
    else if (need_seq && n_count > f.max_n) verdict = 3;
    else if (f.min_mean_q && phred < (unsigned long long)f.min_mean_q * mine.len) verdict = 4;
    else if (f.low_q && 100ull * low_count > (unsigned long long)f.max_low_pct * mine.len) verdict = 5;
  }
  const bool kept = ok && verdict == 0;
  const unsigned hl = mine.seq_off > h0 ? mine.seq_off - h0 : 0u;
  const unsigned long long size64 = (unsigned long long)hl + 2ull * mine.len + 4ull;
  if (kept && size64 > 0xFFFFFFFFull) bad = true;  // (a table that is not this chunk's)
  const unsigned size = kept ? (unsigned)size64 : 0u;
  bool odd = false;
  if (have) {
    ksize[r] = size;
    hstart[r] = h0;
    odd = mine.qual_off != mine.seq_off + mine.len + 3u || mine.seq_off < h0;
    if (r == n_recs - 1u) odd = odd || (unsigned long long)mine.qual_off + mine.len + 1ull > raw_len;
  }
  const unsigned long long kept_mask = __ballot(kept);
  if (lane == 0 && r0 < n_recs) keep[r0 / 64] = kept_mask;
  if (__any(bad) && lane == 0) res->bad = 1u;           // (every writer stores the same value)
  if (__any(odd) && lane == 0) res->not_bare = 1u;

  // the report: over the wave, over the workgroup, one atomic per counter and workgroup
  unsigned cnt[R_COUNTERS];
#pragma unroll
  for (unsigned i = 0; i < R_COUNTERS; i++) cnt[i] = 0;
  cnt[R_KEPT] = kept;
  cnt[R_BASES_IN] = ok ? mine.len : 0u;
  cnt[R_BASES_KEPT] = kept ? mine.len : 0u;
#pragma unroll
  for (unsigned v = 1; v <= 5; v++) cnt[R_DROPPED + v - 1] = verdict == v;
  unsigned long long bytes = size;  // (64 records of up to 2^32 - 1 bytes)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (unsigned i = 1; i < R_COUNTERS; i++)
      if (i != R_BYTES_KEPT) cnt[i] += __shfl_xor(cnt[i], d);
    bytes += __shfl_xor(bytes, d);
  }
  __shared__ unsigned long long wg_bytes;
  if (threadIdx.x == 0) wg_bytes = 0;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (unsigned i = 1; i < R_COUNTERS; i++)
      if (i != R_BYTES_KEPT && cnt[i]) atomicAdd(&wg[i], cnt[i]);
    if (bytes) atomicAdd(&wg_bytes, bytes);
  }
  __syncthreads();
  if (threadIdx.x < R_COUNTERS && threadIdx.x != 0) {
    const unsigned long long v = threadIdx.x == R_BYTES_KEPT ? wg_bytes : wg[threadIdx.x];
    if (v) atomicAdd(&res->w[threadIdx.x], v);
  }
}

// the record that holds byte o of the output: the last r in [lo, hi] with koff[r] <= o (a dropped record has no byte, so
// koff[r] == koff[r + 1] there and the search steps over it); the caller knows koff[lo] <= o
__device__ __forceinline__ unsigned filt_find(const unsigned long long *__restrict__ koff, unsigned lo, unsigned hi, unsigned long long o) {
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1) >> 1);
    if (koff[mid] <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct __attribute__((packed)) FiltU128 { uint32_t a, b, c, d; };  // sixteen bytes at any address

// bare '+' lines: out[koff[r] + i] = raw[hstart[r] + i] for every kept record r
__global__ void __launch_bounds__(FILT_GATHER_THREADS)
k_filter_gather(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ hstart,
                const unsigned long long *__restrict__ koff, unsigned n_recs, unsigned long long total, uint8_t *__restrict__ dst) {
  const unsigned long long t0 = (unsigned long long)blockIdx.x * FILT_TILE_BYTES;
  if (t0 >= total) return;
  const unsigned long long t1 = min(total, t0 + FILT_TILE_BYTES) - 1;  // the tile's last byte
  // (uniform: the compiler keeps these searches in scalar registers)
  const unsigned r_lo = filt_find(koff, 0, n_recs - 1, t0), r_hi = filt_find(koff, r_lo, n_recs - 1, t1);
  const long long d_lo = (long long)hstart[r_lo] - (long long)koff[r_lo], d_hi = (long long)hstart[r_hi] - (long long)koff[r_hi];
  const bool one_run = d_lo == d_hi;  // the records between are kept, or the source would have moved on without the output
#pragma unroll
  for (unsigned k = 0; k < FILT_GATHER_WORDS; k++) {
    const unsigned long long o = t0 + 16ull * (k * FILT_GATHER_THREADS + threadIdx.x);
    if (o >= total) continue;
    const unsigned long long last = min(o + 15, total - 1);
    unsigned ra = r_lo;
    long long delta = d_lo;
    bool whole = one_run;
    if (!one_run) {  // (uniform)
      ra = filt_find(koff, r_lo, r_hi, o);
      const unsigned rb = filt_find(koff, ra, r_hi, last);
      delta = (long long)hstart[ra] - (long long)koff[ra];
      whole = ra == rb || delta == (long long)hstart[rb] - (long long)koff[rb];
    }
    uint4 v;
    if (whole) {  // (sixteen bytes from a byte of the chunk: at most fifteen of the block's spare bytes behind it)
      const FiltU128 s = *reinterpret_cast<const FiltU128 *>(raw + ((long long)o + delta));
      v = make_uint4(s.a, s.b, s.c, s.d);
    } else {  // across a seam between two runs: byte by byte
      unsigned w[4] = {0, 0, 0, 0};
      unsigned rr = ra;
      unsigned long long next = koff[rr + 1];  // the first output byte that is no longer record rr's
      long long dd = delta;
      for (unsigned i = 0; o + i <= last; i++) {
        if (o + i >= next) {
          rr = filt_find(koff, rr + 1, r_hi, o + i);
          next = koff[rr + 1];
          dd = (long long)hstart[rr] - (long long)koff[rr];
        }
        w[i >> 2] |= (unsigned)raw[(long long)(o + i) + dd] << (8 * (i & 3));
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4 *>(dst + o) = v;  // (dst has room up to the next multiple of 16)
  }
}

// text behind a '+': one wave per kept record, the canonical form put together (k_crc_canon_write)
__global__ void __launch_bounds__(256)
k_filter_gather_records(const uint8_t *__restrict__ raw, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
                        const uint32_t *__restrict__ ksize, const uint32_t *__restrict__ hstart,
                        const unsigned long long *__restrict__ koff, uint8_t *__restrict__ dst) {
  const unsigned waves = (gridDim.x * blockDim.x) >> 6, lane = fq_lane();
  for (unsigned r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_recs; r += waves) {
    if (!ksize[r]) continue;  // (uniform)
    const fqgpu_rec rec = recs[r];
    const unsigned h0 = hstart[r], hl = rec.seq_off > h0 ? rec.seq_off - h0 : 0u;
    uint8_t *d = dst + koff[r];
    for (unsigned i = lane; i < hl; i += 64) d[i] = raw[h0 + i];  // (ends with the header's '\n')
    d += hl;
    for (unsigned i = lane; i < rec.len; i += 64) { d[i] = raw[rec.seq_off + i]; d[rec.len + 3 + i] = raw[rec.qual_off + i]; }
    if (lane == 0) { d[rec.len] = '\n'; d[rec.len + 1] = '+'; d[rec.len + 2] = '\n'; d[2 * rec.len + 3] = '\n'; }
  }
}

}  // namespace

void FilterScratch::release() {
  for (DevBuf *b : {&ksize, &hstart, &keep, &koff, &dst, &res, &scan_tmp}) b->release();
  if (host) (void)hipHostFree(host);
  host = nullptr;
}

// The reads of the chunk raw_dev[0, raw_len) with the record table recs_dev that pass *f, on st, waited for.  Two waits: the
// judge's result words decide what is gathered and how much room it needs; the gathered bytes come down in one copy.
// FQGPU_E_ARG with *out_len = 0 and the report zeroed: a byte that cannot be judged, a record that is not inside the chunk,
// has no symbol or more than a readlen_t counts.
int fq_filter_chunk(fqgpu_ctx *ctx, hipStream_t st, const uint8_t *raw_dev, size_t raw_len, const fqgpu_rec *recs_dev, size_t n_recs,
                    const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out) {
  *out_len = 0;
  for (unsigned i = 0; i < FQGPU_FILTER_REPORT_WORDS; i++) report[i] = 0;
  if (n_recs >= ((size_t)1 << 32) || raw_len >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  if (!n_recs) return FQGPU_OK;
  FilterScratch &fs = ctx->filter;
  const unsigned R = (unsigned)n_recs;
  const size_t n_waves = (n_recs + FILT_WAVE_RECORDS - 1) / FILT_WAVE_RECORDS;
  int rc;
  if ((rc = fs.ksize.reserve(n_recs * 4)) || (rc = fs.hstart.reserve(n_recs * 4)) || (rc = fs.keep.reserve(n_waves * 8)) ||
      (rc = fs.koff.reserve((n_recs + 1) * 8)) || (rc = fs.res.reserve(sizeof(FilterResult))))
    return rc;
  if (!fs.host) FQ_HIP(hipHostMalloc(&fs.host, sizeof(FilterResult), hipHostMallocPortable));
  const FilterResult &res = *static_cast<const FilterResult *>(fs.host);
  FQ_HIP(hipMemsetAsync(fs.res.p, 0, sizeof(FilterResult), st));
  fq_timer_span_begin(ctx, "filter", st);
  hipLaunchKernelGGL(k_filter_judge, dim3((unsigned)((n_waves + FILT_THREADS / 64 - 1) / (FILT_THREADS / 64))), dim3(FILT_THREADS), 0, st,
                     raw_dev, (unsigned long long)raw_len, recs_dev, R, *f, fs.ksize.as<uint32_t>(), fs.hstart.as<uint32_t>(),
                     fs.keep.as<unsigned long long>(), fs.res.as<FilterResult>());
  FQ_HIP(hipGetLastError());
  if (out && (rc = fq_scan_u32_to_u64(st, fs.ksize.as<uint32_t>(), n_recs, fs.koff.as<unsigned long long>(), fs.scan_tmp))) {
    fq_timer_span_end(ctx, st);
    return rc;
  }
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipMemcpyAsync(fs.host, fs.res.p, sizeof(FilterResult), hipMemcpyDeviceToHost, st));
  if (keep_out) FQ_HIP(hipMemcpyAsync(keep_out, fs.keep.p, (n_recs + 7) / 8, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  if (res.bad) {
    if (keep_out) memset(keep_out, 0, (n_recs + 7) / 8);
    return FQGPU_E_ARG;
  }
  for (unsigned i = 1; i < FQGPU_FILTER_REPORT_WORDS; i++) report[i] = res.w[i];
  report[0] = n_recs;
  const size_t total = (size_t)res.w[R_BYTES_KEPT];
  *out_len = total;
  if (!out || !total) return FQGPU_OK;
  if (out_cap < total) return FQGPU_E_OVERFLOW;
  if ((rc = fs.dst.reserve(total + 64))) return rc;
  fq_timer_span_begin(ctx, "filter", st);
  if (!res.not_bare)
    hipLaunchKernelGGL(k_filter_gather, dim3((unsigned)((total + FILT_TILE_BYTES - 1) / FILT_TILE_BYTES)), dim3(FILT_GATHER_THREADS), 0, st,
                       raw_dev, fs.hstart.as<uint32_t>(), fs.koff.as<unsigned long long>(), R,
                       (unsigned long long)total, fs.dst.as<uint8_t>());
  else
    hipLaunchKernelGGL(k_filter_gather_records, dim3((unsigned)min((n_recs + 3) / 4, (size_t)8192)), dim3(256), 0, st, raw_dev, recs_dev, R,
                       fs.ksize.as<uint32_t>(), fs.hstart.as<uint32_t>(), fs.koff.as<unsigned long long>(), fs.dst.as<uint8_t>());
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipMemcpyAsync(out, fs.dst.p, total, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  return FQGPU_OK;
}
