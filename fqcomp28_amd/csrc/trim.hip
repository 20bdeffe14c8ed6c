// The reads of a chunk that lies in HBM, trimmed and then filtered (include/fqgpu.h: fqgpu_chunk_trim, fqgpu_dblock_trim), on the
// device, so that only the bytes that are kept come down.  Extension: nothing in the reference.  The file follows filter.hip
// step by step -- judge, scan, destination-driven gather -- and shares nothing with it but fq_scan_u32_to_u64.
//
// k_trim_judge -- filter.hip's judge with a window in front of the verdict.  A wave takes 64 consecutive records, their table
// entries with ONE load, lane = record; the lines are read by eight lanes to a record, eight records at a time, every lane
// ALIGNED 16-byte words, the words of the NEXT eight records on their way while those of the eight in hand are judged; no LDS
// table.  The fixed cuts leave the interval [f, L - t).  The two running-sum walks of the quality trim (s += cutoff - Phred;
// stop at s < 0; the cut is behind the FIRST place of the largest s > 0) are done by all eight lanes at once: a lane sums up its
// word, in walk order, as a PIECE -- total, smallest prefix, largest prefix and the first place of that --, a prefix sum over
// the pieces gives every piece the sum the walk enters it with, the walk stops in the first piece with entering + smallest
// prefix < 0, every piece in front of that one is valid as a whole (its candidate: entering + largest prefix; equal
// candidates: the earlier piece), and only the piece the walk stops in is walked byte by byte.  A request's two words are taken
// in walk order, and a word no record of the wave still needs is left out.  A candidate travels as ONE
// 64-bit key -- the sum above, the place below, so that the larger key is the better AND the earlier one -- and is reduced
// by shuffles.  With the window known, N, the Phred sum and the low count are taken over the window from the words that are
// still in the registers, with new byte masks; a line that is read is JUDGED over all its bytes, the cut ones too.  A read
// whose line fits one request of its eight lanes (256 bytes) loads no word twice; a longer one walks the requests forwards
// for the front walk, backwards for the tail walk and forwards again for the counts, loading as it goes: a correctness path.
// The record's own lane gives the verdict, the kept size, the header start, the window, the keep bit (one ballot per wave)
// and k_crc_check's verdict on the '+' lines; the counters go over the wave by shuffles, over the workgroup in LDS and reach
// global memory as one 64-bit atomic per counter and workgroup.
//
// fq_scan_u32_to_u64 -- the kept sizes become the records' places in the output.
//
// k_trim_gather -- a kept record is FIVE pieces: its header line, the window of the sequence line, the literal "\n+\n", the
// window of the quality line, the literal '\n'; three of them are the chunk shifted by a constant.  Driven by the DESTINATION
// as filter.hip's gather: a workgroup owns an aligned tile of the output, a lane aligned 16-byte words of it, every store a
// full aligned 16-byte store.  A word inside one such piece is one unaligned 16-byte load, a word across a seam is put
// together byte by byte.  Cuts only take bytes away, so hstart[r] - koff[r] never gets smaller with r: when the chunk's '+'
// lines are bare, the records of a tile's first and last byte have the same shift and both are untrimmed, every record
// between them is kept whole and the tile is ONE shifted copy -- a trim that cuts nothing costs what the filter costs.  The
// '+' line is always the literal here, so this one kernel serves chunks with text behind a '+' as well.
//
// All global stores are ordinary vector stores from plain C++.
#include "fqgpu_internal.h"

#include <string.h>

namespace {

constexpr unsigned TRIM_THREADS = 256;        // threads of a judge workgroup: four waves
constexpr unsigned TRIM_WAVE_RECORDS = 64;    // consecutive records a wave takes: lane = record
constexpr unsigned TRIM_GROUP_LANES = 8;      // lanes that read one record's lines together
constexpr unsigned TRIM_UNROLL = 2;           // 16-byte words of a line a lane has in flight
constexpr unsigned TRIM_GATHER_THREADS = 256; // threads of a gather workgroup
constexpr unsigned TRIM_GATHER_WORDS = 4;     // 16-byte words of the output a gather lane writes
constexpr unsigned TRIM_ROUND_RECORDS = TRIM_WAVE_RECORDS / TRIM_GROUP_LANES;  // records a wave reads at a time
constexpr unsigned TRIM_STEP_BYTES = TRIM_GROUP_LANES * 16 * TRIM_UNROLL;      // bytes of a line a record's lanes ask for in one go
constexpr unsigned TRIM_TILE_BYTES = TRIM_GATHER_THREADS * 16 * TRIM_GATHER_WORDS;  // output bytes of a gather workgroup
static_assert(TRIM_WAVE_RECORDS == 64 && TRIM_GROUP_LANES == 8 && TRIM_ROUND_RECORDS == 8 && TRIM_UNROLL == 2, "a wave's records sit in its lanes");

// the result words on the device: the report (include/fqgpu.h; word 0 is filled in by the host) and the two flags
struct TrimResult {
  unsigned long long w[FQGPU_TRIM_REPORT_WORDS];
  unsigned int bad;       // a byte that cannot be judged, a record outside the chunk or without symbols
  unsigned int not_bare;  // k_crc_check's verdict: text behind a '+', or the last '\n' outside the chunk
};
constexpr unsigned R_KEPT = 1, R_BASES_IN = 2, R_BASES_KEPT = 3, R_BYTES_KEPT = 4, R_DROPPED = 5, R_TRIMMED = 10, R_CUT_FRONT = 11,
                   R_CUT_TAIL = 12, R_EMPTIED = 13, R_COUNTERS = 14;

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
__device__ __forceinline__ unsigned trim_bits(int lo, int hi) {
  lo = min(max(lo, 0), 16);
  hi = min(max(hi, 0), 16);
  return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

// what a lane keeps of the record its group reads: the lines' places and the first words of both
struct TrimStage {
  unsigned seq_off, qual_off, len;  // len 0: nothing to read (behind the table's end, or not a record of this chunk)
  uint4 s[TRIM_UNROLL], q[TRIM_UNROLL];
};

// the lane's words of one line: word k of the lane is the aligned word 8 k + sub of the line, counted from the word that
// holds the line's first byte; p0: bytes of the line (from that word on) in front of this request.  Every raw block has 64
// spare bytes behind its chunk (api.hip), so the word that holds the chunk's last byte can be read whole.
__device__ __forceinline__ void trim_load_line(uint4 (&v)[TRIM_UNROLL], const uint8_t *__restrict__ raw, unsigned off, unsigned len, unsigned p0, unsigned sub) {
  const unsigned lead = off & 15u, span = len ? lead + len : 0u;
  const uint8_t *const line = raw + (off - lead);
#pragma unroll
  for (unsigned k = 0; k < TRIM_UNROLL; k++) {
    const unsigned rel = p0 + 16u * (TRIM_GROUP_LANES * k + sub);
    v[k] = rel < span ? *reinterpret_cast<const uint4 *>(line + rel) : make_uint4(0, 0, 0, 0);
  }
}

struct TrimCounts {
  unsigned n, qsum, low;  // over the WINDOW: N of the sequence line; sum of the quality BYTES; quality bytes below the level
  bool bad;               // over the whole line
};

// one word of a sequence line: [first, last) are its bytes inside the line, [wf, wl) those inside the window
__device__ __forceinline__ void trim_judge_seq(TrimCounts &c, const uint4 v, int first, int last, int wf, int wl) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned m = sw_mask(first - 4 * i, last - 4 * i), x = w[i] & m;
    if (x & SW_H) c.bad = true;
    const unsigned y = x & ~SW_H, is_n = sw_eq(y, 'N');
    const unsigned base = sw_eq(y, 'A') | sw_eq(y, 'C') | sw_eq(y, 'G') | sw_eq(y, 'T') | is_n;
    if ((base & m) != (SW_H & m)) c.bad = true;
    c.n += __popc(is_n & sw_mask(wf - 4 * i, wl - 4 * i));
  }
}

// one word of a quality line; level: the first byte value that is not "low" (33 + low_q)
__device__ __forceinline__ void trim_judge_qual(TrimCounts &c, const uint4 v, int first, int last, int wf, int wl, unsigned level) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned m = sw_mask(first - 4 * i, last - 4 * i), x = w[i] & m;
    if (x & SW_H) c.bad = true;
    const unsigned y = x & ~SW_H;
    if ((sw_ge(y, 33u) & m) != (SW_H & m) || (sw_ge(y, 97u) & m)) c.bad = true;
    const unsigned wm = sw_mask(wf - 4 * i, wl - 4 * i);
    c.qsum = __builtin_amdgcn_sad_u8(w[i] & wm, 0u, c.qsum);
    c.low += __popc(~sw_ge(y, level) & SW_H & wm);
  }
}

// ---- the running-sum walk.  A candidate is one key: the sum in the bits from 20 up (at most 64 x 65535 < 2^22), the place
// below, turned so that of two keys with one sum the place the walk reaches FIRST is the larger.  0: no candidate.
constexpr unsigned TRIM_PLACE = 0xFFFFFu;
template <bool FWD>
__device__ __forceinline__ unsigned long long trim_key(int sum, int place) {
  return ((unsigned long long)(unsigned)sum << 20) | (unsigned)(FWD ? (int)TRIM_PLACE - place : place);
}

struct TrimPiece {
  int tot, minp, maxp;  // of the prefixes in walk order (the empty prefix, 0, among them)
  int place;            // the cut the first largest prefix stands for (maxp > 0 only)
};

// The bytes `in` (a bit each) of a word as one piece of a walk; c: cutoff + 33, so that c - byte is the walk's increment;
// pos0: the place in the line of the word's byte 0.  The front walk (FWD) reads byte 0 first and a byte at place i stands for
// the cut "start = i + 1"; the tail walk reads byte 15 first and a byte at place i stands for "stop = i".
template <bool FWD>
__device__ __forceinline__ TrimPiece trim_piece(const uint4 v, unsigned in, int c, int pos0) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  TrimPiece p = {0, 0, 0, 0};
  int s = 0;
#pragma unroll
  for (int jj = 0; jj < 16; jj++) {
    const int j = FWD ? jj : 15 - jj;
    const int byte = (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    s += (in >> j) & 1u ? c - byte : 0;
    p.minp = min(p.minp, s);
    if (s > p.maxp) {
      p.maxp = s;
      p.place = pos0 + j + (FWD ? 1 : 0);
    }
  }
  p.tot = s;
  return p;
}

// The piece the walk stops in, byte by byte: s the sum the walk enters it with, best the best candidate in front of it.
template <bool FWD>
__device__ __forceinline__ unsigned long long trim_walk_piece(const uint4 v, unsigned in, int c, int pos0, int s, unsigned long long best) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  int top = (int)(best >> 20);
  bool dead = false;
#pragma unroll
  for (int jj = 0; jj < 16; jj++) {
    const int j = FWD ? jj : 15 - jj;
    const int byte = (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    s += (in >> j) & 1u ? c - byte : 0;
    dead = dead || s < 0;
    if (!dead && s > top) {
      top = s;
      best = trim_key<FWD>(s, pos0 + j + (FWD ? 1 : 0));
    }
  }
  return best;
}

// a walk on its way through a line; the same in the eight lanes of a record
struct TrimWalk {
  int ent;                  // the sum it enters the next request with
  unsigned long long best;  // the best candidate so far
  bool stopped;
};

// One word of a request of a walk over the places [a, b) of a line: eight pieces, the word of lane sub at place pos0.  Every
// lane of the record's eight calls this together.
template <bool FWD>
__device__ __forceinline__ void trim_walk_word(TrimWalk &wk, const uint4 v, int pos0, unsigned sub, int a, int b, int c) {
  const unsigned in = trim_bits(a - pos0, b - pos0);
  const TrimPiece pc = trim_piece<FWD>(v, in, c, pos0);
  // the sum the walk enters the piece with: a prefix sum over the lanes, in walk order
  int inc = pc.tot;
#pragma unroll
  for (unsigned d = 1; d < TRIM_GROUP_LANES; d <<= 1) {
    const int o = __shfl_up(inc, d, TRIM_GROUP_LANES);
    if (sub >= d) inc += o;
  }
  const int sum = __shfl(inc, TRIM_GROUP_LANES - 1, TRIM_GROUP_LANES);
  const int e = wk.ent + (FWD ? inc - pc.tot : sum - inc);
  const unsigned ord = FWD ? sub : TRIM_GROUP_LANES - 1 - sub;  // the piece's turn in the walk
  // the first piece the walk would stop in
  unsigned stop_at = e + pc.minp < 0 ? ord : TRIM_GROUP_LANES;
#pragma unroll
  for (unsigned d = 1; d < TRIM_GROUP_LANES; d <<= 1) stop_at = min(stop_at, (unsigned)__shfl_xor(stop_at, d, TRIM_GROUP_LANES));
  // the pieces in front of it are valid as a whole
  unsigned long long key = pc.maxp > 0 && ord < stop_at ? trim_key<FWD>(e + pc.maxp, pc.place) : 0ull;
#pragma unroll
  for (unsigned d = 1; d < TRIM_GROUP_LANES; d <<= 1) key = max(key, (unsigned long long)__shfl_xor(key, d, TRIM_GROUP_LANES));
  const unsigned long long best = max(wk.best, key);
  // the piece it stops in, byte by byte, by the lane that holds it (every lane walks its word: no lane waits for less)
  const unsigned long long walked = trim_walk_piece<FWD>(v, in, c, pos0, e, best);
  const unsigned at = min(stop_at, TRIM_GROUP_LANES - 1);
  const unsigned long long from_owner = __shfl(walked, FWD ? at : TRIM_GROUP_LANES - 1 - at, TRIM_GROUP_LANES);
  if (!wk.stopped) {
    wk.best = stop_at < TRIM_GROUP_LANES ? from_owner : best;
    wk.stopped = stop_at < TRIM_GROUP_LANES;
  }
  wk.ent += sum;
}

// One request (word 8 k + sub in lane sub, k = 0, 1) of a walk over the places [a, b) of a line whose first byte sits at byte
// `lead` of its first word: its words in walk order.  A word is left out when no record of the WAVE has anything for the walk
// in it -- the walk has stopped, or the word lies behind the interval; most walks stop in the first word they meet.
template <bool FWD>
__device__ __forceinline__ void trim_walk_step(TrimWalk &wk, const uint4 (&v)[TRIM_UNROLL], unsigned p0, unsigned sub, int lead, int a, int b, int c) {
#pragma unroll
  for (unsigned kk = 0; kk < TRIM_UNROLL; kk++) {
    const unsigned k = FWD ? kk : TRIM_UNROLL - 1 - kk;
    const int first = (int)(p0 + 16u * TRIM_GROUP_LANES * k) - lead;  // the place of the eight words' first byte
    const bool idle = wk.stopped || (FWD ? first >= b : first + (int)(16u * TRIM_GROUP_LANES) <= a);  // (the same in a record's lanes)
    if (__all(idle)) continue;  // (uniform)
    trim_walk_word<FWD>(wk, v[k], first + (int)(16u * sub), sub, a, b, c);
  }
}

__global__ void __launch_bounds__(TRIM_THREADS)
k_trim_judge(const uint8_t *__restrict__ raw, unsigned long long raw_len, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
             const fqgpu_trim t, const fqgpu_filter f, uint32_t *__restrict__ ksize, uint32_t *__restrict__ hstart,
             uint32_t *__restrict__ win, unsigned long long *__restrict__ keep, TrimResult *__restrict__ res) {
  __shared__ unsigned wg[R_COUNTERS];
  if (threadIdx.x < R_COUNTERS) wg[threadIdx.x] = 0;
  __syncthreads();
  const unsigned lane = fq_lane(), sub = lane & (TRIM_GROUP_LANES - 1), group = lane / TRIM_GROUP_LANES;
  const bool walk_f = t.q_front != 0, walk_t = t.q_tail != 0;
  const bool need_seq = f.max_n != FQGPU_FILTER_NONE, need_qual = walk_f || walk_t || f.min_mean_q != 0 || f.low_q != 0;
  const unsigned level = 33u + f.low_q;
  const unsigned long long r0 = ((unsigned long long)blockIdx.x * (TRIM_THREADS / 64) + (threadIdx.x >> 6)) * TRIM_WAVE_RECORDS;
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

  // the window of a read of `len` symbols left by the fixed cuts, and by the two walks' results
  const auto cut_lo = [&](unsigned len) { return min(t.cut_front, len); };
  const auto cut_hi = [&](unsigned len) { return len - min(t.cut_tail, len - min(t.cut_front, len)); };
  const auto window = [&](unsigned start, unsigned stop) {  // -> start | n << 16
    if (start >= stop) return 0u;
    return start | min(stop - start, t.crop) << 16;
  };

  unsigned n_count = 0, q_bytes = 0, low_count = 0;
  unsigned my_win = window(cut_lo(read_len), cut_hi(read_len));  // (what holds when no line is read)
  if (need_seq || need_qual) {  // (uniform)
    // record j of the wave's 64, for the lanes of the group that reads it
    const auto fetch = [&](TrimStage &st, unsigned j) {
      st.seq_off = __shfl(mine.seq_off, j);
      st.qual_off = __shfl(mine.qual_off, j);
      st.len = __shfl(read_len, j);
      if (need_seq) trim_load_line(st.s, raw, st.seq_off, st.len, 0, sub);
      if (need_qual) trim_load_line(st.q, raw, st.qual_off, st.len, 0, sub);
    };
    const auto count_words = [&](TrimCounts &c, const uint4 (&v)[TRIM_UNROLL], unsigned off, unsigned len, unsigned p0, int ws, int we, bool is_seq) {
      const int lead = (int)(off & 15u), span = lead + (int)len;
#pragma unroll
      for (unsigned k = 0; k < TRIM_UNROLL; k++) {
        const int rel = (int)(p0 + 16u * (TRIM_GROUP_LANES * k + sub));
        if (rel >= span) continue;
        const int first = max(lead - rel, 0), last = min(span - rel, 16);
        const int wf = min(max(lead + ws - rel, 0), 16), wl = min(max(lead + we - rel, 0), 16);
        if (is_seq) trim_judge_seq(c, v[k], first, last, wf, wl);
        else trim_judge_qual(c, v[k], first, last, wf, wl, level);
      }
    };
    // steps: the requests the longest line of the eight records in hand takes (the same in every lane of the wave, so that
    // the eight lanes of a record stay together through the shuffles of a walk)
    const auto consume = [&](const TrimStage &st, unsigned steps) {
      const int a = (int)cut_lo(st.len), b = (int)cut_hi(st.len), lead_q = (int)(st.qual_off & 15u);
      unsigned start = (unsigned)a, stop = (unsigned)b;
      if (walk_f) {  // (uniform)
        TrimWalk wk = {0, 0ull, false};
        trim_walk_step<true>(wk, st.q, 0, sub, lead_q, a, b, (int)t.q_front + 33);
        for (unsigned s = 1; s < steps; s++) {  // a long read: the rest, not loaded ahead
          uint4 q[TRIM_UNROLL];
          trim_load_line(q, raw, st.qual_off, st.len, s * TRIM_STEP_BYTES, sub);
          trim_walk_step<true>(wk, q, s * TRIM_STEP_BYTES, sub, lead_q, a, b, (int)t.q_front + 33);
        }
        if (wk.best) start = TRIM_PLACE - (unsigned)(wk.best & TRIM_PLACE);
      }
      if (walk_t) {
        TrimWalk wk = {0, 0ull, false};
        for (unsigned s = steps - 1; s >= 1; s--) {  // a long read: from its last request down
          uint4 q[TRIM_UNROLL];
          trim_load_line(q, raw, st.qual_off, st.len, s * TRIM_STEP_BYTES, sub);
          trim_walk_step<false>(wk, q, s * TRIM_STEP_BYTES, sub, lead_q, a, b, (int)t.q_tail + 33);
        }
        trim_walk_step<false>(wk, st.q, 0, sub, lead_q, a, b, (int)t.q_tail + 33);
        if (wk.best) stop = (unsigned)(wk.best & TRIM_PLACE);
      }
      const unsigned w = window(start, stop);
      const int ws = (int)(w & 0xFFFFu), we = ws + (int)(w >> 16);
      TrimCounts c = {0u, 0u, 0u, false};
      if (need_seq) count_words(c, st.s, st.seq_off, st.len, 0, ws, we, true);
      if (need_qual) count_words(c, st.q, st.qual_off, st.len, 0, ws, we, false);
      for (unsigned s = 1; s < steps; s++) {
        uint4 x[TRIM_UNROLL];
        if (need_seq) {
          trim_load_line(x, raw, st.seq_off, st.len, s * TRIM_STEP_BYTES, sub);
          count_words(c, x, st.seq_off, st.len, s * TRIM_STEP_BYTES, ws, we, true);
        }
        if (need_qual) {
          trim_load_line(x, raw, st.qual_off, st.len, s * TRIM_STEP_BYTES, sub);
          count_words(c, x, st.qual_off, st.len, s * TRIM_STEP_BYTES, ws, we, false);
        }
      }
      // over the record's eight lanes; packed: N and low counts are at most 65535 each, the byte sum below 2^23
      unsigned x = c.n | c.low << 16, y = c.qsum | (c.bad ? 0x80000000u : 0u);
#pragma unroll
      for (unsigned d = 1; d < TRIM_GROUP_LANES; d <<= 1) {
        x += __shfl_xor(x, d);
        const unsigned o = __shfl_xor(y, d);
        y = ((y & 0x7FFFFFFFu) + (o & 0x7FFFFFFFu)) | ((y | o) & 0x80000000u);
      }
      return make_uint3(x, y, w);
    };
    // the requests a record's lines take
    const unsigned my_span = max(need_seq ? (mine.seq_off & 15u) + read_len : 0u, need_qual ? (mine.qual_off & 15u) + read_len : 0u);
    const unsigned my_steps = max((my_span + TRIM_STEP_BYTES - 1) / TRIM_STEP_BYTES, 1u);
    TrimStage cur, nxt;
    fetch(cur, group);
#pragma unroll 1
    for (unsigned k = 0; k < TRIM_GROUP_LANES; k++) {  // round k: group g reads record 8 k + g
      if (k + 1 < TRIM_GROUP_LANES) fetch(nxt, TRIM_ROUND_RECORDS * (k + 1) + group);
      unsigned steps = 1;
      if (__any(my_steps > 1 && lane / TRIM_ROUND_RECORDS == k)) {  // (uniform) a long read among the eight
        steps = lane / TRIM_ROUND_RECORDS == k ? my_steps : 1u;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) steps = max(steps, (unsigned)__shfl_xor(steps, d));
        steps = fq_uniform(steps);
      }
      const uint3 got = consume(cur, steps);
      // back to the record's own lane: lane 8 k + g takes what group g's lanes hold
      const unsigned x = __shfl(got.x, (lane & (TRIM_ROUND_RECORDS - 1)) * TRIM_GROUP_LANES);
      const unsigned y = __shfl(got.y, (lane & (TRIM_ROUND_RECORDS - 1)) * TRIM_GROUP_LANES);
      const unsigned w = __shfl(got.z, (lane & (TRIM_ROUND_RECORDS - 1)) * TRIM_GROUP_LANES);
      if (lane / TRIM_ROUND_RECORDS == k) {
        n_count = x & 0xFFFFu;
        low_count = x >> 16;
        q_bytes = y & 0x7FFFFFFFu;
        bad = bad || (y >> 31);
        my_win = w;
      }
      if (k + 1 < TRIM_GROUP_LANES) cur = nxt;
    }
  }

  // the verdict on what is left: 0 kept, 1 .. 5 the first criterion that fails; a read with nothing left is "short"
  const unsigned start = ok ? my_win & 0xFFFFu : 0u, n = ok ? my_win >> 16 : 0u;
  const bool emptied = ok && n == 0;
  unsigned verdict = 0;
  if (ok) {
    const unsigned long long phred = need_qual ? q_bytes - 33ull * n : 0ull;
    if (emptied || n < f.min_len) verdict = 1;
    else if (n > f.max_len) verdict = 2;
    else if (need_seq && n_count > f.max_n) verdict = 3;
    else if (f.min_mean_q && phred < (unsigned long long)f.min_mean_q * n) verdict = 4;
    else if (f.low_q && 100ull * low_count > (unsigned long long)f.max_low_pct * n) verdict = 5;
  }
  const bool kept = ok && verdict == 0;
  const unsigned hl = mine.seq_off > h0 ? mine.seq_off - h0 : 0u;
  const unsigned long long size64 = (unsigned long long)hl + 2ull * n + 4ull;
  if (kept && size64 > 0xFFFFFFFFull) bad = true;  // (a table that is not this chunk's)
  const unsigned size = kept ? (unsigned)size64 : 0u;
  bool odd = false;
  if (have) {
    ksize[r] = size;
    hstart[r] = h0;
    win[r] = start | n << 16;
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
  cnt[R_BASES_KEPT] = kept ? n : 0u;
#pragma unroll
  for (unsigned v = 1; v <= 5; v++) cnt[R_DROPPED + v - 1] = verdict == v;
  cnt[R_TRIMMED] = ok && n != mine.len;
  cnt[R_CUT_FRONT] = start;
  cnt[R_CUT_TAIL] = ok ? mine.len - start - n : 0u;
  cnt[R_EMPTIED] = emptied;
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
__device__ __forceinline__ unsigned trim_find(const unsigned long long *__restrict__ koff, unsigned lo, unsigned hi, unsigned long long o) {
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1) >> 1);
    if (koff[mid] <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct __attribute__((packed)) TrimU128 { uint32_t a, b, c, d; };  // sixteen bytes at any address

// a kept record as the gather sees it: where its pieces come from
struct TrimRec {
  long long h0, seq, qual;  // the header line, the first kept byte of the sequence and of the quality line, in the chunk
  unsigned hl, n;           // bytes of the header line with its '\n'; symbols of the window
  bool whole;               // untrimmed
};
__device__ __forceinline__ TrimRec trim_rec(const fqgpu_rec *__restrict__ recs, const uint32_t *__restrict__ hstart,
                                            const uint32_t *__restrict__ win, unsigned r) {
  const fqgpu_rec rec = recs[r];
  const unsigned h0 = hstart[r], w = win[r];
  TrimRec c;
  c.h0 = h0;
  c.hl = rec.seq_off > h0 ? rec.seq_off - h0 : 0u;
  c.n = w >> 16;
  c.seq = (long long)rec.seq_off + (w & 0xFFFFu);
  c.qual = (long long)rec.qual_off + (w & 0xFFFFu);
  c.whole = c.n == rec.len;
  return c;
}
// byte j of the record's trimmed canonical form
__device__ __forceinline__ unsigned trim_byte(const uint8_t *__restrict__ raw, const TrimRec &c, unsigned long long j) {
  if (j < c.hl) return raw[c.h0 + (long long)j];
  j -= c.hl;
  if (j < c.n) return raw[c.seq + (long long)j];
  j -= c.n;
  if (j < 3) return j == 1 ? '+' : '\n';
  j -= 3;
  if (j < c.n) return raw[c.qual + (long long)j];
  return '\n';
}

// out[koff[r], koff[r + 1]) = header line | seq[start, start + n) | "\n+\n" | qual[start, start + n) | '\n' for every kept
// record r; bare: the chunk's '+' lines are bare, so an untrimmed record is one span of the chunk
__global__ void __launch_bounds__(TRIM_GATHER_THREADS)
k_trim_gather(const uint8_t *__restrict__ raw, const fqgpu_rec *__restrict__ recs, const uint32_t *__restrict__ hstart,
              const uint32_t *__restrict__ win, const unsigned long long *__restrict__ koff, unsigned n_recs, unsigned long long total,
              const bool bare, uint8_t *__restrict__ dst) {
  const unsigned long long t0 = (unsigned long long)blockIdx.x * TRIM_TILE_BYTES;
  if (t0 >= total) return;
  const unsigned long long t1 = min(total, t0 + TRIM_TILE_BYTES) - 1;  // the tile's last byte
  // (uniform: the compiler keeps these searches in scalar registers)
  const unsigned r_lo = trim_find(koff, 0, n_recs - 1, t0), r_hi = trim_find(koff, r_lo, n_recs - 1, t1);
  const long long d_lo = (long long)hstart[r_lo] - (long long)koff[r_lo], d_hi = (long long)hstart[r_hi] - (long long)koff[r_hi];
  // equal shifts: the records between are kept whole, or the source would have moved on without the output
  const bool one_run = bare && d_lo == d_hi && (win[r_lo] >> 16) == recs[r_lo].len && (win[r_hi] >> 16) == recs[r_hi].len;
#pragma unroll
  for (unsigned k = 0; k < TRIM_GATHER_WORDS; k++) {
    const unsigned long long o = t0 + 16ull * (k * TRIM_GATHER_THREADS + threadIdx.x);
    if (o >= total) continue;
    const unsigned long long last = min(o + 15, total - 1);
    long long src = (long long)o + d_lo;
    bool copy = one_run;
    unsigned ra = r_lo;
    TrimRec ca = {0, 0, 0, 0u, 0u, false};
    if (!one_run) {  // (uniform)
      ra = trim_find(koff, r_lo, r_hi, o);
      const unsigned rb = trim_find(koff, ra, r_hi, last);
      ca = trim_rec(recs, hstart, win, ra);
      const unsigned long long j0 = o - koff[ra], j1 = last - koff[ra];
      const unsigned long long q0 = (unsigned long long)ca.hl + ca.n + 3u;  // the quality window's first byte in the record
      if (bare && ca.whole && (ra == rb || ((win[rb] >> 16) == recs[rb].len &&
                                            ca.h0 - (long long)koff[ra] == (long long)hstart[rb] - (long long)koff[rb]))) {
        copy = true;  // inside one run of whole records
        src = ca.h0 + (long long)j0;
      } else if (ra == rb && last == o + 15) {
        if (j1 < ca.hl) {
          copy = true;
          src = ca.h0 + (long long)j0;
        } else if (j0 >= ca.hl && j1 < (unsigned long long)ca.hl + ca.n) {
          copy = true;
          src = ca.seq + (long long)(j0 - ca.hl);
        } else if (j0 >= q0 && j1 < q0 + ca.n) {
          copy = true;
          src = ca.qual + (long long)(j0 - q0);
        }
      }
    }
    uint4 v;
    if (copy) {  // (sixteen bytes from a byte of the chunk: at most fifteen of the block's spare bytes behind it)
      const TrimU128 s = *reinterpret_cast<const TrimU128 *>(raw + src);
      v = make_uint4(s.a, s.b, s.c, s.d);
    } else {  // across a seam between two pieces or two records: byte by byte
      unsigned w[4] = {0, 0, 0, 0};
      unsigned rr = ra;
      TrimRec c = ca;
      unsigned long long base = koff[rr], next = koff[rr + 1];  // next: the first output byte that is no longer record rr's
      for (unsigned i = 0; o + i <= last; i++) {
        if (o + i >= next) {
          rr = trim_find(koff, rr + 1, r_hi, o + i);
          c = trim_rec(recs, hstart, win, rr);
          base = koff[rr];
          next = koff[rr + 1];
        }
        w[i >> 2] |= trim_byte(raw, c, o + i - base) << (8 * (i & 3));
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4 *>(dst + o) = v;  // (dst has room up to the next multiple of 16)
  }
}

}  // namespace

void TrimScratch::release() {
  for (DevBuf *b : {&ksize, &hstart, &win, &keep, &koff, &dst, &res, &scan_tmp}) b->release();
  if (host) (void)hipHostFree(host);
  host = nullptr;
}

// The reads of the chunk raw_dev[0, raw_len) with the record table recs_dev, trimmed by *t and then judged by *f, on st,
// waited for.  Two waits, as fq_filter_chunk: the judge's result words decide what is gathered and how much room it needs;
// the gathered bytes come down in one copy.  FQGPU_E_ARG with *out_len = 0 and report, keep bits and windows zeroed: a byte
// that cannot be judged, a record that is not inside the chunk, has no symbol or more than a readlen_t counts.
int fq_trim_chunk(fqgpu_ctx *ctx, hipStream_t st, const uint8_t *raw_dev, size_t raw_len, const fqgpu_rec *recs_dev, size_t n_recs,
                  const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report,
                  uint8_t *keep_out, uint32_t *win_out) {
  *out_len = 0;
  for (unsigned i = 0; i < FQGPU_TRIM_REPORT_WORDS; i++) report[i] = 0;
  if (n_recs >= ((size_t)1 << 32) || raw_len >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  if (!n_recs) return FQGPU_OK;
  TrimScratch &ts = ctx->trim;
  const unsigned R = (unsigned)n_recs;
  const size_t n_waves = (n_recs + TRIM_WAVE_RECORDS - 1) / TRIM_WAVE_RECORDS;
  int rc;
  if ((rc = ts.ksize.reserve(n_recs * 4)) || (rc = ts.hstart.reserve(n_recs * 4)) || (rc = ts.win.reserve(n_recs * 4)) ||
      (rc = ts.keep.reserve(n_waves * 8)) || (rc = ts.koff.reserve((n_recs + 1) * 8)) || (rc = ts.res.reserve(sizeof(TrimResult))))
    return rc;
  if (!ts.host) FQ_HIP(hipHostMalloc(&ts.host, sizeof(TrimResult), hipHostMallocPortable));
  const TrimResult &res = *static_cast<const TrimResult *>(ts.host);
  FQ_HIP(hipMemsetAsync(ts.res.p, 0, sizeof(TrimResult), st));
  fq_timer_span_begin(ctx, "trim", st);
  hipLaunchKernelGGL(k_trim_judge, dim3((unsigned)((n_waves + TRIM_THREADS / 64 - 1) / (TRIM_THREADS / 64))), dim3(TRIM_THREADS), 0, st,
                     raw_dev, (unsigned long long)raw_len, recs_dev, R, *t, *f, ts.ksize.as<uint32_t>(), ts.hstart.as<uint32_t>(),
                     ts.win.as<uint32_t>(), ts.keep.as<unsigned long long>(), ts.res.as<TrimResult>());
  FQ_HIP(hipGetLastError());
  if (out && (rc = fq_scan_u32_to_u64(st, ts.ksize.as<uint32_t>(), n_recs, ts.koff.as<unsigned long long>(), ts.scan_tmp))) {
    fq_timer_span_end(ctx, st);
    return rc;
  }
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipMemcpyAsync(ts.host, ts.res.p, sizeof(TrimResult), hipMemcpyDeviceToHost, st));
  if (keep_out) FQ_HIP(hipMemcpyAsync(keep_out, ts.keep.p, (n_recs + 7) / 8, hipMemcpyDeviceToHost, st));
  if (win_out) FQ_HIP(hipMemcpyAsync(win_out, ts.win.p, n_recs * 4, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  if (res.bad) {
    if (keep_out) memset(keep_out, 0, (n_recs + 7) / 8);
    if (win_out) memset(win_out, 0, n_recs * 4);
    return FQGPU_E_ARG;
  }
  for (unsigned i = 1; i < FQGPU_TRIM_REPORT_WORDS; i++) report[i] = res.w[i];
  report[0] = n_recs;
  const size_t total = (size_t)res.w[R_BYTES_KEPT];
  *out_len = total;
  if (!out || !total) return FQGPU_OK;
  if (out_cap < total) return FQGPU_E_OVERFLOW;
  if ((rc = ts.dst.reserve(total + 64))) return rc;
  fq_timer_span_begin(ctx, "trim", st);
  hipLaunchKernelGGL(k_trim_gather, dim3((unsigned)((total + TRIM_TILE_BYTES - 1) / TRIM_TILE_BYTES)), dim3(TRIM_GATHER_THREADS), 0, st,
                     raw_dev, recs_dev, ts.hstart.as<uint32_t>(), ts.win.as<uint32_t>(), ts.koff.as<unsigned long long>(), R,
                     (unsigned long long)total, res.not_bare == 0u, ts.dst.as<uint8_t>());
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipMemcpyAsync(out, ts.dst.p, total, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  return FQGPU_OK;
}
