// The calls on the records of TWO chunks that lie in HBM, mate 1's and mate 2's (include/fqgpu.h: fqgpu_chunk_pair_names,
// fqgpu_chunk_pair_overlap, fqgpu_chunk_pair_correct, fqgpu_chunk_pair_merge and their fqgpu_dblock_* forms).  Extension: nothing in the reference.
// Each takes two views (FqChunkView, fqgpu_internal.h) of one count, is one kernel over the pairs, and lands its verdict in
// the selection's result words (sel_words.h), whose packed byte compares it shares with select.hip.
//
// k_pair_names compares the read ids of the records: eight lanes to a pair, both ids loaded from wherever they start, one
// atomicMin for the first pair that differs.
//
// The MATE OVERLAP.  k_pair_overlap compares the sequence lines of the records: a wave per 64 pairs, each pair's lines as
// 2-bit codes and an N plane in LDS, mate 2's reversed and complemented, a lane per candidate shift, the first hit in the
// rule's order by a ballot; it leaves a summary with the insert-size histogram and per pair the two limits and the insert
// size.  The limits go back into the selection as a limited call's limits (select.hip, k_select_limit).
//
// k_pair_correct is the one kernel of the library that CHANGES a chunk: with the pairs' insert sizes it walks each overlap
// once, eight places to a lane, and where the mates disagree and one base is confident and the other poor it replaces the
// poor one -- launched twice, first to judge and count, then, if nothing was refused, to store.
//
// k_merge_size and k_merge_emit write the two mates of every overlapping pair as ONE read into a buffer of the handle: sizes by
// a lane per pair, places by the selection's scan, the bytes by a lane per 16-byte word of the output.
//
// All global stores are ordinary vector stores from plain C++.
#include "fqgpu_internal.h"
#include "sel_words.h"

#include <string.h>

namespace {

// one of a pair call's two chunks on the device: a FqChunkView without its count, which is the call's
struct PairSide {
  uint8_t *raw;  // (k_pair_correct alone writes through it)
  unsigned long long raw_len;
  const fqgpu_rec *recs;  // the first record of the range
  unsigned prev;          // it has a record in front of it in its table (k_pair_names alone needs its header line)
};
PairSide pair_side(const FqChunkView &v) { return {const_cast<uint8_t *>(v.raw), (unsigned long long)v.raw_len, v.recs, v.prev ? 1u : 0u}; }
// no record, two counts, or more than the kernels' 32-bit indices hold
bool pair_views_bad(const FqChunkView &a, const FqChunkView &b) {
  return !a.n_recs || a.n_recs != b.n_recs || a.n_recs >= ((size_t)1 << 32) || a.raw_len >= ((size_t)1 << 32) || b.raw_len >= ((size_t)1 << 32);
}

// ---- the read ids of two chunks compared (include/fqgpu.h, fqgpu_chunk_pair_names)
constexpr unsigned PAIR_THREADS = 256;
constexpr unsigned PAIR_STEP_BYTES = SW_GROUP_LANES * 16;  // bytes of an id a pair's eight lanes hold at a time
// a record's header line: the first byte of its id (behind the '@'), the bytes from there to the line's '\n'
struct PairLine {
  long long id0;
  unsigned cap;
  bool ok;  // the line has its '@' and its '\n' and lies inside the chunk
};
__device__ __forceinline__ PairLine pair_line(const PairSide &s, unsigned long long i, bool have) {
  PairLine l = {0, 0u, true};
  if (!have) return l;
  const fqgpu_rec rec = s.recs[i];
  unsigned long long h0 = 0;
  if (i || s.prev) {
    const fqgpu_rec before = s.recs[(long long)i - 1];
    h0 = (unsigned long long)before.qual_off + before.len + 1ull;
  }
  l.ok = h0 + 2ull <= rec.seq_off && rec.seq_off <= s.raw_len;
  l.id0 = (long long)h0 + 1;
  l.cap = l.ok ? (unsigned)(rec.seq_off - h0 - 2ull) : 0u;
  return l;
}
// the sixteen bytes of an id from place c on; nothing is read from the line's '\n' on (a word reaches at most fifteen bytes
// behind the '\n', where the sequence line stands, or the spare bytes every raw block has behind its chunk)
__device__ __forceinline__ uint4 pair_word(const PairSide &s, const PairLine &l, unsigned c) {
  if (c >= l.cap) return make_uint4(0, 0, 0, 0);
  const SelU128 v = *reinterpret_cast<const SelU128 *>(s.raw + l.id0 + c);
  return make_uint4(v.a, v.b, v.c, v.d);
}
// a bit for each byte of a word that ends an id: ' ', '\t' or '\n' (a byte >= 128 ends none: the compares see seven bits)
__device__ __forceinline__ unsigned pair_ends(const uint4 v) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned ends = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned y = w[i] & ~SW_H;
    ends |= (((sw_eq(y, ' ') | sw_eq(y, '\t') | sw_eq(y, '\n')) & ~w[i]) * CLIP_GATHER) >> 28 << (4 * i);
  }
  return ends;
}
// the id's length without a "/1" or "/2" at its end
__device__ __forceinline__ unsigned pair_strip(const PairSide &s, const PairLine &l, unsigned e) {
  if (e < 2u) return e;
  const unsigned slash = s.raw[l.id0 + e - 2], mate = s.raw[l.id0 + e - 1];
  return slash == '/' && (mate == '1' || mate == '2') ? e - 2u : e;
}

// *first_diff = min(*first_diff, i) for every i < count at which the read ids of A's record i and B's record i differ in
// length or in a byte.  EIGHT LANES TO A PAIR, the judge's grouping: lane j of the eight holds the bytes [16 j, 16 j + 16)
// of both ids, loaded from wherever the ids start, so that the two words of a lane stand for the same places and are
// compared as they are; a header line of 30 to 80 bytes is then one load instruction per side whose eight addresses fall
// into the one or two cache lines that hold the line, where a lane per pair would walk its line word by word, every load
// instruction of the wave over 64 different lines and as many turns as the longest line of the 64 takes.  An id's end is
// the first ' ', '\t' or '\n' (SWAR byte tests, a min-reduction over the eight lanes by shuffles), the line's own '\n' at
// the latest; the two bytes in front of it decide on "/1" and "/2".  A line longer than 128 bytes takes more turns, every
// lane of the wave the same number: a correctness path.  One atomicMin per wave that has a differing pair.
__global__ void __launch_bounds__(PAIR_THREADS)
k_pair_names(const PairSide A, const PairSide B, unsigned count, unsigned long long *__restrict__ first_diff, unsigned *__restrict__ bad) {
  const unsigned lane = fq_lane(), sub = lane & (SW_GROUP_LANES - 1);
  const unsigned long long i = ((unsigned long long)blockIdx.x * PAIR_THREADS + threadIdx.x) / SW_GROUP_LANES;
  const bool have = i < count;
  const PairLine la = pair_line(A, i, have), lb = pair_line(B, i, have);
  const bool fine = have && la.ok && lb.ok;
  unsigned steps = max((max(la.cap, lb.cap) + PAIR_STEP_BYTES - 1) / PAIR_STEP_BYTES, 1u);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) steps = max(steps, (unsigned)__shfl_xor(steps, d));
  steps = fq_uniform(steps);
  const uint4 xa = pair_word(A, la, 16u * sub), xb = pair_word(B, lb, 16u * sub);
  // the ids' ends
  unsigned ea = la.cap, eb = lb.cap;
  for (unsigned s = 0; s < steps; s++) {
    const unsigned c = s * PAIR_STEP_BYTES + 16u * sub;
    const unsigned fa = pair_ends(s ? pair_word(A, la, c) : xa) & sel_bits(0, (int)la.cap - (int)c);
    const unsigned fb = pair_ends(s ? pair_word(B, lb, c) : xb) & sel_bits(0, (int)lb.cap - (int)c);
    if (fa) ea = min(ea, c + (unsigned)__builtin_ctz(fa));
    if (fb) eb = min(eb, c + (unsigned)__builtin_ctz(fb));
  }
#pragma unroll
  for (unsigned d = 1; d < SW_GROUP_LANES; d <<= 1) {
    ea = min(ea, (unsigned)__shfl_xor(ea, d));
    eb = min(eb, (unsigned)__shfl_xor(eb, d));
  }
  if (fine) {
    ea = pair_strip(A, la, ea);
    eb = pair_strip(B, lb, eb);
  }
  // the bytes in front of them
  unsigned differ = ea != eb;
  for (unsigned s = 0; s < steps; s++) {
    const unsigned c = s * PAIR_STEP_BYTES + 16u * sub;
    const uint4 va = s ? pair_word(A, la, c) : xa, vb = s ? pair_word(B, lb, c) : xb;
    const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
    const int left = (int)min(ea, eb) - (int)c;  // the id's bytes from this word's first on
#pragma unroll
    for (int k = 0; k < 4; k++) differ |= ((wa[k] ^ wb[k]) & sw_mask(-4 * k, left - 4 * k)) != 0u;
  }
#pragma unroll
  for (unsigned d = 1; d < SW_GROUP_LANES; d <<= 1) differ |= __shfl_xor(differ, d);
  const unsigned long long found = __ballot(fine && differ);
  if (found && lane == (unsigned)__builtin_ctzll(found)) atomicMin(first_diff, i);  // (the wave's pairs rise with its lanes)
  if (__any(have && !fine) && lane == 0) *bad = 1u;  // (every writer stores the same value)
}

// ---- the mate overlap of two chunks' records (include/fqgpu.h, fqgpu_chunk_pair_overlap).  A workgroup is ONE wave and takes
// 64 consecutive pairs: their table entries with one load, lane = pair, and their results back to the pair's lane at the
// end, so that the three arrays go out as three coalesced stores.  The pairs are then taken one after the other by all 64
// lanes.  Loading: a line has at most 512 bases, lane j reads the eight bytes [8 j, 8 j + 8) of each line from wherever the
// line starts (the 64 spare bytes behind every chunk let the last word be read whole) and turns them into eight bits of
// three planes -- the base's code A 00, C 01, G 10, T 11 as a low and a high plane, and an N plane -- by the packed compares
// clip_planes uses; a byte that is none of ACGTN refuses the chunk.  The planes lie in LDS as bytes, read back as words: bit i
// of word w is base 32 w + i.  The complement of a code is its inverse, so r = revcomp(s2) is s2's planes bit-reversed over
// all 512 places (byte 63 - j takes the reversed byte j), the two code planes inverted; r[0] then stands at bit 512 - L2,
// an offset that folds into the candidate's shift.  Searching: a lane takes one candidate d, 64 candidates in the order of
// the rule at a time -- d = 0 .. L1 - min_overlap, then -1 .. -(L2 - min_overlap): exactly the shifts with ov >= min_overlap --
// and walks the words of s1: the s1 words are the same for every lane (a broadcast), the bits of r beside them a funnel
// shift of two neighbouring words, of which one is carried over; two XORs, the N planes, the mask of [lo, hi) and a
// population count per word.  The first hit wins, so the round in which a lane hits is the last one (the lowest lane of the
// ballot), and a round's walk ends as soon as no lane can hit any more -- mism only grows --, which for unrelated mates is
// after the first word.  r's planes have 512 bits of slack on either side, so no index is tested.  Counters are kept by
// the wave, the histogram in LDS; both go out as one atomic per touched word and workgroup.
constexpr unsigned OV_THREADS = 64, OV_WG_PAIRS = 64;
constexpr unsigned OV_WORDS = FQGPU_OVERLAP_MAX_LEN / 32;  // words of a plane
constexpr unsigned OV_R_WORDS = 3 * OV_WORDS;              // ... of a plane of r: slack, the plane, slack
constexpr unsigned OV_HEAD = 16;                           // words in front of the rows
static_assert(OV_THREADS == 64 && OV_WG_PAIRS == 64 && FQGPU_OVERLAP_MAX_LEN == 8 * OV_THREADS, "lane = pair, and eight bases of a line to a lane");
static_assert(FQGPU_OVERLAP_ROWS >= 2 * FQGPU_OVERLAP_MAX_LEN && FQGPU_OVERLAP_WORDS == OV_HEAD + FQGPU_OVERLAP_ROWS, "I <= 1023 has a row");
struct OvSpec {
  unsigned min_overlap, max_mism, max_err_pct;
};
struct __attribute__((packed)) OvU64 { uint32_t a, b; };  // eight bytes at any address
struct OvBits {
  unsigned lo, hi, n;  // eight bits each
  bool bad;
};
// the planes of the bases [8 lane, 8 lane + 8) of a line of len <= 512 bases that lies inside its chunk
__device__ __forceinline__ OvBits ov_bits(const uint8_t *__restrict__ raw, unsigned off, unsigned len, unsigned lane) {
  OvBits b = {0u, 0u, 0u, false};
  const unsigned p = 8u * lane;
  if (p >= len) return b;
  const OvU64 v = *reinterpret_cast<const OvU64 *>(raw + off + p);
  const unsigned w[2] = {v.a, v.b}, in = sel_bits(0, (int)(len - p)) & 0xFFu;
  unsigned fine = 0;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const unsigned y = w[i] & ~SW_H;
    const unsigned ea = sw_eq(y, 'A'), ec = sw_eq(y, 'C'), eg = sw_eq(y, 'G'), et = sw_eq(y, 'T'), en = sw_eq(y, 'N');
    b.lo |= ((ec | et) * CLIP_GATHER) >> 28 << (4 * i);
    b.hi |= ((eg | et) * CLIP_GATHER) >> 28 << (4 * i);
    b.n |= (en * CLIP_GATHER) >> 28 << (4 * i);
    fine |= (((ea | ec | eg | et | en) & ~w[i]) * CLIP_GATHER) >> 28 << (4 * i);  // one of ACGTN, and below 128
  }
  b.bad = (~fine & in) != 0u;
  b.lo &= in;
  b.hi &= in;
  b.n &= in;
  return b;
}
// the bits [lo, hi) of a word, any lo and hi
__device__ __forceinline__ unsigned ov_mask(int lo, int hi) {
  const unsigned below_hi = hi <= 0 ? 0u : hi >= 32 ? 0xFFFFFFFFu : (1u << hi) - 1u;
  const unsigned below_lo = lo <= 0 ? 0u : lo >= 32 ? 0xFFFFFFFFu : (1u << lo) - 1u;
  return below_hi & ~below_lo;
}

__global__ void __launch_bounds__(OV_THREADS)
k_pair_overlap(const PairSide A, const PairSide B, unsigned count, const OvSpec sp, unsigned long long *__restrict__ out,
               uint16_t *__restrict__ pairs, unsigned *__restrict__ bad_out) {
  __shared__ unsigned s1[3][OV_WORDS];    // mate 1: the code's low bit, its high bit, N
  __shared__ unsigned rr[3][OV_R_WORDS];  // r, the code planes inverted already; the plane is the words [OV_WORDS, 2 OV_WORDS)
  __shared__ unsigned hist[FQGPU_OVERLAP_ROWS];
  const unsigned lane = threadIdx.x;
  for (unsigned i = lane; i < FQGPU_OVERLAP_ROWS; i += OV_THREADS) hist[i] = 0;
  for (unsigned i = lane; i < 3 * OV_R_WORDS; i += OV_THREADS) (&rr[0][0])[i] = 0;
  const unsigned long long p0 = (unsigned long long)blockIdx.x * OV_WG_PAIRS;
  const bool have = p0 + lane < count;
  fqgpu_rec ra = {0u, 0u, 0u}, rb = {0u, 0u, 0u};
  if (have) {
    ra = A.recs[p0 + lane];
    rb = B.recs[p0 + lane];
  }
  const bool ok = have && sel_line_inside(ra.seq_off, ra.len, A.raw_len) && sel_line_inside(rb.seq_off, rb.len, B.raw_len);
  const bool analysed = ok && ra.len <= FQGPU_OVERLAP_MAX_LEN && rb.len <= FQGPU_OVERLAP_MAX_LEN;
  bool bad = have && !ok;
  unsigned my_limit_a = ra.len, my_limit_b = rb.len, my_insert = 0;  // the lane's pair: no hit so far
  unsigned n_over = 0, n_through = 0, behind_a = 0, behind_b = 0, n_mism = 0, n_ov = 0;  // (the same in every lane; 64 pairs of <= 512 bases)
  uint8_t *const s1_bytes = reinterpret_cast<uint8_t *>(&s1[0][0]);
  uint8_t *const rr_bytes = reinterpret_cast<uint8_t *>(&rr[0][0]);
  unsigned long long todo = __ballot(analysed);
  while (todo) {  // (uniform)
    const unsigned p = (unsigned)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    const unsigned L1 = fq_uniform(__shfl(ra.len, p)), L2 = fq_uniform(__shfl(rb.len, p));
    const unsigned off_a = fq_uniform(__shfl(ra.seq_off, p)), off_b = fq_uniform(__shfl(rb.seq_off, p));
    const OvBits x = ov_bits(A.raw, off_a, L1, lane), y = ov_bits(B.raw, off_b, L2, lane);
    bad = bad || x.bad || y.bad;
    __syncthreads();  // the pair in front has been searched
    s1_bytes[lane] = (uint8_t)x.lo;
    s1_bytes[4 * OV_WORDS + lane] = (uint8_t)x.hi;
    s1_bytes[8 * OV_WORDS + lane] = (uint8_t)x.n;
    rr_bytes[4 * OV_WORDS + 63 - lane] = (uint8_t)(~__brev(y.lo) >> 24);
    rr_bytes[4 * (OV_R_WORDS + OV_WORDS) + 63 - lane] = (uint8_t)(~__brev(y.hi) >> 24);
    rr_bytes[4 * (2 * OV_R_WORDS + OV_WORDS) + 63 - lane] = (uint8_t)(__brev(y.n) >> 24);
    __syncthreads();
    const bool can = L1 >= sp.min_overlap && L2 >= sp.min_overlap;
    const unsigned n_pos = can ? L1 - sp.min_overlap + 1u : 0u, n_cand = can ? n_pos + L2 - sp.min_overlap : 0u;
    const unsigned words = (L1 + 31u) / 32u;
    bool hit = false;
    int hit_d = 0;
    unsigned hit_mism = 0, hit_ov = 0;
    for (unsigned c0 = 0; c0 < n_cand && !hit; c0 += OV_THREADS) {  // (uniform)
      const unsigned c = c0 + lane;
      const bool live = c < n_cand;
      const int d = !live ? 0 : c < n_pos ? (int)c : -(int)(c - n_pos + 1u);
      const int lo = max(d, 0), hi = min((int)L1, d + (int)L2);
      const unsigned ov = (unsigned)(hi - lo), bound = min(sp.max_mism, sp.max_err_pct * ov / 100u);
      // r[i - d] is bit i + q0 of r's planes with their slack: q0 = 512 + (512 - L2) - d, in 1 .. 1023
      const unsigned q0 = (unsigned)(2 * (int)FQGPU_OVERLAP_MAX_LEN - (int)L2 - d), sh = q0 & 31u, qw = q0 >> 5;
      unsigned mism = live ? 0u : 0xFFFF0000u;  // (a lane without a candidate never hits)
      unsigned c_lo = rr[0][qw], c_hi = rr[1][qw], c_n = rr[2][qw];
      for (unsigned w = 0; w < words; w++) {  // (uniform)
        const unsigned n_lo = rr[0][qw + w + 1u], n_hi = rr[1][qw + w + 1u], n_n = rr[2][qw + w + 1u];
        const unsigned r_lo = __builtin_amdgcn_alignbit(n_lo, c_lo, sh), r_hi = __builtin_amdgcn_alignbit(n_hi, c_hi, sh),
                       r_n = __builtin_amdgcn_alignbit(n_n, c_n, sh);
        const unsigned differ = ((s1[0][w] ^ r_lo) | (s1[1][w] ^ r_hi) | s1[2][w] | r_n) & ov_mask(lo - 32 * (int)w, hi - 32 * (int)w);
        mism += (unsigned)__popc(differ);
        c_lo = n_lo;
        c_hi = n_hi;
        c_n = n_n;
        if (!__any(mism <= bound)) break;  // (mism only grows)
      }
      const unsigned long long hits = __ballot(live && mism <= bound);
      if (hits) {  // (uniform) the round's candidates rise with its lanes
        const int first = __builtin_ctzll(hits);
        hit = true;
        hit_d = __shfl(d, first);
        hit_mism = __shfl(mism, first);
        hit_ov = __shfl(ov, first);
      }
    }
    if (hit) {
      const unsigned I = (unsigned)(hit_d + (int)L2), limit_a = min(L1, I), limit_b = min(L2, I);
      n_over++;
      n_through += limit_a < L1 || limit_b < L2;
      behind_a += L1 - limit_a;
      behind_b += L2 - limit_b;
      n_mism += hit_mism;
      n_ov += hit_ov;
      if (lane == p) {
        my_limit_a = limit_a;
        my_limit_b = limit_b;
        my_insert = I;
      }
      if (lane == 0) atomicAdd(&hist[I], 1u);  // (I <= L1 - min_overlap + L2 <= 1023)
    }
  }
  __syncthreads();
  for (unsigned i = lane; i < FQGPU_OVERLAP_ROWS; i += OV_THREADS)
    if (const unsigned v = hist[i]) atomicAdd(&out[OV_HEAD + i], (unsigned long long)v);
  const unsigned skipped = (unsigned)__popcll(__ballot(ok && !analysed));
  const unsigned cnt[8] = {0u, n_over, n_through, behind_a, behind_b, skipped, n_mism, n_ov};
#pragma unroll
  for (unsigned i = 1; i < 8; i++)
    if (lane == i && cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
  if (have) {
    pairs[p0 + lane] = (uint16_t)my_limit_a;
    pairs[(unsigned long long)count + p0 + lane] = (uint16_t)my_limit_b;
    pairs[2ull * count + p0 + lane] = (uint16_t)my_insert;
  }
  if (__any(bad) && lane == 0) *bad_out = 1u;  // (every writer stores the same value)
}

// ---- the correction inside the mate overlap (include/fqgpu.h, fqgpu_chunk_pair_correct): THE kernel that changes a chunk.
// k_pair_overlap's shape -- a wave takes 64 consecutive pairs, table entries and inserts with one load, lane = pair, the
// per-pair results back in the pair's lane -- but no LDS: the wave walks the pairs that have an insert one after the other,
// and a lane takes the eight places [lo + 8 lane, lo + 8 lane + 8) of the overlap.  The bytes of s1 and q1 are one eight-byte
// load from wherever the place lies; those of s2 and q2 are the eight bytes that END at j = I - 1 - i, taken in reverse.
// That window starts up to seven bytes in front of j's line -- bytes of a place behind hi, which is not judged -- and for a
// chunk's first record in front of the chunk: its start is clamped to the chunk's first byte and the word shifted up by what
// was clamped.  Reads behind a line's end fall into the chunk or its 64 spare bytes.  A place is decided from its own four
// bytes, and no byte belongs to two places, so the launch with APPLY = false (it judges, counts and stores nothing into the
// chunks) and the launch with APPLY = true (it stores, and counts nothing) decide alike, and the second one runs only when
// the first refused nothing.  A store goes to s1[i], q1[i], i in [lo, hi), or s2[j], q2[j], j in [0, L2): inside lines that
// the lane = pair check found inside their chunks.  Corrections are rare: plain byte stores under the lane's predicate.
__device__ __forceinline__ unsigned long long cor_load8(const uint8_t *p) {
  const OvU64 v = *reinterpret_cast<const OvU64 *>(p);
  return (unsigned long long)v.b << 32 | v.a;
}
// the eight bytes of a chunk at off + rel (rel >= -7, off + rel + 8 > 0); the bytes in front of the chunk read as zero
__device__ __forceinline__ unsigned long long cor_load8_back(const uint8_t *raw, unsigned off, int rel) {
  const long long at = (long long)off + rel;
  const unsigned clamped = at < 0 ? (unsigned)-at : 0u;
  return cor_load8(raw + (at + clamped)) << (8u * clamped);
}
__device__ __forceinline__ unsigned cor_comp(unsigned b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b; }
__device__ __forceinline__ bool cor_is_base(unsigned b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'N'; }
__device__ __forceinline__ unsigned cor_wave_sum(unsigned v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

template <bool APPLY>
__global__ void __launch_bounds__(OV_THREADS)
k_pair_correct(const PairSide A, const PairSide B, unsigned count, const uint16_t *__restrict__ inserts, unsigned good_q, unsigned bad_q,
               unsigned long long *__restrict__ out, uint16_t *__restrict__ fixed, unsigned *__restrict__ bad_out) {
  const unsigned lane = threadIdx.x;
  const unsigned long long p0 = (unsigned long long)blockIdx.x * OV_WG_PAIRS;
  const bool have = p0 + lane < count;
  fqgpu_rec ra = {0u, 0u, 0u}, rb = {0u, 0u, 0u};
  unsigned ins = 0;
  if (have) ins = inserts[p0 + lane];
  if (ins) {  // (a pair without an insert: none of its lines, and not its table entries either)
    ra = A.recs[p0 + lane];
    rb = B.recs[p0 + lane];
  }
  const auto inside = [](const fqgpu_rec &r, unsigned long long raw_len) {
    return r.len != 0 && r.len <= FQGPU_OVERLAP_MAX_LEN && (unsigned long long)r.seq_off + r.len <= raw_len &&
           (unsigned long long)r.qual_off + r.len <= raw_len;
  };
  const bool ok = ins && inside(ra, A.raw_len) && inside(rb, B.raw_len) && ins <= ra.len + rb.len - 1u;
  bool bad = ins && !ok;
  unsigned my_fixed_a = 0, my_fixed_b = 0;                            // the lane's pair
  unsigned n_fa = 0, n_fb = 0, n_res = 0, n_mism = 0;                 // the lane's places, over all pairs
  unsigned n_pairs_fixed = 0, n_ov = 0;                               // (the same in every lane)
  unsigned long long todo = __ballot(ok);
  while (todo) {  // (uniform)
    const unsigned p = (unsigned)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    const unsigned L1 = fq_uniform(__shfl(ra.len, p)), L2 = fq_uniform(__shfl(rb.len, p)), I = fq_uniform(__shfl(ins, p));
    const unsigned s1_off = fq_uniform(__shfl(ra.seq_off, p)), q1_off = fq_uniform(__shfl(ra.qual_off, p));
    const unsigned s2_off = fq_uniform(__shfl(rb.seq_off, p)), q2_off = fq_uniform(__shfl(rb.qual_off, p));
    const unsigned lo = I > L2 ? I - L2 : 0u, hi = min(L1, I);  // hi - lo >= 1, and <= 512
    n_ov += hi - lo;
    const unsigned i0 = lo + 8u * lane;
    unsigned fa = 0, fb = 0;
    if (i0 < hi) {
      const unsigned n = min(8u, hi - i0);
      const int j0 = (int)I - 1 - (int)i0 - 7;  // the window [j0, j0 + 8) of mate 2: place i0 + t stands beside j0 + 7 - t
      const unsigned long long s1 = cor_load8(A.raw + s1_off + i0), q1 = cor_load8(A.raw + q1_off + i0);
      const unsigned long long s2 = cor_load8_back(B.raw, s2_off, j0), q2 = cor_load8_back(B.raw, q2_off, j0);
#pragma unroll
      for (unsigned t = 0; t < 8; t++) {
        const unsigned b1 = (unsigned)(s1 >> (8u * t)) & 0xFFu, c1 = (unsigned)(q1 >> (8u * t)) & 0xFFu;
        const unsigned b2 = (unsigned)(s2 >> (8u * (7u - t))) & 0xFFu, c2 = (unsigned)(q2 >> (8u * (7u - t))) & 0xFFu;
        const bool in = t < n;
        bad = bad || (in && !(cor_is_base(b1) && cor_is_base(b2) && c1 >= 33u && c1 <= 96u && c2 >= 33u && c2 <= 96u));
        const unsigned p1 = c1 - 33u, p2 = c2 - 33u;
        const bool differ = in && (b1 == 'N' || b2 == 'N' || b1 != cor_comp(b2));
        const bool win1 = differ && b1 != 'N' && p1 >= good_q && p2 <= bad_q;
        const bool win2 = differ && b2 != 'N' && p2 >= good_q && p1 <= bad_q;
        n_mism += differ;
        fb += win1;
        fa += win2;
        n_res += (win1 && b2 == 'N') || (win2 && b1 == 'N');
        if (APPLY) {
          const unsigned j = (unsigned)(j0 + 7 - (int)t);  // (in [0, L2) for a place of the overlap)
          if (win1) {
            B.raw[s2_off + j] = (uint8_t)cor_comp(b1);
            B.raw[q2_off + j] = (uint8_t)c1;
          }
          if (win2) {
            A.raw[s1_off + i0 + t] = (uint8_t)cor_comp(b2);
            A.raw[q1_off + i0 + t] = (uint8_t)c2;
          }
        }
      }
    }
    if (!APPLY && __any(fa | fb)) {  // (uniform, and rare)
      const unsigned pa = cor_wave_sum(fa), pb = cor_wave_sum(fb);
      n_pairs_fixed++;
      if (lane == p) {
        my_fixed_a = pa;
        my_fixed_b = pb;
      }
    }
    n_fa += fa;
    n_fb += fb;
  }
  if (APPLY) return;
  const unsigned cnt[8] = {0u, (unsigned)__popcll(__ballot(ins != 0u)), n_pairs_fixed, cor_wave_sum(n_fa), cor_wave_sum(n_fb),
                           cor_wave_sum(n_res), cor_wave_sum(n_mism), n_ov};
#pragma unroll
  for (unsigned i = 1; i < 8; i++)
    if (lane == i && cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
  if (have) {
    fixed[p0 + lane] = (uint16_t)my_fixed_a;
    fixed[(unsigned long long)count + p0 + lane] = (uint16_t)my_fixed_b;
  }
  if (__any(bad) && lane == 0) *bad_out = 1u;  // (every writer stores the same value)
}

// ---- the two mates merged into one read (include/fqgpu.h, fqgpu_chunk_pair_merge).  Two kernels with the selection's scan
// between them, and no chunk is written.  k_merge_size is lane = pair: the insert, the mark bit and -- for a pair with an insert
// -- the two table entries; it holds the inserts against the lengths, finds the merged pairs and their records inside their
// chunks, and leaves per pair the record's size (the header line without its '\n' + 2 I + 5, or 0), per wave the merged bits and the counters that
// need no line.  fq_scan_u32_to_u64 turns the sizes into the records' places, 64-bit as the selection's koff.  k_merge_emit is
// driven by the OUTPUT, as k_select_gather is: a workgroup owns an aligned 16 KiB tile of the merged bytes and finds the tile's
// first and last record with two uniform searches; a lane owns four aligned 16-byte words of it, one in each of four rounds,
// and finds a word's record with sel_find between those two.  A word inside the header line is one unaligned load from mate 1.  A word inside the bases or inside the
// qualities covers the places [p0, p0 + 16): sixteen bytes of s1 and of q1 at p0 and the sixteen bytes of s2 and of q2 that END
// at j = I - 1 - p0, read in reverse -- both kinds of word need all four lines, the base for the quality and the quality for the
// base.  Such a window of mate 2 starts at I - 16 - p0 >= 0, inside the line, because the whole word lies in front of place I;
// a side none of whose sixteen places exists is not loaded, and a load behind a line's end falls into the chunk or its 64 spare
// bytes.  Every other word -- one that holds a seam: header | bases | "\n+\n" | qualities | '\n' | the next record -- is put
// together byte by byte with mg_byte, as the gather does with sel_byte.  A place is counted and judged once, by the lane that
// owns its BASE byte, so the sums do not depend on the tiling; a wave reduction, then one atomic per workgroup and word.
// Stores go to the handle's merge buffer alone, which reaches to the next multiple of 16.
constexpr unsigned MG_EMIT_THREADS = 256, MG_EMIT_WORDS = 4, MG_TILE_BYTES = MG_EMIT_THREADS * 16 * MG_EMIT_WORDS;  // (the gather's tile)
constexpr unsigned MG_BYTES = 4, MG_OVERLAP = 5, MG_COUNTERS = 12;  // report words: bytes_out; the emit pass's first of three; all
static_assert(FQGPU_MERGE_REPORT_WORDS <= FQGPU_TAIL_REPORT_WORDS, "the counters are the selection result's words");

// the start of record i's header line in its chunk
__device__ __forceinline__ unsigned long long mg_h0(const PairSide &s, unsigned long long i) {
  if (!(i || s.prev)) return 0ull;
  const fqgpu_rec before = s.recs[(long long)i - 1];
  return (unsigned long long)before.qual_off + before.len + 1ull;
}

__global__ void __launch_bounds__(OV_THREADS)
k_merge_size(const PairSide A, const PairSide B, unsigned count, const uint16_t *__restrict__ inserts, const unsigned long long *__restrict__ mark,
             unsigned min_len, uint32_t *__restrict__ msize, unsigned long long *__restrict__ mbits, SelectResult *__restrict__ res) {
  const unsigned lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * OV_WG_PAIRS + lane;
  const bool have = i < count;
  const unsigned ins = have ? inserts[i] : 0u;
  const bool marked = have && (!mark || ((mark[blockIdx.x] >> lane) & 1ull));
  fqgpu_rec ra = {0u, 0u, 0u}, rb = {0u, 0u, 0u};
  if (ins) {  // (a pair without an insert: not its table entries either)
    ra = A.recs[i];
    rb = B.recs[i];
  }
  const bool valid = !ins || (ra.len <= FQGPU_OVERLAP_MAX_LEN && rb.len <= FQGPU_OVERLAP_MAX_LEN && ins + 1u <= ra.len + rb.len);
  bool merged = ins && valid && marked && ins >= min_len, bad = !valid;
  unsigned hl = 0;
  if (merged) {
    const auto inside = [](const fqgpu_rec &r, unsigned long long raw_len) {
      return r.len != 0 && (unsigned long long)r.seq_off + r.len <= raw_len && (unsigned long long)r.qual_off + r.len <= raw_len;
    };
    const unsigned long long h0 = mg_h0(A, i);
    merged = inside(ra, A.raw_len) && inside(rb, B.raw_len) && h0 + 2ull <= ra.seq_off;
    bad = !merged;
    if (merged) hl = (unsigned)(ra.seq_off - h0);
  }
  const unsigned size = merged ? hl + 2u * ins + 4u : 0u;
  if (have) msize[i] = size;
  const unsigned long long bits = __ballot(merged);
  if (lane == 0) mbits[blockIdx.x] = bits;
  const unsigned cnt[MG_COUNTERS] = {0u,
                            (unsigned)__popcll(__ballot(ins != 0u)),
                            (unsigned)__popcll(bits),
                            cor_wave_sum(merged ? ins : 0u),
                            cor_wave_sum(size),
                            0u,
                            0u,
                            0u,
                            cor_wave_sum(merged ? ra.len - min(ra.len, ins) : 0u),
                            cor_wave_sum(merged ? rb.len - min(rb.len, ins) : 0u),
                            (unsigned)__popcll(__ballot(ins != 0u && !marked)),
                            (unsigned)__popcll(__ballot(ins != 0u && marked && ins < min_len))};
#pragma unroll
  for (unsigned k = 1; k < MG_COUNTERS; k++)
    if (lane == k && cnt[k]) atomicAdd(&res->w[k], (unsigned long long)cnt[k]);
  if (__any(bad) && lane == 0) res->bad = 1u;  // (every writer stores the same value)
}

// a merged pair as the emit pass sees it: where its pieces come from
struct MgRec {
  unsigned long long h0;  // mate 1's header line in its chunk
  unsigned hl, I, L1, L2, s1, q1, s2, q2;
};
__device__ __forceinline__ MgRec mg_rec(const PairSide &A, const PairSide &B, const uint16_t *__restrict__ inserts, unsigned r) {
  const fqgpu_rec ra = A.recs[r], rb = B.recs[r];
  MgRec c;
  c.h0 = mg_h0(A, r);
  c.hl = (unsigned)(ra.seq_off - c.h0);
  c.I = inserts[r];
  c.L1 = ra.len;
  c.L2 = rb.len;
  c.s1 = ra.seq_off;
  c.q1 = ra.qual_off;
  c.s2 = rb.seq_off;
  c.q2 = rb.qual_off;
  return c;
}
// one place of a merged read from its up to four bytes (b2: mate 2's base as it stands in its line)
struct MgPlace {
  unsigned base, qual;
  bool both, disagree, n, bad;
};
__device__ __forceinline__ MgPlace mg_place(unsigned b1, unsigned c1, unsigned b2_raw, unsigned c2, bool in1, bool in2, unsigned floor_q) {
  MgPlace o;
  const unsigned b2 = cor_comp(b2_raw), p1 = c1 - 33u, p2 = c2 - 33u;
  o.bad = (in1 && !(cor_is_base(b1) && p1 <= 63u)) || (in2 && !(cor_is_base(b2_raw) && p2 <= 63u));
  const bool n1 = b1 == 'N', n2 = b2 == 'N';
  o.both = in1 && in2;
  o.n = o.both && (n1 || n2);
  o.disagree = o.both && !n1 && !n2 && b1 != b2;
  const bool take1 = !in2 || (in1 && !n1 && (n2 || p1 >= p2 || b1 == b2));  // mate 1's base stands (an equal base is either's)
  const unsigned hi = max(p1, p2), lo = min(p1, p2);
  const unsigned q_both = n1 && n2 ? lo : n1 ? p2 : n2 ? p1 : b1 == b2 ? hi : max(hi - lo, floor_q);
  o.base = !o.both ? (in1 ? b1 : b2) : n1 && n2 ? (unsigned)'N' : take1 ? b1 : b2;
  o.qual = (!o.both ? (in1 ? p1 : p2) : q_both) + 33u;
  return o;
}
struct MgCounts {
  unsigned ov, disagree, n;
  bool bad;
};
__device__ __forceinline__ void mg_count(MgCounts &k, const MgPlace &o) {
  k.ov += o.both;
  k.disagree += o.disagree;
  k.n += o.n;
  k.bad = k.bad || o.bad;
}
// byte j of the pair's merged record; a base byte counts and judges its place
__device__ __forceinline__ unsigned mg_byte(const PairSide &A, const PairSide &B, const MgRec &c, unsigned j, unsigned floor_q, MgCounts &k) {
  if (j < c.hl) return A.raw[c.h0 + j];
  j -= c.hl;
  const bool is_base = j < c.I;
  if (!is_base) {
    j -= c.I;
    if (j < 3u) return j == 1u ? '+' : '\n';
    j -= 3u;
    if (j >= c.I) return '\n';
  }
  const unsigned p = j, jj = c.I - 1u - p;
  const bool in1 = p < c.L1, in2 = jj < c.L2;
  unsigned b1 = 0, c1 = 0, b2 = 0, c2 = 0;
  if (in1) {
    b1 = A.raw[c.s1 + p];
    c1 = A.raw[c.q1 + p];
  }
  if (in2) {
    b2 = B.raw[c.s2 + jj];
    c2 = B.raw[c.q2 + jj];
  }
  const MgPlace o = mg_place(b1, c1, b2, c2, in1, in2, floor_q);
  if (is_base) mg_count(k, o);
  return (is_base ? o.base : o.qual) & 0xFFu;
}
__device__ __forceinline__ uint4 mg_load16(const uint8_t *p, bool any) {
  if (!any) return make_uint4(0, 0, 0, 0);
  const SelU128 v = *reinterpret_cast<const SelU128 *>(p);
  return make_uint4(v.a, v.b, v.c, v.d);
}

__global__ void __launch_bounds__(MG_EMIT_THREADS)
k_merge_emit(const PairSide A, const PairSide B, unsigned count, const uint16_t *__restrict__ inserts, const unsigned long long *__restrict__ koff,
             unsigned long long total, unsigned floor_q, uint8_t *__restrict__ dst, SelectResult *__restrict__ res) {
  __shared__ unsigned wg[4];  // overlap_bases, places_disagree, places_n, refused
  if (threadIdx.x < 4) wg[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long t0 = (unsigned long long)blockIdx.x * MG_TILE_BYTES;  // (below total: the grid is the tiles)
  const unsigned long long t1 = min(total, t0 + MG_TILE_BYTES) - 1;              // the tile's last byte
  const unsigned r_lo = sel_find(koff, 0, count - 1, t0), r_hi = sel_find(koff, r_lo, count - 1, t1);  // (uniform)
  MgCounts k = {0u, 0u, 0u, false};
#pragma unroll 1
  for (unsigned word = 0; word < MG_EMIT_WORDS; word++) {  // (a round's words lie side by side: coalesced stores)
    const unsigned long long o = t0 + 16ull * (word * MG_EMIT_THREADS + threadIdx.x);
    if (o >= total) break;
    unsigned r = sel_find(koff, r_lo, r_hi, o);
    MgRec c = mg_rec(A, B, inserts, r);
    unsigned long long base = koff[r];
    const unsigned j0 = (unsigned)(o - base);
    const unsigned sep0 = c.hl + c.I, q0 = sep0 + 3u, end0 = q0 + c.I;  // "\n+\n" | the qualities | the last '\n'
    uint4 w = make_uint4(0, 0, 0, 0);
    if (j0 + 16u <= c.hl) {
      w = mg_load16(A.raw + c.h0 + j0, true);
    } else if ((j0 >= c.hl && j0 + 16u <= sep0) || (j0 >= q0 && j0 + 16u <= end0)) {
      const bool is_base = j0 < sep0;
      const unsigned p0 = j0 - (is_base ? c.hl : q0), jlo = c.I - 16u - p0;  // place p0 + t stands beside jlo + 15 - t of mate 2
      const bool any1 = p0 < c.L1, any2 = jlo < c.L2;
      const uint4 s1 = mg_load16(A.raw + c.s1 + p0, any1), q1 = mg_load16(A.raw + c.q1 + p0, any1);
      const uint4 s2 = mg_load16(B.raw + c.s2 + jlo, any2), q2 = mg_load16(B.raw + c.q2 + jlo, any2);
      const unsigned s1w[4] = {s1.x, s1.y, s1.z, s1.w}, q1w[4] = {q1.x, q1.y, q1.z, q1.w};
      // mate 2's words in reverse order, their bytes swapped: byte t is the line's byte jlo + 15 - t
      const unsigned s2w[4] = {__builtin_bswap32(s2.w), __builtin_bswap32(s2.z), __builtin_bswap32(s2.y), __builtin_bswap32(s2.x)};
      const unsigned q2w[4] = {__builtin_bswap32(q2.w), __builtin_bswap32(q2.z), __builtin_bswap32(q2.y), __builtin_bswap32(q2.x)};
      unsigned ow[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (unsigned t = 0; t < 16; t++) {
        const unsigned sh = 8u * (t & 3u);
        const MgPlace pl = mg_place((s1w[t >> 2] >> sh) & 0xFFu, (q1w[t >> 2] >> sh) & 0xFFu, (s2w[t >> 2] >> sh) & 0xFFu,
                                    (q2w[t >> 2] >> sh) & 0xFFu, p0 + t < c.L1, jlo + 15u - t < c.L2, floor_q);
        if (is_base) mg_count(k, pl);
        ow[t >> 2] |= ((is_base ? pl.base : pl.qual) & 0xFFu) << sh;
      }
      w = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    } else {  // a seam
      unsigned long long lo = 0, hi = 0;
      unsigned size = end0 + 1u;
      for (unsigned t = 0; t < 16 && o + t < total; t++) {
        if (o + t - base >= size) {  // the next merged record
          r = sel_find(koff, r + 1, r_hi, o + t);
          c = mg_rec(A, B, inserts, r);
          base = koff[r];
          size = c.hl + 2u * c.I + 4u;
        }
        const unsigned long long v = mg_byte(A, B, c, (unsigned)(o + t - base), floor_q, k);
        if (t < 8) lo |= v << (8u * t); else hi |= v << (8u * (t - 8u));
      }
      w = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
    }
    *reinterpret_cast<uint4 *>(dst + o) = w;
  }
  const unsigned n_ov = cor_wave_sum(k.ov), n_dis = cor_wave_sum(k.disagree), n_n = cor_wave_sum(k.n);
  const bool any_bad = __any(k.bad);
  if (fq_lane() == 0) {
    if (n_ov) atomicAdd(&wg[0], n_ov);
    if (n_dis) atomicAdd(&wg[1], n_dis);
    if (n_n) atomicAdd(&wg[2], n_n);
    if (any_bad) wg[3] = 1u;  // (every writer stores the same value)
  }
  __syncthreads();
  if (threadIdx.x < 3 && wg[threadIdx.x]) atomicAdd(&res->w[MG_OVERLAP + threadIdx.x], (unsigned long long)wg[threadIdx.x]);
  if (threadIdx.x == 3 && wg[3]) res->bad = 1u;
}

}  // namespace

// The read ids compared.  One kernel, one wait; the result word is word 0 of the selection's result.
int fq_pair_names(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, size_t *mismatch) {
  *mismatch = (size_t)-1;
  if (pair_views_bad(a, b)) return FQGPU_E_ARG;
  const size_t count = a.n_recs;
  SelectScratch &ss = ctx->select;
  int rc;
  if ((rc = ss.begin(st))) return rc;
  SelectResult *const dev = ss.res.as<SelectResult>();
  FQ_HIP(hipMemsetAsync(dev, 0xFF, sizeof(unsigned long long), st));  // word 0: no pair so far
  const size_t per_wg = PAIR_THREADS / SW_GROUP_LANES;
  fq_timer_span_begin(ctx, "pair_names", st);
  hipLaunchKernelGGL(k_pair_names, dim3((unsigned)((count + per_wg - 1) / per_wg)), dim3(PAIR_THREADS), 0, st, pair_side(a), pair_side(b),
                     (unsigned)count, &dev->w[0], &dev->bad);
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  const SelectResult *res;
  if ((rc = ss.finish(st, res))) return rc;
  if (res->bad) return FQGPU_E_ARG;
  *mismatch = res->w[0] == ~0ull ? (size_t)-1 : (size_t)res->w[0];
  return FQGPU_OK;
}

// The mate overlap.  One kernel, one wait: the result words, the three arrays and the verdict come down behind it.
int fq_pair_overlap(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, const fqgpu_overlap *o, uint64_t *out,
                    uint16_t *limit_a_out, uint16_t *limit_b_out, uint16_t *insert_out) {
  memset(out, 0, FQGPU_OVERLAP_WORDS * sizeof(uint64_t));
  if (pair_views_bad(a, b)) return FQGPU_E_ARG;
  const size_t count = a.n_recs;
  SelectScratch &ss = ctx->select;
  int rc;
  if ((rc = ss.overlap_out.reserve(FQGPU_OVERLAP_WORDS * 8)) || (rc = ss.overlap_pairs.reserve(count * 6)) || (rc = ss.begin(st))) return rc;
  uint16_t *const pairs = ss.overlap_pairs.as<uint16_t>();
  FQ_HIP(hipMemsetAsync(ss.overlap_out.p, 0, FQGPU_OVERLAP_WORDS * 8, st));
  const OvSpec sp = {o->min_overlap, o->max_mism, o->max_err_pct};
  fq_timer_span_begin(ctx, "pair_overlap", st);
  hipLaunchKernelGGL(k_pair_overlap, dim3((unsigned)((count + OV_WG_PAIRS - 1) / OV_WG_PAIRS)), dim3(OV_THREADS), 0, st, pair_side(a),
                     pair_side(b), (unsigned)count, sp, ss.overlap_out.as<unsigned long long>(), pairs, &ss.res.as<SelectResult>()->bad);
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipMemcpyAsync(out, ss.overlap_out.p, FQGPU_OVERLAP_WORDS * 8, hipMemcpyDeviceToHost, st));
  if (limit_a_out) FQ_HIP(hipMemcpyAsync(limit_a_out, pairs, count * 2, hipMemcpyDeviceToHost, st));
  if (limit_b_out) FQ_HIP(hipMemcpyAsync(limit_b_out, pairs + count, count * 2, hipMemcpyDeviceToHost, st));
  if (insert_out) FQ_HIP(hipMemcpyAsync(insert_out, pairs + 2 * count, count * 2, hipMemcpyDeviceToHost, st));
  const SelectResult *res;
  if ((rc = ss.finish(st, res))) return rc;
  if (res->bad) {  // (the caller zeroes the three arrays)
    memset(out, 0, FQGPU_OVERLAP_WORDS * sizeof(uint64_t));
    return FQGPU_E_ARG;
  }
  out[0] = count;
  out[8] = fq_overlap_fingerprint(o);
  return FQGPU_OK;
}

// The correction.  The same kernel twice: the first launch judges and counts and leaves the chunks alone; its result words,
// the two arrays and the verdict come down behind it, and only when nothing was refused and a base is to change does the
// second launch store -- so FQGPU_E_ARG leaves both chunks as they were.  The inserts go up as a limited call's limits do.
int fq_pair_correct(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, const uint16_t *insert_in,
                    const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out, uint16_t *fixed_b_out) {
  memset(report, 0, FQGPU_CORRECT_REPORT_WORDS * sizeof(uint64_t));
  if (pair_views_bad(a, b)) return FQGPU_E_ARG;
  const size_t count = a.n_recs;
  SelectScratch &ss = ctx->select;
  int rc;
  if ((rc = ss.correct_in.reserve(count * 2)) || (rc = ss.correct_fixed.reserve(count * 4)) || (rc = ss.begin(st))) return rc;
  SelectResult *const dev = ss.res.as<SelectResult>();
  uint16_t *const fixed = ss.correct_fixed.as<uint16_t>();
  FQ_HIP(hipMemcpyAsync(ss.correct_in.p, insert_in, count * 2, hipMemcpyHostToDevice, st));
  const PairSide A = pair_side(a), B = pair_side(b);
  const dim3 grid((unsigned)((count + OV_WG_PAIRS - 1) / OV_WG_PAIRS));
  static_assert(FQGPU_CORRECT_REPORT_WORDS <= FQGPU_TAIL_REPORT_WORDS, "the counters are the selection result's words");
  fq_timer_span_begin(ctx, "pair_correct", st);
  hipLaunchKernelGGL(k_pair_correct<false>, grid, dim3(OV_THREADS), 0, st, A, B, (unsigned)count, ss.correct_in.as<uint16_t>(), c->good_q, c->bad_q,
                     &dev->w[0], fixed, &dev->bad);
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  if (fixed_a_out) FQ_HIP(hipMemcpyAsync(fixed_a_out, fixed, count * 2, hipMemcpyDeviceToHost, st));
  if (fixed_b_out) FQ_HIP(hipMemcpyAsync(fixed_b_out, fixed + count, count * 2, hipMemcpyDeviceToHost, st));
  const SelectResult *res;
  if ((rc = ss.finish(st, res))) return rc;
  if (res->bad) return FQGPU_E_ARG;  // (the caller zeroes the two arrays)
  for (unsigned i = 1; i < FQGPU_CORRECT_REPORT_WORDS; i++) report[i] = res->w[i];
  report[0] = count;
  if (report[3] + report[4]) {  // the second launch: the stores
    fq_timer_span_begin(ctx, "pair_correct", st);
    hipLaunchKernelGGL(k_pair_correct<true>, grid, dim3(OV_THREADS), 0, st, A, B, (unsigned)count, ss.correct_in.as<uint16_t>(), c->good_q, c->bad_q,
                       &dev->w[0], fixed, &dev->bad);
    fq_timer_span_end(ctx, st);
    FQ_HIP(hipGetLastError());
    FQ_HIP(hipStreamSynchronize(st));
  }
  return FQGPU_OK;
}

// The merge.  Two phases with a wait each, as the selection has them: the size pass and the scan say how many bytes there are
// and whether an insert or a record is refused; the emit pass builds the records in the handle's merge buffer -- whether the
// caller wants the bytes or not, for it also judges the lines and counts the places -- and only behind its verdict are the
// bytes copied down, so FQGPU_E_ARG leaves `out` untouched.  Inserts and mark go up as a limited call's limits and mark do.
int fq_pair_merge(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, const uint16_t *insert_in, const uint8_t *mark_in,
                  const fqgpu_merge *m, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *merged_out) {
  *out_len = 0;
  memset(report, 0, FQGPU_MERGE_REPORT_WORDS * sizeof(uint64_t));
  if (pair_views_bad(a, b)) return FQGPU_E_ARG;
  const size_t count = a.n_recs, n_waves = (count + OV_WG_PAIRS - 1) / OV_WG_PAIRS;
  SelectScratch &ss = ctx->select;
  int rc;
  if ((rc = ss.merge_in.reserve(count * 2)) || (rc = ss.merge_size.reserve(count * 4)) || (rc = ss.merge_bits.reserve(n_waves * 8)) ||
      (rc = ss.koff.reserve((count + 1) * 8)) || (mark_in && (rc = ss.mark.reserve(n_waves * 8))) || (rc = ss.begin(st)))
    return rc;
  SelectResult *const dev = ss.res.as<SelectResult>();
  const uint16_t *const inserts = ss.merge_in.as<uint16_t>();
  unsigned long long *const koff = ss.koff.as<unsigned long long>();
  FQ_HIP(hipMemcpyAsync(ss.merge_in.p, insert_in, count * 2, hipMemcpyHostToDevice, st));
  if (mark_in) {  // (its last word padded with zeros)
    FQ_HIP(hipMemsetAsync(ss.mark.p, 0, n_waves * 8, st));
    FQ_HIP(hipMemcpyAsync(ss.mark.p, mark_in, (count + 7) / 8, hipMemcpyHostToDevice, st));
  }
  const PairSide A = pair_side(a), B = pair_side(b);
  fq_timer_span_begin(ctx, "pair_merge", st);
  hipLaunchKernelGGL(k_merge_size, dim3((unsigned)n_waves), dim3(OV_THREADS), 0, st, A, B, (unsigned)count, inserts,
                     mark_in ? ss.mark.as<unsigned long long>() : nullptr, m->min_len, ss.merge_size.as<uint32_t>(),
                     ss.merge_bits.as<unsigned long long>(), dev);
  FQ_HIP(hipGetLastError());
  rc = fq_scan_u32_to_u64(st, ss.merge_size.as<uint32_t>(), count, koff, ss.scan_tmp);
  fq_timer_span_end(ctx, st);
  if (rc) return rc;
  if (merged_out) FQ_HIP(hipMemcpyAsync(merged_out, ss.merge_bits.p, (count + 7) / 8, hipMemcpyDeviceToHost, st));
  const SelectResult *res;
  if ((rc = ss.finish(st, res))) return rc;
  if (res->bad) return FQGPU_E_ARG;  // (the caller zeroes merged_out)
  const size_t total = (size_t)res->w[MG_BYTES];
  if (total) {  // the second phase: the records
    if ((rc = ss.merge_out.reserve((total + 15) / 16 * 16))) return rc;
    fq_timer_span_begin(ctx, "pair_merge", st);
    hipLaunchKernelGGL(k_merge_emit, dim3((unsigned)((total + MG_TILE_BYTES - 1) / MG_TILE_BYTES)), dim3(MG_EMIT_THREADS), 0, st, A, B,
                       (unsigned)count, inserts, koff, (unsigned long long)total, m->floor_q, ss.merge_out.as<uint8_t>(), dev);
    fq_timer_span_end(ctx, st);
    FQ_HIP(hipGetLastError());
    if ((rc = ss.finish(st, res))) return rc;
    if (res->bad) return FQGPU_E_ARG;
  }
  for (unsigned i = 1; i < MG_COUNTERS; i++) report[i] = res->w[i];
  report[0] = count;
  *out_len = total;
  if (!out || !total) return FQGPU_OK;
  if (out_cap < total) return FQGPU_E_OVERFLOW;
  FQ_HIP(hipMemcpyAsync(out, ss.merge_out.p, total, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  return FQGPU_OK;
}
