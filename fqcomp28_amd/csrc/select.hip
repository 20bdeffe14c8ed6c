// The reads of a chunk that lies in HBM which pass a filter (include/fqgpu.h: fqgpu_chunk_filter, fqgpu_dblock_filter), or which
// are trimmed first and then judged by the filter (fqgpu_chunk_trim, fqgpu_dblock_trim), gathered on the device so that only
// the kept bytes come down.  Extension: nothing in the reference.  Both are ONE judge, one scan, one gather and one host
// driver; the flag TRIM is a template argument, so that the filter alone carries nothing of the trim: no walk, no window
// store, no window mask, ten counters instead of fourteen.
//
// k_select_judge -- one pass over the lines the criteria need, by the chunk's device record table.  A wave takes 64
// consecutive records: their table entries with ONE load, lane = record.  The bytes are then read by parts of the wave: eight
// lanes to a record, eight records at a time, every lane an ALIGNED 16-byte word of a line per load (a line starts anywhere:
// the bytes in front of it and behind it are masked off, and the 64 spare bytes every raw block has behind its chunk let the
// chunk's last word be read whole), the words of the NEXT eight records on their way while those of the eight in hand are
// judged -- so a wait is for the lines of eight records, not for one, and the kernel holds no LDS table, so a CU holds many
// such waves.  The words are judged four bytes at a time (a byte >= 128 is refused first, which makes the packed compares
// exact): the sum of a line's quality bytes by v_sad_u8, "N", "not a base", "Phred below the level", "not a quality" by
// packed compares and a population count.  A record's eight lanes add up by shuffles and hand the counts back to the
// record's own lane, which gives the verdict, the kept size (the canonical length of what is left, or 0), the start of the
// record's header line, k_crc_check's verdict on the '+' lines and -- by one ballot per wave -- the keep bits.  The sequence
// lines are not loaded at all when max_n is off, the quality lines not when min_mean_q, low_q and the quality trim are off: a
// length-only filter reads the record table alone.  THE BYTES OF A LINE THAT IS NOT LOADED ARE NOT JUDGED: a sequence byte
// outside ACGTN / a quality byte outside 33 .. 96 refuses the chunk only when a criterion reads that line; a line that is read
// is judged over all its bytes, the cut ones too.  The report's counters are summed over the wave by shuffles, over the
// workgroup in LDS, and reach global memory as one 64-bit atomic per counter and workgroup.
//
// TRIM puts a window in front of the verdict.  The fixed cuts leave the interval [f, L - t).  The two running-sum walks of the
// quality trim (s += cutoff - Phred; stop at s < 0; the cut is behind the FIRST place of the largest s > 0) are done by all
// eight lanes at once: a lane sums up its word, in walk order, as a PIECE -- total, smallest prefix, largest prefix and the
// first place of that --, a prefix sum over the pieces gives every piece the sum the walk enters it with, the walk stops in the
// first piece with entering + smallest prefix < 0, every piece in front of that one is valid as a whole (its candidate:
// entering + largest prefix; equal candidates: the earlier piece), and only the piece the walk stops in is walked byte by
// byte.  A request's two words are taken in walk order, and a word no record of the wave still needs is left out.  A
// candidate travels as ONE 64-bit key -- the sum above, the place below, so that the larger key is the better AND the earlier
// one -- and is reduced by shuffles.  With the window known, N, the Phred sum and the low count are taken over the window from
// the words that are still in the registers, with a second set of byte masks.  A read whose line fits one request of its eight
// lanes (256 bytes) loads no word twice; a longer one walks the requests forwards for the front walk, backwards for the tail
// walk and forwards again for the counts, loading as it goes: a correctness path.  Without TRIM the window is the line, and a
// long read is one loop over the rest of its requests.
//
// THE FRAME OF THE LINE READERS -- what the paragraph above says of the judge's way to the bytes holds for the three kernels
// that read lines, k_adapter_find (both forms), k_tail_find and k_select_judge, and exists once: sel_wave is the wave's view
// of its 64 records (one table load, lane = record, "a record of this chunk" by sel_line_inside of sel_words.h); sel_rounds
// owns the eight rounds -- in round k group g's eight lanes read record 8 k + g, sel_fetch for round k + 1 issued in front
// of the kernel's body for round k --; sel_round_steps gives the requests a round takes when a line among its eight is longer
// than one request of 256 bytes, uniform over the wave; sel_planes turns a request's words into bit planes; sel_in_round and
// sel_hand_back take a result back to the record's own lane.  What a kernel does with the words is its own: a lambda it
// hands to sel_rounds.  (One exception, by measurement: the PROBE form of k_adapter_find has the loop of sel_rounds and its
// body in line; it uses the other pieces.)
//
// k_adapter_find -- in front of the judge when an adapter is given (fqgpu_chunk_clip, fqgpu_dblock_clip): one pass over the
// sequence lines on that frame, the search itself bit-parallel -- a word's bases as four bit planes, every
// place a shift, four ANDs with the adapter's planes and a population count.  It leaves one uint16_t per record, the clip
// place, which the judge (its flag CLIP) takes for the read's length in the trim's steps; the gather sees only windows.
// Its template flag PROBE makes it the adapter-content pass (fqgpu_chunk_probe, fqgpu_dblock_probe): the same search with up
// to sixteen adapters over the same planes, the hits counted by read position in LDS; no judge and no gather behind it.
//
// fq_scan_u32_to_u64 -- the kept sizes become the records' places in the output.
//
// k_select_gather -- the compacting copy, driven by the DESTINATION: a workgroup owns an aligned tile of the output, every
// lane aligned 16-byte words of it, every store a full aligned 16-byte store.  The workgroup finds the records of its tile's
// first and last byte (two uniform binary searches in the offsets).  Cuts and drops only take bytes away, so
// hstart[r] - koff[r] never gets smaller with r: when the chunk's '+' lines are bare (there a whole record's canonical bytes
// are one span of the chunk) and both records have the same shift and are whole, every record between them is kept whole and
// the tile is ONE shifted copy, 16 bytes a lane from wherever the source lies -- every tile of a call that keeps everything,
// most tiles behind long runs.  Otherwise every lane searches among the tile's records.  Without TRIM every kept record is
// whole: a word inside one run is copied the same way and a word across a seam between two runs is put together byte by byte
// from the runs' shifts alone.  With TRIM a kept record is FIVE pieces: its header line, the window of the sequence line, the
// literal "\n+\n", the window of the quality line, the literal '\n'; a word inside a run of whole records or inside one piece is
// one unaligned 16-byte load, a word across a seam is put together byte by byte; the '+' line is always the literal there, so
// that form serves chunks with text behind a '+' as well.  k_select_gather_records is the filter's form for such chunks (one
// wave per kept record, as k_crc_canon_write): a correctness path, kept because the five-piece form takes twice its time
// there.
//
// A record RANGE, a MARK and a LIMIT (fqgpu_chunk_select_marked, fqgpu_chunk_select_limited: a paired restore's selection).
// The range is these kernels over a view's recs and n_recs (FqChunkView, fqgpu_internal.h) -- its `prev` gives the range's
// first record its header line --, every scratch array and every output then the range's.  k_select_mark, between the judge
// and the scan, ANDs the caller's mark into the keep words, takes a record that flips out of the kept sizes and the kept
// counters and counts it in report word 20.  k_select_limit, behind k_adapter_find, takes the minimum of a caller's
// per-record limit into the clip places, so that the judge's clip forms serve a limit unchanged.  The calls on two chunks,
// which find such marks and limits, are pair.hip.
//
// All global stores are ordinary vector stores from plain C++.
#include "fqgpu_internal.h"
#include "sel_words.h"

#include <string.h>

namespace {

constexpr unsigned SEL_THREADS = 256;        // threads of a judge workgroup: four waves
constexpr unsigned SEL_WAVE_RECORDS = 64;    // consecutive records a wave takes: lane = record
constexpr unsigned SEL_GROUP_LANES = 8;      // lanes that read one record's lines together
constexpr unsigned SEL_UNROLL = 2;           // 16-byte words of a line a lane has in flight
constexpr unsigned SEL_GATHER_THREADS = 256; // threads of a gather workgroup
constexpr unsigned SEL_GATHER_WORDS = 4;     // 16-byte words of the output a gather lane writes
constexpr unsigned SEL_ROUND_RECORDS = SEL_WAVE_RECORDS / SEL_GROUP_LANES;  // records a wave reads at a time
constexpr unsigned SEL_STEP_BYTES = SEL_GROUP_LANES * 16 * SEL_UNROLL;      // bytes of a line a record's lanes ask for in one go
constexpr unsigned SEL_TILE_BYTES = SEL_GATHER_THREADS * 16 * SEL_GATHER_WORDS;  // output bytes of a gather workgroup
static_assert(SEL_WAVE_RECORDS == 64 && SEL_GROUP_LANES == 8 && SEL_ROUND_RECORDS == 8 && SEL_UNROLL == 2, "a wave's records sit in its lanes");
static_assert(SEL_GROUP_LANES == SW_GROUP_LANES, "pair.hip groups a record's lanes as the judge does");

constexpr unsigned R_KEPT = 1, R_BASES_IN = 2, R_BASES_KEPT = 3, R_BYTES_KEPT = 4, R_DROPPED = 5, R_TRIMMED = 10, R_CUT_FRONT = 11,
                   R_CUT_TAIL = 12, R_EMPTIED = 13;
template <bool TRIM> constexpr unsigned R_COUNTERS = TRIM ? 14 : 10;  // the words a judge counts
constexpr unsigned R_WITH_ADAPTER = 14, R_CUT_ADAPTER = 15, R_COUNTERS_CLIP = 16;  // ... behind an adapter search
constexpr unsigned R_WITH_POLY = 16, R_CUT_POLY = 17, R_WINDOW_CUT = 18, R_CUT_WINDOW = 19, R_COUNTERS_TAIL = 20;  // ... behind the tail trims

// ---- the frame of the line readers (the head of this file)

// the first of the 64 records of this lane's wave
__device__ __forceinline__ unsigned long long sel_wave_first() {
  return ((unsigned long long)blockIdx.x * (SEL_THREADS / 64) + (threadIdx.x >> 6)) * SEL_WAVE_RECORDS;
}

// a wave's 64 records, lane = record
struct SelWave {
  unsigned long long r0, r;  // the wave's first record, this lane's
  bool have, ok;             // r is in the table; ... and a record of this chunk
  fqgpu_rec mine;            // its entry (zeros behind the table's end)
  unsigned read_len;         // its length; 0 where !ok: nothing of a record outside the chunk is read, the judge refuses it
};
// QUAL: the quality line has to lie inside the chunk as well (a reader of the sequence line alone does not ask)
template <bool QUAL>
__device__ __forceinline__ SelWave sel_wave(const fqgpu_rec *__restrict__ recs, unsigned n_recs, unsigned long long raw_len, unsigned lane) {
  SelWave wave;
  wave.r0 = sel_wave_first();
  wave.r = wave.r0 + lane;
  wave.have = wave.r < n_recs;
  wave.mine = {0u, 0u, 0u};
  if (wave.have) wave.mine = recs[wave.r];
  wave.ok = wave.have && sel_line_inside(wave.mine.seq_off, wave.mine.len, raw_len) && (!QUAL || sel_line_inside(wave.mine.qual_off, wave.mine.len, raw_len));
  wave.read_len = wave.ok ? wave.mine.len : 0u;
  return wave;
}

// the requests the lines of this lane's record take: seq, qual: the lines that are read
__device__ __forceinline__ unsigned sel_record_steps(const SelWave &wave, bool seq, bool qual) {
  const unsigned span = max(seq ? (wave.mine.seq_off & 15u) + wave.read_len : 0u, qual ? (wave.mine.qual_off & 15u) + wave.read_len : 0u);
  return max((span + SEL_STEP_BYTES - 1) / SEL_STEP_BYTES, 1u);
}

// "this lane's record is read in round k", and what the record's own lane takes back from its group: lane 8 k + g takes what
// group g's lanes hold
__device__ __forceinline__ bool sel_in_round(unsigned lane, unsigned k) { return lane / SEL_ROUND_RECORDS == k; }
__device__ __forceinline__ unsigned sel_hand_back(unsigned x, unsigned lane) {
  return __shfl(x, (lane & (SEL_ROUND_RECORDS - 1)) * SEL_GROUP_LANES);
}

// The requests round k takes: those of the longest line among its eight records, my_steps being sel_record_steps of the
// lane's own.  The same in every lane of the wave, so that the eight lanes of a record stay together through the shuffles of
// a walk or a search while the long-read steps -- a correctness path -- are taken.
__device__ __forceinline__ unsigned sel_round_steps(unsigned my_steps, unsigned lane, unsigned k) {
  unsigned steps = 1;
  if (__any(my_steps > 1 && sel_in_round(lane, k))) {  // (uniform) a long read among the eight
    steps = sel_in_round(lane, k) ? my_steps : 1u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) steps = max(steps, (unsigned)__shfl_xor(steps, d));
    steps = fq_uniform(steps);
  }
  return steps;
}

// the fixed cuts of a read of len symbols leave [sel_cut_lo, sel_cut_hi)
__device__ __forceinline__ unsigned sel_cut_lo(const fqgpu_trim &t, unsigned len) { return min(t.cut_front, len); }
__device__ __forceinline__ unsigned sel_cut_hi(const fqgpu_trim &t, unsigned len) { return len - min(t.cut_tail, len - min(t.cut_front, len)); }

// what a lane keeps of the record its group reads: the lines' places and the first words of the lines that are read
struct SelStage {
  unsigned seq_off, qual_off, len;  // len 0: nothing to read (behind the table's end, or not a record of this chunk)
  uint4 s[SEL_UNROLL], q[SEL_UNROLL];
};

// the lane's words of one line: word k of the lane is the aligned word 8 k + sub of the line, counted from the word that
// holds the line's first byte; p0: bytes of the line (from that word on) in front of this request.  Every raw block has 64
// spare bytes behind its chunk (api.hip), so the word that holds the chunk's last byte can be read whole; what it holds behind
// the chunk is masked off by the callers.
__device__ __forceinline__ void sel_load_line(uint4 (&v)[SEL_UNROLL], const uint8_t *__restrict__ raw, unsigned off, unsigned len, unsigned p0, unsigned sub) {
  const unsigned lead = off & 15u, span = len ? lead + len : 0u;
  const uint8_t *const line = raw + (off - lead);
#pragma unroll
  for (unsigned k = 0; k < SEL_UNROLL; k++) {
    const unsigned rel = p0 + 16u * (SEL_GROUP_LANES * k + sub);
    v[k] = rel < span ? *reinterpret_cast<const uint4 *>(line + rel) : make_uint4(0, 0, 0, 0);
  }
}

// record j of the wave's 64, for the lanes of the group that reads it: its places, and the first request of the lines asked
// for (seq, qual; a line that is not asked for is not loaded, and one that no caller asks for costs no register)
__device__ __forceinline__ void sel_fetch(SelStage &st, const uint8_t *__restrict__ raw, const SelWave &wave, unsigned j, unsigned sub, bool seq, bool qual) {
  st.seq_off = __shfl(wave.mine.seq_off, j);
  st.qual_off = __shfl(wave.mine.qual_off, j);
  st.len = __shfl(wave.read_len, j);
  if (seq) sel_load_line(st.s, raw, st.seq_off, st.len, 0, sub);
  if (qual) sel_load_line(st.q, raw, st.qual_off, st.len, 0, sub);
}

// The eight rounds of a wave: in round k group g reads record j = 8 k + g, and body(stage, k, j) works on it with the words
// of round k + 1 on their way -- the fetch stands in front of the body, which is the latency hiding.
template <bool COPY_LAST, class Body>
__device__ __forceinline__ void sel_rounds(const uint8_t *__restrict__ raw, const SelWave &wave, unsigned lane, bool seq, bool qual, const Body &body) {
  const unsigned sub = lane & (SEL_GROUP_LANES - 1), group = lane / SEL_GROUP_LANES;
  SelStage cur, nxt;
  sel_fetch(cur, raw, wave, group, sub, seq, qual);
#pragma unroll 1
  for (unsigned k = 0; k < SEL_GROUP_LANES; k++) {
    if (k + 1 < SEL_GROUP_LANES) sel_fetch(nxt, raw, wave, SEL_ROUND_RECORDS * (k + 1) + group, sub, seq, qual);
    body(cur, k, SEL_ROUND_RECORDS * k + group);
    if (COPY_LAST || k + 1 < SEL_GROUP_LANES) cur = nxt;
  }
}

struct SelCounts {
  unsigned n, qsum, low;  // over the WINDOW: N of the sequence line; sum of the quality BYTES; quality bytes below the level
  bool bad;               // over the whole line
};

// one word of a sequence line: [first, last) are its bytes inside the line, [wf, wl) those inside the window (TRIM; without,
// the window is the line and is not looked at)
template <bool TRIM>
__device__ __forceinline__ void sel_judge_seq(SelCounts &c, const uint4 v, int first, int last, int wf, int wl) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned m = sw_mask(first - 4 * i, last - 4 * i), x = w[i] & m;
    if (x & SW_H) c.bad = true;
    const unsigned y = x & ~SW_H, is_n = sw_eq(y, 'N');
    const unsigned base = sw_eq(y, 'A') | sw_eq(y, 'C') | sw_eq(y, 'G') | sw_eq(y, 'T') | is_n;
    if ((base & m) != (SW_H & m)) c.bad = true;
    unsigned wm = m;
    if constexpr (TRIM) wm = sw_mask(wf - 4 * i, wl - 4 * i);
    c.n += __popc(is_n & wm);
  }
}

// one word of a quality line; level: the first byte value that is not "low" (33 + low_q)
template <bool TRIM>
__device__ __forceinline__ void sel_judge_qual(SelCounts &c, const uint4 v, int first, int last, int wf, int wl, unsigned level) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned m = sw_mask(first - 4 * i, last - 4 * i), x = w[i] & m;
    if (x & SW_H) c.bad = true;
    const unsigned y = x & ~SW_H;
    if ((sw_ge(y, 33u) & m) != (SW_H & m) || (sw_ge(y, 97u) & m)) c.bad = true;
    unsigned wm = m;
    if constexpr (TRIM) wm = sw_mask(wf - 4 * i, wl - 4 * i);
    c.qsum = __builtin_amdgcn_sad_u8(w[i] & wm, 0u, c.qsum);
    c.low += __popc(~sw_ge(y, level) & SW_H & wm);
  }
}

// ---- the running-sum walk.  A candidate is one key: the sum in the bits from 20 up (at most 64 x 65535 < 2^22), the place
// below, turned so that of two keys with one sum the place the walk reaches FIRST is the larger.  0: no candidate.
constexpr unsigned SEL_PLACE = 0xFFFFFu;
template <bool FWD>
__device__ __forceinline__ unsigned long long sel_key(int sum, int place) {
  return ((unsigned long long)(unsigned)sum << 20) | (unsigned)(FWD ? (int)SEL_PLACE - place : place);
}

struct SelPiece {
  int tot, minp, maxp;  // of the prefixes in walk order (the empty prefix, 0, among them)
  int place;            // the cut the first largest prefix stands for (maxp > 0 only)
};

// The bytes `in` (a bit each) of a word as one piece of a walk; c: cutoff + 33, so that c - byte is the walk's increment;
// pos0: the place in the line of the word's byte 0.  The front walk (FWD) reads byte 0 first and a byte at place i stands for
// the cut "start = i + 1"; the tail walk reads byte 15 first and a byte at place i stands for "stop = i".
template <bool FWD>
__device__ __forceinline__ SelPiece sel_piece(const uint4 v, unsigned in, int c, int pos0) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  SelPiece p = {0, 0, 0, 0};
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
__device__ __forceinline__ unsigned long long sel_walk_piece(const uint4 v, unsigned in, int c, int pos0, int s, unsigned long long best) {
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
      best = sel_key<FWD>(s, pos0 + j + (FWD ? 1 : 0));
    }
  }
  return best;
}

// a walk on its way through a line; the same in the eight lanes of a record
struct SelWalk {
  int ent;                  // the sum it enters the next request with
  unsigned long long best;  // the best candidate so far
  bool stopped;
};

// One word of a request of a walk over the places [a, b) of a line: eight pieces, the word of lane sub at place pos0.  Every
// lane of the record's eight calls this together.
template <bool FWD>
__device__ __forceinline__ void sel_walk_word(SelWalk &wk, const uint4 v, int pos0, unsigned sub, int a, int b, int c) {
  const unsigned in = sel_bits(a - pos0, b - pos0);
  const SelPiece pc = sel_piece<FWD>(v, in, c, pos0);
  // the sum the walk enters the piece with: a prefix sum over the lanes, in walk order
  int inc = pc.tot;
#pragma unroll
  for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) {
    const int o = __shfl_up(inc, d, SEL_GROUP_LANES);
    if (sub >= d) inc += o;
  }
  const int sum = __shfl(inc, SEL_GROUP_LANES - 1, SEL_GROUP_LANES);
  const int e = wk.ent + (FWD ? inc - pc.tot : sum - inc);
  const unsigned ord = FWD ? sub : SEL_GROUP_LANES - 1 - sub;  // the piece's turn in the walk
  // the first piece the walk would stop in
  unsigned stop_at = e + pc.minp < 0 ? ord : SEL_GROUP_LANES;
#pragma unroll
  for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) stop_at = min(stop_at, (unsigned)__shfl_xor(stop_at, d, SEL_GROUP_LANES));
  // the pieces in front of it are valid as a whole
  unsigned long long key = pc.maxp > 0 && ord < stop_at ? sel_key<FWD>(e + pc.maxp, pc.place) : 0ull;
#pragma unroll
  for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) key = max(key, (unsigned long long)__shfl_xor(key, d, SEL_GROUP_LANES));
  const unsigned long long best = max(wk.best, key);
  // the piece it stops in, byte by byte, by the lane that holds it (every lane walks its word: no lane waits for less)
  const unsigned long long walked = sel_walk_piece<FWD>(v, in, c, pos0, e, best);
  const unsigned at = min(stop_at, SEL_GROUP_LANES - 1);
  const unsigned long long from_owner = __shfl(walked, FWD ? at : SEL_GROUP_LANES - 1 - at, SEL_GROUP_LANES);
  if (!wk.stopped) {
    wk.best = stop_at < SEL_GROUP_LANES ? from_owner : best;
    wk.stopped = stop_at < SEL_GROUP_LANES;
  }
  wk.ent += sum;
}

// One request (word 8 k + sub in lane sub, k = 0, 1) of a walk over the places [a, b) of a line whose first byte sits at byte
// `lead` of its first word: its words in walk order.  A word is left out when no record of the WAVE has anything for the walk
// in it -- the walk has stopped, or the word lies behind the interval; most walks stop in the first word they meet.
template <bool FWD>
__device__ __forceinline__ void sel_walk_step(SelWalk &wk, const uint4 (&v)[SEL_UNROLL], unsigned p0, unsigned sub, int lead, int a, int b, int c) {
#pragma unroll
  for (unsigned kk = 0; kk < SEL_UNROLL; kk++) {
    const unsigned k = FWD ? kk : SEL_UNROLL - 1 - kk;
    const int first = (int)(p0 + 16u * SEL_GROUP_LANES * k) - lead;  // the place of the eight words' first byte
    const bool idle = wk.stopped || (FWD ? first >= b : first + (int)(16u * SEL_GROUP_LANES) <= a);  // (the same in a record's lanes)
    if (__all(idle)) continue;  // (uniform)
    sel_walk_word<FWD>(wk, v[k], first + (int)(16u * sub), sub, a, b, c);
  }
}

// ---- the adapter search.  A word's sixteen bases are four bit planes of sixteen bits (bit j: byte j of the word is that
// base), two planes to a register: A below C, G below T.
struct ClipWord {
  unsigned ac, gt;
};

// The planes of one word; `in`: a bit for each byte inside the line, the others come out as "no base".  bad: a byte inside
// the line that is none of ACGTN.
__device__ __forceinline__ ClipWord clip_planes(const uint4 v, unsigned in, bool &bad) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned pa = 0, pc = 0, pg = 0, pt = 0, fine = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned y = w[i] & ~SW_H;
    const unsigned ea = sw_eq(y, 'A'), ec = sw_eq(y, 'C'), eg = sw_eq(y, 'G'), et = sw_eq(y, 'T');
    pa |= (ea * CLIP_GATHER) >> 28 << (4 * i);
    pc |= (ec * CLIP_GATHER) >> 28 << (4 * i);
    pg |= (eg * CLIP_GATHER) >> 28 << (4 * i);
    pt |= (et * CLIP_GATHER) >> 28 << (4 * i);
    // one of ACGTN, and below 128 (the compares see the low seven bits alone)
    fine |= (((ea | ec | eg | et | sw_eq(y, 'N')) & ~w[i]) * CLIP_GATHER) >> 28 << (4 * i);
  }
  if (~fine & in) bad = true;
  ClipWord r;
  r.ac = (pa & in) | (pc & in) << 16;
  r.gt = (pg & in) | (pt & in) << 16;
  return r;
}
// the planes of the lane's words v of the request at p0 of a record's sequence line; judge: the line is judged on the way
// (ACGTN) and bad told; without, another kernel has done that
__device__ __forceinline__ void sel_planes(ClipWord (&x)[SEL_UNROLL], const uint4 (&v)[SEL_UNROLL], const SelStage &st, unsigned p0, unsigned sub, bool judge,
                                           bool &bad) {
  const int lead = (int)(st.seq_off & 15u), span = st.len ? lead + (int)st.len : 0;
  bool b = bad;
#pragma unroll
  for (unsigned k = 0; k < SEL_UNROLL; k++) {
    const int rel = (int)(p0 + 16u * (SEL_GROUP_LANES * k + sub));
    x[k] = clip_planes(v[k], sel_bits(lead - rel, span - rel), b);
  }
  if (judge) bad = b;
}

// the adapter as the search takes it: its planes (bit j: A[j] is that base), its length and the two limits
struct ClipAdapter {
  unsigned long long a, c, g, t;
  unsigned m, min_overlap, keep_pct;  // keep_pct: 100 - max_err_pct
};

// The sixteen places of one word: own, and the four words behind it (n[0] the next one), give the 80 bases a place can look
// at; place0: the place in the line of the word's byte 0 (negative in front of the line), len: the line's length.  ->  a bit
// for every place that is a hit.  The read's planes are zero outside the line and the adapter's behind its end, so the
// population count IS the number of matches among the ov = min(m, len - p) bases compared.
__device__ __forceinline__ unsigned clip_word_hits(const ClipWord own, const ClipWord (&n)[4], const ClipAdapter &ad, bool wide, int place0, int len) {
  // per plane three registers: the bases 0 .. 31, 32 .. 63, 64 .. 79 from the word's first
  const unsigned a0 = __builtin_amdgcn_perm(n[0].ac, own.ac, 0x05040100u), c0 = __builtin_amdgcn_perm(n[0].ac, own.ac, 0x07060302u);
  const unsigned g0 = __builtin_amdgcn_perm(n[0].gt, own.gt, 0x05040100u), t0 = __builtin_amdgcn_perm(n[0].gt, own.gt, 0x07060302u);
  const unsigned a1 = __builtin_amdgcn_perm(n[2].ac, n[1].ac, 0x05040100u), c1 = __builtin_amdgcn_perm(n[2].ac, n[1].ac, 0x07060302u);
  const unsigned g1 = __builtin_amdgcn_perm(n[2].gt, n[1].gt, 0x05040100u), t1 = __builtin_amdgcn_perm(n[2].gt, n[1].gt, 0x07060302u);
  const unsigned a2 = n[3].ac & 0xFFFFu, c2 = n[3].ac >> 16, g2 = n[3].gt & 0xFFFFu, t2 = n[3].gt >> 16;
  const unsigned al = (unsigned)ad.a, cl = (unsigned)ad.c, gl = (unsigned)ad.g, tl = (unsigned)ad.t;
  const unsigned ah = (unsigned)(ad.a >> 32), ch = (unsigned)(ad.c >> 32), gh = (unsigned)(ad.g >> 32), th = (unsigned)(ad.t >> 32);
  unsigned hits = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    unsigned eq = (__builtin_amdgcn_alignbit(a1, a0, j) & al) | (__builtin_amdgcn_alignbit(c1, c0, j) & cl) |
                  (__builtin_amdgcn_alignbit(g1, g0, j) & gl) | (__builtin_amdgcn_alignbit(t1, t0, j) & tl);
    int matches = __popc(eq);
    if (wide) {  // (uniform) an adapter of more than 32 bases
      eq = (__builtin_amdgcn_alignbit(a2, a1, j) & ah) | (__builtin_amdgcn_alignbit(c2, c1, j) & ch) |
           (__builtin_amdgcn_alignbit(g2, g1, j) & gh) | (__builtin_amdgcn_alignbit(t2, t1, j) & th);
      matches += __popc(eq);
    }
    const int p = place0 + j, ov = min((int)ad.m, len - p);
    // 100 * mism <= max_err_pct * ov, with mism = ov - matches
    const bool hit = p >= 0 && ov >= (int)ad.min_overlap && 100 * matches >= (int)ad.keep_pct * ov;
    hits |= hit ? 1u << j : 0u;
  }
  return hits;
}

// One request of a line (word 8 k + sub in lane sub, k = 0, 1) searched by the record's eight lanes together: x its planes,
// nx those of the NEXT request's first word (zero when the line ends in this one; more: some record of the wave has a next
// request), p0 and lead as in sel_load_line.  -> the smallest hit among the lane's places, or CLIP_NONE.  In two halves, so
// that the probe form does the first once for all its probes: what lies behind the lane's words, then the test.
constexpr unsigned CLIP_NONE = 0xFFFFFFFFu;
struct ClipBehind {
  ClipWord n0[4], n1[4];  // the four words behind each of the lane's two
};
__device__ __forceinline__ ClipBehind clip_behind(const ClipWord (&x)[SEL_UNROLL], const ClipWord nx, bool more, unsigned sub) {
  // from the lanes behind it, and past lane 7 from the next word of lane 0 on
  ClipBehind r;
#pragma unroll
  for (unsigned d = 1; d <= 4; d++) {
    const unsigned src = (sub + d) & (SEL_GROUP_LANES - 1);
    const bool wrap = sub + d >= SEL_GROUP_LANES;
    ClipWord b0, b1, b2 = {0u, 0u};
    b0.ac = __shfl(x[0].ac, src, SEL_GROUP_LANES);
    b0.gt = __shfl(x[0].gt, src, SEL_GROUP_LANES);
    b1.ac = __shfl(x[1].ac, src, SEL_GROUP_LANES);
    b1.gt = __shfl(x[1].gt, src, SEL_GROUP_LANES);
    if (more) {  // (uniform)
      b2.ac = __shfl(nx.ac, src, SEL_GROUP_LANES);
      b2.gt = __shfl(nx.gt, src, SEL_GROUP_LANES);
    }
    r.n0[d - 1] = wrap ? b1 : b0;
    r.n1[d - 1] = wrap ? b2 : b1;
  }
  return r;
}
__device__ __forceinline__ unsigned clip_test(const ClipWord (&x)[SEL_UNROLL], const ClipBehind &bh, const ClipAdapter &ad, bool wide, unsigned p0,
                                              unsigned sub, int lead, int len) {
  unsigned best = CLIP_NONE;
#pragma unroll
  for (unsigned kk = 0; kk < SEL_UNROLL; kk++) {
    const unsigned k = SEL_UNROLL - 1 - kk;  // (the later word first: the earlier one's hit replaces its)
    const int first = (int)(p0 + 16u * SEL_GROUP_LANES * k) - lead;  // the place of the eight words' first byte
    if (__all(first >= len)) continue;  // (uniform) no record of the wave has a base there
    const int place0 = first + (int)(16u * sub);
    const unsigned hits = clip_word_hits(x[k], k ? bh.n1 : bh.n0, ad, wide, place0, len);
    if (hits) best = (unsigned)(place0 + (int)__builtin_ctz(hits));
  }
  return best;
}
__device__ __forceinline__ unsigned clip_request(const ClipWord (&x)[SEL_UNROLL], const ClipWord nx, bool more, const ClipAdapter &ad, bool wide,
                                                 unsigned p0, unsigned sub, int lead, int len) {
  const ClipBehind bh = clip_behind(x, nx, more, sub);
  return clip_test(x, bh, ad, wide, p0, sub, lead, len);
}

// ---- adapter content (include/fqgpu.h, fqgpu_chunk_probe): the probe form's counts.  A workgroup sums in LDS, u32 -- it has
// 256 records of at most 65535 bases, so no cell can overflow --: the chunk's bases, four counters for each of the n + 1
// tables, and PROBE_WINDOW_ROWS rows of n + 1 cells with one more row that stands for row P when P lies beyond the window
// (stats.hip's layout of the same problem).  A hit between the window and P goes to global memory directly: correct, slow,
// rare.  At the end a non-zero word reaches the result as one 64-bit atomic.
constexpr unsigned PROBE_WINDOW_ROWS = 320;
constexpr unsigned PROBE_TABLE_HEAD = 8, PROBE_HEAD = 8;
constexpr unsigned PROBE_LDS_WORDS = 1 + 4 * (FQGPU_PROBES_MAX + 1) + (PROBE_WINDOW_ROWS + 1) * (FQGPU_PROBES_MAX + 1);
constexpr unsigned PW_WITH = 0, PW_BEHIND = 1, PW_WHOLE = 2, PW_EMPTIED = 3;
// the result's word of table t: its counter c / its row
__device__ __forceinline__ unsigned long long probe_word(unsigned P, unsigned t, unsigned c) {
  return PROBE_HEAD + (unsigned long long)t * (PROBE_TABLE_HEAD + P + 1ull) + c;
}
// a read of length len that table t (probe t of m bases; t == n: "any", m 0) cuts at a < len
__device__ __forceinline__ void probe_count(uint32_t *lds, unsigned long long *__restrict__ out, unsigned n, unsigned P, unsigned t, unsigned a,
                                            unsigned len, unsigned m) {
  const unsigned row = min(a, P);
  if (row < PROBE_WINDOW_ROWS || row == P) atomicAdd(&lds[1 + 4 * (n + 1) + min(row, PROBE_WINDOW_ROWS) * (n + 1) + t], 1u);
  else atomicAdd(&out[probe_word(P, t, PROBE_TABLE_HEAD + row)], 1ull);
  atomicAdd(&lds[1 + 4 * t + PW_WITH], 1u);
  atomicAdd(&lds[1 + 4 * t + PW_BEHIND], len - a);
  if (m && a + m <= len) atomicAdd(&lds[1 + 4 * t + PW_WHOLE], 1u);
  if (a == 0) atomicAdd(&lds[1 + 4 * t + PW_EMPTIED], 1u);
}

// what the two forms of k_adapter_find take: one adapter and the records' clip places / a probe set as the search takes it,
// the rows, the result tables and the records' places (nullptr: not wanted)
struct FindOne {
  unsigned long long plane_a, plane_c, plane_g, plane_t;
  unsigned m, min_overlap, max_err_pct;
  uint16_t *clip;
};
struct FindMany {
  ClipAdapter ad[FQGPU_PROBES_MAX];
  unsigned n, P;
  unsigned long long *out;
  uint16_t *places;
};
template <bool PROBE> struct FindArgs { using type = FindOne; };
template <> struct FindArgs<true> { using type = FindMany; };

// the probe form's LDS table, from a function of its own so that the plain form declares none
__device__ __forceinline__ uint32_t *probe_lds() {
  __shared__ uint32_t lds[PROBE_LDS_WORDS];
  return lds;
}

// clip[r] = the clip place of record r (include/fqgpu.h, step 0): the smallest place at which the adapter hits, or the
// read's length.  The frame of the line readers over the sequence lines, and nothing of the judge's arithmetic: a word
// becomes bit planes once, every place of it is then tested with shifts, ANDs and a population count, a lane taking the bases
// behind its word from its neighbours' planes by shuffles.  The line is judged over all its bytes on the way (ACGTN), so the
// judge behind this kernel does not read it again for that.  A read longer than one request walks the requests forwards with
// the next request's planes in hand.
// PROBE (fqgpu_chunk_probe) is the same search with many adapters: a request's planes and what lies behind the lane's words
// are built once, and a uniform loop over the probes -- their planes and limits scalar loads from the kernel's arguments,
// `wide` by the probe -- tests them.  A probe's first hit in a record is counted where it is found, by the first of the
// record's eight lanes (probe_count), and its place stored when places are asked for; `found` keeps a bit per probe so that
// a later request of a long read does not count it again.  There is no verdict to hand on, so a record outside the chunk
// or without symbols is refused here.  Without PROBE nothing of this is compiled: no loop, no LDS.
template <bool PROBE>
__global__ void __launch_bounds__(SEL_THREADS)
k_adapter_find(const uint8_t *__restrict__ raw, unsigned long long raw_len, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
               const typename FindArgs<PROBE>::type arg, SelectResult *__restrict__ res) {
  const unsigned lane = fq_lane(), sub = lane & (SEL_GROUP_LANES - 1);
  const SelWave wave = sel_wave<false>(recs, n_recs, raw_len, lane);
  const unsigned my_steps = sel_record_steps(wave, true, false);
  bool my_bad = PROBE && wave.have && !wave.ok;
  // the planes of the request behind request s of a long read (not loaded ahead), zero behind the line's last
  const auto next_planes = [&](ClipWord (&y)[SEL_UNROLL], const SelStage &cur, unsigned s, unsigned steps, bool &bad) {
    y[0] = y[1] = ClipWord{0u, 0u};
    if (s + 1 < steps) {  // (uniform)
      uint4 v[SEL_UNROLL];
      sel_load_line(v, raw, cur.seq_off, cur.len, (s + 1) * SEL_STEP_BYTES, sub);
      sel_planes(y, v, cur, (s + 1) * SEL_STEP_BYTES, sub, true, bad);
    }
  };
  if constexpr (PROBE) {
    // The probe form has sel_rounds' loop and its body in line: handed over as a lambda, the loop over the probes came out
    // 2.5 % slower with sixteen probes (The frame of the line readers).
    uint32_t *const lds = probe_lds();
    const unsigned n = arg.n, P = arg.P, used = 1 + (4 + PROBE_WINDOW_ROWS + 1) * (n + 1), group = lane / SEL_GROUP_LANES;
    for (unsigned i = threadIdx.x; i < used; i += SEL_THREADS) lds[i] = 0;
    __syncthreads();
    SelStage cur, nxt;
    sel_fetch(cur, raw, wave, group, sub, true, false);
#pragma unroll 1
    for (unsigned k = 0; k < SEL_GROUP_LANES; k++) {  // (as sel_rounds)
      if (k + 1 < SEL_GROUP_LANES) sel_fetch(nxt, raw, wave, SEL_ROUND_RECORDS * (k + 1) + group, sub, true, false);
      const unsigned steps = sel_round_steps(my_steps, lane, k);
      const int lead = (int)(cur.seq_off & 15u);
      const unsigned long long rec = wave.r0 + SEL_ROUND_RECORDS * k + group;  // the record of this lane's group
      bool bad = false;
      ClipWord x[SEL_UNROLL];
      sel_planes(x, cur.s, cur, 0, sub, true, bad);
      unsigned found = 0, any = CLIP_NONE;  // (the same in a record's eight lanes)
      for (unsigned s = 0; s < steps; s++) {
        ClipWord y[SEL_UNROLL];
        next_planes(y, cur, s, steps, bad);
        const ClipBehind bh = clip_behind(x, y[0], s + 1 < steps, sub);
#pragma unroll 1
        for (unsigned p = 0; p < n; p++) {  // (uniform)
          const ClipAdapter ad = arg.ad[p];
          unsigned got = clip_test(x, bh, ad, ad.m > 32u, s * SEL_STEP_BYTES, sub, lead, (int)cur.len);
#pragma unroll
          for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) got = min(got, (unsigned)__shfl_xor(got, d));
          if (got != CLIP_NONE && !(found >> p & 1u)) {  // the probe's first hit in this record
            found |= 1u << p;
            any = min(any, got);
            if (sub == 0) probe_count(lds, arg.out, n, P, p, got, cur.len, ad.m);
            if (sub == 1 && arg.places) arg.places[rec * n + p] = (uint16_t)got;
          }
        }
#pragma unroll
        for (unsigned i = 0; i < SEL_UNROLL; i++) x[i] = y[i];
      }
      if (cur.len) {  // (a record of this chunk)
        if (any != CLIP_NONE && sub == 0) probe_count(lds, arg.out, n, P, n, any, cur.len, 0u);
        if (arg.places)  // the probes without a hit: lane i of the record takes the probes i, i + 8
          for (unsigned p = sub; p < n; p += SEL_GROUP_LANES)
            if (!(found >> p & 1u)) arg.places[rec * n + p] = (uint16_t)cur.len;
      }
      if (__any(bad)) my_bad = true;  // (one flag for the chunk: whose byte it was does not matter)
      if (k + 1 < SEL_GROUP_LANES) cur = nxt;
    }
    unsigned bases = wave.read_len;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bases += __shfl_xor(bases, d);
    if (lane == 0 && bases) atomicAdd(&lds[0], bases);
    __syncthreads();
    // a word of the workgroup's sums -> its word of the result
    for (unsigned i = threadIdx.x; i < used; i += SEL_THREADS) {
      const unsigned v = lds[i];
      if (!v) continue;
      unsigned long long at = 1;  // n_bases
      if (i >= 1 + 4 * (n + 1)) {
        const unsigned c = i - (1 + 4 * (n + 1)), place = c / (n + 1), t = c % (n + 1);
        at = probe_word(P, t, PROBE_TABLE_HEAD + (place < PROBE_WINDOW_ROWS ? place : P));
      } else if (i >= 1) {
        at = probe_word(P, (i - 1) / 4, (i - 1) % 4);
      }
      atomicAdd(&arg.out[at], (unsigned long long)v);
    }
  } else {
    const ClipAdapter ad = {arg.plane_a, arg.plane_c, arg.plane_g, arg.plane_t, arg.m, arg.min_overlap, 100u - arg.max_err_pct};
    const bool wide = arg.m > 32u;
    unsigned my_clip = wave.read_len;
    sel_rounds<true>(raw, wave, lane, true, false, [&](const SelStage &cur, unsigned k, unsigned) {
      const unsigned steps = sel_round_steps(my_steps, lane, k);
      const int lead = (int)(cur.seq_off & 15u);
      bool bad = false;
      ClipWord x[SEL_UNROLL];
      sel_planes(x, cur.s, cur, 0, sub, true, bad);
      unsigned best = CLIP_NONE;
      for (unsigned s = 0; s < steps; s++) {
        ClipWord y[SEL_UNROLL];
        next_planes(y, cur, s, steps, bad);
        best = min(best, clip_request(x, y[0], s + 1 < steps, ad, wide, s * SEL_STEP_BYTES, sub, lead, (int)cur.len));
#pragma unroll
        for (unsigned i = 0; i < SEL_UNROLL; i++) x[i] = y[i];
      }
      // over the record's eight lanes: the smallest hit, and "a byte that cannot be judged" in the top bit
      unsigned got = min(best, cur.len) | (bad ? 0x80000000u : 0u);
#pragma unroll
      for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) {
        const unsigned o = __shfl_xor(got, d);
        got = min(got & 0x7FFFFFFFu, o & 0x7FFFFFFFu) | ((got | o) & 0x80000000u);
      }
      const unsigned mine_got = sel_hand_back(got, lane);
      if (sel_in_round(lane, k)) {
        my_clip = mine_got & 0x7FFFFFFFu;
        my_bad = mine_got >> 31;
      }
    });
    if (wave.have) arg.clip[wave.r] = (uint16_t)my_clip;
  }
  if (__any(my_bad) && lane == 0) res->bad = 1u;  // (every writer stores the same value)
}

// ---- the tail trims (include/fqgpu.h, steps 0b and 1b): both are "the first place where a prefix property fails", a
// min-reduction over places.
constexpr unsigned TAIL_NONE = 0xFFFFFFFFu;
struct TailSpec {
  unsigned bases, min_len, every, max_mism;  // the poly rule; bases 0: off
  unsigned W, level, thr;                    // the window rule in quality BYTES: level = Q + 33, thr = level * W; W 0: off
};

// a poly walk on its way down a line, per base X; the same in the eight lanes of a record
struct PolyWalk {
  unsigned ent[4];  // the mismatches the walk enters the next word with
  unsigned v[4];    // the first violation, a tail place i = a0 - place; TAIL_NONE: none so far
  unsigned t[4];    // the largest tail place in front of it at which X stands
};
__device__ __forceinline__ bool poly_done(const PolyWalk &pw, unsigned bases) {
  bool done = true;
#pragma unroll
  for (unsigned X = 0; X < 4; X++) done = done && (!((bases >> X) & 1u) || pw.v[X] != TAIL_NONE);
  return done;
}

// One word of the poly walk over s[0, a0): x the planes of lane sub's word, whose byte 0 stands at place pos0 of the line.
// The walk comes from the line's end, so the word is entered with the mismatches of the lanes behind it.  Every lane of the
// record's eight calls this together.  mism <= min(i / every, max_mism) is mism <= max_mism && mism * every <= i: no division.
__device__ __forceinline__ void tail_poly_word(PolyWalk &pw, const ClipWord x, int pos0, unsigned sub, int a0, const TailSpec &sp) {
  const unsigned in = sel_bits(-pos0, a0 - pos0);
  const unsigned plane[4] = {x.ac & 0xFFFFu, x.ac >> 16, x.gt & 0xFFFFu, x.gt >> 16};
  const int i0 = a0 - pos0;  // the tail place of byte j is i0 - j
#pragma unroll
  for (unsigned X = 0; X < 4; X++) {
    if (!((sp.bases >> X) & 1u)) continue;  // (uniform)
    const unsigned mm = in & ~plane[X];
    unsigned inc = __popc(mm);
#pragma unroll
    for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) {
      const unsigned o = __shfl_up(inc, d, SEL_GROUP_LANES);
      if (sub >= d) inc += o;
    }
    const unsigned sum = __shfl(inc, SEL_GROUP_LANES - 1, SEL_GROUP_LANES);
    const unsigned e = pw.ent[X] + (sum - inc);
    unsigned viol = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const unsigned c = e + __popc(mm >> j);  // mism(i0 - j): the mismatches from byte j to the line's end
      const bool over = c > sp.max_mism || (int)(c * sp.every) > i0 - j;
      viol |= over ? 1u << j : 0u;
    }
    viol &= in;
    // the first violation is the one at the highest byte
    unsigned first = viol ? (unsigned)(i0 - (31 - (int)__builtin_clz(viol))) : TAIL_NONE;
#pragma unroll
    for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) first = min(first, (unsigned)__shfl_xor(first, d, SEL_GROUP_LANES));
    if (pw.v[X] == TAIL_NONE) pw.v[X] = first;
    // the X in front of it: tail places i < v, bytes j > i0 - v
    const int lo = pw.v[X] == TAIL_NONE ? 0 : i0 - (int)pw.v[X] + 1;
    const unsigned hits = plane[X] & in & sel_bits(lo, 16);
    unsigned far = hits ? (unsigned)(i0 - (int)__builtin_ctz(hits)) : 0u;
#pragma unroll
    for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) far = max(far, (unsigned)__shfl_xor(far, d, SEL_GROUP_LANES));
    pw.t[X] = max(pw.t[X], far);
    pw.ent[X] += sum;
  }
}

// One request of the poly walk (word 8 k + sub in lane sub, k = 0, 1), the later word first.  A word is left out when no
// record of the WAVE has anything for the walk in it: it lies behind a0, or every walk has met its violation.
__device__ __forceinline__ void tail_poly_step(PolyWalk &pw, const ClipWord (&x)[SEL_UNROLL], unsigned p0, unsigned sub, int lead, int a0, const TailSpec &sp) {
#pragma unroll
  for (unsigned kk = 0; kk < SEL_UNROLL; kk++) {
    const unsigned k = SEL_UNROLL - 1 - kk;
    const int first = (int)(p0 + 16u * SEL_GROUP_LANES * k) - lead;
    const bool idle = first >= a0 || poly_done(pw, sp.bases);  // (the same in a record's lanes)
    if (__all(idle)) continue;                                 // (uniform)
    tail_poly_word(pw, x[k], first + (int)(16u * sub), sub, a0, sp);
  }
}

__device__ __forceinline__ uint4 tail_shfl4(const uint4 v, unsigned src) {
  return make_uint4(__shfl(v.x, src, SEL_GROUP_LANES), __shfl(v.y, src, SEL_GROUP_LANES), __shfl(v.z, src, SEL_GROUP_LANES),
                    __shfl(v.w, src, SEL_GROUP_LANES));
}
// w[i] for an i that is the same in every lane, without an indexed register file; an i of 12 or more gives 0.  (The
// window asks for w[12] when W >= 29: that word only feeds the bytes behind W + 15 -- the upper half of an alignbyte by 0
// for W = 32, the byte that would enter behind place 15 otherwise -- and no sum that is tested holds them.)
__device__ __forceinline__ unsigned tail_pick(const unsigned (&w)[12], unsigned i) {
  unsigned r = 0;
#pragma unroll
  for (unsigned k = 0; k < 12; k++) r = i == k ? w[k] : r;
  return r;
}

// The sixteen windows that start in one word of a quality line: own, and the two words behind it, give the 47 bytes they can
// look at; pos0: the place in the line of the word's byte 0.  The window at byte 0 is summed by v_sad_u8, every next one
// takes a byte in and lets one out.  -> a bit for every place p in [f, e - W] whose W bytes sum to less than thr.
__device__ __forceinline__ unsigned tail_window_word(const uint4 own, const uint4 n1, const uint4 n2, int pos0, int f, int e, const TailSpec &sp) {
  const unsigned w[12] = {own.x, own.y, own.z, own.w, n1.x, n1.y, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w};
  unsigned s = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) s = __builtin_amdgcn_sad_u8(w[i] & sw_mask(-4 * i, (int)sp.W - 4 * i), 0u, s);
  // the bytes W .. W + 15
  const unsigned wq = sp.W >> 2, wr = sp.W & 3u;
  unsigned t[5], in4[4];
#pragma unroll
  for (unsigned i = 0; i < 5; i++) t[i] = tail_pick(w, wq + i);
#pragma unroll
  for (unsigned i = 0; i < 4; i++) in4[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], wr);
  unsigned fails = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    fails |= s < sp.thr ? 1u << j : 0u;
    s += ((in4[j >> 2] >> (8 * (j & 3))) & 0xFFu) - ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
  }
  return fails & sel_bits(f - pos0, e - (int)sp.W + 1 - pos0);
}

// One request of a quality line (word 8 k + sub in lane sub, k = 0, 1) tested by the record's eight lanes together: y0 the
// NEXT request's first word (zero when the line ends in this one; more: some record of the wave has a next request), done: the
// record has its window already.  -> the smallest failing place among the lane's, or TAIL_NONE.
__device__ __forceinline__ unsigned tail_window_request(const uint4 (&x)[SEL_UNROLL], const uint4 y0, bool more, bool done, unsigned p0, unsigned sub,
                                                        int lead, int f, int e, const TailSpec &sp) {
  uint4 n0[2], n1[2];
#pragma unroll
  for (unsigned d = 1; d <= 2; d++) {
    const unsigned src = (sub + d) & (SEL_GROUP_LANES - 1);
    const bool wrap = sub + d >= SEL_GROUP_LANES;
    const uint4 b0 = tail_shfl4(x[0], src), b1 = tail_shfl4(x[1], src);
    uint4 b2 = make_uint4(0, 0, 0, 0);
    if (more) b2 = tail_shfl4(y0, src);  // (uniform)
    n0[d - 1] = wrap ? b1 : b0;
    n1[d - 1] = wrap ? b2 : b1;
  }
  unsigned best = TAIL_NONE;
#pragma unroll
  for (unsigned kk = 0; kk < SEL_UNROLL; kk++) {
    const unsigned k = SEL_UNROLL - 1 - kk;  // (the later word first: the earlier one's place replaces its)
    const int first = (int)(p0 + 16u * SEL_GROUP_LANES * k) - lead;
    // (uniform) no record of the wave has a window that starts there
    if (__all(done || first + (int)sp.W > e || first + (int)(16u * SEL_GROUP_LANES) <= f)) continue;
    const int pos0 = first + (int)(16u * sub);
    const unsigned fails = k ? tail_window_word(x[1], n1[0], n1[1], pos0, f, e, sp) : tail_window_word(x[0], n0[0], n0[1], pos0, f, e, sp);
    if (fails) best = (unsigned)(pos0 + (int)__builtin_ctz(fails));
  }
  return done ? TAIL_NONE : best;
}

// the first place in [from, to) of a word at which the quality byte is below the level, or TAIL_NONE
__device__ __forceinline__ unsigned tail_low_place(const uint4 v, int pos0, int from, int to, unsigned level) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned low = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) low |= ((~sw_ge(w[i] & ~SW_H, level) & SW_H) * CLIP_GATHER) >> 28 << (4 * i);
  low &= sel_bits(from - pos0, to - pos0);
  return low ? (unsigned)(pos0 + (int)__builtin_ctz(low)) : TAIL_NONE;
}

// places[r] = a0, a1, e, e2 of record r (include/fqgpu.h, steps 0 to 1b): the clip place (clip[r] behind k_adapter_find, else
// the read's length), the place in front of the poly-X tail, the end the fixed cuts leave and the place of the window cut.
// The frame of the line readers over both lines.  Poly: a word's planes (sel_planes, which judges ACGTN on the way -- left
// to k_adapter_find where that has run), per base X the mismatches counted in tail order, a prefix sum over the record's eight
// lanes for the count a word is entered with, sixteen places tested per lane, the first violation a min-reduction and the
// largest X place in front of it a max-reduction by shuffles.  Window: a lane takes the bytes behind its word from its
// neighbours by shuffles, forms its sixteen window sums, the first failing window is a min-reduction and e2 the first low
// byte from there.  A read longer than one request walks the requests backwards for the poly tail and forwards for the
// window, every lane of the wave the same number of steps: a correctness path.  A line that is read here is judged over all
// its bytes.
__global__ void __launch_bounds__(SEL_THREADS)
k_tail_find(const uint8_t *__restrict__ raw, unsigned long long raw_len, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
            const fqgpu_tail x, const fqgpu_trim t, const uint16_t *__restrict__ clip, uint2 *__restrict__ places,
            SelectResult *__restrict__ res) {
  const unsigned lane = fq_lane(), sub = lane & (SEL_GROUP_LANES - 1);
  const TailSpec sp = {x.poly_bases, x.poly_min_len, x.poly_every, x.poly_max_mism, x.window_len, x.window_q + 33u, (x.window_q + 33u) * x.window_len};
  const bool poly = sp.bases != 0, window = sp.W != 0, judge_seq = clip == nullptr;
  const SelWave wave = sel_wave<true>(recs, n_recs, raw_len, lane);
  unsigned my_a0 = wave.read_len;
  if (clip != nullptr && wave.ok) my_a0 = min((unsigned)clip[wave.r], wave.read_len);
  const unsigned my_steps = sel_record_steps(wave, poly, window);

  unsigned my_a1 = my_a0, my_e2 = sel_cut_hi(t, my_a0);  // (what holds when no line is read)
  bool my_bad = false;
  if (poly || window) {  // (uniform)
    // the lane's words of the request at p0 of the quality line, judged: 33 .. 96
    const auto judge_qual = [&](const uint4 (&v)[SEL_UNROLL], const SelStage &st, unsigned p0, bool &bad) {
      const int lead = (int)(st.qual_off & 15u), span = st.len ? lead + (int)st.len : 0;
      SelCounts c = {0u, 0u, 0u, false};
#pragma unroll
      for (unsigned k = 0; k < SEL_UNROLL; k++) {
        const int rel = (int)(p0 + 16u * (SEL_GROUP_LANES * k + sub));
        if (rel >= span) continue;
        sel_judge_qual<false>(c, v[k], max(lead - rel, 0), min(span - rel, 16), 0, 0, sp.level);
      }
      bad = bad || c.bad;
    };
    sel_rounds<false>(raw, wave, lane, poly, window, [&](const SelStage &cur, unsigned k, unsigned j) {
      const unsigned a0 = __shfl(my_a0, j);
      const unsigned steps = sel_round_steps(my_steps, lane, k);
      bool bad = false;
      unsigned a1 = a0;
      if (poly) {  // (uniform) from the line's last request down
        PolyWalk pw = {{0u, 0u, 0u, 0u}, {TAIL_NONE, TAIL_NONE, TAIL_NONE, TAIL_NONE}, {0u, 0u, 0u, 0u}};
        const int lead = (int)(cur.seq_off & 15u);
        ClipWord y[SEL_UNROLL];
        for (unsigned s = steps - 1; s >= 1; s--) {  // a long read: not loaded ahead
          uint4 v[SEL_UNROLL];
          sel_load_line(v, raw, cur.seq_off, cur.len, s * SEL_STEP_BYTES, sub);
          sel_planes(y, v, cur, s * SEL_STEP_BYTES, sub, judge_seq, bad);
          tail_poly_step(pw, y, s * SEL_STEP_BYTES, sub, lead, (int)a0, sp);
        }
        sel_planes(y, cur.s, cur, 0, sub, judge_seq, bad);
        tail_poly_step(pw, y, 0, sub, lead, (int)a0, sp);
        unsigned tl = 0;
#pragma unroll
        for (unsigned X = 0; X < 4; X++)
          if ((sp.bases >> X) & 1u) tl = max(tl, pw.t[X] >= sp.min_len ? pw.t[X] : 0u);
        a1 = a0 - tl;
      }
      const unsigned f = sel_cut_lo(t, a1), e = sel_cut_hi(t, a1);
      unsigned e2 = e;
      if (window) {  // (uniform) from the line's first request up
        const int lead = (int)(cur.qual_off & 15u);
        uint4 q[SEL_UNROLL];
#pragma unroll
        for (unsigned i = 0; i < SEL_UNROLL; i++) q[i] = cur.q[i];
        unsigned at = TAIL_NONE;  // the first failing window
        for (unsigned s = 0; s < steps; s++) {
          uint4 y[SEL_UNROLL] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
          if (s + 1 < steps) sel_load_line(y, raw, cur.qual_off, cur.len, (s + 1) * SEL_STEP_BYTES, sub);  // (uniform) a long read
          judge_qual(q, cur, s * SEL_STEP_BYTES, bad);
          unsigned got = tail_window_request(q, y[0], s + 1 < steps, at != TAIL_NONE, s * SEL_STEP_BYTES, sub, lead, (int)f, (int)e, sp);
#pragma unroll
          for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) got = min(got, (unsigned)__shfl_xor(got, d));
          const bool fresh = at == TAIL_NONE && got != TAIL_NONE;  // (the same in a record's lanes)
          if (__any(fresh)) {  // (uniform) the first low byte from there: in this request, or in the next one's first words
            const int from = fresh ? (int)got : (int)e, rel0 = (int)(s * SEL_STEP_BYTES + 16u * sub) - lead;
            unsigned low = tail_low_place(q[0], rel0, from, (int)e, sp.level);
            low = min(low, tail_low_place(q[1], rel0 + (int)(16u * SEL_GROUP_LANES), from, (int)e, sp.level));
            low = min(low, tail_low_place(y[0], rel0 + (int)SEL_STEP_BYTES, from, (int)e, sp.level));
#pragma unroll
            for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) low = min(low, (unsigned)__shfl_xor(low, d));
            if (fresh) {
              at = got;
              e2 = min(low, e);
            }
          }
#pragma unroll
          for (unsigned i = 0; i < SEL_UNROLL; i++) q[i] = y[i];
        }
      }
      // over the record's eight lanes: "a byte that cannot be judged"; then back to the record's own lane
      unsigned got = a1 | e2 << 16, flag = bad;
#pragma unroll
      for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) flag |= __shfl_xor(flag, d);
      const unsigned mine_got = sel_hand_back(got, lane), mine_flag = sel_hand_back(flag, lane);
      if (sel_in_round(lane, k)) {
        my_a1 = mine_got & 0xFFFFu;
        my_e2 = mine_got >> 16;
        my_bad = mine_flag != 0u;
      }
    });
  }
  if (wave.have) places[wave.r] = make_uint2(my_a0 | my_a1 << 16, sel_cut_hi(t, my_a1) | my_e2 << 16);
  if (__any(my_bad) && lane == 0) res->bad = 1u;  // (every writer stores the same value)
}

// TRIM: the reads are trimmed by t, the windows go to win; without, t and win are not looked at.  STEP0 (with TRIM): what
// stands in front of the trim's steps.  SEL_CLIP: clip[r] stands for the read's length in the trim's steps 1 to 4
// (k_adapter_find has written it, and has judged the sequence line).  prev != 0: recs is not the front of the chunk's table
// (fqgpu_chunk_select_marked's range) and recs[-1] is the record in front of its first.  SEL_TAIL: k_tail_find has left a0, a1, e, e2 in
// places[r]; the walks run over [min(cut_front, e2), e2) -- which is [f, e2), since f = min(cut_front, a1) and
// f <= e2 <= a1 -- and cut_tail, which is in e already, is not applied again.
constexpr unsigned SEL_PLAIN = 0, SEL_CLIP = 1, SEL_TAIL = 2;
template <bool TRIM, unsigned STEP0 = SEL_PLAIN>
__global__ void __launch_bounds__(SEL_THREADS)
k_select_judge(const uint8_t *__restrict__ raw, unsigned long long raw_len, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
               const fqgpu_trim t, const fqgpu_filter f, uint32_t *__restrict__ ksize, uint32_t *__restrict__ hstart,
               uint32_t *__restrict__ win, unsigned long long *__restrict__ keep, SelectResult *__restrict__ res,
               const uint16_t *__restrict__ clip, const uint2 *__restrict__ places, const unsigned prev) {
  static_assert(TRIM || STEP0 == SEL_PLAIN, "a clip and a tail trim stand in front of a trim's steps");
  static_assert(STEP0 <= SEL_TAIL, "plain, clip or tail");
  constexpr bool CLIP = STEP0 != SEL_PLAIN;  // the trim's steps see another length than the read's
  constexpr unsigned NC = STEP0 == SEL_TAIL ? R_COUNTERS_TAIL : CLIP ? R_COUNTERS_CLIP : R_COUNTERS<TRIM>;
  __shared__ unsigned wg[NC];
  if (threadIdx.x < NC) wg[threadIdx.x] = 0;
  __syncthreads();
  const unsigned lane = fq_lane(), sub = lane & (SEL_GROUP_LANES - 1);
  const bool walk_f = TRIM && t.q_front != 0, walk_t = TRIM && t.q_tail != 0;
  const bool need_seq = f.max_n != FQGPU_FILTER_NONE, need_qual = walk_f || walk_t || f.min_mean_q != 0 || f.low_q != 0;
  const unsigned level = 33u + f.low_q;
  const SelWave wave = sel_wave<true>(recs, n_recs, raw_len, lane);
  const unsigned long long r0 = wave.r0, r = wave.r;
  const bool have = wave.have, ok = wave.ok;
  const fqgpu_rec mine = wave.mine;
  const unsigned read_len = wave.read_len;
  // the start of the record's header line: behind the record in front (its entry sits in the lane in front; prev: the table
  // is a range of a chunk's and its first record has one in front of it as well)
  unsigned h0 = __shfl_up(mine.qual_off + mine.len + 1u, 1);
  if (lane == 0) h0 = have && (r || prev) ? recs[(long long)r - 1].qual_off + recs[(long long)r - 1].len + 1u : 0u;
  bool bad = have && !ok;

  // the window the two walks' results leave
  const auto window = [&](unsigned start, unsigned stop) {  // -> start | n << 16
    if (start >= stop) return 0u;
    return start | min(stop - start, t.crop) << 16;
  };

  unsigned n_count = 0, q_bytes = 0, low_count = 0;
  unsigned my_win = 0;
  unsigned eff_len = read_len;  // the length the trim sees: the clip place behind an adapter search
  uint2 my_places = make_uint2(0u, 0u);  // SEL_TAIL: a0 | a1 << 16, e | e2 << 16
  if constexpr (STEP0 == SEL_CLIP) eff_len = ok ? min((unsigned)clip[r], read_len) : 0u;
  if constexpr (STEP0 == SEL_TAIL) {
    if (ok) my_places = places[r];
    eff_len = min(my_places.y >> 16, read_len);
  }
  if constexpr (TRIM) {  // (what holds when no line is read)
    unsigned hi = eff_len;  // SEL_TAIL: it is e2, and cut_tail is in that
    if constexpr (STEP0 != SEL_TAIL) hi = sel_cut_hi(t, eff_len);
    my_win = window(sel_cut_lo(t, eff_len), hi);
  }
  if (need_seq || need_qual) {  // (uniform)
    // the lane's words of the request at p0 of a line; [ws, we): the window, in places of the line (TRIM)
    const auto judge_words = [&](SelCounts &c, const uint4 (&v)[SEL_UNROLL], unsigned off, unsigned len, unsigned p0, int ws, int we, bool is_seq) {
      const int lead = (int)(off & 15u), span = lead + (int)len;
#pragma unroll
      for (unsigned k = 0; k < SEL_UNROLL; k++) {
        const int rel = (int)(p0 + 16u * (SEL_GROUP_LANES * k + sub));
        if (rel >= span) continue;
        const int first = max(lead - rel, 0), last = min(span - rel, 16);
        int wf = 0, wl = 0;
        if constexpr (TRIM) {
          wf = min(max(lead + ws - rel, 0), 16);
          wl = min(max(lead + we - rel, 0), 16);
        }
        if (is_seq) sel_judge_seq<TRIM>(c, v[k], first, last, wf, wl);
        else sel_judge_qual<TRIM>(c, v[k], first, last, wf, wl, level);
      }
    };
    // steps (TRIM): sel_round_steps of the round
    const auto consume = [&](const SelStage &st, unsigned steps, unsigned eff) {  // eff: CLIP, the record's eff_len
      SelCounts c = {0u, 0u, 0u, false};
      unsigned w = 0;
      if constexpr (TRIM) {
        const unsigned cut_len = CLIP ? eff : st.len;
        unsigned hi = cut_len;  // SEL_TAIL: it is e2, and cut_tail is in that
        if constexpr (STEP0 != SEL_TAIL) hi = sel_cut_hi(t, cut_len);
        const int a = (int)sel_cut_lo(t, cut_len), b = (int)hi, lead_q = (int)(st.qual_off & 15u);
        unsigned start = (unsigned)a, stop = (unsigned)b;
        if (walk_f) {  // (uniform)
          SelWalk wk = {0, 0ull, false};
          sel_walk_step<true>(wk, st.q, 0, sub, lead_q, a, b, (int)t.q_front + 33);
          for (unsigned s = 1; s < steps; s++) {  // a long read: the rest, not loaded ahead
            uint4 q[SEL_UNROLL];
            sel_load_line(q, raw, st.qual_off, st.len, s * SEL_STEP_BYTES, sub);
            sel_walk_step<true>(wk, q, s * SEL_STEP_BYTES, sub, lead_q, a, b, (int)t.q_front + 33);
          }
          if (wk.best) start = SEL_PLACE - (unsigned)(wk.best & SEL_PLACE);
        }
        if (walk_t) {
          SelWalk wk = {0, 0ull, false};
          for (unsigned s = steps - 1; s >= 1; s--) {  // a long read: from its last request down
            uint4 q[SEL_UNROLL];
            sel_load_line(q, raw, st.qual_off, st.len, s * SEL_STEP_BYTES, sub);
            sel_walk_step<false>(wk, q, s * SEL_STEP_BYTES, sub, lead_q, a, b, (int)t.q_tail + 33);
          }
          sel_walk_step<false>(wk, st.q, 0, sub, lead_q, a, b, (int)t.q_tail + 33);
          if (wk.best) stop = (unsigned)(wk.best & SEL_PLACE);
        }
        w = window(start, stop);
        const int ws = (int)(w & 0xFFFFu), we = ws + (int)(w >> 16);
        if (need_seq) judge_words(c, st.s, st.seq_off, st.len, 0, ws, we, true);
        if (need_qual) judge_words(c, st.q, st.qual_off, st.len, 0, ws, we, false);
        for (unsigned s = 1; s < steps; s++) {
          uint4 x[SEL_UNROLL];
          if (need_seq) {
            sel_load_line(x, raw, st.seq_off, st.len, s * SEL_STEP_BYTES, sub);
            judge_words(c, x, st.seq_off, st.len, s * SEL_STEP_BYTES, ws, we, true);
          }
          if (need_qual) {
            sel_load_line(x, raw, st.qual_off, st.len, s * SEL_STEP_BYTES, sub);
            judge_words(c, x, st.qual_off, st.len, s * SEL_STEP_BYTES, ws, we, false);
          }
        }
      } else {
        // the words a line can touch, counted from the aligned word of its first byte: the two lines start at different places
        const unsigned span_s = need_seq && st.len ? (st.seq_off & 15u) + st.len : 0u, span_q = need_qual && st.len ? (st.qual_off & 15u) + st.len : 0u;
        if (span_s) judge_words(c, st.s, st.seq_off, st.len, 0, 0, 0, true);
        if (span_q) judge_words(c, st.q, st.qual_off, st.len, 0, 0, 0, false);
        for (unsigned p0 = SEL_STEP_BYTES; p0 < max(span_s, span_q); p0 += SEL_STEP_BYTES) {  // a long read: the rest, not loaded ahead
          uint4 s[SEL_UNROLL], q[SEL_UNROLL];
          if (p0 < span_s) sel_load_line(s, raw, st.seq_off, st.len, p0, sub);
          if (p0 < span_q) sel_load_line(q, raw, st.qual_off, st.len, p0, sub);
          if (p0 < span_s) judge_words(c, s, st.seq_off, st.len, p0, 0, 0, true);
          if (p0 < span_q) judge_words(c, q, st.qual_off, st.len, p0, 0, 0, false);
        }
      }
      // over the record's eight lanes; packed: N and low counts are at most 65535 each, the byte sum below 2^23
      unsigned x = c.n | c.low << 16, y = c.qsum | (c.bad ? 0x80000000u : 0u);
#pragma unroll
      for (unsigned d = 1; d < SEL_GROUP_LANES; d <<= 1) {
        x += __shfl_xor(x, d);
        const unsigned o = __shfl_xor(y, d);
        y = ((y & 0x7FFFFFFFu) + (o & 0x7FFFFFFFu)) | ((y | o) & 0x80000000u);
      }
      return make_uint3(x, y, w);
    };
    const unsigned my_steps = sel_record_steps(wave, need_seq, need_qual);
    sel_rounds<false>(raw, wave, lane, need_seq, need_qual, [&](const SelStage &cur, unsigned k, unsigned j) {
      unsigned eff = 0, steps = 1;  // (without TRIM a long read is one loop over the rest of its requests: no steps)
      if constexpr (CLIP) eff = __shfl(eff_len, j);
      if constexpr (TRIM) steps = sel_round_steps(my_steps, lane, k);
      const uint3 got = consume(cur, steps, eff);
      const unsigned x = sel_hand_back(got.x, lane), y = sel_hand_back(got.y, lane);
      unsigned win_back = 0;
      if constexpr (TRIM) win_back = sel_hand_back(got.z, lane);
      if (sel_in_round(lane, k)) {
        n_count = x & 0xFFFFu;
        low_count = x >> 16;
        q_bytes = y & 0x7FFFFFFFu;
        bad = bad || (y >> 31);
        my_win = win_back;
      }
    });
  }

  // the verdict on what is left [start, start + n): 0 kept, 1 .. 5 the first criterion that fails; a read with nothing left
  // is "short"
  unsigned start = 0, n = mine.len;
  if constexpr (TRIM) {
    start = ok ? my_win & 0xFFFFu : 0u;
    n = ok ? my_win >> 16 : 0u;
  }
  const bool emptied = TRIM && ok && n == 0;
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
    if constexpr (TRIM) win[r] = start | n << 16;
    odd = mine.qual_off != mine.seq_off + mine.len + 3u || mine.seq_off < h0;
    if (r == n_recs - 1u) odd = odd || (unsigned long long)mine.qual_off + mine.len + 1ull > raw_len;
  }
  const unsigned long long kept_mask = __ballot(kept);
  if (lane == 0 && r0 < n_recs) keep[r0 / 64] = kept_mask;
  if (__any(bad) && lane == 0) res->bad = 1u;           // (every writer stores the same value)
  if (__any(odd) && lane == 0) res->not_bare = 1u;

  // the report: over the wave, over the workgroup, one atomic per counter and workgroup
  unsigned cnt[NC];
#pragma unroll
  for (unsigned i = 0; i < NC; i++) cnt[i] = 0;
  cnt[R_KEPT] = kept;
  cnt[R_BASES_IN] = ok ? mine.len : 0u;
  cnt[R_BASES_KEPT] = kept ? n : 0u;
#pragma unroll
  for (unsigned v = 1; v <= 5; v++) cnt[R_DROPPED + v - 1] = verdict == v;
  if constexpr (TRIM) {
    cnt[R_TRIMMED] = ok && n != mine.len;
    cnt[R_CUT_FRONT] = start;
    cnt[R_CUT_TAIL] = ok ? mine.len - start - n : 0u;
    cnt[R_EMPTIED] = emptied;
  }
  if constexpr (STEP0 == SEL_CLIP) {
    cnt[R_WITH_ADAPTER] = ok && eff_len < mine.len;
    cnt[R_CUT_ADAPTER] = ok ? mine.len - eff_len : 0u;
  }
  if constexpr (STEP0 == SEL_TAIL) {  // (zero in a record that is not ok)
    const unsigned a0 = min(my_places.x & 0xFFFFu, read_len), a1 = min(my_places.x >> 16, a0), e = min(my_places.y & 0xFFFFu, a1);
    cnt[R_WITH_ADAPTER] = a0 < read_len;
    cnt[R_CUT_ADAPTER] = read_len - a0;
    cnt[R_WITH_POLY] = a1 < a0;
    cnt[R_CUT_POLY] = a0 - a1;
    cnt[R_WINDOW_CUT] = eff_len < e;
    cnt[R_CUT_WINDOW] = e - min(eff_len, e);
  }
  unsigned long long bytes = size;  // (64 records of up to 2^32 - 1 bytes)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (unsigned i = 1; i < NC; i++)
      if (i != R_BYTES_KEPT) cnt[i] += __shfl_xor(cnt[i], d);
    bytes += __shfl_xor(bytes, d);
  }
  __shared__ unsigned long long wg_bytes;
  if (threadIdx.x == 0) wg_bytes = 0;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (unsigned i = 1; i < NC; i++)
      if (i != R_BYTES_KEPT && cnt[i]) atomicAdd(&wg[i], cnt[i]);
    if (bytes) atomicAdd(&wg_bytes, bytes);
  }
  __syncthreads();
  if (threadIdx.x < NC && threadIdx.x != 0) {
    const unsigned long long v = threadIdx.x == R_BYTES_KEPT ? wg_bytes : wg[threadIdx.x];
    if (v) atomicAdd(&res->w[threadIdx.x], v);
  }
}

// a kept record as the gather sees it: where its pieces come from
struct SelRec {
  long long h0, seq, qual;  // the header line, the first kept byte of the sequence and of the quality line, in the chunk
  unsigned hl, n;           // bytes of the header line with its '\n'; symbols of the window
  bool whole;               // untrimmed
};
__device__ __forceinline__ SelRec sel_rec(const fqgpu_rec *__restrict__ recs, const uint32_t *__restrict__ hstart,
                                          const uint32_t *__restrict__ win, unsigned r) {
  const fqgpu_rec rec = recs[r];
  const unsigned h0 = hstart[r], w = win[r];
  SelRec c;
  c.h0 = h0;
  c.hl = rec.seq_off > h0 ? rec.seq_off - h0 : 0u;
  c.n = w >> 16;
  c.seq = (long long)rec.seq_off + (w & 0xFFFFu);
  c.qual = (long long)rec.qual_off + (w & 0xFFFFu);
  c.whole = c.n == rec.len;
  return c;
}
// byte j of the record's trimmed canonical form
__device__ __forceinline__ unsigned sel_byte(const uint8_t *__restrict__ raw, const SelRec &c, unsigned long long j) {
  if (j < c.hl) return raw[c.h0 + (long long)j];
  j -= c.hl;
  if (j < c.n) return raw[c.seq + (long long)j];
  j -= c.n;
  if (j < 3) return j == 1 ? '+' : '\n';
  j -= 3;
  if (j < c.n) return raw[c.qual + (long long)j];
  return '\n';
}

// TRIM: out[koff[r], koff[r + 1]) = header line | seq[start, start + n) | "\n+\n" | qual[start, start + n) | '\n' for every
// kept record r; bare: the chunk's '+' lines are bare, so a whole record is one span of the chunk.  Without TRIM every kept
// record is whole and the kernel is for bare '+' lines alone (k_select_gather_records takes the others): out[koff[r] + i] =
// raw[hstart[r] + i]; recs, win and bare are not looked at.
template <bool TRIM>
__global__ void __launch_bounds__(SEL_GATHER_THREADS)
k_select_gather(const uint8_t *__restrict__ raw, const fqgpu_rec *__restrict__ recs, const uint32_t *__restrict__ hstart,
                const uint32_t *__restrict__ win, const unsigned long long *__restrict__ koff, unsigned n_recs, unsigned long long total,
                const bool bare, uint8_t *__restrict__ dst) {
  const unsigned long long t0 = (unsigned long long)blockIdx.x * SEL_TILE_BYTES;
  if (t0 >= total) return;
  const unsigned long long t1 = min(total, t0 + SEL_TILE_BYTES) - 1;  // the tile's last byte
  // (uniform: the compiler keeps these searches in scalar registers)
  const unsigned r_lo = sel_find(koff, 0, n_recs - 1, t0), r_hi = sel_find(koff, r_lo, n_recs - 1, t1);
  const long long d_lo = (long long)hstart[r_lo] - (long long)koff[r_lo], d_hi = (long long)hstart[r_hi] - (long long)koff[r_hi];
  // equal shifts: the records between are kept whole, or the source would have moved on without the output
  bool one_run = d_lo == d_hi;
  if constexpr (TRIM) one_run = bare && d_lo == d_hi && (win[r_lo] >> 16) == recs[r_lo].len && (win[r_hi] >> 16) == recs[r_hi].len;
#pragma unroll
  for (unsigned k = 0; k < SEL_GATHER_WORDS; k++) {
    const unsigned long long o = t0 + 16ull * (k * SEL_GATHER_THREADS + threadIdx.x);
    if (o >= total) continue;
    const unsigned long long last = min(o + 15, total - 1);
    long long src = (long long)o + d_lo;
    bool copy = one_run;
    unsigned ra = r_lo;
    SelRec ca = {0, 0, 0, 0u, 0u, false};
    if (!one_run) {  // (uniform)
      ra = sel_find(koff, r_lo, r_hi, o);
      const unsigned rb = sel_find(koff, ra, r_hi, last);
      if constexpr (!TRIM) {
        const long long delta = (long long)hstart[ra] - (long long)koff[ra];
        copy = ra == rb || delta == (long long)hstart[rb] - (long long)koff[rb];  // inside one run
        src = (long long)o + delta;
      } else {
        ca = sel_rec(recs, hstart, win, ra);
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
    }
    uint4 v;
    if (copy) {  // (sixteen bytes from a byte of the chunk: at most fifteen of the block's spare bytes behind it)
      const SelU128 s = *reinterpret_cast<const SelU128 *>(raw + src);
      v = make_uint4(s.a, s.b, s.c, s.d);
    } else if constexpr (!TRIM) {  // across a seam between two runs: byte by byte, every byte by its run's shift
      unsigned w[4] = {0, 0, 0, 0};
      unsigned rr = ra;
      unsigned long long next = koff[rr + 1];  // the first output byte that is no longer record rr's
      long long dd = src - (long long)o;
      for (unsigned i = 0; o + i <= last; i++) {
        if (o + i >= next) {
          rr = sel_find(koff, rr + 1, r_hi, o + i);
          next = koff[rr + 1];
          dd = (long long)hstart[rr] - (long long)koff[rr];
        }
        w[i >> 2] |= (unsigned)raw[(long long)(o + i) + dd] << (8 * (i & 3));
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    } else {  // across a seam between two pieces or two records: byte by byte
      unsigned w[4] = {0, 0, 0, 0};
      unsigned rr = ra;
      SelRec c = ca;
      unsigned long long base = koff[rr], next = koff[rr + 1];
      for (unsigned i = 0; o + i <= last; i++) {
        if (o + i >= next) {
          rr = sel_find(koff, rr + 1, r_hi, o + i);
          c = sel_rec(recs, hstart, win, rr);
          base = koff[rr];
          next = koff[rr + 1];
        }
        w[i >> 2] |= sel_byte(raw, c, o + i - base) << (8 * (i & 3));
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4 *>(dst + o) = v;  // (dst has room up to the next multiple of 16)
  }
}

// a filter alone on a chunk with text behind a '+': one wave per kept record, the canonical form put together
// (k_crc_canon_write); a correctness path, but twice as fast there as k_select_gather<true>'s pieces
__global__ void __launch_bounds__(256)
k_select_gather_records(const uint8_t *__restrict__ raw, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
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

// ---- a record range and a mark (include/fqgpu.h, fqgpu_chunk_select_marked).  The range needs no kernel of its own: every
// kernel above indexes by a record table and a count, and takes recs + first and end - first; the judge's `prev` gives the
// range's first record its header line.  The mark is this kernel, between the judge and the scan: a wave per 64 records --
// the judge's keep word --, keep &= mark, and for every record that flips ksize[r] = 0, so that the scan and the gather
// never see it.  What the flipped records had added to n_kept, bases_kept and bytes_kept is summed over the wave by
// shuffles, over the workgroup in LDS, and taken back with one atomic per counter and workgroup; the same count goes to
// word 20.  The judge leaves the keep bits behind the table's end zero, so mark bits there change nothing.
constexpr unsigned R_UNMARKED = 20;
__global__ void __launch_bounds__(SEL_THREADS)
k_select_mark(const unsigned long long *__restrict__ mark, unsigned n_recs, uint32_t *__restrict__ ksize, const uint32_t *__restrict__ win,
              unsigned long long *__restrict__ keep, SelectResult *__restrict__ res) {
  __shared__ unsigned wg_n, wg_bases;
  __shared__ unsigned long long wg_bytes;
  if (threadIdx.x == 0) {
    wg_n = 0;
    wg_bases = 0;
    wg_bytes = 0;
  }
  __syncthreads();
  const unsigned lane = fq_lane();
  const unsigned long long r0 = sel_wave_first();
  if (r0 < n_recs) {  // (uniform)
    const unsigned long long kw = keep[r0 / 64], gone = kw & ~mark[r0 / 64];
    if (gone) {  // (uniform)
      unsigned bases = 0;  // (64 records of at most 65535 bases)
      unsigned long long bytes = 0;
      if ((gone >> lane) & 1ull) {
        bytes = ksize[r0 + lane];
        bases = win[r0 + lane] >> 16;
        ksize[r0 + lane] = 0;
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        bases += __shfl_xor(bases, d);
        bytes += __shfl_xor(bytes, d);
      }
      if (lane == 0) {
        keep[r0 / 64] = kw & ~gone;
        atomicAdd(&wg_n, (unsigned)__popcll(gone));
        atomicAdd(&wg_bases, bases);
        atomicAdd(&wg_bytes, bytes);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && wg_n) {  // (a subtraction is the addition of the two's complement)
    const unsigned long long n = wg_n;
    if (threadIdx.x == 0) atomicAdd(&res->w[R_KEPT], 0ull - n);
    if (threadIdx.x == 1) atomicAdd(&res->w[R_BASES_KEPT], 0ull - wg_bases);
    if (threadIdx.x == 2) atomicAdd(&res->w[R_BYTES_KEPT], 0ull - wg_bytes);
    if (threadIdx.x == 3) atomicAdd(&res->w[R_UNMARKED], n);
  }
}

// ---- a per-record limit in front of the trim's steps (include/fqgpu.h, fqgpu_chunk_select_limited): behind k_adapter_find,
// clip[r] = min(clip[r], limit[r]); without an adapter clip[r] is filled from the record's length first.  The judge and
// k_tail_find then see the clip forms and nothing else changes.  Words 21 / 22 -- the records whose limit lies in front of
// the adapter's place, and the bases between the two -- are summed over the wave by shuffles, over the workgroup in LDS, and
// go out as one atomic per word and workgroup.  No line is read.
constexpr unsigned R_CUT_LIMIT_READS = 21, R_CUT_LIMIT_BASES = 22;
__global__ void __launch_bounds__(SEL_THREADS)
k_select_limit(const fqgpu_rec *__restrict__ recs, unsigned n_recs, const uint16_t *__restrict__ limit, uint16_t *__restrict__ clip,
               const unsigned have_clip, SelectResult *__restrict__ res) {
  __shared__ unsigned wg_reads, wg_bases;
  if (threadIdx.x == 0) {
    wg_reads = 0;
    wg_bases = 0;
  }
  __syncthreads();
  const unsigned long long r = (unsigned long long)blockIdx.x * SEL_THREADS + threadIdx.x;
  unsigned reads = 0, bases = 0;  // (256 records of at most 65535 bases)
  if (r < n_recs) {
    const unsigned len = min(recs[r].len, 65535u);  // (a longer one is refused by the judge)
    const unsigned a = have_clip ? min((unsigned)clip[r], len) : len, a0 = min(a, (unsigned)limit[r]);
    clip[r] = (uint16_t)a0;
    reads = a0 < a;
    bases = a - a0;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    reads += __shfl_xor(reads, d);
    bases += __shfl_xor(bases, d);
  }
  if (fq_lane() == 0 && reads) {
    atomicAdd(&wg_reads, reads);
    atomicAdd(&wg_bases, bases);
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_reads) {
    atomicAdd(&res->w[R_CUT_LIMIT_READS], (unsigned long long)wg_reads);
    atomicAdd(&res->w[R_CUT_LIMIT_BASES], (unsigned long long)wg_bases);
  }
}

}  // namespace

void SelectScratch::release_host() {
  if (host) (void)hipHostFree(host);
  host = nullptr;
}

int SelectScratch::begin(hipStream_t st) {
  if (const int rc = res.reserve(sizeof(SelectResult))) return rc;
  if (!host) FQ_HIP(hipHostMalloc(&host, sizeof(SelectResult), hipHostMallocPortable));
  FQ_HIP(hipMemsetAsync(res.p, 0, sizeof(SelectResult), st));
  return FQGPU_OK;
}

int SelectScratch::finish(hipStream_t st, const SelectResult *&result) {
  FQ_HIP(hipMemcpyAsync(host, res.p, sizeof(SelectResult), hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  result = static_cast<const SelectResult *>(host);
  return FQGPU_OK;
}

// The selection of a normalised job (fqgpu_internal.h) over the records of v, on st, waited for.  Two waits: the judge's
// result words decide what is gathered and how much room it needs; the gathered bytes come down in one copy.  FQGPU_E_ARG
// with *out_len and the report as the front left them -- zero -- and keep bits, windows and places zeroed: a byte that cannot
// be judged, a record that is not inside the chunk, has no symbol or more than a readlen_t counts.
int fq_select_chunk(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, const FqSelectJob &job, const FqSelectOut &o) {
  const size_t n_recs = v.n_recs;
  if (n_recs >= ((size_t)1 << 32) || v.raw_len >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  if (!n_recs) return FQGPU_OK;
  SelectScratch &ss = ctx->select;
  const fqgpu_adapter *const a = job.adapter;
  const fqgpu_tail *const x = job.tail;
  const fqgpu_trim *const t = job.trim;
  const bool clipped = a || job.limit;  // clip[r] stands in front of the trim's steps
  const unsigned R = (unsigned)n_recs;
  const unsigned long long raw_len = v.raw_len;
  const size_t n_waves = (n_recs + SEL_WAVE_RECORDS - 1) / SEL_WAVE_RECORDS;
  int rc;
  if ((rc = ss.ksize.reserve(n_recs * 4)) || (rc = ss.hstart.reserve(n_recs * 4)) || (t && (rc = ss.win.reserve(n_recs * 4))) ||
      (clipped && (rc = ss.clip.reserve(n_recs * 2))) || (x && (rc = ss.places.reserve(n_recs * 8))) ||
      (job.mark && (rc = ss.mark.reserve(n_waves * 8))) || (job.limit && (rc = ss.limit.reserve(n_recs * 2))) ||
      (rc = ss.keep.reserve(n_waves * 8)) || (rc = ss.koff.reserve((n_recs + 1) * 8)) || (rc = ss.begin(st)))
    return rc;
  uint32_t *const win = t ? ss.win.as<uint32_t>() : nullptr;
  uint16_t *const clip = clipped ? ss.clip.as<uint16_t>() : nullptr;
  uint2 *const places = x ? ss.places.as<uint2>() : nullptr;
  SelectResult *const dev = ss.res.as<SelectResult>();
  if (job.mark) {  // (its last word padded with zeros)
    FQ_HIP(hipMemsetAsync(ss.mark.p, 0, n_waves * 8, st));
    FQ_HIP(hipMemcpyAsync(ss.mark.p, job.mark, (n_recs + 7) / 8, hipMemcpyHostToDevice, st));
  }
  if (job.limit) FQ_HIP(hipMemcpyAsync(ss.limit.p, job.limit, n_recs * 2, hipMemcpyHostToDevice, st));
  fq_timer_span_begin(ctx, job.span, st);
  const dim3 judge_grid((unsigned)((n_waves + SEL_THREADS / 64 - 1) / (SEL_THREADS / 64)));
  if (a) {  // the adapter's bit planes: bit j of a plane is set iff A[j] is that base
    unsigned long long plane[4] = {0, 0, 0, 0};
    for (unsigned j = 0; j < a->len; j++) plane[a->seq[j] == 'A' ? 0 : a->seq[j] == 'C' ? 1 : a->seq[j] == 'G' ? 2 : 3] |= 1ull << j;
    const FindOne one = {plane[0], plane[1], plane[2], plane[3], a->len, a->min_overlap, a->max_err_pct, clip};
    hipLaunchKernelGGL(k_adapter_find<false>, judge_grid, dim3(SEL_THREADS), 0, st, v.raw, raw_len, v.recs, R, one, dev);
    FQ_HIP(hipGetLastError());
  }
  if (job.limit) {
    hipLaunchKernelGGL(k_select_limit, dim3((unsigned)((n_recs + SEL_THREADS - 1) / SEL_THREADS)), dim3(SEL_THREADS), 0, st, v.recs, R,
                       ss.limit.as<uint16_t>(), clip, a ? 1u : 0u, dev);
    FQ_HIP(hipGetLastError());
  }
  if (x) {
    hipLaunchKernelGGL(k_tail_find, judge_grid, dim3(SEL_THREADS), 0, st, v.raw, raw_len, v.recs, R, *x, *t, clip, places, dev);
    FQ_HIP(hipGetLastError());
  }
  const auto judge = x ? &k_select_judge<true, SEL_TAIL> : clipped ? &k_select_judge<true, SEL_CLIP> : t ? &k_select_judge<true> : &k_select_judge<false>;
  const auto gather = t ? &k_select_gather<true> : &k_select_gather<false>;
  hipLaunchKernelGGL(judge, judge_grid, dim3(SEL_THREADS), 0, st, v.raw, raw_len, v.recs, R, t ? *t : fqgpu_trim{}, *job.filter,
                     ss.ksize.as<uint32_t>(), ss.hstart.as<uint32_t>(), win, ss.keep.as<unsigned long long>(), dev, clip, places,
                     v.prev ? 1u : 0u);
  FQ_HIP(hipGetLastError());
  if (job.mark) {
    hipLaunchKernelGGL(k_select_mark, judge_grid, dim3(SEL_THREADS), 0, st, ss.mark.as<unsigned long long>(), R, ss.ksize.as<uint32_t>(), win,
                       ss.keep.as<unsigned long long>(), dev);
    FQ_HIP(hipGetLastError());
  }
  if (o.out && (rc = fq_scan_u32_to_u64(st, ss.ksize.as<uint32_t>(), n_recs, ss.koff.as<unsigned long long>(), ss.scan_tmp))) {
    fq_timer_span_end(ctx, st);
    return rc;
  }
  fq_timer_span_end(ctx, st);
  if (o.keep) FQ_HIP(hipMemcpyAsync(o.keep, ss.keep.p, (n_recs + 7) / 8, hipMemcpyDeviceToHost, st));
  if (o.win) FQ_HIP(hipMemcpyAsync(o.win, win, n_recs * 4, hipMemcpyDeviceToHost, st));
  if (o.places) FQ_HIP(hipMemcpyAsync(o.places, places, n_recs * 8, hipMemcpyDeviceToHost, st));
  const SelectResult *res;
  if ((rc = ss.finish(st, res))) return rc;
  if (res->bad) {
    if (o.keep) memset(o.keep, 0, (n_recs + 7) / 8);
    if (o.win) memset(o.win, 0, n_recs * 4);
    if (o.places) memset(o.places, 0, n_recs * 8);
    return FQGPU_E_ARG;
  }
  for (unsigned i = 1; i < o.report_words; i++) o.report[i] = res->w[i];
  o.report[0] = n_recs;
  const size_t total = (size_t)res->w[R_BYTES_KEPT];
  *o.out_len = total;
  if (!o.out || !total) return FQGPU_OK;
  if (o.out_cap < total) return FQGPU_E_OVERFLOW;
  if ((rc = ss.dst.reserve(total + 64))) return rc;
  // the second phase: the gather, then one copy down
  fq_timer_span_begin(ctx, job.span, st);
  if (t || !res->not_bare)
    hipLaunchKernelGGL(gather, dim3((unsigned)((total + SEL_TILE_BYTES - 1) / SEL_TILE_BYTES)), dim3(SEL_GATHER_THREADS), 0, st, v.raw, v.recs,
                       ss.hstart.as<uint32_t>(), win, ss.koff.as<unsigned long long>(), R, (unsigned long long)total, res->not_bare == 0u,
                       ss.dst.as<uint8_t>());
  else
    hipLaunchKernelGGL(k_select_gather_records, dim3((unsigned)min((n_recs + 3) / 4, (size_t)8192)), dim3(256), 0, st, v.raw, v.recs, R,
                       ss.ksize.as<uint32_t>(), ss.hstart.as<uint32_t>(), ss.koff.as<unsigned long long>(), ss.dst.as<uint8_t>());
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipMemcpyAsync(o.out, ss.dst.p, total, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  return FQGPU_OK;
}

// Adapter content of the records of v, on st, waited for: out[0, fqgpu_probe_words(p->n, P)) and -- places_out != nullptr --
// p->n places per record.  One kernel, k_adapter_find's probe form, and one wait.  FQGPU_E_ARG with out and places_out zeroed:
// a sequence byte outside ACGTN, a record that is not inside the chunk, has no symbol or more than a readlen_t counts.
int fq_probe_chunk(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, const fqgpu_probes *p, unsigned P, uint64_t *out,
                   uint16_t *places_out) {
  const unsigned n = p->n;
  const size_t words = fqgpu_probe_words(n, P), n_recs = v.n_recs;
  if (!words || n_recs >= ((size_t)1 << 32) || v.raw_len >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  for (size_t i = 0; i < words; i++) out[i] = 0;
  SelectScratch &ss = ctx->select;
  const size_t n_waves = (n_recs + SEL_WAVE_RECORDS - 1) / SEL_WAVE_RECORDS, places_bytes = n_recs * n * sizeof(uint16_t);
  int rc;
  if ((rc = ss.probe_out.reserve(words * 8)) || (places_out && n_recs && (rc = ss.probe_places.reserve(places_bytes))) || (rc = ss.begin(st)))
    return rc;
  FindMany many = {};
  for (unsigned k = 0; k < n; k++) {  // the probes' bit planes: bit j of a plane is set iff A[j] is that base
    const fqgpu_adapter &a = p->probe[k];
    ClipAdapter &ad = many.ad[k];
    for (unsigned j = 0; j < a.len; j++) (a.seq[j] == 'A' ? ad.a : a.seq[j] == 'C' ? ad.c : a.seq[j] == 'G' ? ad.g : ad.t) |= 1ull << j;
    ad.m = a.len;
    ad.min_overlap = a.min_overlap;
    ad.keep_pct = 100u - a.max_err_pct;
  }
  many.n = n;
  many.P = P;
  many.out = ss.probe_out.as<unsigned long long>();
  many.places = places_out && n_recs ? ss.probe_places.as<uint16_t>() : nullptr;
  FQ_HIP(hipMemsetAsync(ss.probe_out.p, 0, words * 8, st));
  if (n_recs) {
    fq_timer_span_begin(ctx, "probe", st);
    hipLaunchKernelGGL(k_adapter_find<true>, dim3((unsigned)((n_waves + SEL_THREADS / 64 - 1) / (SEL_THREADS / 64))), dim3(SEL_THREADS), 0, st,
                       v.raw, (unsigned long long)v.raw_len, v.recs, (unsigned)n_recs, many, ss.res.as<SelectResult>());
    fq_timer_span_end(ctx, st);
    FQ_HIP(hipGetLastError());
  }
  FQ_HIP(hipMemcpyAsync(out, ss.probe_out.p, words * 8, hipMemcpyDeviceToHost, st));
  if (many.places) FQ_HIP(hipMemcpyAsync(places_out, ss.probe_places.p, places_bytes, hipMemcpyDeviceToHost, st));
  const SelectResult *res;
  if ((rc = ss.finish(st, res))) return rc;
  if (res->bad) {
    for (size_t i = 0; i < words; i++) out[i] = 0;
    if (many.places) memset(places_out, 0, places_bytes);
    return FQGPU_E_ARG;
  }
  out[0] = n_recs;
  out[2] = n;
  out[3] = P;
  out[4] = fq_probes_fingerprint(p);
  return FQGPU_OK;
}
