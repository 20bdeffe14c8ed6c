// Internal declarations shared by the HIP translation units of libfqgpu.so.
// gfx950 (MI355X, wave64) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <new>

#include "../../include/fqgpu.h"

#define FQ_WAVE 64

// ---------------------------------------------------------------- models
// Context/symbol definition of the two streams (reference a2/a4 in SURVEY.md 8(a)).
struct SeqModel {
  static constexpr int B = FQGPU_SEQ_MODELS;  // contexts
  static constexpr int A = FQGPU_SEQ_ALPHA;   // alphabet
  static constexpr int KEYBITS = 8;
  static constexpr int STREAM = 0;
};
struct QualModel {
  static constexpr int B = FQGPU_QUAL_MODELS;
  static constexpr int A = FQGPU_QUAL_ALPHA;
  static constexpr int KEYBITS = 13;
  static constexpr int STREAM = 1;
};

// Device-side tables of one stream, built once per handle.
// Decoder entry (one per state, behind the table's zstd header word): the fields of zstd's FSE_decode_t
// arranged for the decode walk -- [31:16] newState * 4 (byte offset inside the table), [12:9] nbBits,
// [8:3] symbol (= symbol * 8, the stride of the walk's per-context LDS slots).  fqgpu_ctx_dump_tables
// hands out zstd's layout {u16 newState; u8 symbol; u8 nbBits}.
#define FQ_DENTRY(new_state, sym, nb) ((((uint32_t)(new_state)) << 18) | ((uint32_t)(nb) << 9) | ((uint32_t)(sym) << 3))
#define FQ_DENTRY_TO_ZSTD(w) ((((uint32_t)(w)) >> 18) | (((((uint32_t)(w)) >> 3) & 63u) << 16) | (((((uint32_t)(w)) >> 9) & 15u) << 24))

struct DevTables {
  int16_t *norm = nullptr;      // [B][A]
  uint32_t *logs = nullptr;     // [B]
  uint32_t *log_prefix = nullptr;  // [B+1] exclusive prefix of logs (bit offsets of the state flush)
  uint32_t *ct = nullptr;       // CTable pool, zstd word layout per context
  uint32_t *ct_off = nullptr;   // [B] word offset of each CTable
  uint32_t *dt = nullptr;       // DTable pool, zstd word layout per context
  uint32_t *dt_off = nullptr;   // [B]
  unsigned long long *reset_mask = nullptr;  // [B] bit s set: symbol s has normalised count 1 or -1
  uint16_t *next1 = nullptr;    // sequence stream only: [B][4 << max_log] one-symbol transition tables,
                                // next[s][x - size] = ((state after coding s in state x) - size) * 2
  uint16_t *next2 = nullptr;    // sequence stream, max_log <= 11: [B][16 << max_log] two-symbol tables,
                                // next2[s1 | s2 << 2][x - size] = next[s2][next[s1][x - size]]
  uint16_t *seq_pow[4] = {nullptr, nullptr, nullptr, nullptr};  // sequence stream: next1-shaped tables of S-fold powers,
  unsigned seq_pow_S[4] = {0, 0, 0, 0};                         // pow[s][x - size] = next[s]^S, for the S named here
  uint32_t max_log = 0;
  size_t ct_words = 0, dt_words = 0;
};
#define FQ_SEQ_POW_SETS 4
#ifndef FQ_SEQ_CAND_CAP_DEFAULT  // (A/B variants: make variant DEFS=-DFQ_SEQ_CAND_CAP_DEFAULT=...)
#define FQ_SEQ_CAND_CAP_DEFAULT 32u
#endif
#ifndef FQ_SEQ_CAND_PREFIX_DEFAULT
#define FQ_SEQ_CAND_PREFIX_DEFAULT 1u
#endif

// Result block of one (block, stream) coding job, in device memory.
struct StreamResult {
  unsigned long long total_bits;  // payload bits (before state flush)
  unsigned long long len;         // bytes of the finished stream
  unsigned int overflow;          // reference capacity rule violated
  unsigned int bad_symbol;        // quality above Q63 seen
  unsigned int refixed;           // segments the fix-up pass had to re-run
  unsigned int corrupt;           // decode: bad end mark / bits left over
};

struct BlockResult {
  StreamResult s[2];
  unsigned long long n_pos_len;  // number of u16 entries in n_pos
  unsigned int seq_groups_handed;  // sequence chains: segment groups k_seq_setfunc handed over to k_seq_candwalk ...
  unsigned int seq_groups_kept;    // ... and groups it walked to their end (both 0 when nothing may be handed over)
};

// ---------------------------------------------------------------- helpers
#define FQ_HIP(call)                                                 \
  do {                                                               \
    hipError_t e_ = (call);                                          \
    if (e_ != hipSuccess) return fq_hip_error(e_, __FILE__, __LINE__); \
  } while (0)

int fq_hip_error(hipError_t e, const char *file, int line);

template <class T> static inline T *fq_dev_alloc(size_t n) {
  void *p = nullptr;
  if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
  return reinterpret_cast<T *>(p);
}

// A typed device array: pointer and ELEMENTS allocated, the one record of what stands behind a block's buffer.  Reads as its
// pointer.  grow: room for `need` elements, allocated with `slack` more; never shrinks; the outgrown buffer is freed first
// (check_free: a failing hipFree is an error); on failure the array is empty.
template <class T> struct DevArray {
  T *p = nullptr;
  size_t n = 0;
  operator T *() const { return p; }
  T *operator->() const { return p; }
  size_t bytes() const { return n * sizeof(T); }
  int grow(size_t need, size_t slack = 0, bool check_free = false) {
    if (p && need <= n) return FQGPU_OK;
    const hipError_t e = release();
    if (check_free) FQ_HIP(e);
    if (!(p = fq_dev_alloc<T>(need + slack))) return FQGPU_E_NOMEM;
    n = need + slack;
    return FQGPU_OK;
  }
  hipError_t release() {
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    n = 0;
    return e;
  }
};

// Growable device buffer (never shrinks): the per-handle scratch.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return FQGPU_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return FQGPU_E_NOMEM; }
    cap = want;
    return FQGPU_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// The DevBufs of a scratch struct, ONE list per struct: what frees a handle and what fills its scratch with a byte
// (fqgpu_ctx_fill_scratch) both walk it, so a buffer cannot be freed but never filled.  FQ_SCRATCH_BUFS(T, FQ_B(T, m), ...)
// stands behind the struct; tests/test_build_invariants.py holds every list against the DevBuf members of its struct.
template <class T> struct FqBufOf { const char *name; DevBuf T::*m; };
#define FQ_B(T, m) {#m, &T::m}
#define FQ_SCRATCH_BUFS(T, ...)                                                      \
  inline constexpr FqBufOf<T> fq_bufs_##T[] = {__VA_ARGS__};                         \
  template <class F> static inline void fq_each_buf(T &s, F &&f) {                   \
    for (const FqBufOf<T> &e : fq_bufs_##T) f(e.name, s.*(e.m));                     \
  }
template <class T> static inline void fq_release_bufs(T &s) { fq_each_buf(s, [](const char *, DevBuf &b) { b.release(); }); }

struct KernelTimer;  // api.cpp

// grow-only scratch of the device record parser (parse.hip)
struct ParseScratch {
  DevBuf cnt, base, sum, nl_pos, scan_tmp;
  size_t total_nl = 0;  // newlines counted by fq_parse_count
};
FQ_SCRATCH_BUFS(ParseScratch, FQ_B(ParseScratch, cnt), FQ_B(ParseScratch, base), FQ_B(ParseScratch, sum), FQ_B(ParseScratch, nl_pos),
                FQ_B(ParseScratch, scan_tmp))

// Result words of the device header coder (headers.hip), and its grow-only scratch
struct HdrResult {
  unsigned long long first_error;  // record << 8 | code (1: numeric field, 2: string field too long, 3: the streams would not fit -- a record
                                   // table that is not this chunk's) of the first header that cannot be coded; ~0: none
  unsigned long long total;        // bytes of the output buffer in use
  unsigned long long off[3 * FQGPU_HDR_MAX_FIELDS];  // per field: flags, content, lengths
  uint32_t size[3 * FQGPU_HDR_MAX_FIELDS];
};
struct HdrScratch {
  DevBuf wg_sum, wg_base, out, first, res;
  HdrResult *host_res = nullptr;  // page-locked
  uint8_t *host_first = nullptr;  // page-locked staging of the dataset's first header
  unsigned n_fields = 0;
  size_t bound = 0;
  bool pending = false;           // kernels queued for the block in flight, results not collected yet
  bool collected = false;
  void release_host() {  // (the device buffers: fq_release_bufs)
    if (host_res) (void)hipHostFree(host_res);
    if (host_first) (void)hipHostFree(host_first);
    host_res = nullptr; host_first = nullptr; pending = collected = false;
  }
};
FQ_SCRATCH_BUFS(HdrScratch, FQ_B(HdrScratch, wg_sum), FQ_B(HdrScratch, wg_base), FQ_B(HdrScratch, out), FQ_B(HdrScratch, first),
                FQ_B(HdrScratch, res))

// Scratch of the encode pipeline for one stream.  What each buffer holds, its size and the sub-arrays inside it: EncPlan
// (enc_plan.h), which both fqgpu_ctx_reserve and a launch reserve from.
struct EncScratch {
  DevBuf slot_of, keys, sorted_sym, out16, tile_hist, tile_base, group_sum, ctx_arrays, seg_state, seg_arrays;
  DevBuf seq_bdesc, seq_plan, seq_fbuf, seq_cbuf, seq_cand, tile_bits, tile_bit_base, tile_runs, tile_sync;
  DevBuf dbg_enc16;   // timing experiments only (FQGPU_DEBUG_NO_ALIAS): enc16 apart from the keys, so that stale keys stay valid
};
FQ_SCRATCH_BUFS(EncScratch, FQ_B(EncScratch, slot_of), FQ_B(EncScratch, keys), FQ_B(EncScratch, sorted_sym), FQ_B(EncScratch, out16),
                FQ_B(EncScratch, tile_hist), FQ_B(EncScratch, tile_base), FQ_B(EncScratch, group_sum), FQ_B(EncScratch, ctx_arrays),
                FQ_B(EncScratch, seg_state), FQ_B(EncScratch, seg_arrays), FQ_B(EncScratch, seq_bdesc), FQ_B(EncScratch, seq_plan),
                FQ_B(EncScratch, seq_fbuf), FQ_B(EncScratch, seq_cbuf), FQ_B(EncScratch, seq_cand), FQ_B(EncScratch, tile_bits),
                FQ_B(EncScratch, tile_bit_base), FQ_B(EncScratch, dbg_enc16), FQ_B(EncScratch, tile_runs), FQ_B(EncScratch, tile_sync))

// One encode lane: everything a block needs while it is being coded, so that several
// blocks can be in flight on one GPU (two HIP streams: sequence pipeline, quality pipeline).
struct EncLane {
  hipStream_t st_seq = nullptr, st_qual = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  DevBuf rec_start;   // u32 [R+1] first encode index of each record
  DevBuf n_cnt32;     // u32 [R] N count | u32 [R] length
  DevBuf n_off;       // u32 [R+1]
  DevBuf first_sym;   // u8 [R] sequence | u8 [R] quality: every record's first symbol in encode order (fused K1 -> K3)
  DevBuf tile_first;  // u32 [tiles] the record that holds each tile's first encode index (fused K1 -> K3: no record search there)
  DevBuf rscan;       // k_record_scan: u32 ticket, pad | u64 status[chunks] (zero when allocated; epochs and tickets count on)
  unsigned rscan_epoch = 0, rscan_tickets = 0;  // launches so far (24 bits used) / tickets handed out so far
  DevBuf scan_tmp;
  EncScratch enc[2];
  // diagnostics (fqgpu_dblock_qual_segment_classes): where the lane's last encode left the classes of its quality segments
  // and their number (in enc[1], set after its buffers are reserved), and that encode's stamp (fqgpu_ctx::encodes; 0: none)
  const uint8_t *diag_cls = nullptr;
  const uint32_t *diag_anchor = nullptr;  // (fqgpu_dblock_qual_segments: SegArrays::anchor of the same encode)
  const uint32_t *diag_n_segs = nullptr;  // = seg_base + B: the B + 1 words that end here are the contexts' first segments
  unsigned long long diag_stamp = 0;
  // whatever may move or overwrite enc[1] without being an encode (reserving ahead, set_lanes, fill_scratch) calls this first
  void forget_diag() { diag_cls = nullptr; diag_anchor = nullptr; diag_n_segs = nullptr; diag_stamp = 0; }
};
FQ_SCRATCH_BUFS(EncLane, FQ_B(EncLane, rec_start), FQ_B(EncLane, n_cnt32), FQ_B(EncLane, n_off), FQ_B(EncLane, first_sym),
                FQ_B(EncLane, tile_first), FQ_B(EncLane, rscan), FQ_B(EncLane, scan_tmp))

// Header decode and chunk layout (decode_headers.hip, fqgpu_decode_chunk): the format, the dataset's first header and
// the offsets of every stream in ONE staging buffer (this struct first, then readlens, the first header, per field
// flags | content | lengths, each 16-byte aligned)
struct FqChunkField {
  unsigned long long flags, content, lengths;  // byte offsets in the stage
  uint32_t n_flags, n_content, n_lengths;
  uint32_t first_off, first_len;  // this field of the dataset's first header: offset in it, length
  int32_t first_val;              // ... its value (NUMERIC)
  uint32_t type;                  // 0 = NUMERIC, 1 = STRING
  uint32_t sep;                   // separator behind the field (none behind the last)
};
struct FqChunkFmt {
  uint32_t n_fields, n_recs, n_tiles, pad;
  unsigned long long raw_len, stage_len, readlens, first;  // first: offset of the first header in the stage
  FqChunkField f[FQGPU_HDR_MAX_FIELDS];
};
struct FqChunkResult {
  unsigned long long bad;    // first record the host decoder throws on (~0: none)
  unsigned long long total;  // bytes laid out
};
struct ChunkScratch {
  DevBuf stage, agg, cls, clp, hlen, tlen, toff, res, scan_tmp;
  DevBuf pick;  // fq_chunk_layout of a window: u64 [4] record offsets
  uint8_t *host = nullptr;  // host stage (grow-only, pageable: small copies stay out of the DMA queues' way)
  size_t host_cap = 0, stage_len = 0;
  unsigned n_fields = 0, n_tiles = 0;
  bool host_grow(size_t n) {
    if (n <= host_cap) return true;
    delete[] host;
    host = new (std::nothrow) uint8_t[n + n / 8];
    host_cap = host ? n + n / 8 : 0;
    return host != nullptr;
  }
  void release_host() {
    delete[] host;
    host = nullptr;
    host_cap = 0;
  }
};
FQ_SCRATCH_BUFS(ChunkScratch, FQ_B(ChunkScratch, stage), FQ_B(ChunkScratch, agg), FQ_B(ChunkScratch, cls), FQ_B(ChunkScratch, clp),
                FQ_B(ChunkScratch, hlen), FQ_B(ChunkScratch, tlen), FQ_B(ChunkScratch, toff), FQ_B(ChunkScratch, res),
                FQ_B(ChunkScratch, scan_tmp), FQ_B(ChunkScratch, pick))

// CRC-32 of a chunk in HBM (crc.hip): multiplier tables (built once per handle), the slices' remainders, the result words
// and, for a chunk with text behind its '+' lines, the canonical bytes gathered into `flat`
struct CrcScratch {
  DevBuf tab, rem, res, chk, clen, coff, flat, scan_tmp;
  uint32_t *host = nullptr;  // page-locked landing place of {crc32, len lo, len hi, 0} and, behind them, the record check's verdict
  bool tab_built = false;
  void release_host();
};
FQ_SCRATCH_BUFS(CrcScratch, FQ_B(CrcScratch, tab), FQ_B(CrcScratch, rem), FQ_B(CrcScratch, res), FQ_B(CrcScratch, chk),
                FQ_B(CrcScratch, clen), FQ_B(CrcScratch, coff), FQ_B(CrcScratch, flat), FQ_B(CrcScratch, scan_tmp))

// Read summary of a chunk in HBM (stats.hip): the u64 result table, the workgroups' u32 slabs, the "a byte that cannot be
// counted" flag and its page-locked landing place; all grown on demand
struct StatsScratch {
  DevBuf out, slabs, bad;
  unsigned *host_bad = nullptr;
  bool attr_set = false;  // the count kernel's LDS size has been asked for
  void release_host();
};
FQ_SCRATCH_BUFS(StatsScratch, FQ_B(StatsScratch, out), FQ_B(StatsScratch, slabs), FQ_B(StatsScratch, bad))

// The scratch of the calls on chunks at rest in HBM (select.hip, pair.hip); all grown on demand, and one for all of them: each
// call is waited for before it returns.
//   the selection  per record the kept size, the start of its header line and -- a trim's -- its window, its clip place (a
//                  uint16_t: k_adapter_find or k_select_limit writes it, the judge reads it) and -- a tail's -- its places a0,
//                  a1, e, e2; the keep bits, the offsets of the kept records in the output, the gathered output; the caller's
//                  mark (a u64 word per 64 records) and limits (a uint16_t per record)
//   the probe      its u64 result tables and -- when asked for -- the records' places, n uint16_t each
//   the overlap    its u64 result words and the pairs' limit1, limit2 and I, three arrays of uint16_t
//   the correction the caller's inserts and the pairs' changed places, two arrays of uint16_t; its counters are the result words
//   the merge      the caller's inserts, per pair the merged record's size (a uint32_t), the merged bits (a u64 word per 64
//                  pairs) and the merged records themselves, to the next multiple of 16 bytes; the records' places are `koff`,
//                  the caller's mark `mark`; its counters are the result words
//   every call     `res`, the result words (SelectResult, sel_words.h), and `host`, their page-locked landing place, between
//                  begin and finish
struct SelectResult;
struct SelectScratch {
  DevBuf ksize, hstart, win, clip, places, keep, koff, dst, res, scan_tmp;
  DevBuf probe_out, probe_places;
  DevBuf mark, limit;
  DevBuf overlap_out, overlap_pairs;
  DevBuf correct_in, correct_fixed;
  DevBuf merge_in, merge_size, merge_bits, merge_out;
  void *host = nullptr;
  void release_host();
  // The frame of a call: begin reserves `res`, allocates `host` once and queues the zeroing of the result words on st; finish
  // queues their copy to `host` behind whatever the driver queued, waits for st -- the call's one wait, or its first of two --
  // and hands the words back.
  int begin(hipStream_t st);
  int finish(hipStream_t st, const SelectResult *&result);
};
FQ_SCRATCH_BUFS(SelectScratch, FQ_B(SelectScratch, ksize), FQ_B(SelectScratch, hstart), FQ_B(SelectScratch, win), FQ_B(SelectScratch, clip),
                FQ_B(SelectScratch, places), FQ_B(SelectScratch, keep), FQ_B(SelectScratch, koff), FQ_B(SelectScratch, dst),
                FQ_B(SelectScratch, res), FQ_B(SelectScratch, scan_tmp), FQ_B(SelectScratch, probe_out), FQ_B(SelectScratch, probe_places),
                FQ_B(SelectScratch, mark), FQ_B(SelectScratch, limit), FQ_B(SelectScratch, overlap_out), FQ_B(SelectScratch, overlap_pairs),
                FQ_B(SelectScratch, correct_in), FQ_B(SelectScratch, correct_fixed), FQ_B(SelectScratch, merge_in),
                FQ_B(SelectScratch, merge_size), FQ_B(SelectScratch, merge_bits), FQ_B(SelectScratch, merge_out))

#define FQ_MAX_LANES 8
#define FQ_RECENT_BLOCKS 8

// The staging block of the host-pointer calls, kept between calls (grow-only device arrays), and what it holds:
//   - `pending` spans fqgpu_encode_begin .. fqgpu_encode_end; flags, done and used describe the block begun last (done also
//     serves fqgpu_encode_index behind its end) and mean nothing before one;
//   - crc_what says what fqgpu_chunk_crc32 and the other chunk calls may read: 0 nothing, 1 the chunk fqgpu_encode_begin
//     uploaded (its canonical bytes, by its record table), 2 the crc_len bytes a whole-chunk decode has just restored;
//   - index_built: the block holds the indexes fqgpu_decode_chunk_indexing built (fqgpu_decode_index).  A refused decode call
//     ends the digest and keeps the indexes, so the two are apart;
//   - clear() is the ONLY writer of "holds nothing", the handle's part and the block's: whoever acquires the block, fills the
//     scratch, cancels or fails calls it.
struct HpStage {
  fqgpu_dblock *block = nullptr;
  bool pending = false;
  unsigned flags = 0;
  hipStream_t done = nullptr;  // the stream the pending block's last kernel runs on
  size_t used = 0;             // bytes of the pending chunk up to its last complete record
  bool index_built = false;
  int crc_what = 0;
  size_t crc_len = 0;
  inline void clear();
  // the named part of clear() a decode call starts with, before its arguments are looked at: also a refused call ends the
  // last chunk's digest (and_index: and an indexing decode drops the indexes built before it)
  void end_digest(bool and_index = false) { crc_what = 0; if (and_index) index_built = false; }
};

struct fqgpu_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // uploads, decode
  hipStream_t dec_stream2 = nullptr;  // decode: the sequence streams, beside the quality streams on `stream`
  hipEvent_t dec_fork = nullptr, dec_join = nullptr;
  DevTables tab[2];
  unsigned seg_len = 0;          // segment of the generic chain kernels (0 = by block size: 1024..4096)
  int seq_generic = 0;           // 1: sequence stream also uses the reset-cut kernel
  unsigned seq_segment = 0;      // segment length of the sequence chain kernels (0 = default)
  unsigned seq_group = 8;        // segments a k_seq_setfunc wave walks in one go, at most (<= SETS_MAX_GROUP)
  unsigned seq_group_min = 16;   // ... as long as a chain keeps this many groups (one per wave of a workgroup)
  unsigned seq_cand_cap = FQ_SEQ_CAND_CAP_DEFAULT;  // a group down to this many states behind its prefix goes to k_seq_candwalk (0: none does)
  unsigned seq_cand_prefix = FQ_SEQ_CAND_PREFIX_DEFAULT;  // ... segments of that prefix
  bool lds_atomics_ordered = false;  // probed at creation: k_scatter may rank with LDS atomics
  bool tile_sorted = true;           // tile-sorted partition + fused gather/pack (needs lds_atomics_ordered); false: slot-based path
  unsigned index_stride = 1u << 20;  // symbols between the snapshots of a decode index
  unsigned n_cus = 256;          // compute units of the device
  unsigned setfunc_wgs = 0;      // persistent workgroups of k_seq_setfunc (0 = default, see fqgpu_ctx_create)
  unsigned n_lanes = 0, next_lane = 0;  // n_lanes 0 = by block size: fq_lanes_for()
  unsigned long long encodes = 0;       // encode launches so far: the stamp a lane and a block keep of their last one
  const void *recent[FQ_RECENT_BLOCKS] = {};  // the blocks coded last (compared, never followed: api.hip fq_next_lane)
  unsigned recent_at = 0;
  EncLane lanes[FQ_MAX_LANES];
  // decode scratch
  DevBuf n_cnt32, n_off, scan_tmp;
  DevBuf dec_desc;    // decode job descriptors
  DevBuf dec_chunks, dec_recstart;  // chunk list and per-block rec_start of the indexed decode
  DevBuf dec_idx, dec_entries;      // indexing decode: its job descriptors, the contexts' entries at every snapshot
  // what the last fq_decode_launch launched (fqgpu_ctx_decode_forms: a diagnostic for tests): FQGPU_DEC_FORM_* bits, the
  // quality chains of its whole-stream walks and the quality strides of its stride walks
  unsigned dec_forms = 0, dec_qual_chains = 0, dec_qual_strides = 0;
  KernelTimer *timer = nullptr;
  HpStage hp;                         // the staging block of the host-pointer calls and what it holds
  hipEvent_t hp_ev_h2d = nullptr;     // "the block's inputs have arrived": the lane's streams wait for it
  BlockResult *hp_result = nullptr;   // page-locked landing place of the result block
  ParseScratch hp_parse;              // fqgpu_encode_begin without a record table: the table is built on the device
  HdrScratch hp_hdr;                  // fqgpu_encode_headers_*: the header fields of the block in flight
  ChunkScratch hp_chunk;              // fqgpu_decode_chunk: header decode and layout
  bool check_only = false;            // fqgpu_ctx_set_check_only: fqgpu_decode_chunk takes raw_out == NULL
  CrcScratch crc;
  StatsScratch stats;
  SelectScratch select;
};

// (the handle's own DevBufs: the decode scratch)
FQ_SCRATCH_BUFS(fqgpu_ctx, FQ_B(fqgpu_ctx, n_cnt32), FQ_B(fqgpu_ctx, n_off), FQ_B(fqgpu_ctx, scan_tmp), FQ_B(fqgpu_ctx, dec_desc),
                FQ_B(fqgpu_ctx, dec_chunks), FQ_B(fqgpu_ctx, dec_recstart), FQ_B(fqgpu_ctx, dec_idx), FQ_B(fqgpu_ctx, dec_entries))

EncLane *fq_next_lane(fqgpu_ctx *ctx, size_t n_bases, fqgpu_dblock *b = nullptr);  // api.hip: the next lane in turn or the block's own; creates streams on first use
// Blocks a handle keeps in flight when the caller has not said (fqgpu_ctx_set_lanes(ctx, 0), the default): four -- two
// already fill the chip with 256 MiB blocks --, six for blocks of less than 48 M symbols (about 100 MiB), whose chains of
// short kernels leave more gaps to fill: 16 x 64 MiB blocks 70.6 -> 75.6 GB/s (eight: 71.2).
static inline unsigned fq_lanes_for(const fqgpu_ctx *ctx, size_t n_bases) {
  return ctx->n_lanes ? ctx->n_lanes : (n_bases && n_bases < ((size_t)48 << 20) ? 6u : 4u);
}

struct fqgpu_dblock {
  int device = 0;
  fqgpu_ctx *owner = nullptr;  // the handle whose lanes code this block (status / fetch synchronise it)
  DevArray<uint8_t> raw;   // raw_len + 64: the kernels' loads run past a line's end
  size_t raw_len = 0;
  DevArray<fqgpu_rec> recs;
  size_t n_recs = 0;
  size_t n_bases = 0;
  // seq_cap, qual_cap: the capacities the overflow rule is judged against (reference rule or the caller's); the arrays hold
  // 64 bytes more at least.  n_pos_cap: entries of n_pos provided for; the array holds 16 more at least
  DevArray<uint8_t> seq, qual;
  size_t seq_cap = 0, qual_cap = 0;
  DevArray<uint16_t> readlens, n_count, n_pos;
  size_t n_pos_cap = 0;
  DevArray<BlockResult> result;
  BlockResult host_result;        // filled by fqgpu_sync-ing calls
  size_t seq_len = 0, qual_len = 0, n_pos_len = 0;  // stream sizes used by decode
  // "the block's last encode is through", recorded behind its last kernel: the next encode of the SAME block -- on whichever lane it
  // lands -- waits for it, so that two encodes of one block never write its streams and result words at the same time (a caller
  // that queues a block again without a sync in between, with more lanes than blocks; recorded on and waited for by streams of
  // one lane it is free)
  hipEvent_t ev_encoded = nullptr;
  int home_lane = -1;  // the lane of the block's last encode (api.hip: fq_next_lane)
  int last_op = 0;  // 1 = encode, 2 = decode: which fields of the result block are meaningful
  bool result_pulled = true;  // host_result / stream sizes reflect the last launched operation
  void launched(int op) { last_op = op; result_pulled = false; }
  // the result block and the indexes describe no streams any more
  void drop_results() { last_op = 0; result_pulled = true; index_bytes[0] = index_bytes[1] = 0; }
  // decode index (extension): device copy per stream (64 spare bytes behind it), valid bytes
  DevArray<uint8_t> index[2];
  size_t index_bytes[2] = {0, 0};
  // diagnostics (fqgpu_dblock_qual_segment_classes): the stamp of the block's last encode; lane home_lane of the owner holds
  // its segment classes as long as that lane's stamp is the same
  unsigned long long diag_stamp = 0;
};

// The device arrays of a block, ONE list: fqgpu_dblock_destroy frees and fqgpu_ctx_fill_scratch fills what it visits, as
// f(name, array).  tests/test_build_invariants.py holds it against the DevArray members of the struct.
#define FQ_DBLOCK_BUFS(X) X(raw) X(recs) X(seq) X(qual) X(readlens) X(n_count) X(n_pos) X(result) X(index[0]) X(index[1])
template <class F> static inline void fq_dblock_each_buf(fqgpu_dblock &b, F &&f) {
#define FQ_X(m) f(#m, b.m);
  FQ_DBLOCK_BUFS(FQ_X)
#undef FQ_X
}

inline void HpStage::clear() {
  pending = index_built = false;
  crc_what = 0;
  if (!block) return;
  block->drop_results();
  block->seq_len = block->qual_len = block->n_pos_len = 0;
  block->host_result = BlockResult();
}

// Decode index of one stream: header, then one snapshot per multiple of `stride` symbols.
struct FqIndexHeader {
  uint32_t magic;    // 'FQIX'
  uint32_t stream;   // 0 = sequence, 1 = quality
  uint32_t stride;   // symbols between snapshots (multiple of 65536)
  uint32_t n_snap;   // snapshots: encode indices stride, 2 stride, ... < n_sym
  uint64_t n_sym;
  uint64_t reserved;
};
// snapshot k (k = 1 .. n_snap) at encode index e = k * stride, FQ_INDEX_SNAP_HEAD + 2 B bytes:
//   u64 bitpos     bits of the stream in front of symbol e
//   u8  prev[4]    bytes at positions p-1 .. p-4 of the record of symbol e-1 (p = its position;
//                  0xFF in front of the read): what the context model has seen when the decoder,
//                  coming from the stream's end, is about to decode symbol e-1
//   u32 reserved
//   u16 state[B]   decoder state (encoder state - table size) of every context at that point
constexpr unsigned FQ_INDEX_MAGIC = 0x58495146u, FQ_INDEX_SNAP_HEAD = 16;
// The layout's arithmetic, host and device, here and nowhere else (B = contexts of the stream's model).
#if defined(__HIPCC__)
#define FQ_HD __host__ __device__
#else
#define FQ_HD
#endif
template <class N> FQ_HD static inline unsigned fq_index_n_snap(N n_sym, unsigned stride) { return n_sym ? (unsigned)((n_sym - 1) / stride) : 0u; }
FQ_HD static inline size_t fq_index_snap_bytes(unsigned B) { return FQ_INDEX_SNAP_HEAD + 2 * (size_t)B; }
FQ_HD static inline size_t fq_index_bytes(size_t n_snap, unsigned B) { return sizeof(FqIndexHeader) + n_snap * fq_index_snap_bytes(B); }
// snapshot k = 1 .. n_snap (u64 bitpos first) and its u16 state[B]
template <class P> FQ_HD static inline P *fq_index_snap(P *index, unsigned B, unsigned k) { return index + fq_index_bytes(k - 1, B); }
FQ_HD static inline uint16_t *fq_index_states(uint8_t *index, unsigned B, unsigned k) {
  return reinterpret_cast<uint16_t *>(fq_index_snap(index, B, k) + FQ_INDEX_SNAP_HEAD);
}
FQ_HD static inline const uint16_t *fq_index_states(const uint8_t *index, unsigned B, unsigned k) { return fq_index_states(const_cast<uint8_t *>(index), B, k); }
// ---------------------------------------------------------------- launches (encode.hip / decode.hip / tables.hip)
int fq_build_freq_tables(int device, hipStream_t st, const uint8_t *raw_dev, const fqgpu_rec *recs_dev,
                         size_t n_recs, uint32_t *seq_counts_dev, uint32_t *qual_counts_dev, size_t n_bases, unsigned min_len);
int fq_normalize_counts(hipStream_t st, const uint32_t *counts_dev, int n_models, int alpha,
                        int16_t *norm_dev, uint32_t *logs_dev, uint32_t *max_log_dev, uint32_t *err_dev);
int fq_build_tables(hipStream_t st, DevTables &t, int n_models, int alpha, uint32_t *err_dev);
int fq_seq_pow_ensure(hipStream_t st, DevTables &t, unsigned n_models, unsigned S);

// wait: event the lane's first kernel waits for (inputs arriving on another stream), or nullptr;
// done: receives the stream on which the block's last kernel was launched (copies of the results
// ordered behind the encode go there), may be nullptr
int fq_encode_launch(fqgpu_ctx *ctx, fqgpu_dblock *b, unsigned flags, hipEvent_t wait = nullptr, hipStream_t *done = nullptr);
int fq_encode_reserve(fqgpu_ctx *ctx, const fqgpu_dblock *b);  // the scratch of a block of b's shape on the next lane in turn, nothing launched
int fq_encode_init_device();  // once per handle, on its device: the dynamic-LDS limit of k_seq_setfunc
int fq_probe_lds_atomic_order(hipStream_t st, bool *ordered);
// Part of one block that holds both decode indexes (fqgpu_decode_chunk_range): stream s (0 = sequence) walks its strides
// k_lo[s] .. k_hi[s] alone, with the kernels and the placement rule of a whole decode, and the N pass patches the records
// [w0, w1), the ones those strides write (through b->recs[r], into b->raw).  rec_start: the encode index of every
// record's first symbol (host, n_recs + 1 entries).
struct FqStridePlan {
  unsigned k_lo[2], k_hi[2];
  unsigned w0, w1;
  const uint32_t *rec_start;
};
// build_index (no plan): every block is walked from its streams' ends by the indexing walk, whatever index it holds, and
// is left with both decode indexes, stride ctx->index_stride (index_bytes set; a caller that finds the block's streams
// corrupt drops them)
// streams: which of a block's streams are decoded -- both, or the sequence stream alone (no plan entry, index or byte of
// the quality stream is then looked at)
constexpr unsigned FQ_DEC_SEQ = 1u, FQ_DEC_QUAL = 2u, FQ_DEC_BOTH = FQ_DEC_SEQ | FQ_DEC_QUAL;
int fq_decode_launch(fqgpu_ctx *ctx, fqgpu_dblock *const *blocks, size_t n_blocks, const FqStridePlan *plan = nullptr,
                     bool build_index = false, unsigned streams = FQ_DEC_BOTH);
int fq_wipe_launch(fqgpu_ctx *ctx, fqgpu_dblock *b);
int fq_qual_counts_sorted(hipStream_t st, const uint8_t *raw_dev, const fqgpu_rec *recs_dev, size_t n_recs, size_t n_bases,
                          uint32_t *counts_dev, uint32_t *err_dev);
int fq_parse_count(hipStream_t st, const uint8_t *raw_dev, size_t raw_len, ParseScratch &ps, size_t *n_recs);
size_t fq_headers_bound(size_t raw_len, size_t n_recs, size_t n_bases, unsigned n_fields);
int fq_headers_launch(hipStream_t st, const uint8_t *raw_dev, size_t raw_len, const fqgpu_rec *recs_dev, size_t n_recs, size_t n_bases,
                      const uint8_t *field_types, const char *separators, unsigned n_fields, const uint8_t *first_header,
                      size_t first_header_len, HdrScratch &hs);
int fq_chunk_prepare(const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs, size_t raw_len, ChunkScratch &cs);
int fq_chunk_layout(hipStream_t st, ChunkScratch &cs, uint8_t *raw_dev, fqgpu_rec *recs_dev, const unsigned q[4], bool write,
                    unsigned long long *bad, unsigned long long *total, unsigned long long at[4], bool fasta = false);
int fq_parse_records(hipStream_t st, const uint8_t *raw_dev, size_t raw_len, ParseScratch &ps, fqgpu_rec *recs_dev,
                     size_t n_recs, size_t *n_bases, size_t *n_n, size_t *used_len);

// ---------------------------------------------------------------- calls on a chunk at rest in HBM
// A chunk, or a record range of one, as every driver below takes it; the bytes and the table lie on the device.  Everything a
// driver hands back per record is relative to recs[0].
struct FqChunkView {
  const uint8_t *raw;     // the WHOLE chunk, whatever the range (a record's offsets count from here)
  size_t raw_len;
  const fqgpu_rec *recs;  // the range's first record
  size_t n_recs;          // the range's count
  bool prev;              // recs[-1] exists: the range's first record is not the table's first
};

// CRC-32 of device bytes (crc.hip), on st, waited for: of data_dev[0, len) as it lies / of the canonical bytes of a chunk
int fq_crc_bytes(fqgpu_ctx *ctx, hipStream_t st, const uint8_t *data_dev, size_t len, uint32_t *crc);
int fq_crc_canonical(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, uint32_t *crc, size_t *len);

// Read summary of a chunk in HBM (stats.hip), on st, waited for: out[0, fqgpu_stats_words(positions)) on the host
int fq_stats_chunk(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, unsigned positions, uint64_t *out);

// The selection (select.hip): the reads of v clipped, trimmed and judged as the job says, on st, waited for.  The job is
// NORMALISED by its one front (api.hip, select_call), and the driver does not look again: every spec has passed its check; an
// adapter, a tail, a mark or a limit stands beside a trim (one that cuts nothing, if the caller gave none); the filter is
// never nullptr; out.win is nullptr without a trim, out.places without a tail.
struct FqSelectJob {
  const fqgpu_adapter *adapter;  // nullptr: none.  k_adapter_find in front of the judge
  const fqgpu_tail *tail;        // nullptr: none.  k_tail_find between the clip and the trim
  const fqgpu_trim *trim;        // nullptr: the filter alone
  const fqgpu_filter *filter;
  const uint8_t *mark;           // host: (n_recs + 7) / 8 bytes in keep's layout; nullptr: every record is marked.  Word 20 is counted
  const uint16_t *limit;         // host: n_recs limits in front of the trim's steps; nullptr: none.  Words 21 / 22 are counted
  const char *span;              // the name its launches are timed under
};
// report[0, report_words), *out_len, keep, win (a window per record), places (a0, a1, e, e2 per record) -- each of the three
// where not nullptr -- and, out != nullptr and out_cap enough, ONE copy of *out_len bytes into out.  The front has zeroed
// *out_len and the report.
struct FqSelectOut {
  uint8_t *out;
  size_t out_cap;
  size_t *out_len;
  uint64_t *report;
  unsigned report_words;
  uint8_t *keep;
  uint32_t *win;
  uint16_t *places;
};
int fq_select_chunk(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, const FqSelectJob &job, const FqSelectOut &o);

// Adapter content of a chunk in HBM (select.hip; the probe set has passed its check, positions is 1 .. 65535), on st, waited
// for: out[0, fqgpu_probe_words(p->n, positions)) on the host and -- places_out != nullptr -- p->n places per record
int fq_probe_chunk(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, const fqgpu_probes *p, unsigned positions, uint64_t *out,
                   uint16_t *places_out);

// The calls on two chunks (pair.hip): the records a.recs[i] (mate 1) and b.recs[i] (mate 2), i < a.n_recs == b.n_recs, of two
// chunks on ctx's device, both at rest, on st, waited for.  FQGPU_E_ARG: no record, or two counts.
// The read ids (include/fqgpu.h) compared.  *mismatch: the smallest i whose ids differ, (size_t)-1 when there is none.
// FQGPU_E_ARG: a header line outside its chunk
int fq_pair_names(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, size_t *mismatch);
// The mate overlap (the spec has passed its check): out[0, FQGPU_OVERLAP_WORDS) on the host and -- each where not nullptr --
// a uint16_t per pair of limit1, limit2 and I.  FQGPU_E_ARG with `out` zeroed, the three arrays then the caller's to zero: a
// record outside its chunk or of length 0, a byte outside ACGTN in an analysed line
int fq_pair_overlap(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, const fqgpu_overlap *o, uint64_t *out,
                    uint16_t *limit_a_out, uint16_t *limit_b_out, uint16_t *insert_out);
uint32_t fq_overlap_fingerprint(const fqgpu_overlap *o);  // fq_host.cpp: zlib's CRC-32 of the spec's 32 bytes
// The correction inside the mate overlap (the spec has passed its check) of two DIFFERENT chunks, with the host's insert_in[i]:
// it CHANGES both chunks, writing through the views' raw.  report[0, FQGPU_CORRECT_REPORT_WORDS) on the host and -- each where
// not nullptr -- a uint16_t per pair of the places changed in either mate.  FQGPU_E_ARG with the report zeroed, both chunks as
// they were and the two arrays the caller's to zero: an insert the lengths do not allow, a record with an insert outside its
// chunk, of length 0 or above 512, a byte inside an overlap that cannot be judged
int fq_pair_correct(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, const uint16_t *insert_in,
                    const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out, uint16_t *fixed_b_out);
// The merge of the mates into one read (the spec has passed its check), with the host's insert_in[i] and mark_in (nullptr: every
// pair is marked); both chunks stay as they are.  *out_len, report[0, FQGPU_MERGE_REPORT_WORDS) and -- where not nullptr --
// merged_out on the host, and, out != nullptr and out_cap enough, one copy of *out_len bytes into out (else FQGPU_E_OVERFLOW).
// FQGPU_E_ARG with `out` untouched, *out_len and the report zeroed and merged_out the caller's to zero: an insert the lengths
// do not allow, a merged pair's record outside its chunk or of length 0, a byte of a merged pair that cannot be judged
int fq_pair_merge(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &a, const FqChunkView &b, const uint16_t *insert_in, const uint8_t *mark_in,
                  const fqgpu_merge *m, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *merged_out);
uint32_t fq_probes_fingerprint(const fqgpu_probes *p);  // fq_host.cpp: zlib's CRC-32 of the bytes of probe[0 .. n)

// generic exclusive scans (scan.hip): out has n+1 entries, out[n] = total
int fq_scan_u32_to_u32(hipStream_t st, const uint32_t *in, size_t n, uint32_t *out, DevBuf &tmp);
int fq_scan2_u32_to_u32(hipStream_t st, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out_a,
                        uint32_t *out_b, DevBuf &tmp);
int fq_scan_u32_to_u64(hipStream_t st, const uint32_t *in, size_t n, unsigned long long *out, DevBuf &tmp);

// kernel timing hooks (api.hip): HIP events on the stream the kernels are launched on
void fq_timer_span_begin(fqgpu_ctx *ctx, const char *name, hipStream_t st);
void fq_timer_span_end(fqgpu_ctx *ctx, hipStream_t st);

// ---------------------------------------------------------------- device helpers
#if defined(__HIPCC__)

__device__ __forceinline__ unsigned fq_lane() { return threadIdx.x & 63u; }

// v_readfirstlane as an UNSIGNED value.  The builtin's type is int: `u64 | __builtin_amdgcn_readfirstlane(x)`
// sign-extends, i.e. ORs thirty-two ones into the upper half whenever bit 31 of x is set.  That -- not a
// hardware hazard -- was the "wrong bits" of round 2's scalar bit window in the decode walk (the ISA showed
// s_ashr_i32 hi, lo, 31 in front of the s_or_b64 that slides the window; tests/test_build_invariants.py
// keeps both out of decode.hip).  decode.hip uses this wrapper only.
__device__ __forceinline__ unsigned fq_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }

// LDS ordering inside ONE wave (single-wave workgroups): the LDS executes a wave's
// instructions in order, so all that is needed is that earlier LDS operations have completed
// and that the compiler does not move LDS accesses across this point.  __syncthreads() would
// also drain vmcnt(0) -- every outstanding global load AND store -- once per loop iteration.
__device__ __forceinline__ void fq_lds_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs (each with its own
// 4 MiB L2), so with the identity mapping neighbouring tiles never share an L2.  This
// bijective remap gives every XCD a contiguous range of tiles, walked in order: tiles that
// run at the same time on one XCD then touch adjacent bytes of every context's run and the
// partial lines of the permutation passes are completed inside L2 instead of in HBM.
__device__ __forceinline__ unsigned fq_xcd_tile(unsigned b, unsigned n) {
  const unsigned q = n >> 3, r = n & 7u, xcd = b & 7u, idx = b >> 3;
  return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
}

// number of set bits of m below the calling lane
__device__ __forceinline__ unsigned fq_mbcnt(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// lanes of the wave holding the same key as the caller (among valid lanes).
// The partition loops are VALU-bound on this function (SQ counters: 164 VALU instructions per
// 64-symbol iteration for 13-bit keys), so it is written for instruction count: the per-lane
// mask is kept as two 32-bit halves of MISMATCH bits, two key bits are folded per v_or3.
template <int BITS>
__device__ __forceinline__ unsigned long long fq_match_any(unsigned key, bool valid) {
  const unsigned long long vm = __ballot(valid);
  unsigned mis_lo = 0, mis_hi = 0;  // lanes whose key differs from mine in some bit
#pragma unroll
  for (int b = 0; b + 1 < BITS; b += 2) {
    const int m0 = __builtin_amdgcn_sbfe((int)key, b, 1), m1 = __builtin_amdgcn_sbfe((int)key, b + 1, 1);  // 0 / -1
    const unsigned long long b0 = __ballot(m0 != 0), b1 = __ballot(m1 != 0);
    mis_lo |= ((unsigned)b0 ^ (unsigned)m0) | ((unsigned)b1 ^ (unsigned)m1);
    mis_hi |= ((unsigned)(b0 >> 32) ^ (unsigned)m0) | ((unsigned)(b1 >> 32) ^ (unsigned)m1);
  }
  if (BITS & 1) {
    const int m0 = __builtin_amdgcn_sbfe((int)key, BITS - 1, 1);
    const unsigned long long b0 = __ballot(m0 != 0);
    mis_lo |= (unsigned)b0 ^ (unsigned)m0;
    mis_hi |= (unsigned)(b0 >> 32) ^ (unsigned)m0;
  }
  return vm & ~(((unsigned long long)mis_hi << 32) | mis_lo);
}

// A0 C1 G2 T3, everything else (N, which the coder treats as A: src/fse_sequence.cpp:44) -> 0
// (three independent selects: the nested form compiles to a chain of exec-mask branches, five
// times per symbol in K1)
__device__ __forceinline__ unsigned fq_base_code(unsigned c) {
  return (c == 'C' ? 1u : 0u) | (c == 'G' ? 2u : 0u) | (c == 'T' ? 3u : 0u);
}
// The reference's base2bits_arr (src/fse_sequence.cpp:6-14) maps everything but A, C, G, T to
// UINT_MAX -- lowercase, IUPAC codes, '.', a stray '\r' index out of its tables (assert / UB); N is
// legal because replaceAndEncodeNs (:35-51) has turned it into 'A' before.  A lossless coder must
// not code such a byte as 'A' silently: symbol code as above, 4 for a byte that is not a base.
__device__ __forceinline__ unsigned fq_base_sym(unsigned c) {
  return (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') ? fq_base_code(c) : 4u;
}
// the same with bit 6 set for 'N' (K1 of the tile-sorted path counts the N's of every read on the way)
constexpr unsigned FQ_SYM_IS_N = 0x40u, FQ_SYM_BAD_MASK = 0x3Cu;
__device__ __forceinline__ unsigned fq_base_sym_n(unsigned c) { return fq_base_sym(c) | (c == 'N' ? FQ_SYM_IS_N : 0u); }

// FSE_Quality::calcContext (src/fse_quality.h:40-44)
__device__ __forceinline__ unsigned fq_qual_ctx(unsigned q, unsigned q1, unsigned q2) {
  unsigned ctx = ((((q1 > q2) ? q1 : q2) << 6) + q) & 0xFFFu;
  ctx += (unsigned)(q1 == q2) << 12;
  return ctx;
}

// largest r in [lo, hi] with rec_start[r] <= e
__device__ __forceinline__ unsigned fq_locate(const uint32_t *__restrict__ rec_start, unsigned lo,
                                              unsigned hi, unsigned e) {
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1) >> 1);
    if (rec_start[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Decode index of stream M of a block as it lies in raw / recs (the block the encoder coded, or the restored one), everything
// but bit positions and states.  k = 0: the header.  k = 1 .. n_snap: the `prev` bytes of snapshot k -- symbol k stride - 1 is
// position p of record r (encode order walks a record from its last position), the four bytes in front of it -- and the
// reserved word; returns the snapshot.  nullptr: nothing left for the caller to write.
template <class M>
__device__ __forceinline__ uint8_t *fq_index_write_meta(uint8_t *index, unsigned k, unsigned n_sym, unsigned stride, const uint8_t *raw,
                                                        const fqgpu_rec *recs, const uint32_t *rec_start, unsigned R) {
  const unsigned n_snap = fq_index_n_snap(n_sym, stride);
  if (k == 0) {
    FqIndexHeader h;
    h.magic = FQ_INDEX_MAGIC; h.stream = M::STREAM; h.stride = stride; h.n_snap = n_snap;
    h.n_sym = n_sym; h.reserved = 0;
    *reinterpret_cast<FqIndexHeader *>(index) = h;
    return nullptr;
  }
  if (k > n_snap) return nullptr;
  const unsigned e = k * stride;
  uint8_t *snap = fq_index_snap(index, M::B, k);
  const unsigned r = fq_locate(rec_start, 0, R - 1, e - 1);
  const fqgpu_rec rec = recs[r];
  const unsigned p = rec.len - 1u - (e - 1u - rec_start[r]);
  const uint8_t *line = raw + (M::STREAM == 0 ? rec.seq_off : rec.qual_off);
  unsigned packed = 0;
  for (unsigned i = 0; i < 4; i++) packed |= (p >= i + 1 ? (unsigned)line[p - 1 - i] : 0xFFu) << (8 * i);
  reinterpret_cast<uint32_t *>(snap)[2] = packed;
  reinterpret_cast<uint32_t *>(snap)[3] = 0;
  return snap;
}

// ---- (context, symbol) of position p of a record, encode-side definition, in two halves so
// that callers can issue the loads of the NEXT chunk before they consume (and store results
// of) the current one: vmcnt retires in order, a store between two loads would serialise them.
//   sequence (SequenceEncoder::encodeRecord src/fse_sequence.cpp:53-112): context = the four
//     bases in front of p, nearest in bits 7:6, virtual T,C,C,T = 0xD7 before the read
//   quality (QualityEncoder::encodeRecord src/fse_quality.cpp:5-53, L >= 3): context of p is
//     calcContext(Q[p-1], Q[p-2], Q[p-3]) with zeros in front of the read
// The symbol at position p of a read and the up to four (three) symbols in front of it, as the
// raw bytes q .. q + 7 (q .. q + 3) of the line with q = max(p, 4) - 4 (max(p, 3) - 3): ONE
// unaligned load per symbol instead of five (four) byte loads with an address computation each --
// K1 is bound by instruction issue.
struct SymBytes {
  unsigned lo, hi;  // bytes q .. q + 3, q + 4 .. q + 7 (hi: sequence stream only)
};
struct __attribute__((packed)) FqU32x2 { uint32_t a, b; };  // eight bytes at any address
struct __attribute__((packed)) FqU32x1 { uint32_t a; };

template <class M>
__device__ __forceinline__ SymBytes fq_load_sym_bytes(const uint8_t *__restrict__ raw, const fqgpu_rec &rec,
                                                      unsigned p, bool valid) {
  // Unconditional loads (an idle lane has rec = {0, 0, 0}, p = 0 and reads the first bytes of the
  // block; a read's last positions read a few bytes of what follows its line: the block has 64
  // spare bytes behind raw): straight-line code lets the compiler keep several chunks' loads in flight.
  (void)valid;
  constexpr unsigned K = M::STREAM == 0 ? 4u : 3u;
  const uint8_t *s = raw + (M::STREAM == 0 ? rec.seq_off : rec.qual_off) + (p > K ? p - K : 0u);
  SymBytes r;
  if (M::STREAM == 0) {
    const FqU32x2 v = *reinterpret_cast<const FqU32x2 *>(s);
    r.lo = v.a; r.hi = v.b;
  } else {
    r.lo = reinterpret_cast<const FqU32x1 *>(s)->a; r.hi = 0;
  }
  return r;
}

// Context and symbol of position p from its window (fq_load_sym_bytes), without a branch or a
// compare: K1 is bound by instruction issue, and "p >= k ? code(byte k) : virtual" compiled to four
// exec-mask branches plus fifteen compare/select pairs per symbol.
//  sequence: the bytes in front of the symbol are shifted to the top of a word (missing ones
//            become 0), every byte goes through a 256-entry code table in LDS (exactly
//            fq_base_code: 0 for anything but C, G, T -- so missing bytes add nothing), and the
//            virtual bases in front of the read are 0xD7 >> 2 p (src/fse_sequence.h:22-24 applied p times)
//  quality:  33 is subtracted from all four bytes at once (a byte < 33 borrows from its upper
//            neighbour, but then the block is refused anyway: that byte is somebody's symbol >= 64)
//            The SYMBOL goes through a second table (sym_lut = fq_base_sym): 4 for a byte that is
//            no base at all, which the caller turns into FQGPU_E_ARG -- same instruction count.
template <class M>
__device__ __forceinline__ void fq_ctx_from_bytes(const SymBytes &r, unsigned p, unsigned &ctx, unsigned &sym,
                                                  const uint8_t *code_lut, const uint8_t *sym_lut) {
  constexpr unsigned K = M::STREAM == 0 ? 4u : 3u;
  const unsigned pq = min(p, K), sh = 8u * pq;  // the symbol is byte pq of the window
  if (M::STREAM == 0) {
    const unsigned long long w = ((unsigned long long)r.hi << 32) | r.lo;
    sym = sym_lut[(unsigned)(w >> sh) & 0xFFu];
    const unsigned prev = (unsigned)((unsigned long long)r.lo << (32u - sh));  // bytes p-1 | p-2 | p-3 | p-4
    ctx = ((unsigned)code_lut[prev >> 24] << 6) | ((unsigned)code_lut[(prev >> 16) & 0xFFu] << 4) |
          ((unsigned)code_lut[(prev >> 8) & 0xFFu] << 2) | (unsigned)code_lut[prev & 0xFFu] | (0xD7u >> (2u * pq));
  } else {
    (void)code_lut; (void)sym_lut;
    const unsigned w33 = r.lo - 0x21212121u;
    sym = (w33 >> sh) & 0xFFu;
    const unsigned prev = (unsigned)((unsigned long long)w33 << (32u - sh));  // q | q1 | q2 | -
    ctx = fq_qual_ctx((prev >> 24) & 63u, (prev >> 16) & 63u, (prev >> 8) & 63u);
  }
}

#endif  // __HIPCC__
