// The shape of one (block, stream) coding job of encode.hip, computed once: every derived size, every scratch buffer's
// byte size and the offset of every sub-array inside a buffer.  Reserving ahead (fqgpu_ctx_reserve) and launching read the
// SAME plan, so "what reserve allocates" is "what a launch needs" by construction, and a sub-array's offset is written in
// one place.  Plain C++ without HIP types: tests/cpp/enc_plan_check.cpp holds the numbers against a recorded table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/fqgpu.h"

// ---- constants the kernels (enc_*.h) and the plan share
constexpr unsigned TILE_SEQ = 32768;   // symbols per partition tile of the slot path (one wave each in K3)
constexpr unsigned TILE_QUAL = 65536;
constexpr unsigned TS_TILE = 32768;    // symbols per tile of the tile-sorted path (lpos16 and the 16-bit cursors hold 0 .. 32768)
constexpr unsigned GROUP_TILES = 64;   // tiles per group in the two-level tile scan
constexpr unsigned PACK_TILE = 4096;   // symbols per bit-packing tile
constexpr unsigned CTX_PAD = 16;       // every context's sorted run starts 16-aligned
constexpr unsigned SC_BATCH_SEQ = 8192;  // sequence: 32 bytes per context and batch
constexpr unsigned SETS_WAVES = 8;          // segments (waves) per workgroup in step A, one-symbol table
constexpr unsigned SETS_WAVES2 = 16;        // ... with the 64 KB two-symbol table (one workgroup per CU)
constexpr unsigned SETS_ROUNDS = 4;         // a workgroup owns WAVES * max(SETS_ROUNDS / group, 1) groups, handed out to its waves one by one
constexpr unsigned SETS_MAX_GROUP = 16;     // segments a wave walks in one go, at most
constexpr unsigned SETS_BLOCK = 1024;       // symbols per 16-byte-per-lane load; S is a multiple
constexpr unsigned SEQ_CAND_MAX = 64;        // candidates of a handed-over group, at most (one wave-instruction)
// plan[]: fitem_base[B+1] (step A workgroups before every context) | fseg_base[B+1] (functions
// before every context) | seg_base[B+1] (segments) | eitem_base[B+1] (step C waves) |
// citem_base[B+1] (step B items: 64 groups each, for chains of more than SEQ_ITEM_GROUPS groups)
constexpr unsigned SEGPLAN_WORDS = 5 * (FQGPU_SEQ_MODELS + 1) + 4;  // + the work counter of step A
constexpr unsigned SEQ_ITEM_GROUPS = 64;
constexpr unsigned SEG_MAX_CAND = 64;  // candidates of an anchored segment, at most (enc_chains_generic.h)
constexpr unsigned SEG_SLOT = 16;  // lanes of one candidate walk: four walks share a wave

// A sub-array of a buffer, and the carver that hands them out one behind the other
struct EncSpan {
  size_t off = 0, bytes = 0;
};
struct EncCarve {
  size_t total = 0;
  EncSpan take(size_t bytes, size_t align = 1) {
    EncSpan s;
    s.off = (total + align - 1) & ~(align - 1);
    s.bytes = bytes;
    total = s.off + bytes;
    return s;
  }
};

// Bytes reserved per EncScratch buffer (0: this path does not use it)
struct EncBytes {
  size_t slot_of = 0;        // slot path: u32 [n_pad] sorted position of every symbol; tile path: lpos16, u16 [n_pad] position inside the tile's run
  size_t keys = 0;           // ckey | csym (below); dead after K3, then enc16 u16 [n_pad] over both
  size_t sorted_sym = 0;     // u8 [padded]
  size_t out16 = 0;          // u16 [padded] (nb << 12 | bits) at sorted position
  size_t tile_hist = 0;      // [tiles][B], u16 on the tile path, u32 on the slot path (sized for u32 on both)
  size_t tile_base = 0;      // u32 [tiles][B]
  size_t group_sum = 0;      // u32 [groups][B]
  size_t ctx_arrays = 0;     // ctx_count | ctx_start | seg_base | item_base (below)
  size_t seg_state = 0;      // u16 final_state[B], then 8 bytes per context of the generic walks
  size_t seg_arrays = 0;     // generic chains: SegArrays, then ItemArrays (below)
  size_t seq_plan = 0;       // sequence chains: plan words | entry states (below)
  size_t seq_fbuf = 0;       // u16 [functions][1 << max_log] segment functions (generic chains: + one power table per context)
  size_t seq_cbuf = 0;       // sequence chains: composed functions | entry states of the items of long chains (below)
  size_t seq_cand = 0;       // sequence chains: cand0 | cand (below)
  size_t seq_bdesc = 0;      // batch-sorted sequence partition: SeqBatchDesc start | pre (below)
  size_t tile_bits = 0;      // u32 [ptiles]
  size_t tile_bit_base = 0;  // u64 [ptiles + 1]
  size_t tile_runs = 0;      // tile path: uint2 [tiles][min(B, tile)] run list of every tile
  size_t tile_sync = 0;      // tile path: status | counter | run counts | edge words (below)
};

// What follows from the block's size, the model and the tile alone (fq_qual_counts_sorted needs no more)
struct EncShape {
  unsigned n_sym = 0, R = 0, B = 0, T = 0;
  unsigned n_tiles = 0, n_groups = 0, n_ptiles = 0;
  size_t n_pad = 0;   // symbols padded by one batch, a multiple of 16: keeps every sub-array of `keys` 16-byte aligned
  size_t padded = 0;  // sorted symbols: every context's run 16-aligned
  size_t lpos16_bytes = 0, tile_runs_bytes = 0;  // the tile path's slot_of (u16 [n_pad]) and tile_runs (uint2 [tiles][min(B, tile)]: ts_run_stride)
  EncBytes bytes;
  EncSpan ckey, csym;  // keys: u16 [n_pad] context | u8 [n_pad] symbol (quality; the fused K1 writes contexts alone)
  EncSpan ctx_count, ctx_start, seg_base;  // ctx_arrays (item_base behind them: the host never addresses it): u32 [B] | [B+1] | [B+1] | [B+1] (k_ctx_layout: arrays, + B, + B + 1 ...)

  EncShape() = default;
  EncShape(unsigned n_sym_, unsigned R_, unsigned B_, unsigned T_) : n_sym(n_sym_), R(R_), B(B_), T(T_) {
    n_tiles = (n_sym + T - 1) / T;
    n_groups = (n_tiles + GROUP_TILES - 1) / GROUP_TILES;
    n_ptiles = (n_sym + PACK_TILE - 1) / PACK_TILE;
    n_pad = ((size_t)n_sym + SC_BATCH_SEQ + 15) & ~(size_t)15;
    padded = (size_t)n_sym + (size_t)CTX_PAD * B + 64;
    lpos16_bytes = n_pad * 2;
    tile_runs_bytes = (size_t)n_tiles * std::min(B, TS_TILE) * 8;
    EncCarve k, a;
    ckey = k.take(n_pad * 2);
    csym = k.take(n_pad);
    bytes.keys = k.total;
    bytes.sorted_sym = padded;
    bytes.tile_hist = bytes.tile_base = (size_t)n_tiles * B * 4;
    bytes.group_sum = (size_t)n_groups * B * 4;
    ctx_count = a.take((size_t)B * 4);
    ctx_start = a.take((size_t)(B + 1) * 4);
    seg_base = a.take((size_t)(B + 1) * 4);
    a.take((size_t)(B + 1) * 4);
    bytes.ctx_arrays = a.total;
  }
};

struct EncPlanIn {
  unsigned n_sym = 0, R = 0;
  int stream = 0;  // 0 = sequence, 1 = quality
  unsigned B = 0, A = 0, max_log = 0;
  bool two_sym = false;  // two-symbol transition tables exist (sequence stream, max_log <= 11)
  bool tile_path = false, serial_seq = false;
  unsigned seg_len = 0, seq_segment = 0, seq_group = 0, seq_group_min = 0, seq_cand_cap = 0, seq_cand_prefix = 0, n_cus = 0;  // the handle's
};

struct EncPlan : EncShape {
  bool tile_path = false, serial_seq = false, two_sym = false;
  unsigned max_log = 0;
  unsigned S = 0;      // segment of the generic chain kernels
  unsigned seq_S = 0;  // segment of the sequence chain kernels
  unsigned max_items = 0, gen_max_segs = 0, seq_max_segs = 0;
  unsigned fstride = 0;      // u16 per segment function (both chain kinds)
  unsigned next_stride = 0;  // u16 per one-symbol transition table
  unsigned gen_pbase = 0;    // generic chains' function slots: one per segment, then one power table per context
  unsigned cand_grid = 0;    // workgroups of the generic chains' candidate walks
  unsigned cand_cap = 0, cand_W = 0, cand_P = 0;  // hand-over of collapsed groups (two-symbol tables only): cap, slots per group, prefix
  unsigned wpg = 0, Q = 0, gmin = 0, rounds = 0;  // k_seq_setfunc: waves per workgroup, group, groups a chain keeps, rounds
  unsigned max_fitems = 0, max_eitems = 0, max_citems = 0;
  unsigned lds_ct = 0;  // LDS of the kernels that keep one context's CTable there

  EncSpan sa_anchor, sa_usym, sa_entry, sa_cand, sa_cls;  // seg_arrays: SegArrays, every array 16-byte aligned ...
  EncSpan ia_has_g, ia_entry, ia_g;                       // ... then ItemArrays
  EncSpan sp_fitem, sp_seg, sp_work, sp_entry;  // seq_plan: of the SEGPLAN_WORDS (k_seq_segplan) the bases the host hands out | u16 entry [segments]
  EncSpan cb_func, cb_item_entry;  // seq_cbuf: u16 [items][fstride] | u16 [items]
  EncSpan cand0, cand;             // seq_cand: u16 [segments][W] twice (SeqHandover)
  EncSpan bd_start, bd_pre;        // seq_bdesc: u32 [ptiles + 1][B] | u16 [ptiles + 1][B] (SeqBatchDesc)
  EncSpan ts_status, ts_counter, ts_run_count, ts_edges;  // tile_sync: u64 [tiles] | ticket counter, pad | u32 [tiles] | uint4 [tiles] (16-aligned)

  EncPlan() = default;
  explicit EncPlan(const EncPlanIn &in)
      : EncShape(in.n_sym, in.R, in.B, in.tile_path ? TS_TILE : in.stream == 0 ? TILE_SEQ : TILE_QUAL),
        tile_path(in.tile_path), serial_seq(in.serial_seq), two_sym(in.two_sym), max_log(in.max_log) {
    const auto whole_blocks = [](unsigned s) { return (unsigned)std::min(((size_t)s + SETS_BLOCK - 1) / SETS_BLOCK * SETS_BLOCK, (size_t)1 << 30); };
    // Generic chains: 4096 symbols by default; shorter for small blocks, which are chains of short, latency-bound kernels (a
    // lane of the walk/emit kernels walks one segment): 16 MiB blocks +8 %, 4 MiB blocks +25 % with 1024-2048 (measured)
    S = whole_blocks(in.seg_len ? in.seg_len : n_sym >= (24u << 20) ? 4096u : n_sym >= (4u << 20) ? 2048u : 1024u);
    // Sequence chains: a lane of k_seq_emit walks one whole segment, so the kernel's length grows with the segment -- blocks
    // of 64 MiB and less gained 4 % from 2048-symbol segments, 256 MiB blocks nothing (measured with the kernel that emitted
    // 16 symbols per round; not measured again with the 64-symbol rounds, which left the walk one lane per segment).
    // The result never depends on either length.
    seq_S = whole_blocks(in.seq_segment ? in.seq_segment : n_sym >= (48u << 20) ? 4096u : n_sym >= (4u << 20) ? 2048u : 1024u);
    max_items = (unsigned)((size_t)n_sym / ((size_t)S * 64) + B + 1);
    gen_max_segs = n_sym / S + B + 1;
    seq_max_segs = n_sym / seq_S + B + 1;
    fstride = 1u << max_log;
    next_stride = 4u << max_log;
    gen_pbase = gen_max_segs;
    cand_grid = std::min(gen_max_segs / (64 / SEG_SLOT) + 1, 32u * in.n_cus);
    cand_cap = serial_seq && two_sym ? std::min(in.seq_cand_cap, SEQ_CAND_MAX) : 0u;
    cand_W = cand_cap == 0 ? 0u : cand_cap <= 16 ? 16u : cand_cap <= 32 ? 32u : 64u;
    cand_P = std::min(std::max(in.seq_cand_prefix, 1u), SETS_MAX_GROUP);
    wpg = two_sym ? SETS_WAVES2 : SETS_WAVES;
    Q = std::min(std::max(in.seq_group, 1u), SETS_MAX_GROUP);
    gmin = std::max(in.seq_group_min, 1u);
    rounds = std::max(SETS_ROUNDS / Q, 1u);
    max_fitems = seq_max_segs / (wpg * rounds) + B + 1;
    max_eitems = seq_max_segs / 64 + B + 1;
    max_citems = seq_max_segs / SEQ_ITEM_GROUPS + B + 1;
    lds_ct = (1u + (1u << (max_log - 1)) + 2u * in.A) * 4u;

    bytes.slot_of = tile_path ? lpos16_bytes : n_pad * 4;
    bytes.out16 = padded * 2;
    bytes.seg_state = (size_t)B * 2 + (size_t)B * 8;
    bytes.tile_bits = (size_t)n_ptiles * 4;
    bytes.tile_bit_base = (size_t)(n_ptiles + 1) * 8;

    const size_t gs = gen_max_segs;
    EncCarve g;
    sa_anchor = g.take(gs * 4, 16);
    sa_usym = g.take((size_t)B * 4, 16);
    sa_entry = g.take(gs * 2, 16);
    sa_cand = g.take(gs * SEG_MAX_CAND * 2, 16);
    sa_cls = g.take(gs, 16);
    ia_has_g = g.take((size_t)max_items * 4, 16);
    ia_entry = g.take((size_t)max_items * 2, 16);
    ia_g = g.take((size_t)max_items * fstride * 2, 16);
    g.take(64);
    EncCarve sp, cb, cd, bd, ts;
    const size_t base_bytes = (size_t)(FQGPU_SEQ_MODELS + 1) * 4;
    sp_fitem = sp.take(2 * base_bytes);  // (fitem_base | fseg_base)
    sp_seg = sp.take(3 * base_bytes);    // (seg_base | eitem_base | citem_base)
    sp_work = sp.take(16);
    sp_entry = sp.take((size_t)seq_max_segs * 2);
    sp.take(64);
    cb_func = cb.take((size_t)max_citems * fstride * 2);
    cb_item_entry = cb.take((size_t)max_citems * 2);
    cb.take(64);
    cand0 = cd.take((size_t)seq_max_segs * cand_W * 2);
    cand = cd.take((size_t)seq_max_segs * cand_W * 2);
    cd.take(64);
    bd_start = bd.take((size_t)(n_ptiles + 1) * FQGPU_SEQ_MODELS * 4);
    bd_pre = bd.take((size_t)(n_ptiles + 1) * FQGPU_SEQ_MODELS * 2);
    bd.take(64);
    ts_status = ts.take((size_t)n_tiles * 8);
    ts_counter = ts.take(16);
    ts_run_count = ts.take((size_t)n_tiles * 4);
    ts_edges = ts.take((size_t)n_tiles * 16, 16);
    if (serial_seq) {
      bytes.seq_plan = sp.total;
      bytes.seq_fbuf = (size_t)seq_max_segs * fstride * 2 + 64;
      bytes.seq_cand = cand_W ? cd.total : 0;
      bytes.seq_cbuf = cb.total;
      bytes.seq_bdesc = bd.total;
    } else {
      bytes.seg_arrays = g.total;
      bytes.seq_fbuf = ((size_t)gen_max_segs + B) * fstride * 2 + 64;
    }
    if (tile_path) {
      bytes.tile_runs = tile_runs_bytes;
      bytes.tile_sync = ts.total;
    }
  }
};

// The lane-level buffers of one block (EncLane)
struct EncLanePlan {
  size_t rec_start = 0;   // u32 [R + 1]
  size_t n_cnt32 = 0;     // n_cnt | lens
  size_t n_off = 0;       // u32 [R + 1]
  size_t first_sym = 0;   // first_sym_of[0] | [1], pad
  size_t tile_first = 0;  // u32 [tiles of the tile-sorted path]
  size_t scan_tmp = 0;    // ahead of time only: an upper bound of what the record scans (scan.hip) size themselves at a launch
  EncSpan n_cnt, lens;      // n_cnt32: u32 [R] N count | u32 [R] length
  EncSpan first_sym_of[2];  // first_sym: u8 [R] sequence | u8 [R] quality

  EncLanePlan(unsigned R, size_t n_bases) {
    EncCarve c, f;
    rec_start = n_off = (size_t)(R + 1) * 4;
    n_cnt = c.take((size_t)R * 4);
    lens = c.take((size_t)R * 4);
    n_cnt32 = c.total;
    first_sym_of[0] = f.take(R);
    first_sym_of[1] = f.take(R);
    f.take(16);
    first_sym = f.total;
    tile_first = (n_bases + TS_TILE - 1) / TS_TILE * 4;
    scan_tmp = ((size_t)R / 1024 + 64) * 16;
  }
};
