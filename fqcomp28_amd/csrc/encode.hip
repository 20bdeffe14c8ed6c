// Bit-exact parallel encoder of one (block, stream) -- replaces the per-record
// loop of CompressionWorkspace::encodeChunk (reference src/workspace.cpp:25-31)
// with its SequenceEncoder::encodeRecord (src/fse_sequence.cpp:53-112) /
// QualityEncoder::encodeRecord (src/fse_quality.cpp:5-53) bodies and
// FSE_Encoder::startChunk/endChunk (src/fse_common.hpp:77-90).
//
// The reference interleaves one tANS state per context into ONE bitstream:
//   for every symbol e in encode order (records in file order, positions L-1..0):
//       emit low nb(e) bits of state[ctx(e)];  state[ctx(e)] = T[ctx(e)][sym(e)](state)
//   then flush all states (ctx ascending), one '1' end-mark bit, zero pad.
// ctx(e)/sym(e) depend on the INPUT only, each context's state chain only on the
// symbols of that context.  Hence the decomposition:
//   K1 tile_hist / K2 layout : counting sort keys = context, per-tile histograms + scan
//   K3 scatter               : stable partition of the symbols by context (rank inside a
//                              (tile, context) = one lane-ordered LDS atomic per symbol); the
//                              sequence stream sorts every 4 K batch by context in LDS and
//                              writes runs instead of scattered bytes
//   K4 chains                : a tANS encoder state never forgets its history completely, but
//                              the SET of states it can be in collapses fast.  A chain is cut
//                              into segments of 4096 symbols; the state is known without its
//                              past right after a symbol whose normalised count is 1 or -1 (one
//                              table cell: "reset"), and for a segment without such a symbol
//                              one wave computes the segment's FUNCTION entry state -> exit
//                              state for every possible entry state over collapsing state sets.
//                              Entry states follow by applying the functions along the chain;
//                              then one lane per segment emits (nb, bits).  No serial chain,
//                              no speculation.
//   K6 bitcount/scan/pack    : per-symbol (nb,bits) brought back into encode order (quality:
//                              gather by slot; sequence: runs of the batch read into LDS),
//                              exclusive scan of nb = bit offsets, bit packing through LDS
//   K7 epilogue              : state flush + end mark + size/overflow
#include "fqgpu_internal.h"
#include "enc_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifdef FQGPU_EXPERIMENTS
__device__ unsigned long long g_ts_prof[48];  // [32 ..]: K3's loader clock (thread 64), eight slots per stream
void fq_ts_prof_dump() {
  unsigned long long h[48];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ts_prof), sizeof(h)) != hipSuccess) return;
  const char *names[4] = {"partition<Qual>", "partition<Seq>", "gather_pack<Qual>", "gather_pack<Seq>"};
  for (int k = 0; k < 4; k++)
    fprintf(stderr, "ts_prof %-18s phase ticks (100 MHz, summed over workgroups): %llu %llu %llu %llu | ranker alone %llu | K3: store wait %llu patch %llu run map %llu\n",
            names[k], h[8 * k], h[8 * k + 1], h[8 * k + 2], h[8 * k + 3], h[8 * k + 4], h[8 * k + 5], h[8 * k + 6], h[8 * k + 7]);
  for (int k = 0; k < 2; k++)
    fprintf(stderr, "ts_prof %-18s loader thread 64, ticks summed over workgroups: wait for the requested batch (taken in front of finish) %llu | finish %llu | deposit %llu | request %llu | barrier %llu\n",
            names[k], h[32 + 8 * k], h[33 + 8 * k], h[34 + 8 * k], h[35 + 8 * k], h[36 + 8 * k]);
}
#endif

namespace {

constexpr unsigned PACK_THREADS = 256;
constexpr unsigned PACK_PER_THREAD = PACK_TILE / PACK_THREADS;  // 16

#include "enc_records_hist.h"
#include "enc_partition.h"
#include "enc_chains_seq.h"
#include "enc_chains_generic.h"
#include "enc_gather.h"
#include "enc_seq_batch.h"
#include "enc_index.h"
#include "enc_pack.h"
#include "enc_tile_sort.h"

// ------------------------------------------------------------------ host orchestration

// Timing experiments (tools/traffic_experiment.py) exist only in a library built with
// -DFQGPU_EXPERIMENTS (make experiments -> tools/_build/libfqgpu_experiments.so); the product
// library contains none of these switches.  FQGPU_DEBUG_SKIP = bit mask of kernel groups that are
// NOT launched (their outputs keep the values of the previous encode of the same lane: wrong output
// by design); FQGPU_DEBUG_NO_SYM_STORE: 1 = both streams, 2 = sequence only, 3 = quality only.
#ifdef FQGPU_EXPERIMENTS
static int fq_debug_no_sym(int stream) {
  const char *e = getenv("FQGPU_DEBUG_NO_SYM_STORE");
  const int v = e ? atoi(e) : 0;
  return v == 1 || (v == 2 && stream == 0) || (v == 3 && stream == 1);
}
static unsigned fq_debug_skip() {
  const char *e = getenv("FQGPU_DEBUG_SKIP");
  return e ? (unsigned)strtoul(e, nullptr, 0) : 0u;
}
static int fq_debug_k1() { const char *e = getenv("FQGPU_DEBUG_K1"); return e ? atoi(e) : 0; }
static bool fq_debug_flag(const char *name) { return getenv(name) != nullptr; }
// FQGPU_DEBUG_SKIPK=name,name,...: single kernels that are not launched (k1 k3s k3q setfunc resolve emit scan stage1 heads qresolve walk2 k6s k6q k2s k2q)
static bool fq_debug_skipk(const char *name) {
  const char *e = getenv("FQGPU_DEBUG_SKIPK");
  if (!e) return false;
  const size_t n = strlen(name);
  for (const char *p = e; (p = strstr(p, name)) != nullptr; p += n)
    if ((p == e || p[-1] == ',') && (p[n] == 0 || p[n] == ',')) return true;
  return false;
}
#else
static constexpr int fq_debug_no_sym(int) { return 0; }
static constexpr unsigned fq_debug_skip() { return 0u; }
static constexpr int fq_debug_k1() { return 0; }
static constexpr bool fq_debug_flag(const char *) { return false; }
static constexpr bool fq_debug_skipk(const char *) { return false; }
#endif

// true: both streams take the tile-sorted path, so K1 can run once for both (k_tile_hist2)
static bool fused_k1(const fqgpu_ctx *ctx) {
  return ctx->lds_atomics_ordered && ctx->tile_sorted && !ctx->seq_generic && !fq_debug_skip() && !fq_debug_k1();
}
// timing experiments that skip K1 or its stores: enc16 apart from the keys, so that stale keys stay valid
static bool dbg_no_alias() {
  static const bool on = fq_debug_flag("FQGPU_DEBUG_NO_ALIAS");
  return on;
}

// One stage of a pipeline: its timing span (tools/ and bench.py read the names) and whether an experiment switch takes its
// kernels out -- bit `bit` of the stream's FQGPU_DEBUG_SKIP mask, or `skipk` named in FQGPU_DEBUG_SKIPK.  The span ends
// with the stage:  if (EncStage s{ctx, st, "name", mask, bit}; !s.off) launch(...);
struct EncStage {
  fqgpu_ctx *ctx;
  hipStream_t st;
  bool off;
  EncStage(fqgpu_ctx *c, hipStream_t s, const char *span, unsigned mask = 0, unsigned bit = 0, const char *skipk = nullptr)
      : ctx(c), st(s), off((mask & bit) != 0 || (skipk && fq_debug_skipk(skipk))) { fq_timer_span_begin(ctx, span, st); }
  ~EncStage() { fq_timer_span_end(ctx, st); }
  EncStage(const EncStage &) = delete;
};
#define FQ_SPAN(x) (M::STREAM ? "qual." x : "seq." x)

// ---- the plan of one (block, stream) from the handle's settings (enc_plan.h), what it reserves, and typed views of it
template <class M>
EncPlan make_plan(const fqgpu_ctx *ctx, const fqgpu_dblock *b) {
  const DevTables &tab = ctx->tab[M::STREAM];
  EncPlanIn in;
  in.n_sym = (unsigned)b->n_bases;
  in.R = (unsigned)b->n_recs;
  in.stream = M::STREAM; in.B = M::B; in.A = M::A;
  in.max_log = tab.max_log;
  in.two_sym = tab.next2 != nullptr;  // two-symbol tables exist up to log 11
  in.serial_seq = M::STREAM == 0 && !ctx->seq_generic;
  // tile-sorted partition + fused gather/pack: whenever the rank may come from lane-ordered LDS atomics
  // (the generic sequence mode keeps the slot-based kernels: it exists for comparisons only)
  in.tile_path = ctx->lds_atomics_ordered && ctx->tile_sorted && (M::STREAM == 1 || in.serial_seq);
  in.seg_len = ctx->seg_len; in.seq_segment = ctx->seq_segment;
  in.seq_group = ctx->seq_group; in.seq_group_min = ctx->seq_group_min;
  in.seq_cand_cap = ctx->seq_cand_cap; in.seq_cand_prefix = ctx->seq_cand_prefix;
  in.n_cus = ctx->n_cus;
  return EncPlan(in);
}
static_assert(TILE_SEQ % SEQ_BATCH == 0 && SEQ_BATCH % PACK_TILE == 0 && TILE_QUAL % PACK_TILE == 0, "a packing tile lies inside one partition tile");
static_assert(ts_run_stride<SeqModel>() == (unsigned)SeqModel::B && ts_run_stride<QualModel>() == (unsigned)QualModel::B, "EncPlan sizes tile_runs by min(B, TS_TILE)");

// keys and tile histograms of one stream exist before its pipeline starts (fused K1)
static int reserve_k1(EncScratch &sc, const EncShape &sh) {
  int rc;
  if ((rc = sc.keys.reserve(sh.bytes.keys))) return rc;
  return sc.tile_hist.reserve(sh.bytes.tile_hist);
}
// every scratch buffer of one stream at the plan's size (0: the path does not use the buffer)
static int reserve(EncScratch &sc, const EncPlan &p) {
  const EncBytes &n = p.bytes;
  const struct { DevBuf &buf; size_t bytes; } want[] = {
      {sc.slot_of, n.slot_of}, {sc.keys, n.keys}, {sc.sorted_sym, n.sorted_sym}, {sc.out16, n.out16}, {sc.tile_hist, n.tile_hist},
      {sc.tile_base, n.tile_base}, {sc.group_sum, n.group_sum}, {sc.ctx_arrays, n.ctx_arrays}, {sc.seg_state, n.seg_state},
      {sc.seg_arrays, n.seg_arrays}, {sc.seq_plan, n.seq_plan}, {sc.seq_fbuf, n.seq_fbuf}, {sc.seq_cand, n.seq_cand},
      {sc.seq_cbuf, n.seq_cbuf}, {sc.seq_bdesc, n.seq_bdesc}, {sc.tile_bits, n.tile_bits}, {sc.tile_bit_base, n.tile_bit_base},
      {sc.tile_runs, n.tile_runs}, {sc.tile_sync, n.tile_sync}, {sc.dbg_enc16, dbg_no_alias() ? p.n_pad * 2 : 0}};
  for (const auto &w : want)
    if (int rc = w.bytes ? w.buf.reserve(w.bytes) : FQGPU_OK) return rc;
  return FQGPU_OK;
}
// the lane-level buffers of a block
static int reserve(EncLane &lane, const EncLanePlan &lp) {
  int rc;
  if ((rc = lane.rec_start.reserve(lp.rec_start)) || (rc = lane.n_cnt32.reserve(lp.n_cnt32)) || (rc = lane.n_off.reserve(lp.n_off)) ||
      (rc = lane.first_sym.reserve(lp.first_sym)))
    return rc;
  return lane.tile_first.reserve(lp.tile_first);
}

// (a buffer the path never reserved: nullptr, not null + offset)
template <class T> T *at(const DevBuf &b, const EncSpan &s) { return b.p ? reinterpret_cast<T *>(b.as<uint8_t>() + s.off) : nullptr; }

// Typed pointers into one stream's scratch as its plan laid it out (taken after reserve: a buffer that grows moves)
struct EncViews {
  const uint32_t *rec_start;
  StreamResult *res;
  uint16_t *ckey;
  uint8_t *csym;
  uint16_t *enc16;  // over the keys, which are dead after K3
  uint32_t *arrays, *ctx_start, *seg_base;  // ctx_arrays: its head ctx_count, (device: arrays + B), (arrays + B + B + 1; seg_base[B] = segments of the block)
  uint16_t *final_state;
  uint16_t *lpos16;  // in slot_of: the tile path and the batch-sorted sequence partition have no slots
  SeqBatchDesc bd;
  unsigned long long *ts_status;  // tile_sync
  unsigned *ts_counter;
  uint32_t *ts_run_count;
  uint4 *ts_edges;
  const uint8_t *first_sym;    // fused K1 -> K3: the records' first symbols in encode order, and the record that holds
  const uint32_t *tile_first;  // each tile's first encode index (nullptr otherwise)
  SegArrays sa;  // generic chains (all nullptr on the sequence chains' path)
  ItemArrays ia;
  uint32_t *plan, *plan_work, *plan_seg_base;  // sequence chains: the plan's words, (device: plan + 5 (B + 1)), (plan + 2 (B + 1))
  uint16_t *entry, *fbuf, *cbuf, *item_entry;
  SeqHandover hand;
};

template <class M>
EncViews make_views(EncLane &lane, const EncPlan &p, const EncLanePlan &lp, fqgpu_dblock *b, bool fused) {
  EncScratch &sc = lane.enc[M::STREAM];
  EncViews v{};
  v.rec_start = lane.rec_start.as<uint32_t>();
  v.res = &b->result->s[M::STREAM];
  v.ckey = at<uint16_t>(sc.keys, p.ckey);
  v.csym = at<uint8_t>(sc.keys, p.csym);
  v.enc16 = dbg_no_alias() ? sc.dbg_enc16.as<uint16_t>() : v.ckey;
  v.arrays = at<uint32_t>(sc.ctx_arrays, p.ctx_count);
  v.ctx_start = at<uint32_t>(sc.ctx_arrays, p.ctx_start);
  v.seg_base = at<uint32_t>(sc.ctx_arrays, p.seg_base);
  v.final_state = sc.seg_state.as<uint16_t>();
  v.lpos16 = sc.slot_of.as<uint16_t>();
  v.bd.start = at<uint32_t>(sc.seq_bdesc, p.bd_start);
  v.bd.pre = at<uint16_t>(sc.seq_bdesc, p.bd_pre);
  v.ts_status = at<unsigned long long>(sc.tile_sync, p.ts_status);
  v.ts_counter = at<unsigned>(sc.tile_sync, p.ts_counter);
  v.ts_run_count = at<uint32_t>(sc.tile_sync, p.ts_run_count);
  v.ts_edges = at<uint4>(sc.tile_sync, p.ts_edges);
  if (fused) {
    v.first_sym = at<uint8_t>(lane.first_sym, lp.first_sym_of[M::STREAM]);
    v.tile_first = lane.tile_first.as<uint32_t>();
  }
  v.fbuf = sc.seq_fbuf.as<uint16_t>();
  if (p.serial_seq) {
    v.plan = at<uint32_t>(sc.seq_plan, p.sp_fitem);
    v.plan_work = at<uint32_t>(sc.seq_plan, p.sp_work);
    v.plan_seg_base = at<uint32_t>(sc.seq_plan, p.sp_seg);
    v.entry = at<uint16_t>(sc.seq_plan, p.sp_entry);
    v.cbuf = at<uint16_t>(sc.seq_cbuf, p.cb_func);
    v.item_entry = at<uint16_t>(sc.seq_cbuf, p.cb_item_entry);
    v.hand.W = p.cand_W; v.hand.cap = p.cand_cap; v.hand.P = p.cand_P;
    if (p.cand_W) {
      v.hand.cand0 = at<uint16_t>(sc.seq_cand, p.cand0);
      v.hand.cand = at<uint16_t>(sc.seq_cand, p.cand);
      v.hand.counts = &b->result->seq_groups_handed;
    }
  } else {
    v.sa.anchor = at<uint32_t>(sc.seg_arrays, p.sa_anchor);
    v.sa.usym = at<uint32_t>(sc.seg_arrays, p.sa_usym);
    v.sa.entry_state = at<uint16_t>(sc.seg_arrays, p.sa_entry);
    v.sa.cand_exit = at<uint16_t>(sc.seg_arrays, p.sa_cand);
    v.sa.cls = at<uint8_t>(sc.seg_arrays, p.sa_cls);
    v.ia.has_g = at<uint32_t>(sc.seg_arrays, p.ia_has_g);
    v.ia.item_entry = at<uint16_t>(sc.seg_arrays, p.ia_entry);
    v.ia.g = at<uint16_t>(sc.seg_arrays, p.ia_g);
  }
  return v;
}

// ---- dispatch on what a kernel is templated by
// the tile histograms' counters: u16 on the tile-sorted path, u32 on the slot path
template <class F> void with_hist_type(bool tile_path, F &&f) {
  if (tile_path) f((uint16_t *)nullptr); else f((uint32_t *)nullptr);
}
#define FQ_HIST_TYPE(h) std::remove_pointer_t<decltype(h)>
// words of a state bitmap: 32 up to table log 11, 64 for log 12
template <class F> void with_log_width(unsigned max_log, F &&f) {
  if (max_log <= 11) f(std::integral_constant<unsigned, 32>()); else f(std::integral_constant<unsigned, 64>());
}
// candidate slots per handed-over group
template <class F> void with_cand_width(unsigned W, F &&f) {
  if (W == 16) f(std::integral_constant<unsigned, 16>());
  else if (W == 32) f(std::integral_constant<unsigned, 32>());
  else f(std::integral_constant<unsigned, 64>());
}

// ---- the stages
template <class M>
void launch_hist(EncScratch &sc, const EncPlan &p, const EncViews &v, hipStream_t st, const fqgpu_dblock *b) {
  with_hist_type(p.tile_path, [&](auto *h) {
    using H = FQ_HIST_TYPE(h);
    hipLaunchKernelGGL((k_tile_hist<M, H>), dim3(p.n_tiles), dim3(256), 0, st, b->raw, b->recs, v.rec_start, p.R, p.n_sym, p.T,
                       sc.tile_hist.as<H>(), v.ckey, v.csym, v.res, fq_debug_k1());
  });
}

// K2: tile histograms -> group sums -> context layout -> every tile's base per context.  usym: SegArrays::usym of the generic chains
static void launch_layout(EncScratch &sc, const EncShape &sh, bool tile_path, unsigned S, uint32_t *usym, hipStream_t st) {
  const unsigned B = sh.B;
  const dim3 grid((B + 255) / 256, sh.n_groups);
  uint32_t *arrays = at<uint32_t>(sc.ctx_arrays, sh.ctx_count), *group_sum = sc.group_sum.as<uint32_t>();
  with_hist_type(tile_path, [&](auto *h) {
    using H = FQ_HIST_TYPE(h);
    hipLaunchKernelGGL(k_group_sum<H>, grid, dim3(256), 0, st, sc.tile_hist.as<H>(), sh.n_tiles, B, group_sum);
    hipLaunchKernelGGL(k_group_prefix, dim3((B + 255) / 256), dim3(256), 0, st, group_sum, sh.n_groups, B, arrays);
    hipLaunchKernelGGL(k_ctx_layout, dim3(1), dim3(1024), 0, st, B, S, arrays, usym);
    hipLaunchKernelGGL(k_tile_base<H>, grid, dim3(256), 0, st, sc.tile_hist.as<H>(), group_sum, at<uint32_t>(sc.ctx_arrays, sh.ctx_start),
                       sh.n_tiles, B, sc.tile_base.as<uint32_t>());
  });
}

// K3 of the tile-sorted path.  FUSED: the keys are the fused K1's -- contexts alone, the symbols derived from them
template <class M, bool FUSED>
void launch_tile_partition(EncScratch &sc, const EncShape &sh, hipStream_t st, const uint16_t *ckey, const uint8_t *csym, uint32_t *run_count,
                           unsigned long long *status, unsigned *counter, const uint32_t *rec_start, const uint8_t *first_sym, const uint32_t *tile_first) {
  hipLaunchKernelGGL((k_tile_partition<M, FUSED>), dim3(sh.n_tiles), dim3(TS_THREADS), 0, st, ckey, csym, sh.n_sym, sc.tile_hist.as<uint16_t>(),
                     sc.tile_base.as<uint32_t>(), sc.sorted_sym.as<uint8_t>(), sc.slot_of.as<uint16_t>(), sc.tile_runs.as<uint2>(), run_count, status, counter,
                     rec_start, sh.R, first_sym, tile_first);
}

// K3: tile-sorted / batch-sorted sequence stream / slots
template <class M>
void launch_partition(const fqgpu_ctx *ctx, EncScratch &sc, const EncPlan &p, const EncViews &v, hipStream_t st, bool fused) {
  const bool ordered = ctx->lds_atomics_ordered;
  if (p.tile_path) {
    if (fused) launch_tile_partition<M, true>(sc, p, st, v.ckey, v.csym, v.ts_run_count, v.ts_status, v.ts_counter, v.rec_start, v.first_sym, v.tile_first);
    else launch_tile_partition<M, false>(sc, p, st, v.ckey, v.csym, v.ts_run_count, v.ts_status, v.ts_counter, v.rec_start, v.first_sym, v.tile_first);
  } else if (p.serial_seq) {
    if (ordered)
      hipLaunchKernelGGL(k_scatter_seq<true>, dim3(p.n_tiles), dim3(64), 0, st, v.ckey, p.n_sym, p.T, sc.tile_base.as<uint32_t>(),
                         sc.sorted_sym.as<uint8_t>(), v.lpos16, v.bd, fq_debug_no_sym(0));
    else
      hipLaunchKernelGGL(k_scatter_seq<false>, dim3(p.n_tiles), dim3(64), 0, st, v.ckey, p.n_sym, p.T, sc.tile_base.as<uint32_t>(),
                         sc.sorted_sym.as<uint8_t>(), v.lpos16, v.bd, fq_debug_no_sym(0));
  } else if (ordered) {
    hipLaunchKernelGGL((k_scatter<M, true>), dim3(p.n_tiles), dim3(64), 0, st, v.ckey, v.csym, p.n_sym, p.T, sc.tile_base.as<uint32_t>(),
                       sc.sorted_sym.as<uint8_t>(), sc.slot_of.as<uint32_t>(), fq_debug_no_sym(M::STREAM));
  } else {
    hipLaunchKernelGGL((k_scatter<M, false>), dim3(p.n_tiles), dim3(64), 0, st, v.ckey, v.csym, p.n_sym, p.T, sc.tile_base.as<uint32_t>(),
                       sc.sorted_sym.as<uint8_t>(), sc.slot_of.as<uint32_t>(), fq_debug_no_sym(M::STREAM));
  }
}

// K4, sequence chains (enc_chains_seq.h): plan, segment functions, the rest of the handed-over groups, entry states, emit
static void launch_seq_chains(fqgpu_ctx *ctx, EncScratch &sc, const EncPlan &p, const EncViews &v, hipStream_t st, unsigned mask) {
  const DevTables &tab = ctx->tab[0];
  const uint8_t *sym = sc.sorted_sym.as<uint8_t>();
  const uint16_t *pow = nullptr;  // power tables for this segment length (uniform segments), if the handle has them
  for (unsigned i = 0; i < FQ_SEQ_POW_SETS; i++)
    if (tab.seq_pow[i] && tab.seq_pow_S[i] == p.seq_S) pow = tab.seq_pow[i];
  const SeqHandover no_hand{};
  const unsigned log_size = 1u << tab.max_log;
  if (EncStage s{ctx, st, "seq.plan", mask, 8u}; !s.off)
    hipLaunchKernelGGL(k_seq_segplan, dim3(1), dim3(256), 0, st, v.arrays, p.seq_S, p.Q, p.gmin, p.wpg * p.rounds, v.plan);
  const bool dbg_skip = fq_debug_flag("FQGPU_DEBUG_SKIP_SEQ_CHAIN");  // timing experiment only: wrong output
  // (all of k_seq_setfunc's LDS is dynamic, 118 KB with the two-symbol table: fq_encode_init_device has asked for it)
  if (EncStage s{ctx, st, "seq.setfunc", mask, 8u, "setfunc"}; s.off || dbg_skip) {
  } else if (p.two_sym) {
    hipLaunchKernelGGL((k_seq_setfunc<32, true>), dim3(min(p.max_fitems, ctx->setfunc_wgs ? ctx->setfunc_wgs : ctx->n_cus)), dim3(SETS_WAVES2 * 64),
                       32 * log_size + SETS_WAVES2 * sizeof(SetsWaveLds11) + 16, st, sym, v.arrays, v.plan, tab.logs, tab.next2,
                       4 * p.next_stride, pow, p.next_stride, p.seq_S, p.Q, p.gmin, p.rounds, p.fstride, v.fbuf, v.plan_work, 32 * log_size, v.hand);
  } else {
    hipLaunchKernelGGL((k_seq_setfunc<64, false>), dim3(min(p.max_fitems, 2 * ctx->n_cus)), dim3(SETS_WAVES * 64),
                       8 * log_size + SETS_WAVES * sizeof(SetsWaveLds) + 16, st, sym, v.arrays, v.plan, tab.logs, tab.next1,
                       p.next_stride, pow, p.next_stride, p.seq_S, p.Q, p.gmin, p.rounds, p.fstride, v.fbuf, v.plan_work, 8 * log_size, no_hand);
  }
  if (dbg_skip) return;
  if (p.cand_W) {  // one workgroup per k_seq_setfunc item, nothing but the table in LDS
    const unsigned clds = 32u << tab.max_log;  // (tests/test_build_seq_candwalk.py reads this line)
    if (EncStage s{ctx, st, "seq.candwalk", mask, 8u, "candwalk"}; !s.off)
      with_cand_width(p.cand_W, [&](auto w) {
        hipLaunchKernelGGL(k_seq_candwalk<decltype(w)::value>, dim3(p.max_fitems), dim3(CANDW_WAVES * 64), clds, st, sym, v.arrays, v.plan, tab.logs,
                           tab.next2, 4 * p.next_stride, p.seq_S, p.Q, p.gmin, p.rounds, v.hand);
      });
  }
  if (EncStage s{ctx, st, "seq.resolve", mask, 8u, "resolve"}; !s.off)
    with_log_width(tab.max_log, [&](auto w) {
      constexpr unsigned W = decltype(w)::value;
      hipLaunchKernelGGL(k_seq_resolve<W>, dim3(1), dim3(SEQ_RESOLVE_THREADS), 0, st, v.plan, tab.logs, v.fbuf, p.fstride, p.Q, p.gmin, v.cbuf,
                         v.item_entry, v.entry, W == 32 ? v.hand : no_hand);
    });
  if (EncStage s{ctx, st, "seq.chains", mask, 8u, "emit"}; !s.off)
    hipLaunchKernelGGL(k_seq_emit, dim3(p.max_eitems), dim3(64), 8 * log_size, st, sym, sc.out16.as<uint16_t>(), v.arrays, v.plan, tab.ct, tab.ct_off,
                       tab.next1, p.next_stride, p.seq_S, v.entry, v.final_state, v.res);
}

// K4, generic chains (enc_chains_generic.h): segment classes, stage 1, heads, entry states, walk
template <class M>
void launch_generic_chains(fqgpu_ctx *ctx, EncScratch &sc, const EncPlan &p, const EncViews &v, hipStream_t st, unsigned mask) {
  const DevTables &tab = ctx->tab[M::STREAM];
  constexpr unsigned B = M::B;
  const uint8_t *sym = sc.sorted_sym.as<uint8_t>();
  uint16_t *out16 = sc.out16.as<uint16_t>();
  if (EncStage s{ctx, st, FQ_SPAN("scan"), mask, 8u, "scan"}; !s.off)
    hipLaunchKernelGGL(k_seg_scan<M>, dim3((p.gen_max_segs + 3) / 4), dim3(256), 0, st, sym, v.arrays, tab.reset_mask, tab.norm, tab.logs, p.S, v.sa);
  if (EncStage s{ctx, st, FQ_SPAN("stage1"), mask, 8u, "stage1"}; !s.off)
    with_log_width(tab.max_log, [&](auto w) {
      hipLaunchKernelGGL((k_seg_stage1<M, decltype(w)::value>), dim3(p.max_items + p.cand_grid + p.gen_pbase + B), dim3(64), p.lds_ct, st, sym, out16,
                         v.arrays, tab.ct, tab.ct_off, v.final_state, p.S, p.max_items, p.cand_grid, p.gen_pbase, p.fstride, v.sa, v.fbuf, v.res);
    });
  if (EncStage s{ctx, st, FQ_SPAN("heads"), mask, 8u, "heads"}; !s.off)
    hipLaunchKernelGGL(k_seg_heads<M>, dim3(p.cand_grid), dim3(64), p.lds_ct, st, sym, v.arrays, tab.ct, tab.ct_off, p.S, p.fstride, v.sa, v.fbuf);
  if (EncStage s{ctx, st, FQ_SPAN("resolve"), mask, 8u, "qresolve"}; !s.off) {
    with_log_width(tab.max_log, [&](auto w) {
      hipLaunchKernelGGL((k_seg_compose<M, decltype(w)::value>), dim3(p.max_items), dim3(64), 0, st, v.arrays, tab.logs, v.fbuf, p.gen_pbase, p.fstride, v.sa, v.ia);
    });
    hipLaunchKernelGGL(k_seg_resolve2<M>, dim3((B + 255) / 256), dim3(256), 0, st, v.arrays, tab.logs, p.fstride, v.sa, v.ia);
    hipLaunchKernelGGL(k_seg_resolve3<M>, dim3((p.max_items + 255) / 256), dim3(256), 0, st, v.arrays, tab.logs, v.fbuf, p.gen_pbase, p.fstride, v.sa, v.ia);
  }
  if (EncStage s{ctx, st, FQ_SPAN("walk2"), mask, 8u, "walk2"}; !s.off)
    hipLaunchKernelGGL((k_seg_walk<M, 2>), dim3(p.max_items), dim3(64), p.lds_ct, st, sym, out16, v.arrays, tab.ct, tab.ct_off, v.final_state, p.S, v.sa, v.res);
}

// K6: (nb, bits) back into encode order and packed -- one fused kernel on the tile path, count / scan / pack otherwise
template <class M>
void launch_pack(fqgpu_ctx *ctx, EncScratch &sc, const EncPlan &p, const EncViews &v, hipStream_t st, unsigned mask, uint8_t *out_dev, size_t cap) {
  const DevTables &tab = ctx->tab[M::STREAM];
  uint16_t *out16 = sc.out16.as<uint16_t>();
  uint32_t *out = reinterpret_cast<uint32_t *>(out_dev);
  unsigned long long *bit_base = sc.tile_bit_base.as<unsigned long long>();
  if (p.tile_path) {
    // the stream starts from zeros (words shared by two tiles are OR-ed into), the look-back from clean flags
    if (EncStage s{ctx, st, FQ_SPAN("gatherpack"), mask, 16u, M::STREAM ? "k6q" : "k6s"}; !s.off)
      hipLaunchKernelGGL(k_tile_gather_pack<M>, dim3(p.n_tiles), dim3(TS_GP_THREADS), 0, st, v.lpos16, sc.tile_runs.as<uint2>(), v.ts_run_count, out16,
                         p.n_sym, p.n_tiles, v.ts_status, v.ts_counter, tab.log_prefix, (unsigned long long)cap, out, v.res, bit_base, v.ts_edges);
    return;
  }
  if (EncStage s{ctx, st, FQ_SPAN("bitcount"), mask, 16u}; s.off) {
  } else if (p.serial_seq) {
    hipLaunchKernelGGL(k_bitcount_seq, dim3((p.n_sym + SEQ_BATCH - 1) / SEQ_BATCH), dim3(PACK_THREADS), 0, st, v.lpos16, v.bd, out16, p.n_sym,
                       sc.tile_bits.as<uint32_t>(), v.enc16);
  } else {
    hipLaunchKernelGGL(k_bitcount, dim3(p.n_ptiles), dim3(PACK_THREADS), 0, st, sc.slot_of.as<uint32_t>(), out16, p.n_sym, sc.tile_bits.as<uint32_t>(), v.enc16);
  }
  if (EncStage s{ctx, st, FQ_SPAN("bitscan"), mask, 32u}; !s.off)
    hipLaunchKernelGGL(k_bitscan, dim3(1), dim3(1024), 0, st, sc.tile_bits.as<uint32_t>(), p.n_ptiles, bit_base, tab.log_prefix, p.B, (unsigned long long)cap, out, v.res);
  if (EncStage s{ctx, st, FQ_SPAN("pack"), mask, 64u}; !s.off)
    hipLaunchKernelGGL(k_pack, dim3(p.n_ptiles), dim3(PACK_THREADS), 0, st, v.enc16, p.n_sym, bit_base, out, v.res);
}

// the optional decode index of the stream (FQGPU_F_DECODE_INDEX)
template <class M>
int launch_index(fqgpu_ctx *ctx, EncScratch &sc, const EncPlan &p, const EncViews &v, hipStream_t st, fqgpu_dblock *b) {
  const DevTables &tab = ctx->tab[M::STREAM];
  const unsigned stride = ctx->index_stride;
  const unsigned n_snap = fq_index_n_snap(p.n_sym, stride);
  const size_t bytes = fq_index_bytes(n_snap, M::B);
  if (int rc = b->index[M::STREAM].grow(bytes + 64, 0, true)) return rc;
  {
    EncStage s{ctx, st, FQ_SPAN("index")};
    hipLaunchKernelGGL(k_index_meta<M>, dim3(n_snap / 256 + 1), dim3(256), 0, st, b->raw, b->recs, v.rec_start, p.R, p.n_sym, stride,
                       sc.tile_bit_base.as<unsigned long long>(), p.tile_path ? TS_TILE : PACK_TILE, b->index[M::STREAM]);
    if (n_snap)
      hipLaunchKernelGGL(k_index_states<M>, dim3(M::B, (n_snap + 63) / 64), dim3(64), p.lds_ct, st, sc.sorted_sym.as<uint8_t>(), v.arrays,
                         sc.tile_base.as<uint32_t>(), p.T, p.n_sym, stride, p.serial_seq ? v.plan_seg_base : v.seg_base,
                         p.serial_seq ? v.entry : v.sa.entry_state, p.serial_seq ? 1 : 0, p.serial_seq ? p.seq_S : p.S, tab.ct, tab.ct_off,
                         v.final_state, b->index[M::STREAM]);
  }
  b->index_bytes[M::STREAM] = bytes;
  return FQGPU_OK;
}

// One stream of one block: reserve what the plan says, then the stages in order on st
template <class M>
int encode_stream(fqgpu_ctx *ctx, EncLane &lane, const EncPlan &p, const EncLanePlan &lp, hipStream_t st, fqgpu_dblock *b,
                  uint8_t *out_dev, size_t cap, unsigned flags) {
  EncScratch &sc = lane.enc[M::STREAM];
  const DevTables &tab = ctx->tab[M::STREAM];
  unsigned mask = fq_debug_skip();
  if ((mask & 256u) && M::STREAM == 1) mask = 0;  // 256: sequence stream only
  if ((mask & 512u) && M::STREAM == 0) mask = 0;  // 512: quality stream only
  const bool fused = fused_k1(ctx);
  if (int rc = reserve(sc, p)) return rc;
  const EncViews v = make_views<M>(lane, p, lp, b, fused);
  if (M::STREAM == 1) {  // diagnostics (fqgpu_dblock_qual_segment_classes): where this encode leaves its classes and their number
    lane.diag_cls = v.sa.cls;
    lane.diag_anchor = v.sa.anchor;
    lane.diag_n_segs = v.seg_base + M::B;
  }

  if (EncStage s{ctx, st, FQ_SPAN("tile_hist"), mask, 1u}; !s.off && !fused) launch_hist<M>(sc, p, v, st, b);
  if (EncStage s{ctx, st, FQ_SPAN("layout"), mask, 2u, M::STREAM ? "k2q" : "k2s"}; !s.off) launch_layout(sc, p, p.tile_path, p.S, v.sa.usym, st);
  if (EncStage s{ctx, st, FQ_SPAN("scatter"), mask, 4u, M::STREAM ? "k3q" : "k3s"}; !s.off) launch_partition<M>(ctx, sc, p, v, st, fused);
  if (p.serial_seq) launch_seq_chains(ctx, sc, p, v, st, mask);
  else launch_generic_chains<M>(ctx, sc, p, v, st, mask);
  launch_pack<M>(ctx, sc, p, v, st, mask, out_dev, cap);
  if (EncStage s{ctx, st, FQ_SPAN("epilogue"), mask, 128u}; !s.off)
    hipLaunchKernelGGL(k_epilogue<M>, dim3(1), dim3(256), 0, st, v.arrays, v.final_state, tab.logs, tab.log_prefix, reinterpret_cast<uint32_t *>(out_dev),
                       v.res, p.tile_path ? v.ts_edges : (const uint4 *)nullptr, p.n_tiles);
  b->index_bytes[M::STREAM] = 0;
  if ((flags & FQGPU_F_DECODE_INDEX) && !mask)
    if (int rc = launch_index<M>(ctx, sc, p, v, st, b)) return rc;
  FQ_HIP(hipGetLastError());
  return FQGPU_OK;
}

#undef FQ_SPAN
#undef FQ_HIST_TYPE

}  // namespace

// All of k_seq_setfunc's LDS is dynamic (118 KB with the two-symbol table): the limit is a property of the function on the
// CURRENT device, so every handle asks for it on its own (fqgpu_ctx_create, behind use_device)
int fq_encode_init_device() {
  FQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_seq_setfunc<32, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  FQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_seq_setfunc<64, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return FQGPU_OK;
}

namespace {
// Verifies on the device that same-address LDS atomics of one wave instruction are applied in
// lane order (what k_scatter<ORDERED> relies on): random keys, some lanes idle, plain and packed
// counters, compared with the rank counted by shuffles.
__global__ void __launch_bounds__(256)
k_probe_lds_atomic_order(unsigned iters, unsigned *__restrict__ bad) {
  __shared__ unsigned cnt[4][1024];
  const unsigned wave = threadIdx.x >> 6, lane = fq_lane();
  unsigned s = (blockIdx.x * blockDim.x + threadIdx.x) * 40503u + 12345u;
  unsigned nbad = 0;
  for (unsigned it = 0; it < iters; it++) {
    for (unsigned c = lane; c < 1024; c += 64) cnt[wave][c] = 0;
    fq_lds_wave_sync();
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    const unsigned range = 1u << ((it % 6) * 2);  // 1, 4, 16, ... 1024 distinct keys
    const unsigned key = (s >> 8) % range;
    const bool active = (s & 15u) != 0;
    const bool packed = (it & 1u) != 0;
    unsigned got = 0;
    if (active) {
      if (packed) got = (atomicAdd(&cnt[wave][key >> 1], 1u << (16 * (key & 1u))) >> (16 * (key & 1u))) & 0xFFFFu;
      else got = atomicAdd(&cnt[wave][key], 1u);
    }
    unsigned ref = 0;
    for (int l = 0; l < 64; l++) {
      const unsigned k2 = (unsigned)__shfl((int)key, l);
      const int a2 = __shfl((int)active, l);
      if ((unsigned)l < lane && a2 && k2 == key) ref++;
    }
    if (active && got != ref) nbad++;
    fq_lds_wave_sync();
  }
  if (nbad) atomicAdd(bad, nbad);
}

}  // namespace

int fq_probe_lds_atomic_order(hipStream_t st, bool *ordered) {
  unsigned *bad = fq_dev_alloc<unsigned>(1);
  if (!bad) return FQGPU_E_NOMEM;
  unsigned h = 1;
  hipError_t e = hipMemsetAsync(bad, 0, 4, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_probe_lds_atomic_order, dim3(512), dim3(256), 0, st, 96u, bad);
    e = hipMemcpyAsync(&h, bad, 4, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(bad);
  if (e != hipSuccess) return FQGPU_E_HIP;
  *ordered = h == 0;
  return FQGPU_OK;
}

namespace {
// (context, symbol) counts from the sorted symbols: one wave per 4096 symbols of one context's run,
// a 64-bin histogram per wave in LDS (lanes that meet on the run's most frequent symbols are folded
// into one add first), one global add per non-empty bin.
__global__ void __launch_bounds__(256)
k_hist_sorted_qual(const uint8_t *__restrict__ sorted_sym, const uint32_t *__restrict__ arrays, unsigned S,
                   uint32_t *__restrict__ counts) {
  constexpr unsigned B = QualModel::B, A = QualModel::A;
  __shared__ uint32_t s_bins[4][A];
  const uint32_t *ctx_count = arrays, *ctx_start = arrays + B, *seg_base = ctx_start + B + 1;
  const unsigned wave = threadIdx.x >> 6, lane = fq_lane(), seg = blockIdx.x * 4 + wave;
  if (seg >= seg_base[B]) return;  // the grid is an upper bound
  const unsigned c = seg_ctx_of<QualModel>(seg_base, seg), k = seg - seg_base[c];
  const unsigned n = ctx_count[c], begin = k * S, end = min(n, begin + S);
  const uint8_t *sym = sorted_sym + ctx_start[c];
  uint32_t *bins = s_bins[wave];
  bins[lane] = 0;
  fq_lds_wave_sync();
  for (unsigned p0 = begin; p0 < end; p0 += 1024) {
    const unsigned p = p0 + 16 * lane;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p < end) v = *reinterpret_cast<const uint4 *>(sym + p);  // (runs are padded to 16 bytes)
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const unsigned s = (w[j >> 2] >> (8 * (j & 3))) & (A - 1);
      bool on = p + j < end;
      // the symbol of the first live lane: everybody who has it too is counted by that lane
      const unsigned long long live = __ballot(on);
      if (!live) break;  // (uniform)
      const unsigned lead = (unsigned)__ffsll((long long)live) - 1u;
      const unsigned s_lead = (unsigned)__shfl((int)s, (int)lead);
      const unsigned long long same = __ballot(on && s == s_lead);
      if (lane == lead) atomicAdd(&bins[s_lead], (unsigned)__popcll(same));
      if (on && s != s_lead) atomicAdd(&bins[s], 1u);
    }
  }
  fq_lds_wave_sync();
  if (bins[lane]) atomicAdd(&counts[(size_t)c * A + lane], bins[lane]);
}
}  // namespace

namespace {
// K1 of both streams in one pass (the tile-sorted path): keys, tile histograms, the records' first symbols, the N counts
void launch_hist2(EncLane &lane, const EncLanePlan &lp, hipStream_t st, const uint8_t *raw, const fqgpu_rec *recs, unsigned R, unsigned n_sym,
                  BlockResult *res) {
  hipLaunchKernelGGL(k_tile_hist2, dim3((n_sym + TS_TILE - 1) / TS_TILE), dim3(256), 0, st, raw, recs, lane.rec_start.as<uint32_t>(), R, n_sym, TS_TILE,
                     lane.enc[0].tile_hist.as<uint16_t>(), lane.enc[0].keys.as<uint8_t>(), lane.enc[1].tile_hist.as<uint16_t>(),
                     lane.enc[1].keys.as<uint16_t>(), at<uint8_t>(lane.first_sym, lp.first_sym_of[0]), at<uint8_t>(lane.first_sym, lp.first_sym_of[1]),
                     lane.tile_first.as<uint32_t>(), at<uint32_t>(lane.n_cnt32, lp.n_cnt), res);
}
}  // namespace

// FSE_Quality::calculateFreqTable (reference src/fse_quality.cpp:69-97) at the encoder's speed: the
// (context, symbol) pairs of the sample are the ones the encoder's K1 computes (the context of a
// position is the same from either end of the read), so K1 + K2 + K3 sort the symbols by context and
// the counts are small local histograms of contiguous runs -- instead of 60 M atomics scattered
// over a 2 MiB table in HBM (9 ms for a 128 MiB sample, 250 ms when one context holds most of it).
// counts_dev: [8192][64], already filled with the reference's initial 1.  Reads of length >= 3 only.
// Waits for st before it returns (its scratch is local: a smaller set of buffers than an encode's, sized by the same shapes;
// tile_sync holds nothing but the run counts here).
int fq_qual_counts_sorted(hipStream_t st, const uint8_t *raw_dev, const fqgpu_rec *recs_dev, size_t n_recs, size_t n_bases,
                          uint32_t *counts_dev, uint32_t *err_dev) {
  constexpr unsigned S = 4096;
  const unsigned R = (unsigned)n_recs, n_sym = (unsigned)n_bases;
  const EncShape shq(n_sym, R, QualModel::B, TS_TILE), shs(n_sym, R, SeqModel::B, TS_TILE);
  const EncLanePlan lp(R, n_bases);
  const unsigned max_segs = n_sym / S + shq.B + 1;
  EncLane lane;
  EncScratch &sq = lane.enc[1], &ss = lane.enc[0];
  DevBuf readlens, result;
  int rc = FQGPU_OK;
  do {
    if ((rc = lane.rec_start.reserve(lp.rec_start)) || (rc = lane.n_cnt32.reserve(lp.n_cnt32)) ||
        (rc = readlens.reserve((size_t)R * 2)) || (rc = result.reserve(sizeof(BlockResult))) || (rc = lane.first_sym.reserve(lp.first_sym)) ||
        (rc = lane.tile_first.reserve(lp.tile_first)) || (rc = reserve_k1(ss, shs)) || (rc = reserve_k1(sq, shq)) ||
        (rc = sq.slot_of.reserve(shq.lpos16_bytes)) || (rc = sq.sorted_sym.reserve(shq.bytes.sorted_sym)) || (rc = sq.tile_base.reserve(shq.bytes.tile_base)) ||
        (rc = sq.group_sum.reserve(shq.bytes.group_sum)) || (rc = sq.ctx_arrays.reserve(shq.bytes.ctx_arrays)) ||
        (rc = sq.tile_runs.reserve(shq.tile_runs_bytes)) || (rc = sq.tile_sync.reserve((size_t)shq.n_tiles * 4 + 64)))
      break;
    uint32_t *n_cnt32 = at<uint32_t>(lane.n_cnt32, lp.n_cnt), *lens32 = at<uint32_t>(lane.n_cnt32, lp.lens), *rec_start = lane.rec_start.as<uint32_t>();
    BlockResult *res = result.as<BlockResult>();
    if (hipMemsetAsync(res, 0, sizeof(BlockResult), st) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    hipLaunchKernelGGL(k_readlens, dim3((unsigned)min((size_t)(R + 255) / 256, (size_t)2048)), dim3(256), 0, st, recs_dev, R,
                       readlens.as<uint16_t>(), n_cnt32, lens32, (BlockResult *)nullptr);
    if ((rc = fq_scan_u32_to_u32(st, lens32, R, rec_start, lane.scan_tmp))) break;
    launch_hist2(lane, lp, st, raw_dev, recs_dev, R, n_sym, res);
    launch_layout(sq, shq, true, S, nullptr, st);
    // (the rank only has to be a permutation here, not a stable one: no lane-ordered atomics are relied on)
    launch_tile_partition<QualModel, true>(sq, shq, st, sq.keys.as<uint16_t>(), nullptr, sq.tile_sync.as<uint32_t>(), nullptr, nullptr, rec_start,
                                           at<uint8_t>(lane.first_sym, lp.first_sym_of[1]), lane.tile_first.as<uint32_t>());
    hipLaunchKernelGGL(k_hist_sorted_qual, dim3((max_segs + 3) / 4), dim3(256), 0, st, sq.sorted_sym.as<uint8_t>(), sq.ctx_arrays.as<uint32_t>(), S, counts_dev);
    BlockResult h;
    if (hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
        hipGetLastError() != hipSuccess) { rc = FQGPU_E_HIP; break; }
    if (h.s[0].bad_symbol || h.s[1].bad_symbol) {  // a quality above Q63 / a byte that is no base: the caller reads the flag
      uint32_t one = 1;
      if (hipMemcpy(err_dev, &one, 4, hipMemcpyHostToDevice) != hipSuccess) rc = FQGPU_E_HIP;
    }
  } while (0);
  (void)hipStreamSynchronize(st);
  readlens.release();
  result.release();
  fq_release_bufs(lane);  // (the lane is this call's own: the lists of fqgpu_internal.h)
  fq_release_bufs(ss);
  fq_release_bufs(sq);
  return rc;
}

namespace {
// k_record_scan (mode 0: lengths -> rec_start and readlens; mode 1: N counts -> n_off and n_count) with its look-back
// words: zero when (re)allocated, then epochs and tickets count on from launch to launch
int launch_record_scan(EncLane &lane, const EncLanePlan &lp, hipStream_t st, const fqgpu_dblock *b, int mode) {
  const unsigned R = (unsigned)b->n_recs, rscan_chunks = (R + RSCAN_CHUNK - 1) / RSCAN_CHUNK;
  const size_t need = (size_t)rscan_chunks * 8 + 16;
  if (need > lane.rscan.cap) {
    int rr = lane.rscan.reserve(need);
    if (rr) return rr;
    FQ_HIP(hipMemsetAsync(lane.rscan.p, 0, lane.rscan.cap, st));
    lane.rscan_tickets = 0;
  }
  lane.rscan_epoch = (lane.rscan_epoch + 1u) & 0xFFFFFFu;
  if (lane.rscan_epoch == 0u) {  // (every 16 M launches: words of the previous round of epochs must not be taken for new ones)
    FQ_HIP(hipMemsetAsync(lane.rscan.p, 0, lane.rscan.cap, st));
    lane.rscan_tickets = 0;
    lane.rscan_epoch = 1u;
  }
  unsigned *ticket = lane.rscan.as<unsigned>();
  unsigned long long *status = reinterpret_cast<unsigned long long *>(lane.rscan.as<uint8_t>() + 16);
  uint32_t *n_cnt32 = at<uint32_t>(lane.n_cnt32, lp.n_cnt);
  if (mode == 0)
    hipLaunchKernelGGL(k_record_scan<0>, dim3(rscan_chunks), dim3(RSCAN_THREADS), 0, st, b->recs, n_cnt32, R, b->readlens, lane.rec_start.as<uint32_t>(),
                       status, ticket, lane.rscan_tickets, lane.rscan_epoch, b->result);
  else
    hipLaunchKernelGGL(k_record_scan<1>, dim3(rscan_chunks), dim3(RSCAN_THREADS), 0, st, b->recs, n_cnt32, R, b->n_count, lane.n_off.as<uint32_t>(),
                       status, ticket, lane.rscan_tickets, lane.rscan_epoch, b->result);
  lane.rscan_tickets += rscan_chunks;
  return FQGPU_OK;
}
}  // namespace

// fqgpu_ctx_reserve: every allocation a block of this shape needs on the next lane in turn, nothing launched
int fq_encode_reserve(fqgpu_ctx *ctx, const fqgpu_dblock *b) {
  if (b->n_recs == 0 || b->n_bases == 0) return FQGPU_E_ARG;
  EncLane *lane = fq_next_lane(ctx, b->n_bases);
  if (!lane) return FQGPU_E_NOMEM;
  const EncLanePlan lp((unsigned)b->n_recs, b->n_bases);
  const EncPlan seq = make_plan<SeqModel>(ctx, b), qual = make_plan<QualModel>(ctx, b);
  lane->forget_diag();  // a buffer that grows moves: the lane answers for no earlier encode (fqgpu_dblock_qual_segment_classes)
  int rc;
  if ((rc = reserve(*lane, lp))) return rc;
  if (fused_k1(ctx) && ((rc = reserve_k1(lane->enc[0], seq)) || (rc = reserve_k1(lane->enc[1], qual)))) return rc;
  // (a launch leaves scan_tmp to the record scans of scan.hip, which size it themselves: ahead of time, their upper bound)
  if ((rc = lane->scan_tmp.reserve(lp.scan_tmp)) || (rc = reserve(lane->enc[1], qual))) return rc;
  return reserve(lane->enc[0], seq);
}

// One block = one encode lane: two HIP streams (sequence pipeline, quality pipeline) forked
// after the record-level kernels and joined before the N-position pass.  Blocks handed to
// different lanes overlap on the device: the serial sequence chains of one block hide behind
// the bandwidth-bound passes of the others.
int fq_encode_launch(fqgpu_ctx *ctx, fqgpu_dblock *b, unsigned flags, hipEvent_t wait, hipStream_t *done) {
  const unsigned R = (unsigned)b->n_recs, n_sym = (unsigned)b->n_bases;
  if (R == 0 || b->n_bases == 0) return FQGPU_E_ARG;
  EncLane *lanep = fq_next_lane(ctx, b->n_bases, b);
  if (!lanep) return FQGPU_E_NOMEM;
  EncLane &lane = *lanep;
  hipStream_t st = lane.st_seq;
  if (done) *done = st;
  int rc;
  if (wait) FQ_HIP(hipStreamWaitEvent(st, wait, 0));
  if (b->ev_encoded) FQ_HIP(hipStreamWaitEvent(st, b->ev_encoded, 0));  // the block's previous encode (fqgpu_internal.h)
  // from here on the lane's segment classes are this encode's, or nobody's (fqgpu_dblock_qual_segment_classes)
  lane.forget_diag();
  lane.diag_stamp = ++ctx->encodes;
  b->diag_stamp = b->owner == ctx ? lane.diag_stamp : 0;  // (a block of another handle: that handle has no lane to ask)
  const bool fused = fused_k1(ctx);
  const EncLanePlan lp(R, b->n_bases);
  const EncPlan seq = make_plan<SeqModel>(ctx, b), qual = make_plan<QualModel>(ctx, b);
  if ((rc = reserve(lane, lp))) return rc;
  uint32_t *n_cnt32 = at<uint32_t>(lane.n_cnt32, lp.n_cnt), *lens32 = at<uint32_t>(lane.n_cnt32, lp.lens);
  uint32_t *rec_start = lane.rec_start.as<uint32_t>(), *n_off = lane.n_off.as<uint32_t>();

  if (EncStage s{ctx, st, "records"}; fused) {  // lengths from the record table alone, scanned in the same launch; K1 counts the N's (the raw block is read once less)
    if ((rc = launch_record_scan(lane, lp, st, b, 0))) return rc;
  } else {
    const unsigned len_blocks = (unsigned)min((size_t)(R + 15) / 16, (size_t)4096);  // four records per wave
    hipLaunchKernelGGL(k_readlens_ncount, dim3(len_blocks), dim3(256), 0, st, b->raw, b->recs, R, b->readlens, b->n_count, n_cnt32, lens32, b->result);
    if ((rc = fq_scan2_u32_to_u32(st, lens32, n_cnt32, R, rec_start, n_off, lane.scan_tmp))) return rc;
    hipLaunchKernelGGL(k_store_npos_len, dim3(1), dim3(1), 0, st, n_off, R, b->result);
  }
  if (fused) {  // K1 of both streams in one pass, in front of the fork
    if ((rc = reserve_k1(lane.enc[0], seq)) || (rc = reserve_k1(lane.enc[1], qual))) return rc;
    if (EncStage s{ctx, st, "tile_hist2", 0, 0, "k1"}; !s.off) launch_hist2(lane, lp, st, b->raw, b->recs, R, n_sym, b->result);
  }
  FQ_HIP(hipEventRecord(lane.ev_fork, lane.st_seq));
  FQ_HIP(hipStreamWaitEvent(lane.st_qual, lane.ev_fork, 0));
  // timing experiments only (wrong output): one stream at a time
  const bool dbg_no_qual = fq_debug_flag("FQGPU_DEBUG_SKIP_QUAL"), dbg_no_seq = fq_debug_flag("FQGPU_DEBUG_SKIP_SEQ");
  if (!dbg_no_qual && (rc = encode_stream<QualModel>(ctx, lane, qual, lp, lane.st_qual, b, b->qual, b->qual_cap, flags))) return rc;
  if (!dbg_no_seq && (rc = encode_stream<SeqModel>(ctx, lane, seq, lp, lane.st_seq, b, b->seq, b->seq_cap, flags))) return rc;
  FQ_HIP(hipEventRecord(lane.ev_join, lane.st_qual));
  FQ_HIP(hipStreamWaitEvent(lane.st_seq, lane.ev_join, 0));

  // after both streams: the optional in-place N -> A must not race with their reads of raw
  {
    EncStage s{ctx, st, "npos"};
    // K1 left the N counts: 16-bit copy for the caller, offsets of the position deltas, their total -- one launch
    if (fused && (rc = launch_record_scan(lane, lp, st, b, 1))) return rc;
    const unsigned rec_blocks = (unsigned)min((size_t)(R + 3) / 4, (size_t)8192);  // k_npos: a wave per record
    hipLaunchKernelGGL(k_npos, dim3(rec_blocks), dim3(256), 0, st, b->raw, b->recs, R, n_off, b->n_pos, (flags & FQGPU_F_WRITE_BACK_N) ? 1 : 0);
  }
  FQ_HIP(hipGetLastError());
  if (!b->ev_encoded) FQ_HIP(hipEventCreateWithFlags(&b->ev_encoded, hipEventDisableTiming));
  FQ_HIP(hipEventRecord(b->ev_encoded, st));
  return FQGPU_OK;
}
