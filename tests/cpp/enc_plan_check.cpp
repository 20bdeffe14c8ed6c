// EncPlan / EncLanePlan (fqcomp28_amd/csrc/enc_plan.h) against the recorded table enc_plan_table.inc: every derived size, every
// buffer's byte size and every sub-array offset of a set of configurations, plus alignment and "sub-arrays of one buffer do
// not overlap and end inside it".  No GPU, no HIP: g++ -fsanitize=address,undefined (tests/test_enc_plan_host.py).
#include <cstdio>
#include <set>
#include <vector>

#include "../../fqcomp28_amd/csrc/enc_plan.h"

enum Field {
  // the configuration
  N_SYM, RECS, STREAM, TILE_PATH, SERIAL_SEQ, SEG_LEN, SEQ_SEGMENT, CAND_CAP, MAX_LOG,
  // derived numbers
  T_, S_, SEQ_S, N_TILES, N_GROUPS, N_PTILES, N_PAD, PADDED, MAX_ITEMS, GEN_MAX_SEGS, SEQ_MAX_SEGS, CAND_W, CAND_P, MAX_FITEMS, MAX_EITEMS,
  MAX_CITEMS, SEQ_FSTRIDE, GEN_FSTRIDE, CAND_GRID, LDS_CT,
  // bytes reserved per buffer (0: not reserved on this path)
  R_SLOT_OF, R_KEYS, R_SORTED_SYM, R_OUT16, R_TILE_HIST, R_TILE_BASE, R_GROUP_SUM, R_CTX_ARRAYS, R_SEG_STATE, R_SEG_ARRAYS, R_SEQ_PLAN,
  R_SEQ_FBUF, R_SEQ_CBUF, R_SEQ_CAND, R_SEQ_BDESC, R_TILE_BITS, R_TILE_BIT_BASE, R_TILE_RUNS, R_TILE_SYNC,
  // offsets of sub-arrays
  O_CSYM, O_CTX_START, O_SEG_BASE, O_ITEM_BASE, O_SA_ANCHOR, O_SA_USYM, O_SA_ENTRY, O_SA_CAND, O_SA_CLS, O_IA_HAS_G, O_IA_ENTRY, O_IA_G,
  O_SP_SEG, O_SP_WORK, O_SP_ENTRY, O_ITEM_ENTRY, O_CAND, O_BD_PRE, O_TS_COUNTER, O_TS_RUN_COUNT, O_TS_EDGES,
  // the lane's buffers and the offsets inside them
  L_REC_START, L_N_CNT32, L_N_OFF, L_FIRST_SYM, L_TILE_FIRST, L_SCAN_TMP, O_LENS, O_FIRST_QUAL,
  N_FIELDS
};

static const unsigned long long kTable[][N_FIELDS] = {
#include "enc_plan_table.inc"
};

static int g_bad = 0;
static int g_row = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) { printf("row %d: %s\n", g_row, #cond); g_bad++; }                   \
  } while (0)
#define SAME(field, got)                                                                                                        \
  do {                                                                                                                          \
    if ((unsigned long long)(got) != row[field]) {                                                                              \
      printf("row %d: %s is %llu, recorded %llu\n", g_row, #field, (unsigned long long)(got), row[field]);                      \
      g_bad++;                                                                                                                  \
    }                                                                                                                           \
  } while (0)

// consecutive, inside the buffer (total 0: the buffer is not reserved on this path, nothing to end in)
static void laid_out(const char *buf, size_t total, const std::vector<EncSpan> &spans) {
  size_t end = 0;
  for (const EncSpan &s : spans) {
    if (s.off < end) { printf("row %d: sub-arrays of %s overlap\n", g_row, buf); g_bad++; }
    end = s.off + s.bytes;
  }
  if (total && end > total) { printf("row %d: the sub-arrays of %s end at %zu, behind its %zu bytes\n", g_row, buf, end, total); g_bad++; }
}

int main() {
  std::set<unsigned long long> seen[MAX_LOG + 1], widths;
  for (const auto &row : kTable) {
    EncPlanIn in;
    in.n_sym = (unsigned)row[N_SYM]; in.R = (unsigned)row[RECS]; in.stream = (int)row[STREAM];
    in.B = in.stream ? FQGPU_QUAL_MODELS : FQGPU_SEQ_MODELS; in.A = in.stream ? FQGPU_QUAL_ALPHA : FQGPU_SEQ_ALPHA;
    in.max_log = (unsigned)row[MAX_LOG];
    in.two_sym = in.stream == 0 && in.max_log <= 11;
    in.tile_path = row[TILE_PATH] != 0; in.serial_seq = row[SERIAL_SEQ] != 0;
    in.seg_len = (unsigned)row[SEG_LEN]; in.seq_segment = (unsigned)row[SEQ_SEGMENT]; in.seq_cand_cap = (unsigned)row[CAND_CAP];
    in.seq_group = 8; in.seq_group_min = 16; in.seq_cand_prefix = 1; in.n_cus = 256;  // the handle's defaults on an MI355X
    for (int f = 0; f <= MAX_LOG; f++) seen[f].insert(row[f]);
    const EncPlan p(in);
    const EncLanePlan lp(in.R, in.n_sym);
    widths.insert(p.cand_W);

    SAME(T_, p.T); SAME(S_, p.S); SAME(SEQ_S, p.seq_S); SAME(N_TILES, p.n_tiles); SAME(N_GROUPS, p.n_groups); SAME(N_PTILES, p.n_ptiles);
    SAME(N_PAD, p.n_pad); SAME(PADDED, p.padded); SAME(MAX_ITEMS, p.max_items); SAME(GEN_MAX_SEGS, p.gen_max_segs);
    SAME(SEQ_MAX_SEGS, p.seq_max_segs); SAME(CAND_W, p.cand_W); SAME(CAND_P, p.cand_P); SAME(MAX_FITEMS, p.max_fitems);
    SAME(MAX_EITEMS, p.max_eitems); SAME(MAX_CITEMS, p.max_citems);
    SAME(SEQ_FSTRIDE, p.fstride); SAME(GEN_FSTRIDE, p.fstride);  // two columns of the recorded code (1 << max_log both), one number in the plan
    SAME(CAND_GRID, p.cand_grid); SAME(LDS_CT, p.lds_ct);
    const EncBytes &n = p.bytes;
    SAME(R_SLOT_OF, n.slot_of); SAME(R_KEYS, n.keys); SAME(R_SORTED_SYM, n.sorted_sym); SAME(R_OUT16, n.out16); SAME(R_TILE_HIST, n.tile_hist);
    SAME(R_TILE_BASE, n.tile_base); SAME(R_GROUP_SUM, n.group_sum); SAME(R_CTX_ARRAYS, n.ctx_arrays); SAME(R_SEG_STATE, n.seg_state);
    SAME(R_SEG_ARRAYS, n.seg_arrays); SAME(R_SEQ_PLAN, n.seq_plan); SAME(R_SEQ_FBUF, n.seq_fbuf); SAME(R_SEQ_CBUF, n.seq_cbuf);
    SAME(R_SEQ_CAND, n.seq_cand); SAME(R_SEQ_BDESC, n.seq_bdesc); SAME(R_TILE_BITS, n.tile_bits); SAME(R_TILE_BIT_BASE, n.tile_bit_base);
    SAME(R_TILE_RUNS, n.tile_runs); SAME(R_TILE_SYNC, n.tile_sync);
    CHECK(p.ckey.off == 0 && p.ctx_count.off == 0 && p.sp_fitem.off == 0 && p.cb_func.off == 0 && p.cand0.off == 0 && p.bd_start.off == 0 &&
          p.ts_status.off == 0);
    SAME(O_CSYM, p.csym.off); SAME(O_CTX_START, p.ctx_start.off); SAME(O_SEG_BASE, p.seg_base.off);
    SAME(O_ITEM_BASE, p.seg_base.off + p.seg_base.bytes);  // (behind seg_base; the host never addresses it)
    SAME(O_SA_ANCHOR, p.sa_anchor.off); SAME(O_SA_USYM, p.sa_usym.off); SAME(O_SA_ENTRY, p.sa_entry.off); SAME(O_SA_CAND, p.sa_cand.off);
    SAME(O_SA_CLS, p.sa_cls.off); SAME(O_IA_HAS_G, p.ia_has_g.off); SAME(O_IA_ENTRY, p.ia_entry.off); SAME(O_IA_G, p.ia_g.off);
    SAME(O_SP_SEG, p.sp_seg.off); SAME(O_SP_WORK, p.sp_work.off); SAME(O_SP_ENTRY, p.sp_entry.off); SAME(O_ITEM_ENTRY, p.cb_item_entry.off);
    SAME(O_CAND, p.cand.off); SAME(O_BD_PRE, p.bd_pre.off); SAME(O_TS_COUNTER, p.ts_counter.off); SAME(O_TS_RUN_COUNT, p.ts_run_count.off);
    SAME(O_TS_EDGES, p.ts_edges.off);
    // alignment: what the recorded code kept 16-byte aligned, and the kernels load as 16-byte vectors
    for (const EncSpan *s : {&p.csym, &p.sa_anchor, &p.sa_usym, &p.sa_entry, &p.sa_cand, &p.sa_cls, &p.ia_has_g, &p.ia_entry, &p.ia_g, &p.ts_edges})
      CHECK(s->off % 16 == 0);
    laid_out("keys", n.keys, {p.ckey, p.csym});
    laid_out("ctx_arrays", n.ctx_arrays, {p.ctx_count, p.ctx_start, p.seg_base});
    laid_out("seg_arrays", n.seg_arrays, {p.sa_anchor, p.sa_usym, p.sa_entry, p.sa_cand, p.sa_cls, p.ia_has_g, p.ia_entry, p.ia_g});
    laid_out("seq_plan", n.seq_plan, {p.sp_fitem, p.sp_seg, p.sp_work, p.sp_entry});
    laid_out("seq_cbuf", n.seq_cbuf, {p.cb_func, p.cb_item_entry});
    laid_out("seq_cand", n.seq_cand, {p.cand0, p.cand});
    laid_out("seq_bdesc", n.seq_bdesc, {p.bd_start, p.bd_pre});
    laid_out("tile_sync", n.tile_sync, {p.ts_status, p.ts_counter, p.ts_run_count, p.ts_edges});
    CHECK(p.sp_work.off + p.sp_work.bytes == (size_t)SEGPLAN_WORDS * 4);

    SAME(L_REC_START, lp.rec_start); SAME(L_N_CNT32, lp.n_cnt32); SAME(L_N_OFF, lp.n_off); SAME(L_FIRST_SYM, lp.first_sym);
    SAME(L_TILE_FIRST, lp.tile_first); SAME(L_SCAN_TMP, lp.scan_tmp); SAME(O_LENS, lp.lens.off); SAME(O_FIRST_QUAL, lp.first_sym_of[1].off);
    CHECK(lp.n_cnt.off == 0 && lp.first_sym_of[0].off == 0);
    laid_out("n_cnt32", lp.n_cnt32, {lp.n_cnt, lp.lens});
    laid_out("first_sym", lp.first_sym, {lp.first_sym_of[0], lp.first_sym_of[1]});
    g_row++;
  }
  // the table covers what it was asked to cover
  const size_t want[] = {9, 2, 2, 2, 2, 3, 2, 4, 2};  // values of n_sym, R, stream, tile_path, serial_seq, seg_len, seq_segment, cand_cap, max_log
  for (int f = 0; f <= MAX_LOG; f++)
    if (seen[f].size() != want[f]) { printf("field %d takes %zu values, not %zu\n", f, seen[f].size(), want[f]); g_bad++; }
  if (widths != std::set<unsigned long long>{0, 16, 32, 64}) { printf("not every hand-over width is met\n"); g_bad++; }
  printf("%d rows, %d failures\n", g_row, g_bad);
  return g_bad ? 1 : 0;
}
