// N restoration for a window of records (fqgpu_decode_chunk_range): the tail of SequenceDecoder::decodeRecord
// (src/fse_sequence.cpp:138-142) as k_npatch (decode.hip) states it, for the records [w0, w1) alone.  Where a
// record's N positions start in n_pos depends on every record in front of it, so the offsets are still scanned over
// the whole chunk (one pass over n_count); only the patch and its bounds checks are limited to the window.
#include "fqgpu_internal.h"

namespace {

__global__ void __launch_bounds__(256)
k_widen_ncount(const uint16_t *__restrict__ n_count, unsigned n, uint32_t *__restrict__ cnt32) {
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) cnt32[r] = n_count[r];
}

// off: exclusive scan of n_count over the whole chunk (n + 1 entries); the reference pops counts and deltas from the
// END of n_count / n_pos, which equals forward indexing from n_pos_len - (total N of the chunk)
__global__ void __launch_bounds__(256)
k_npatch_window(const uint16_t *__restrict__ n_count, const uint32_t *__restrict__ off, unsigned n, const uint16_t *__restrict__ n_pos,
                unsigned n_pos_len, const fqgpu_rec *__restrict__ recs, uint8_t *__restrict__ raw, unsigned w0, unsigned w1,
                BlockResult *__restrict__ res) {
  const unsigned total = off[n];
  if (total > n_pos_len) {
    if (blockIdx.x == 0 && threadIdx.x == 0) res->s[0].corrupt = 1;
    return;
  }
  const unsigned shift = n_pos_len - total;
  for (unsigned r = w0 + blockIdx.x * blockDim.x + threadIdx.x; r < w1; r += gridDim.x * blockDim.x) {
    const unsigned cnt = n_count[r];
    if (!cnt) continue;
    const fqgpu_rec rec = recs[r];
    const uint16_t *d = n_pos + shift + off[r];
    unsigned at = 0;
    for (unsigned k = 0; k < cnt; k++) {
      at += d[k];
      if (at >= rec.len) { res->s[0].corrupt = 1; break; }
      raw[rec.seq_off + at] = 'N';
    }
  }
}

}  // namespace

// b: the staging block, n_count / n_pos uploaded, recs[w0 .. w1) and raw laid out for the window, the walk queued on
// ctx->stream in front of this
int fq_npatch_window(fqgpu_ctx *ctx, fqgpu_dblock *b, unsigned w0, unsigned w1) {
  hipStream_t st = ctx->stream;
  const size_t n = b->n_recs;
  int rc;
  if ((rc = ctx->n_cnt32.reserve((n + 1) * 4)) || (rc = ctx->n_off.reserve((n + 1) * 4))) return rc;
  const unsigned gx = (unsigned)min((n + 255) / 256, (size_t)4096);
  fq_timer_span_begin(ctx, "npatch", st);
  hipLaunchKernelGGL(k_widen_ncount, dim3(gx ? gx : 1), dim3(256), 0, st, b->n_count, (unsigned)n, ctx->n_cnt32.as<uint32_t>());
  FQ_HIP(hipGetLastError());
  if ((rc = fq_scan_u32_to_u32(st, ctx->n_cnt32.as<uint32_t>(), n, ctx->n_off.as<uint32_t>(), ctx->scan_tmp))) return rc;
  const unsigned gw = (unsigned)min(((size_t)(w1 - w0) + 255) / 256, (size_t)4096);
  hipLaunchKernelGGL(k_npatch_window, dim3(gw ? gw : 1), dim3(256), 0, st, b->n_count, ctx->n_off.as<uint32_t>(), (unsigned)n,
                     b->n_pos, (unsigned)b->n_pos_len, b->recs, b->raw, w0, w1, b->result);
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  return FQGPU_OK;
}
