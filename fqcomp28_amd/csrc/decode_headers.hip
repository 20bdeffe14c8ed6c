// Header decode and chunk layout on the device: the first pass of DecompressionWorkspace::decodeChunk
// (reference src/workspace.cpp:47-80 over decodeHeader, :128-157, and FieldStorageSrc::loadNextString /
// loadNextNumeric, src/headers.cpp:93-108, 122-133) for all records at once, for fqgpu_decode_chunk.
//
// Every field is coded against the previous header, but every dependency is a prefix:
//   STRING  field, record r: new when its flag byte is nonzero; the exclusive count of new flags indexes
//                  contentLength, the exclusive sum of those lengths is the offset into content; a "same"
//                  record takes the value of the last new record <= r (the (count - 1)-th content slice) or,
//                  with none, the field of the dataset's first header (Workspace::startNewChunk)
//   NUMERIC field: first header's value + inclusive sum of the u32 deltas at content[4 r], mod 2^32
// Workgroup = 256 records, one per thread:
//   k_chunk_agg     per workgroup and field: new flags / delta sum; per 256 contentLength entries: their sum
//   k_chunk_scan    one workgroup per field: exclusive prefixes of both over the workgroups
//   k_chunk_measure per record: every field's text length -> header length; stream checks; workgroup sums of the
//                   record lengths (then fq_scan_u32_to_u64 over the workgroups: every record's offset)
//   k_chunk_write   layout check against raw_len; only when every check passed: the record table, the fixed
//                   bytes and the headers (built in LDS, stored by consecutive lanes to consecutive bytes)
// fqgpu_decode_chunk_range runs the same passes, then k_chunk_pick (the offsets of a few records) and the WINDOW
// instance of k_chunk_write, which writes only the records of a window, rebased to the window's first byte.
// The host's out_of_range cases are checked record by record and the first failing record wins
// (atomicMin): flags, contentLength or content exhausted, numeric content short, laid-out end > raw_len.
// Every stream read is bounds-checked; content bytes are read only by the write pass, which runs only on a good
// verdict.
// fqgpu_decode_chunk_fasta places the second record form, FastaForm (">hdr\nSEQ\n"), with the same kernels: the chunk
// is still judged on the FASTQ layout -- same checks, same first failing record -- so measure, write and pick carry two
// running sums where the forms differ, the FASTQ offsets to judge by and the FASTA offsets to place by.  The second sums
// live behind the first in the same buffers (tlen[n_tiles ..], toff[n_tiles + 1 ..]): the kernels' arguments, and the
// FASTQ instances with them, are what they were.
#include "fqgpu_internal.h"

#include <charconv>
#include <cstring>
#include <string>
#include <string_view>

namespace {

constexpr unsigned CL_THREADS = 256;
constexpr unsigned CL_STAGE_BYTES = 32768;  // LDS staging of a workgroup's headers (more: written directly)

// ------------------------------------------------------------------ block scans (256 threads)
__device__ __forceinline__ unsigned long long cl_wave_incl(unsigned long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(v, d);
    if (fq_lane() >= (unsigned)d) v += o;
  }
  return v;
}

// exclusive prefix of v over the workgroup, *total = workgroup sum; every thread must call it
__device__ unsigned long long cl_block_excl(unsigned long long v, unsigned long long *total) {
  __shared__ unsigned long long wsum[CL_THREADS / 64];
  const unsigned long long inc = cl_wave_incl(v);
  const unsigned w = threadIdx.x >> 6;
  if (fq_lane() == 63) wsum[w] = inc;
  __syncthreads();
  unsigned long long base = 0, tot = 0;
#pragma unroll
  for (unsigned i = 0; i < CL_THREADS / 64; i++) {
    if (i < w) base += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// text length of std::to_chars(int32)
__device__ __forceinline__ unsigned cl_num_len(uint32_t v) {
  const bool neg = (int32_t)v < 0;
  uint32_t m = neg ? 0u - v : v;
  unsigned d = 1;
  while (m >= 10u) { m /= 10u; d++; }
  return d + (neg ? 1u : 0u);
}

__device__ __forceinline__ void cl_num_write(uint8_t *dst, uint32_t v, unsigned len) {
  const bool neg = (int32_t)v < 0;
  uint32_t m = neg ? 0u - v : v;
  if (neg) dst[0] = '-';
  for (unsigned i = len; i > (neg ? 1u : 0u); i--) {
    dst[i - 1] = (uint8_t)('0' + m % 10u);
    m /= 10u;
  }
}

// The record forms the layout kernels place.  The chunk is judged on FastqForm whichever is placed.
struct FastqForm {  // @hdr\nSEQ\n+\nQUAL\n
  static constexpr bool FASTA = false;
  static constexpr uint8_t LEAD = '@';
  __device__ static uint32_t rec_len(uint32_t hlen, uint32_t len) { return hlen + 2u * len + 5u; }
};
struct FastaForm {  // >hdr\nSEQ\n
  static constexpr bool FASTA = true;
  static constexpr uint8_t LEAD = '>';
  __device__ static uint32_t rec_len(uint32_t hlen, uint32_t len) { return hlen + len + 2u; }
};

struct FieldLds {
  unsigned long long off[CL_THREADS];  // content offset of the workgroup's k-th new value
  uint32_t len[CL_THREADS];
};

// Field f of record r (workgroup t, one record per thread; every thread calls it): text length and source --
// STRING: byte offset of the text in the stage, NUMERIC: the value.  bad: a stream this record needs is exhausted.
__device__ void cl_field(const FqChunkFmt *__restrict__ fmt, const uint8_t *__restrict__ stage, unsigned f, unsigned t,
                         unsigned r, bool in, const uint32_t *__restrict__ agg, const unsigned long long *__restrict__ clp,
                         FieldLds &lds, uint32_t &len, unsigned long long &src, bool &bad) {
  const FqChunkField &F = fmt->f[f];
  const unsigned nt = fmt->n_tiles;
  const uint32_t before = agg[(size_t)f * nt + t];  // new flags / delta sum of the workgroups in front
  if (F.type == 1) {
    const bool has = in && r < F.n_flags;
    if (in && !has) bad = true;
    const bool isnew = has && stage[F.flags + r] != 0;
    const uint32_t Nt = before;
    unsigned long long tmp;
    const uint32_t loc = (uint32_t)cl_block_excl(isnew ? 1ull : 0ull, &tmp);
    const unsigned long long j = (unsigned long long)Nt + loc;  // this record's contentLength index
    uint32_t l = 0;
    if (isnew) {
      if (j < F.n_lengths) l = stage[F.lengths + j];
      else bad = true;
    }
    // Σ contentLength[0 .. min(Nt, n_lengths)) = prefix of whole groups of 256 + the rest of one group
    const uint32_t lim = Nt < F.n_lengths ? Nt : F.n_lengths;
    const uint32_t ct = Nt / CL_THREADS;
    const unsigned long long k = (unsigned long long)ct * CL_THREADS + threadIdx.x;
    const uint32_t part = k < lim ? stage[F.lengths + k] : 0u;
    unsigned long long both;
    const unsigned long long ex = cl_block_excl(((unsigned long long)part << 32) | l, &both);
    const unsigned long long base = clp[(size_t)f * (nt + 1) + ct] + (both >> 32);
    const unsigned long long off = base + (ex & 0xFFFFFFFFull);
    if (isnew && j < F.n_lengths && off + l > F.n_content) bad = true;
    if (isnew) { lds.off[loc] = off; lds.len[loc] = l; }
    __syncthreads();
    len = 0; src = 0;
    if (isnew) {
      len = l; src = F.content + off;
    } else if (has) {
      if (loc > 0) {
        len = lds.len[loc - 1]; src = F.content + lds.off[loc - 1];
      } else if (Nt > 0) {  // the last new value lies in front of the workgroup: contentLength index Nt - 1
        const uint32_t pl = Nt - 1 < F.n_lengths ? stage[F.lengths + Nt - 1] : 0u;
        len = pl; src = F.content + (base >= pl ? base - pl : 0);
      } else {
        len = F.first_len; src = fmt->first + F.first_off;
      }
    }
    __syncthreads();
  } else {
    const bool has = in && 4ull * r + 4 <= F.n_content;
    if (in && !has) bad = true;
    const uint32_t d = has ? *reinterpret_cast<const uint32_t *>(stage + F.content + 4ull * r) : 0u;
    unsigned long long tmp;
    const unsigned long long ex = cl_block_excl(d, &tmp);
    const uint32_t v = (uint32_t)F.first_val + before + (uint32_t)(ex + d);
    src = v;
    len = in ? cl_num_len(v) : 0u;
  }
}

__global__ __launch_bounds__(CL_THREADS) void k_chunk_agg(const FqChunkFmt *__restrict__ fmt, const uint8_t *__restrict__ stage,
                                                          uint32_t *__restrict__ agg, uint32_t *__restrict__ cls) {
  const unsigned t = blockIdx.x, f = blockIdx.y, nt = fmt->n_tiles;
  const FqChunkField &F = fmt->f[f];
  const unsigned r = t * CL_THREADS + threadIdx.x;
  const bool in = r < fmt->n_recs;
  unsigned long long a = 0, c = 0;
  if (F.type == 1) {
    a = (in && r < F.n_flags && stage[F.flags + r] != 0) ? 1u : 0u;
    c = r < F.n_lengths ? stage[F.lengths + r] : 0u;  // contentLength entries r (group t)
  } else if (in && 4ull * r + 4 <= F.n_content) {
    a = *reinterpret_cast<const uint32_t *>(stage + F.content + 4ull * r);
  }
  unsigned long long sa, sc;
  (void)cl_block_excl(a, &sa);
  (void)cl_block_excl(c, &sc);
  if (threadIdx.x == 0) {
    agg[(size_t)f * nt + t] = (uint32_t)sa;  // (delta sums wrap mod 2^32 like the values)
    cls[(size_t)f * nt + t] = (uint32_t)sc;
  }
}

// one workgroup per field: agg -> exclusive prefix in place (mod 2^32), cls -> clp[0 .. n_tiles] (u64)
__global__ __launch_bounds__(CL_THREADS) void k_chunk_scan(const FqChunkFmt *__restrict__ fmt, uint32_t *__restrict__ agg,
                                                           const uint32_t *__restrict__ cls, unsigned long long *__restrict__ clp) {
  const unsigned f = blockIdx.x, nt = fmt->n_tiles;
  uint32_t *a = agg + (size_t)f * nt;
  const uint32_t *c = cls + (size_t)f * nt;
  unsigned long long *p = clp + (size_t)f * (nt + 1);
  unsigned long long ca = 0, cc = 0;
  for (unsigned b = 0; b < nt; b += CL_THREADS) {
    const unsigned i = b + threadIdx.x;
    const unsigned long long va = i < nt ? a[i] : 0u, vc = i < nt ? c[i] : 0u;
    unsigned long long ta, tc;
    const unsigned long long ea = cl_block_excl(va, &ta), ec = cl_block_excl(vc, &tc);
    if (i < nt) { a[i] = (uint32_t)(ca + ea); p[i] = cc + ec; }
    ca += ta; cc += tc;
  }
  if (threadIdx.x == 0) p[nt] = cc;
}

template <class FORM>
__global__ __launch_bounds__(CL_THREADS) void k_chunk_measure(const FqChunkFmt *__restrict__ fmt, const uint8_t *__restrict__ stage,
                                                              const uint32_t *__restrict__ agg, const unsigned long long *__restrict__ clp,
                                                              uint32_t *__restrict__ hlen_out, uint32_t *__restrict__ tlen,
                                                              FqChunkResult *__restrict__ res) {
  __shared__ FieldLds lds;
  const unsigned t = blockIdx.x, nf = fmt->n_fields;
  const unsigned r = t * CL_THREADS + threadIdx.x;
  const bool in = r < fmt->n_recs;
  uint32_t hlen = in ? nf : 0u;  // '@' and the separators
  bool bad = false;
  for (unsigned f = 0; f < nf; f++) {
    uint32_t len;
    unsigned long long src;
    cl_field(fmt, stage, f, t, r, in, agg, clp, lds, len, src, bad);
    hlen += len;
  }
  if (in && bad) atomicMin(&res->bad, (unsigned long long)r);
  const uint16_t *readlens = reinterpret_cast<const uint16_t *>(stage + fmt->readlens);
  const uint32_t rlen = in ? FastqForm::rec_len(hlen, readlens[r]) : 0u;
  if (in) hlen_out[r] = hlen;
  unsigned long long tot;
  (void)cl_block_excl(rlen, &tot);
  if (threadIdx.x == 0) tlen[t] = (uint32_t)tot;
  if constexpr (FORM::FASTA) {  // the sums to place by, behind the sums to judge by
    (void)cl_block_excl(in ? FORM::rec_len(hlen, readlens[r]) : 0u, &tot);
    if (threadIdx.x == 0) tlen[fmt->n_tiles + t] = (uint32_t)tot;
  }
}

// WINDOW (fqgpu_decode_chunk_range): only the records [win.w0, win.w1) are written -- record table entries at their
// numbers in the chunk, bytes at offsets relative to the window's first byte (*win.base) -- while the check against
// raw_len still covers every record.  A workgroup without window records returns at once when the chunk fits.
struct ChunkWindow {
  unsigned w0, w1;
  const unsigned long long *base;  // device: the offset of record w0 in the whole chunk (k_chunk_pick)
};

template <bool WINDOW, class FORM>
__global__ __launch_bounds__(CL_THREADS) void k_chunk_write(const FqChunkFmt *__restrict__ fmt, const uint8_t *__restrict__ stage,
                                                            const uint32_t *__restrict__ agg, const unsigned long long *__restrict__ clp,
                                                            const uint32_t *__restrict__ hlen_in, const unsigned long long *__restrict__ toff,
                                                            FqChunkResult *__restrict__ res, uint8_t *__restrict__ raw,
                                                            fqgpu_rec *__restrict__ recs, ChunkWindow win) {
  __shared__ FieldLds lds;
  __shared__ uint8_t hbuf[CL_STAGE_BYTES];
  __shared__ uint32_t s_hoff[CL_THREADS + 1];
  __shared__ unsigned long long s_roff[CL_THREADS];
  __shared__ int s_ok;
  const unsigned t = blockIdx.x, nf = fmt->n_fields, nt = fmt->n_tiles;
  const unsigned r = t * CL_THREADS + threadIdx.x;
  const bool in = r < fmt->n_recs;
  const unsigned long long raw_len = fmt->raw_len, total = toff[nt];
  if (WINDOW && (t * CL_THREADS + CL_THREADS <= win.w0 || t * CL_THREADS >= win.w1) && total <= raw_len) {
    if (t == 0 && threadIdx.x == 0) res->total = total;
    return;
  }
  const bool win_rec = WINDOW ? in && r >= win.w0 && r < win.w1 : in;
  const unsigned long long base = WINDOW ? *win.base : 0ull;
  const uint16_t *readlens = reinterpret_cast<const uint16_t *>(stage + fmt->readlens);
  const uint32_t hlen = in ? hlen_in[r] : 0u, rl = in ? readlens[r] : 0u;
  const uint32_t rlen = in ? FastqForm::rec_len(hlen, rl) : 0u;
  unsigned long long tmp;
  const unsigned long long roff = toff[t] + cl_block_excl(rlen, &tmp);
  unsigned long long poff = roff;  // where the record lies in the form that is placed
  if constexpr (FORM::FASTA) poff = toff[nt + 1 + t] + cl_block_excl(in ? FORM::rec_len(hlen, rl) : 0u, &tmp);
  // records only move forward: the first one that ends behind raw_len is the host's failing record
  if (in && roff + rlen > raw_len) atomicMin(&res->bad, (unsigned long long)r);
  if (t == 0 && threadIdx.x == 0) res->total = total;
  // (only a total > raw_len makes this kernel touch res->bad, and then no workgroup writes)
  if (threadIdx.x == 0) s_ok = total <= raw_len && __hip_atomic_load(&res->bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ~0ull;
  __syncthreads();
  if (!s_ok) return;
  const unsigned long long wroff = WINDOW ? (win_rec ? poff - base : 0ull) : poff;  // where the record goes
  if (win_rec) {
    const uint32_t seq_off = (uint32_t)(wroff + hlen + 1), qual_off = FORM::FASTA ? 0u : seq_off + rl + 3u;
    fqgpu_rec rec;
    rec.seq_off = seq_off; rec.qual_off = qual_off; rec.len = rl;
    recs[r] = rec;
    raw[seq_off - 1] = '\n';
    raw[seq_off + rl] = '\n';
    if constexpr (!FORM::FASTA) {
      raw[seq_off + rl + 1] = '+'; raw[seq_off + rl + 2] = '\n';
      raw[qual_off + rl] = '\n';
    }
  }
  unsigned long long htot;
  const unsigned long long hex = cl_block_excl(win_rec ? hlen : 0u, &htot);
  const bool staged = htot <= CL_STAGE_BYTES;  // (uniform)
  s_hoff[threadIdx.x] = (uint32_t)hex;
  s_roff[threadIdx.x] = wroff;
  if (threadIdx.x == 0) s_hoff[CL_THREADS] = (uint32_t)htot;
  uint8_t *dst = staged ? hbuf + hex : raw + wroff;
  if (win_rec) dst[0] = FORM::LEAD;
  uint32_t p = 1;
  const unsigned long long stage_len = fmt->stage_len;
  for (unsigned f = 0; f < nf; f++) {
    uint32_t len;
    unsigned long long src;
    bool bad = false;
    cl_field(fmt, stage, f, t, r, in, agg, clp, lds, len, src, bad);
    if (!win_rec) continue;
    if (fmt->f[f].type == 1) {
      if (src + len <= stage_len)
        for (uint32_t i = 0; i < len; i++) dst[p + i] = stage[src + i];
    } else {
      cl_num_write(dst + p, (uint32_t)src, len);
    }
    p += len;
    if (f + 1 < nf) dst[p++] = fmt->f[f].sep;
  }
  __syncthreads();
  if (!staged) return;
  // consecutive lanes -> consecutive bytes of one header (mostly)
  for (uint32_t k = threadIdx.x; k < (uint32_t)htot; k += CL_THREADS) {
    unsigned lo = 0, hi = CL_THREADS - 1;  // the last record whose header starts at or before k (WINDOW: records
                                           // outside the window have empty headers in front of or behind it)
    while (lo < hi) {
      const unsigned mid = (lo + hi + 1) >> 1;
      if (s_hoff[mid] <= k) lo = mid; else hi = mid - 1;
    }
    raw[s_roff[lo] + (k - s_hoff[lo])] = hbuf[k];
  }
}

// the offset of record q.r[i] in the whole chunk (n_recs: the end of the last record) -> at[i]; one workgroup per record
struct ChunkPicks {
  unsigned r[4];
};
template <class FORM>
__global__ __launch_bounds__(CL_THREADS) void k_chunk_pick(const FqChunkFmt *__restrict__ fmt, const uint8_t *__restrict__ stage,
                                                           const uint32_t *__restrict__ hlen_in, const unsigned long long *__restrict__ toff,
                                                           ChunkPicks q, unsigned long long *__restrict__ at) {
  const unsigned rq = q.r[blockIdx.x], nt = fmt->n_tiles, t = rq / CL_THREADS;
  const unsigned long long *poff = FORM::FASTA ? toff + nt + 1 : toff;  // the offsets of the form that is placed
  if (t >= nt) {  // rq = n_recs, a multiple of 256
    if (threadIdx.x == 0) at[blockIdx.x] = poff[nt];
    return;
  }
  const unsigned r = t * CL_THREADS + threadIdx.x;
  const bool in = r < fmt->n_recs;
  const uint16_t *readlens = reinterpret_cast<const uint16_t *>(stage + fmt->readlens);
  const uint32_t rlen = in ? FORM::rec_len(hlen_in[r], readlens[r]) : 0u;
  unsigned long long tmp;
  const unsigned long long ex = cl_block_excl(rlen, &tmp);
  if (r == rq) at[blockIdx.x] = poff[t] + ex;
}

}  // namespace

// Checks the format and the dataset's first header, gathers the header streams, readlens and the first header into
// the host stage (one upload).  FQGPU_E_ARG: a format the host coder does not take.
int fq_chunk_prepare(const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs, size_t raw_len, ChunkScratch &cs) {
  const unsigned nf = hdr->n_fields;
  if (!nf || nf > FQGPU_HDR_MAX_FIELDS || !hdr->field_types || (nf > 1 && !hdr->separators) || !hdr->first_header ||
      !hdr->sizes || !hdr->streams)
    return FQGPU_E_ARG;
  if (hdr->first_header_len < 1 || hdr->first_header_len > 65535 || hdr->first_header[0] != '@') return FQGPU_E_ARG;
  FqChunkFmt fmt;
  memset(&fmt, 0, sizeof(fmt));
  fmt.n_fields = nf;
  fmt.n_recs = (uint32_t)n_recs;
  fmt.n_tiles = (uint32_t)((n_recs + CL_THREADS - 1) / CL_THREADS);
  fmt.raw_len = raw_len;
  auto align = [](size_t x) { return (x + 15) & ~(size_t)15; };
  size_t at = align(sizeof(FqChunkFmt));
  fmt.readlens = at; at = align(at + n_recs * 2);
  fmt.first = at; at = align(at + hdr->first_header_len);
  // the first header's fields (headers::fromHeader: a field ends at the first separator from its second byte on)
  const char *h = reinterpret_cast<const char *>(hdr->first_header);
  const char *s = h + 1, *const end = h + hdr->first_header_len;
  for (unsigned i = 0; i < nf; i++) {
    FqChunkField &F = fmt.f[i];
    if (hdr->field_types[i] > 1) return FQGPU_E_ARG;
    F.type = hdr->field_types[i];
    F.sep = i + 1 < nf ? (uint8_t)hdr->separators[i] : 0;
    const char *e = end;
    if (i + 1 < nf) {
      e = s < end ? s + 1 : end;
      while (e < end && *e != hdr->separators[i]) ++e;
    }
    F.first_off = (uint32_t)(s - h);
    F.first_len = (uint32_t)(e - s);
    if (F.type == 0) {
      int32_t v = 0;
      if (std::from_chars(s, e, v).ec != std::errc()) return FQGPU_E_ARG;  // the host's parseNumeric throws
      F.first_val = v;
    }
    s = e < end ? e + 1 : end;
    const fqgpu_field_sizes &z = hdr->sizes[i];
    const uint8_t *const *st = hdr->streams + 3 * (size_t)i;
    if ((z.isDifferentFlag && !st[0]) || (z.content && !st[1]) || (z.contentLength && !st[2])) return FQGPU_E_ARG;
    F.n_flags = z.isDifferentFlag; F.n_content = z.content; F.n_lengths = z.contentLength;
    F.flags = at; at = align(at + z.isDifferentFlag);
    F.content = at; at = align(at + z.content);
    F.lengths = at; at = align(at + z.contentLength);
  }
  fmt.stage_len = at;
  if (!cs.host_grow(at)) return FQGPU_E_NOMEM;
  uint8_t *b = cs.host;
  memcpy(b, &fmt, sizeof(fmt));
  memcpy(b + fmt.readlens, readlens, n_recs * 2);
  memcpy(b + fmt.first, hdr->first_header, hdr->first_header_len);
  for (unsigned i = 0; i < nf; i++) {
    const FqChunkField &F = fmt.f[i];
    const uint8_t *const *st = hdr->streams + 3 * (size_t)i;
    if (F.n_flags) memcpy(b + F.flags, st[0], F.n_flags);
    if (F.n_content) memcpy(b + F.content, st[1], F.n_content);
    if (F.n_lengths) memcpy(b + F.lengths, st[2], F.n_lengths);
  }
  cs.stage_len = at;
  cs.n_fields = nf;
  cs.n_tiles = fmt.n_tiles;
  return FQGPU_OK;
}

// Uploads the stage and runs the passes every record's offset depends on: per-workgroup counts and sums, their scans,
// the measure pass, the scan of the record offsets (fasta: of both forms' offsets).
static int chunk_prefix(hipStream_t st, ChunkScratch &cs, bool fasta) {
  const unsigned nt = cs.n_tiles, nf = cs.n_fields;
  int rc;
  if ((rc = cs.stage.reserve(cs.stage_len)) || (rc = cs.agg.reserve((size_t)nf * nt * 4)) ||
      (rc = cs.cls.reserve((size_t)nf * nt * 4)) || (rc = cs.clp.reserve((size_t)nf * (nt + 1) * 8)) ||
      (rc = cs.hlen.reserve((size_t)nt * CL_THREADS * 4)) || (rc = cs.tlen.reserve((size_t)nt * 2 * 4)) ||
      (rc = cs.toff.reserve((size_t)(nt + 1) * 2 * 8)) || (rc = cs.res.reserve(sizeof(FqChunkResult))))
    return rc;
  const FqChunkFmt *fmt = cs.stage.as<FqChunkFmt>();
  const uint8_t *stage = cs.stage.as<uint8_t>();
  FqChunkResult *res = cs.res.as<FqChunkResult>();
  FQ_HIP(hipMemcpyAsync(cs.stage.p, cs.host, cs.stage_len, hipMemcpyHostToDevice, st));
  FQ_HIP(hipMemsetAsync(res, 0xFF, sizeof(unsigned long long), st));
  FQ_HIP(hipMemsetAsync(&res->total, 0, sizeof(unsigned long long), st));
  if (nt) {
    hipLaunchKernelGGL(k_chunk_agg, dim3(nt, nf), dim3(CL_THREADS), 0, st, fmt, stage, cs.agg.as<uint32_t>(), cs.cls.as<uint32_t>());
    FQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_chunk_scan, dim3(nf), dim3(CL_THREADS), 0, st, fmt, cs.agg.as<uint32_t>(), cs.cls.as<uint32_t>(),
                       cs.clp.as<unsigned long long>());
    FQ_HIP(hipGetLastError());
    const auto measure = fasta ? k_chunk_measure<FastaForm> : k_chunk_measure<FastqForm>;
    hipLaunchKernelGGL(measure, dim3(nt), dim3(CL_THREADS), 0, st, fmt, stage, cs.agg.as<uint32_t>(),
                       cs.clp.as<unsigned long long>(), cs.hlen.as<uint32_t>(), cs.tlen.as<uint32_t>(), res);
    FQ_HIP(hipGetLastError());
    if ((rc = fq_scan_u32_to_u64(st, cs.tlen.as<uint32_t>(), nt, cs.toff.as<unsigned long long>(), cs.scan_tmp))) return rc;
    if (fasta && (rc = fq_scan_u32_to_u64(st, cs.tlen.as<uint32_t>() + nt, nt, cs.toff.as<unsigned long long>() + nt + 1, cs.scan_tmp)))
      return rc;
  }
  return FQGPU_OK;
}

// Uploads the stage, decodes and lays out the chunk into raw_dev / recs_dev, waits, and reports: *bad = the first
// failing record (~0: none), *total = bytes laid out.  Nothing is written to raw_dev / recs_dev unless *bad is ~0 and
// *total <= raw_len.
// q != NULL (fqgpu_decode_chunk_range): the records [q[0], q[3]) alone; at[i] = the offset of record q[i] in the whole
// chunk (q[i] = n_recs: its end); with `write`, the window's records go to recs_dev[r] and to raw_dev at offsets
// relative to at[0] (only the window's bytes are written).  Without, nothing is written and the layout is still judged.
// fasta (with q): the records are placed as FASTA -- at[] and the record table speak of that layout -- while *bad and
// *total are still those of the FASTQ layout.
int fq_chunk_layout(hipStream_t st, ChunkScratch &cs, uint8_t *raw_dev, fqgpu_rec *recs_dev, const unsigned q[4], bool write,
                    unsigned long long *bad, unsigned long long *total, unsigned long long at[4], bool fasta) {
  const unsigned nt = cs.n_tiles;
  int rc;
  if (fasta && !q) return FQGPU_E_ARG;
  if ((rc = chunk_prefix(st, cs, fasta)) || (q && (rc = cs.pick.reserve(4 * sizeof(unsigned long long))))) return rc;
  FqChunkResult *res = cs.res.as<FqChunkResult>();
  unsigned long long *pick = cs.pick.as<unsigned long long>();
  const auto write_pass = [&](auto kernel, ChunkWindow win) {
    hipLaunchKernelGGL(kernel, dim3(nt), dim3(CL_THREADS), 0, st, cs.stage.as<FqChunkFmt>(), cs.stage.as<uint8_t>(),
                       cs.agg.as<uint32_t>(), cs.clp.as<unsigned long long>(), cs.hlen.as<uint32_t>(),
                       cs.toff.as<unsigned long long>(), res, raw_dev, recs_dev, win);
    return hipGetLastError();
  };
  if (nt && q) {
    hipLaunchKernelGGL(fasta ? k_chunk_pick<FastaForm> : k_chunk_pick<FastqForm>, dim3(4), dim3(CL_THREADS), 0, st,
                       cs.stage.as<FqChunkFmt>(), cs.stage.as<uint8_t>(), cs.hlen.as<uint32_t>(), cs.toff.as<unsigned long long>(),
                       ChunkPicks{{q[0], q[1], q[2], q[3]}}, pick);
    FQ_HIP(hipGetLastError());
    const ChunkWindow win{write ? q[0] : 0u, write ? q[3] : 0u, pick};
    FQ_HIP(fasta ? write_pass(k_chunk_write<true, FastaForm>, win) : write_pass(k_chunk_write<true, FastqForm>, win));
  } else if (nt) {
    FQ_HIP(write_pass(k_chunk_write<false, FastqForm>, ChunkWindow{}));
  } else if (q) {
    FQ_HIP(hipMemsetAsync(pick, 0, 4 * sizeof(unsigned long long), st));
  }
  FqChunkResult h;
  FQ_HIP(hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, st));
  if (q) FQ_HIP(hipMemcpyAsync(at, pick, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  *bad = h.bad;
  *total = h.total;
  return FQGPU_OK;
}
