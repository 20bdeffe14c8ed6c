// CRC-32 (zlib: reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF) of a chunk that lies in HBM
// (include/fqgpu.h: fqgpu_chunk_crc32, fqgpu_dblock_crc32).  Extension: nothing in the reference.
//
// A CRC is the remainder of a polynomial division over GF(2), and remainders add: the remainder of A || B is
// rem(A) x^(8 |B|) + rem(B).  So every workgroup takes the remainder of its own slice (k_crc_slices), and one
// workgroup folds the slices' remainders with the powers of x that stand for the bytes behind each slice and
// adds the init / final-xor terms for the whole length (k_crc_fold): no serial pass over the data anywhere.
//
// Inside a slice the reads are coalesced 16-byte loads: thread t of 256 owns the words 4 t .. 4 t + 3 of every
// 4 KiB row, and its four running remainders are advanced from row to row by the FIXED multiplier x^(8 * 4096) --
// four byte-table lookups in LDS per word, like slice-by-4 -- so that the rows of a slice need no communication.
// At the end of the slice each thread's remainders get the factor that stands for their place in the row
// (x^(32 (1024 - word)): a table too) and the workgroup xors them together.
//
// Values are in the CRC's own bit order: bit 31 of a word is the coefficient of x^0, bit 0 that of x^31.  A
// "remainder" below is D(x) x^32 mod P for the data D so far (the state of the table-driven algorithm started
// from 0), so that appending a little-endian word w to state s gives (s ^ w) x^32.
#include "fqgpu_internal.h"

namespace {

constexpr unsigned CRC_POLY = 0xEDB88320u;
constexpr unsigned CRC_THREADS = 256;       // threads of a slice workgroup, 16 bytes each per row
constexpr unsigned CRC_ROW_BYTES = 4096;    // one row: CRC_THREADS * 16
constexpr unsigned CRC_SLICE_BYTES = 131072;  // one workgroup's slice: 32 rows
constexpr unsigned CRC_FOLD_THREADS = 1024;
static_assert(CRC_ROW_BYTES == CRC_THREADS * 16 && CRC_SLICE_BYTES % (4 * CRC_ROW_BYTES) == 0, "slice = whole groups of four rows");

// tables (u32 words): [0, 1024) byte tables of the multiplier x^(8 CRC_ROW_BYTES), [1024, 2048) of x^32,
// [2048, 2304) the place factor of every thread
constexpr unsigned TAB_ROW = 0, TAB_W32 = 1024, TAB_FAC = 2048, TAB_WORDS = 2304;

// a * b mod P (32 steps: one bit of a, one multiplication of b by x)
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= (a & 0x80000000u) ? b : 0u;
    a <<= 1;
    b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
  }
  return p;
}
// x^n mod P, square and multiply
__host__ __device__ inline uint32_t crc_xpow(unsigned long long n) {
  uint32_t r = 0x80000000u, sq = 0x40000000u;
  for (; n; n >>= 1) {
    if (n & 1u) r = crc_mul(r, sq);
    sq = crc_mul(sq, sq);
  }
  return r;
}

__global__ void __launch_bounds__(256) k_crc_tables(uint32_t *__restrict__ tab) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TAB_WORDS) return;
  if (t < TAB_FAC) {
    const uint32_t m = crc_xpow(t < TAB_W32 ? 8ull * CRC_ROW_BYTES : 32ull);
    tab[t] = crc_mul((t & 255u) << (8u * ((t >> 8) & 3u)), m);
  } else {
    tab[t] = crc_xpow(32ull * (CRC_ROW_BYTES / 4 - 3 - 4 * (t - TAB_FAC)));  // the thread's LAST word is 3 + 4 t
  }
}

// v * (the table's multiplier): linear in v, one lookup per byte
__device__ __forceinline__ uint32_t crc_by_table(const uint32_t *tab, uint32_t v) {
  return tab[v & 255u] ^ tab[256u + ((v >> 8) & 255u)] ^ tab[512u + ((v >> 16) & 255u)] ^ tab[768u + (v >> 24)];
}

struct CrcRow {
  uint32_t l[4];
  __device__ __forceinline__ void add(const uint32_t *tab, const uint4 w) {
    l[0] = crc_by_table(tab + TAB_ROW, l[0]) ^ w.x;
    l[1] = crc_by_table(tab + TAB_ROW, l[1]) ^ w.y;
    l[2] = crc_by_table(tab + TAB_ROW, l[2]) ^ w.z;
    l[3] = crc_by_table(tab + TAB_ROW, l[3]) ^ w.w;
  }
  // the thread's share of the remainder of the rows seen
  __device__ __forceinline__ uint32_t close(const uint32_t *tab) const {
    uint32_t v = l[0];
    for (int u = 1; u < 4; u++) v = crc_by_table(tab + TAB_W32, v) ^ l[u];
    return crc_mul(v, tab[TAB_FAC + threadIdx.x]);
  }
};

// rem[g] = remainder of slice g: bytes [g CRC_SLICE_BYTES, min(len, (g + 1) CRC_SLICE_BYTES)).  data is 16-byte aligned.
// The last slice may be short: its whole rows go the same way; what is left behind them (less than a row) is read byte by
// byte, with bounds, as a row of its own whose FRONT is padded with zeros -- zeros in front of data do not change a
// remainder -- and joins the rest as rem(rows) x^(8 left) + rem(left).
__global__ void __launch_bounds__(CRC_THREADS)
k_crc_slices(const uint8_t *__restrict__ data, unsigned long long len, const uint32_t *__restrict__ tab_g, uint32_t *__restrict__ rem) {
  __shared__ uint32_t tab[TAB_WORDS];
  __shared__ uint32_t wave_x[CRC_THREADS / 64];
  for (unsigned i = threadIdx.x; i < TAB_WORDS; i += CRC_THREADS) tab[i] = tab_g[i];
  __syncthreads();
  const unsigned long long base = (unsigned long long)blockIdx.x * CRC_SLICE_BYTES;
  const unsigned long long here = len - base < CRC_SLICE_BYTES ? len - base : CRC_SLICE_BYTES;
  const unsigned rows = (unsigned)(here / CRC_ROW_BYTES), left = (unsigned)(here % CRC_ROW_BYTES);
  const uint4 *p = reinterpret_cast<const uint4 *>(data + base) + threadIdx.x;
  CrcRow acc = {{0, 0, 0, 0}};
  unsigned k = 0;
  for (; k + 4 <= rows; k += 4) {  // four loads in flight in front of the dependent lookups
    const uint4 w0 = p[(k + 0) * CRC_THREADS], w1 = p[(k + 1) * CRC_THREADS], w2 = p[(k + 2) * CRC_THREADS], w3 = p[(k + 3) * CRC_THREADS];
    acc.add(tab, w0); acc.add(tab, w1); acc.add(tab, w2); acc.add(tab, w3);
  }
  for (; k < rows; k++) acc.add(tab, p[k * CRC_THREADS]);
  uint32_t x = acc.close(tab);
  if (left) {  // (uniform: the last workgroup alone)
    const uint8_t *tail = data + base + (unsigned long long)rows * CRC_ROW_BYTES;
    const unsigned pad = CRC_ROW_BYTES - left;
    uint32_t w[4] = {0, 0, 0, 0};
    for (unsigned i = 0; i < 16; i++) {
      const unsigned v = threadIdx.x * 16 + i;
      if (v >= pad) w[i >> 2] |= (uint32_t)tail[v - pad] << (8 * (i & 3));
    }
    CrcRow last = {{w[0], w[1], w[2], w[3]}};
    x = crc_mul(x, crc_xpow(8ull * left)) ^ last.close(tab);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x ^= __shfl_xor(x, d);
  if (fq_lane() == 0) wave_x[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned w = 1; w < CRC_THREADS / 64; w++) x ^= wave_x[w];
    rem[blockIdx.x] = x;
  }
}

// out = {crc32, len lo, len hi, 0} from the remainders of n_full whole slices and, len % CRC_SLICE_BYTES != 0, of the
// short one behind them.  One workgroup: thread t folds a run of c consecutive remainders (Horner with x^(8 slice)),
// the runs are joined pairwise in ten levels whose multiplier is squared from level to level.  The list is padded with
// zeros in FRONT to 1024 c entries.
__global__ void __launch_bounds__(CRC_FOLD_THREADS)
k_crc_fold(const uint32_t *__restrict__ rem, unsigned n_full, unsigned long long len, uint32_t *__restrict__ out) {
  __shared__ uint32_t v[CRC_FOLD_THREADS];
  const unsigned t = threadIdx.x;
  const unsigned c = (n_full + CRC_FOLD_THREADS - 1) / CRC_FOLD_THREADS;
  const unsigned long long pad = (unsigned long long)c * CRC_FOLD_THREADS - n_full;
  const uint32_t f = crc_xpow(8ull * CRC_SLICE_BYTES);
  uint32_t acc = 0;
  for (unsigned q = 0; q < c; q++) {
    const unsigned long long at = (unsigned long long)t * c + q;
    acc = crc_mul(acc, f) ^ (at >= pad ? rem[at - pad] : 0u);
  }
  v[t] = acc;
  uint32_t g = crc_xpow(8ull * CRC_SLICE_BYTES * c);
  for (unsigned s = 1; s < CRC_FOLD_THREADS; s <<= 1) {
    __syncthreads();
    if ((t & (2 * s - 1)) == 2 * s - 1) v[t] = crc_mul(v[t - s], g) ^ v[t];
    g = crc_mul(g, g);
  }
  if (t == CRC_FOLD_THREADS - 1) {
    const unsigned long long left = len % CRC_SLICE_BYTES;
    const uint32_t pure = crc_mul(v[t], crc_xpow(8ull * left)) ^ (left ? rem[n_full] : 0u);
    // started from 0xFFFFFFFF instead of 0: that state, carried over all len bytes, comes on top; then the final xor
    out[0] = pure ^ crc_mul(0xFFFFFFFFu, crc_xpow(8ull * len)) ^ 0xFFFFFFFFu;
    out[1] = (uint32_t)len;
    out[2] = (uint32_t)(len >> 32);
    out[3] = 0;
  }
}

// ---- canonical bytes of a chunk: per record the header line with its '\n', the sequence, "\n+\n", the quality line, '\n'.
// A chunk whose '+' lines are bare IS its canonical bytes, up to the end of its last record.
struct CrcCheck {
  unsigned long long end;  // end of the last record's quality line, '\n' included
  unsigned int not_bare;   // a record with text behind its '+', or whose last '\n' is not inside the chunk
  unsigned int pad;
};

__device__ __forceinline__ unsigned crc_header_start(const fqgpu_rec *recs, unsigned r) {
  return r ? recs[r - 1].qual_off + recs[r - 1].len + 1u : 0u;
}

__global__ void __launch_bounds__(256)
k_crc_check(const fqgpu_rec *__restrict__ recs, unsigned n_recs, unsigned long long raw_len, CrcCheck *__restrict__ chk) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_recs) return;
  const fqgpu_rec rec = recs[r];
  bool odd = rec.qual_off != rec.seq_off + rec.len + 3u || rec.seq_off < crc_header_start(recs, r);
  if (r == n_recs - 1) {
    chk->end = (unsigned long long)rec.qual_off + rec.len + 1ull;
    odd = odd || chk->end > raw_len;
  }
  if (odd) chk->not_bare = 1u;  // (every writer stores the same value)
}

__global__ void __launch_bounds__(256)
k_crc_canon_len(const fqgpu_rec *__restrict__ recs, unsigned n_recs, uint32_t *__restrict__ clen) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_recs) return;
  const unsigned h0 = crc_header_start(recs, r);
  clen[r] = (recs[r].seq_off > h0 ? recs[r].seq_off - h0 : 0u) + 2u * recs[r].len + 4u;
}

// one wave per record
__global__ void __launch_bounds__(256)
k_crc_canon_write(const uint8_t *__restrict__ raw, const fqgpu_rec *__restrict__ recs, unsigned n_recs,
                  const unsigned long long *__restrict__ off, uint8_t *__restrict__ dst) {
  const unsigned waves = (gridDim.x * blockDim.x) >> 6, lane = fq_lane();
  for (unsigned r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_recs; r += waves) {
    const fqgpu_rec rec = recs[r];
    const unsigned h0 = crc_header_start(recs, r), hl = rec.seq_off > h0 ? rec.seq_off - h0 : 0u;
    uint8_t *d = dst + off[r];
    for (unsigned i = lane; i < hl; i += 64) d[i] = raw[h0 + i];  // (ends with the header's '\n')
    d += hl;
    for (unsigned i = lane; i < rec.len; i += 64) { d[i] = raw[rec.seq_off + i]; d[rec.len + 3 + i] = raw[rec.qual_off + i]; }
    if (lane == 0) { d[rec.len] = '\n'; d[rec.len + 1] = '+'; d[rec.len + 2] = '\n'; d[2 * rec.len + 3] = '\n'; }
  }
}

int crc_prepare(fqgpu_ctx *ctx, hipStream_t st) {
  CrcScratch &cs = ctx->crc;
  int rc;
  if (!cs.host) FQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&cs.host), 32, hipHostMallocPortable));
  if ((rc = cs.res.reserve(16)) || (rc = cs.tab.reserve(TAB_WORDS * 4))) return rc;
  if (!cs.tab_built) {
    hipLaunchKernelGGL(k_crc_tables, dim3((TAB_WORDS + 255) / 256), dim3(256), 0, st, cs.tab.as<uint32_t>());
    FQ_HIP(hipGetLastError());
    cs.tab_built = true;
  }
  return FQGPU_OK;
}

// Queues the digest of data_dev[0, len) on st; {crc32, len lo, len hi} land in ctx->crc.host behind it.  data_dev: 16-byte
// aligned (every hipMalloc'ed block is).
int crc_launch(fqgpu_ctx *ctx, hipStream_t st, const uint8_t *data_dev, size_t len) {
  if ((reinterpret_cast<uintptr_t>(data_dev) & 15u) || len >= ((size_t)1 << 44)) return FQGPU_E_ARG;
  int rc = crc_prepare(ctx, st);
  if (rc) return rc;
  CrcScratch &cs = ctx->crc;
  const size_t n_slices = (len + CRC_SLICE_BYTES - 1) / CRC_SLICE_BYTES;
  if ((rc = cs.rem.reserve((n_slices + 1) * 4))) return rc;
  fq_timer_span_begin(ctx, "crc32", st);
  if (n_slices)
    hipLaunchKernelGGL(k_crc_slices, dim3((unsigned)n_slices), dim3(CRC_THREADS), 0, st, data_dev, (unsigned long long)len,
                       cs.tab.as<uint32_t>(), cs.rem.as<uint32_t>());
  hipLaunchKernelGGL(k_crc_fold, dim3(1), dim3(CRC_FOLD_THREADS), 0, st, cs.rem.as<uint32_t>(), (unsigned)(len / CRC_SLICE_BYTES),
                     (unsigned long long)len, cs.res.as<uint32_t>());
  fq_timer_span_end(ctx, st);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipMemcpyAsync(cs.host, cs.res.p, 16, hipMemcpyDeviceToHost, st));
  return FQGPU_OK;
}

}  // namespace

void CrcScratch::release_host() {
  if (host) (void)hipHostFree(host);
  host = nullptr;
  tab_built = false;
}

// The digest of data_dev[0, len), waited for.
int fq_crc_bytes(fqgpu_ctx *ctx, hipStream_t st, const uint8_t *data_dev, size_t len, uint32_t *crc) {
  const int rc = crc_launch(ctx, st, data_dev, len);
  if (rc) return rc;
  FQ_HIP(hipStreamSynchronize(st));
  *crc = ctx->crc.host[0];
  return FQGPU_OK;
}

// The digest of the canonical bytes of the chunk v (raw_dev[0, raw_len) with the record table recs_dev), on st, waited for;
// *len = their number.  Bare '+' lines: the chunk itself up to the end of its last record -- which is raw_len for every
// chunk the parsers cut, so the check of the record table and the digest of raw_dev[0, raw_len) are queued together and
// waited for ONCE (32 bytes come back); a chunk that ends elsewhere is digested again up to there.  Otherwise the
// canonical bytes are gathered into scratch first (one more pass over the chunk: correctness only).
int fq_crc_canonical(fqgpu_ctx *ctx, hipStream_t st, const FqChunkView &v, uint32_t *crc, size_t *len) {
  const uint8_t *const raw_dev = v.raw;
  const fqgpu_rec *const recs_dev = v.recs;
  const size_t raw_len = v.raw_len, n_recs = v.n_recs;
  if (!n_recs || n_recs >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  CrcScratch &cs = ctx->crc;
  int rc;
  if ((rc = crc_prepare(ctx, st)) || (rc = cs.chk.reserve(sizeof(CrcCheck)))) return rc;
  const unsigned R = (unsigned)n_recs, rec_wgs = (R + 255u) / 256u;
  static_assert(sizeof(CrcCheck) == 16, "lands behind the result words in the page-locked block");
  const CrcCheck &chk = *reinterpret_cast<const CrcCheck *>(cs.host + 4);
  FQ_HIP(hipMemsetAsync(cs.chk.p, 0, sizeof(CrcCheck), st));
  hipLaunchKernelGGL(k_crc_check, dim3(rec_wgs), dim3(256), 0, st, recs_dev, R, (unsigned long long)raw_len, cs.chk.as<CrcCheck>());
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipMemcpyAsync(cs.host + 4, cs.chk.p, sizeof(CrcCheck), hipMemcpyDeviceToHost, st));
  if ((rc = crc_launch(ctx, st, raw_dev, raw_len))) return rc;
  FQ_HIP(hipStreamSynchronize(st));
  if (!chk.not_bare) {
    *len = (size_t)chk.end;
    if (*len != raw_len) return fq_crc_bytes(ctx, st, raw_dev, *len, crc);  // (bytes behind the last record: a caller's own table)
    *crc = cs.host[0];
    return FQGPU_OK;
  }
  if ((rc = cs.clen.reserve(n_recs * 4)) || (rc = cs.coff.reserve((n_recs + 1) * 8))) return rc;
  hipLaunchKernelGGL(k_crc_canon_len, dim3(rec_wgs), dim3(256), 0, st, recs_dev, R, cs.clen.as<uint32_t>());
  FQ_HIP(hipGetLastError());
  if ((rc = fq_scan_u32_to_u64(st, cs.clen.as<uint32_t>(), n_recs, cs.coff.as<unsigned long long>(), cs.scan_tmp))) return rc;
  unsigned long long total = 0;
  FQ_HIP(hipMemcpyAsync(&total, cs.coff.as<unsigned long long>() + n_recs, 8, hipMemcpyDeviceToHost, st));
  FQ_HIP(hipStreamSynchronize(st));
  if ((rc = cs.flat.reserve((size_t)total + 64))) return rc;
  hipLaunchKernelGGL(k_crc_canon_write, dim3((unsigned)min((n_recs + 3) / 4, (size_t)8192)), dim3(256), 0, st, raw_dev, recs_dev, R,
                     cs.coff.as<unsigned long long>(), cs.flat.as<uint8_t>());
  FQ_HIP(hipGetLastError());
  *len = (size_t)total;
  return fq_crc_bytes(ctx, st, cs.flat.as<uint8_t>(), *len, crc);
}
