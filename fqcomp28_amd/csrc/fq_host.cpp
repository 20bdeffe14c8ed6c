// Host-side helpers of the path's callers: the minimal FASTQ parser that turns a raw
// block into the record table the kernels consume, and the deterministic synthetic
// FASTQ generator for the BASELINE.json configurations.  No GPU code.
#include "../../include/fqgpu.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

// FastqReader::parseRecords semantics (reference src/fastq_io.cpp:67-125): four lines per
// record, '@' header, sequence, '+' line, quality of the same length; a trailing partial
// record is ignored (the reference carries it over to the next chunk).
extern "C" long fqgpu_parse_fastq(const uint8_t *raw, size_t len, fqgpu_rec *recs, size_t cap) {
  size_t pos = 0;
  long n = 0;
  while (pos < len) {
    size_t start[4], end[4];
    size_t p = pos;
    int ln;
    for (ln = 0; ln < 4; ln++) {
      const void *nl = p < len ? memchr(raw + p, '\n', len - p) : nullptr;
      if (!nl) break;
      start[ln] = p;
      end[ln] = (size_t)(static_cast<const uint8_t *>(nl) - raw);
      p = end[ln] + 1;
    }
    if (ln < 4) break;  // partial record at the end of the block
    if (raw[start[0]] != '@' || raw[start[2]] != '+') return -1;
    const size_t l1 = end[1] - start[1], l3 = end[3] - start[3];
    if (l1 != l3 || l1 > 65535 || start[3] > 0xFFFFFFFFull) return -1;
    if ((size_t)n < cap && recs) {
      recs[n].seq_off = (uint32_t)start[1];
      recs[n].qual_off = (uint32_t)start[3];
      recs[n].len = (uint32_t)l1;
    }
    n++;
    pos = p;
  }
  return n;
}

// CRC-32 (zlib) of A || B from the digests of A and B and the length of B: crc(A) x^(8 len_b) + crc(B) over GF(2),
// in the CRC's bit order (bit 31 = x^0); the init and final-xor terms of the two digests cancel.
static uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= (a & 0x80000000u) ? b : 0u;
    a <<= 1;
    b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
  }
  return p;
}
extern "C" uint32_t fqgpu_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8: the exponent counts bytes (any uint64 length, no overflow)
  for (; len_b; len_b >>= 1) {
    if (len_b & 1u) r = crc_mul(r, sq);
    sq = crc_mul(sq, sq);
  }
  return crc_mul(crc_a, r) ^ crc_b;
}

// Read summaries (stats.hip fills them): the size of one for `positions` rows, and dst += src.
extern "C" size_t fqgpu_stats_words(unsigned positions) {
  return positions && positions <= 65535u ? 176u + 70u * ((size_t)positions + 1u) : 0u;
}
extern "C" int fqgpu_stats_merge(uint64_t *dst, size_t dst_words, const uint64_t *src, size_t src_words) {
  if (!dst || !src || !src_words || dst_words != src_words || src[5] > 65535u || src_words != fqgpu_stats_words((unsigned)src[5]))
    return FQGPU_E_ARG;
  const bool empty = dst[0] == 0;  // (a block of zeros is an empty summary of any P)
  if (dst[5] != src[5] && !(empty && dst[5] == 0)) return FQGPU_E_ARG;
  if (empty) {
    memcpy(dst, src, src_words * sizeof(uint64_t));
    return FQGPU_OK;
  }
  if (!src[0]) return FQGPU_OK;
  const uint64_t lo = dst[2] < src[2] ? dst[2] : src[2], hi = dst[3] > src[3] ? dst[3] : src[3];
  for (size_t i = 0; i < dst_words; i++) dst[i] += src[i];
  dst[2] = lo;
  dst[3] = hi;
  dst[5] = src[5];
  return FQGPU_OK;
}

// Read filters (select.hip applies them): what a filter may say.
extern "C" int fqgpu_filter_check(const fqgpu_filter *f) {
  if (!f || f->min_len > f->max_len || f->min_mean_q > 63u || f->low_q > 64u || f->max_low_pct > 100u || f->reserved[0] || f->reserved[1])
    return FQGPU_E_ARG;
  return FQGPU_OK;
}

// Read trimming (select.hip applies it): what a trim may say.
extern "C" int fqgpu_trim_check(const fqgpu_trim *t) {
  if (!t || t->cut_front > 65535u || t->cut_tail > 65535u || t->q_front > 64u || t->q_tail > 64u || t->crop == 0u || t->reserved[0] ||
      t->reserved[1] || t->reserved[2])
    return FQGPU_E_ARG;
  return FQGPU_OK;
}

// Adapter clipping (select.hip applies it): what an adapter may say.
extern "C" int fqgpu_adapter_check(const fqgpu_adapter *a) {
  if (!a || a->len < 1u || a->len > FQGPU_ADAPTER_MAX || a->min_overlap < 1u || a->min_overlap > a->len || a->max_err_pct > 50u || a->reserved)
    return FQGPU_E_ARG;
  for (unsigned j = 0; j < FQGPU_ADAPTER_MAX; j++) {
    const uint8_t c = a->seq[j];
    if (j < a->len ? c != 'A' && c != 'C' && c != 'G' && c != 'T' : c != 0) return FQGPU_E_ARG;
  }
  return FQGPU_OK;
}

// Adapter content (select.hip counts it): the size of a result, what a probe set may say, its fingerprint, and dst += src.
extern "C" size_t fqgpu_probe_words(unsigned n_probes, unsigned positions) {
  if (n_probes < 1u || n_probes > FQGPU_PROBES_MAX || positions < 1u || positions > 65535u) return 0u;
  return 8u + ((size_t)n_probes + 1u) * (8u + (size_t)positions + 1u);
}
extern "C" int fqgpu_probes_check(const fqgpu_probes *p) {
  if (!p || p->n < 1u || p->n > FQGPU_PROBES_MAX || p->reserved[0] || p->reserved[1] || p->reserved[2]) return FQGPU_E_ARG;
  for (unsigned k = 0; k < p->n; k++)
    if (fqgpu_adapter_check(&p->probe[k]) != FQGPU_OK) return FQGPU_E_ARG;
  const uint8_t *const rest = reinterpret_cast<const uint8_t *>(&p->probe[p->n]);
  for (size_t i = 0; i < (FQGPU_PROBES_MAX - p->n) * sizeof(fqgpu_adapter); i++)
    if (rest[i]) return FQGPU_E_ARG;
  return FQGPU_OK;
}
// zlib's CRC-32 of the bytes of probe[0 .. n) (bit by bit: at most 1280 bytes, once per call)
uint32_t fq_probes_fingerprint(const fqgpu_probes *p) {
  static_assert(sizeof(fqgpu_adapter) == 80, "the fingerprint is taken over 80 bytes a probe");
  const uint8_t *const b = reinterpret_cast<const uint8_t *>(p->probe);
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < p->n * sizeof(fqgpu_adapter); i++) {
    c ^= b[i];
    for (int j = 0; j < 8; j++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
  }
  return ~c;
}
extern "C" int fqgpu_probe_merge(uint64_t *dst, size_t dst_words, const uint64_t *src, size_t src_words) {
  if (!dst || !src || src_words < 8u || dst_words != src_words || src[2] > FQGPU_PROBES_MAX || src[3] > 65535u ||
      src_words != fqgpu_probe_words((unsigned)src[2], (unsigned)src[3]))
    return FQGPU_E_ARG;
  const bool empty = dst[0] == 0;  // (a block of zeros is an empty result of any probe set)
  const bool blank = empty && !dst[2] && !dst[3] && !dst[4];
  if (!blank && (dst[2] != src[2] || dst[3] != src[3] || dst[4] != src[4])) return FQGPU_E_ARG;
  if (empty) {
    memcpy(dst, src, src_words * sizeof(uint64_t));
    return FQGPU_OK;
  }
  if (!src[0]) return FQGPU_OK;
  for (size_t i = 0; i < dst_words; i++)
    if (i < 2u || i >= 8u) dst[i] += src[i];
  return FQGPU_OK;
}

// Mate overlap (pair.hip finds it): what a spec may say, its fingerprint, and dst += src.
extern "C" int fqgpu_overlap_check(const fqgpu_overlap *o) {
  if (!o || o->min_overlap < 1u || o->min_overlap > FQGPU_OVERLAP_MAX_LEN || o->max_mism > 65535u || o->max_err_pct > 50u) return FQGPU_E_ARG;
  for (uint32_t r : o->reserved)
    if (r) return FQGPU_E_ARG;
  return FQGPU_OK;
}
// zlib's CRC-32 of the spec's 32 bytes (bit by bit, once per call)
uint32_t fq_overlap_fingerprint(const fqgpu_overlap *o) {
  static_assert(sizeof(fqgpu_overlap) == 32, "the fingerprint is taken over 32 bytes");
  const uint8_t *const b = reinterpret_cast<const uint8_t *>(o);
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < sizeof(fqgpu_overlap); i++) {
    c ^= b[i];
    for (int j = 0; j < 8; j++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
  }
  return ~c;
}
extern "C" int fqgpu_overlap_merge(uint64_t *dst, size_t dst_words, const uint64_t *src, size_t src_words) {
  if (!dst || !src || dst_words != FQGPU_OVERLAP_WORDS || src_words != FQGPU_OVERLAP_WORDS) return FQGPU_E_ARG;
  const bool empty = dst[0] == 0;  // (a block of zeros is an empty result of any spec)
  if (!(empty && !dst[8]) && dst[8] != src[8]) return FQGPU_E_ARG;
  if (empty) {
    memcpy(dst, src, src_words * sizeof(uint64_t));
    return FQGPU_OK;
  }
  if (!src[0]) return FQGPU_OK;
  for (size_t i = 0; i < dst_words; i++)
    if (i != 8u) dst[i] += src[i];
  return FQGPU_OK;
}

// The correction inside the mate overlap (pair.hip applies it): what a spec may say.
extern "C" int fqgpu_correct_check(const fqgpu_correct *c) {
  if (!c || c->good_q < 1u || c->good_q > 63u || c->bad_q >= c->good_q) return FQGPU_E_ARG;
  for (uint32_t r : c->reserved)
    if (r) return FQGPU_E_ARG;
  return FQGPU_OK;
}

// The merge of two mates into one read (pair.hip builds it): what a spec may say.
extern "C" int fqgpu_merge_check(const fqgpu_merge *m) {
  if (!m || m->floor_q > 63u || m->min_len < 1u || m->min_len > 1023u) return FQGPU_E_ARG;
  for (uint32_t r : m->reserved)
    if (r) return FQGPU_E_ARG;
  return FQGPU_OK;
}

// Poly-X tails and the sliding-window cut (select.hip applies them): what a tail may say.
extern "C" int fqgpu_tail_check(const fqgpu_tail *x) {
  if (!x || x->poly_bases > 15u || x->poly_max_mism > 255u || x->window_len > 32u || x->reserved[0] || x->reserved[1]) return FQGPU_E_ARG;
  if (x->poly_bases ? x->poly_min_len < 1u || x->poly_min_len > 65535u || x->poly_every < 2u || x->poly_every > 255u
                    : x->poly_min_len || x->poly_every)
    return FQGPU_E_ARG;
  if (x->window_len ? x->window_q < 1u || x->window_q > 64u : x->window_q != 0u) return FQGPU_E_ARG;
  return FQGPU_OK;
}

// The read id of a header line (pair.hip compares them, k_pair_names): the bytes behind the line's first byte, the '@', up
// to the first ' ', '\t' or '\n' or the end of what is given, without a "/1" or "/2" at their end.
extern "C" size_t fqgpu_read_id_len(const uint8_t *header_line, size_t len) {
  if (!header_line || len < 2) return 0;
  size_t n = 0;
  while (1 + n < len && header_line[1 + n] != ' ' && header_line[1 + n] != '\t' && header_line[1 + n] != '\n') n++;
  if (n >= 2 && header_line[n - 1] == '/' && (header_line[n] == '1' || header_line[n] == '2')) n -= 2;
  return n;
}

namespace {
struct SplitMix {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

// Phred ~ round(N(34, 5)) clipped to [2, 41], integer arithmetic only: the sum of twelve
// 16-bit uniforms is the classic Irwin-Hall stand-in for a unit normal.
inline unsigned phred_normal(SplitMix &g) {
  uint64_t a = g.next(), b = g.next(), c = g.next();
  int64_t sum = 0;
  for (int i = 0; i < 4; i++) {
    sum += (int64_t)((a >> (16 * i)) & 0xFFFF) + (int64_t)((b >> (16 * i)) & 0xFFFF) +
           (int64_t)((c >> (16 * i)) & 0xFFFF);
  }
  // z = (sum - 6*65536) / 65536 ; q = floor(34 + 5 z + 0.5)
  int64_t q = (34 * 65536 + 5 * (sum - 6 * 65536) + 32768) >> 16;
  if (q < 2) q = 2;
  if (q > 41) q = 41;
  return (unsigned)q;
}
}  // namespace

extern "C" size_t fqgpu_synth_fastq(uint8_t *dst, size_t cap, int mode, uint64_t seed, uint64_t first_read_id,
                                    uint64_t *n_reads_out) {
  static const char ACGT[4] = {'A', 'C', 'G', 'T'};
  size_t pos = 0;
  uint64_t id = first_read_id, n = 0;
  for (;;) {
    // every read draws from its own generator so blocks can be produced independently
    SplitMix g{seed * 0xD1342543DE82EF95ull + id * 0x2545F4914F6CDD1Dull + 28};
    unsigned L = 150;
    if (mode == 4) L = 50 + (unsigned)(g.next() % 251);
    char hdr[96];
    const int hl = snprintf(hdr, sizeof(hdr), "@SYN.%llu %llu length=%u\n", (unsigned long long)id,
                            (unsigned long long)id, L);
    const size_t need = (size_t)hl + 2 * (size_t)L + 4;
    if (pos + need > cap) break;
    memcpy(dst + pos, hdr, (size_t)hl);
    uint8_t *s = dst + pos + hl;
    uint8_t *q = s + L + 3;
    uint64_t bits = 0;
    int have = 0;
    for (unsigned i = 0; i < L; i++) {
      if (have < 2) { bits = g.next(); have = 64; }
      s[i] = (uint8_t)ACGT[bits & 3];
      bits >>= 2; have -= 2;
    }
    s[L] = '\n'; s[L + 1] = '+'; s[L + 2] = '\n';
    if (mode == 1) {
      memset(q, 'I', L);
      for (unsigned i = 0; i < L; i++) if (g.next() % 1000 == 0) s[i] = 'N';
    } else if (mode == 3) {  // binned: four levels at 5/10/15/70 %, the level of the previous position kept with p = 0.85
      static const char LEVELS[4] = {'#', '-', '8', 'F'};
      unsigned level = 3;
      uint64_t r = 0;
      for (unsigned i = 0; i < L; i++) {
        if ((i & 1u) == 0) r = g.next();
        const unsigned keep = (unsigned)(r & 0xFFFF), pick = (unsigned)((r >> 16) & 0xFFFF);
        r >>= 32;
        if (i == 0 || keep >= 55705u)  // 0.85 * 65536
          level = pick < 3277u ? 0u : pick < 9830u ? 1u : pick < 19661u ? 2u : 3u;
        q[i] = (uint8_t)LEVELS[level];
      }
    } else if (mode == 5) {  // constant: one base, one quality (one context per stream from the fourth symbol on)
      memset(s, 'A', L);
      memset(q, 'F', L);
    } else if (mode == 6) {  // two quality levels, i.i.d. at 30/70 %, nothing else: no reset symbol, no narrow symbol, no uniform segment
      uint64_t r = 0;
      for (unsigned i = 0; i < L; i++) {
        if ((i & 3u) == 0) r = g.next();
        q[i] = (uint8_t)(((r & 0xFFFFu) < 19661u) ? '-' : 'F');  // 0.3 * 65536
        r >>= 16;
      }
    } else {
      for (unsigned i = 0; i < L; i++) q[i] = (uint8_t)(33 + phred_normal(g));
      if (mode == 4)
        for (unsigned i = 0; i < L; i++) if (g.next() % 100 == 0) { s[i] = 'N'; q[i] = '#'; }
    }
    q[L] = '\n';
    pos += need;
    id++; n++;
  }
  if (n_reads_out) *n_reads_out = n;
  return pos;
}
