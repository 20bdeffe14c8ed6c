// workspace.hpp -- the reference's block-codec surface on top of the fqgpu C ABI.
//
// Mirrors, name for name, what the reference exposes for this path so that its pipeline
// (src/process.cpp:46-68, 93-104) and its tests read the same:
//   FastqRecord / FastqChunk                       src/defs.h:22-52
//   CompressedBuffersDst / CompressedBuffersSrc    src/compressed_buffers.h:34-101
//   DatasetMeta (ft_seq / ft_qual part)            src/prepare.h:14-57
//   CompressionWorkspace::encodeChunk              src/workspace.h:69,  src/workspace.cpp:14-45
//   DecompressionWorkspace::decodeChunk            src/workspace.h:112, src/workspace.cpp:47-88
//   Workspace::compressBoundSequence/Quality       src/workspace.h:21-35
//   FSE_{Sequence,Quality}::calculateFreqTable     src/fse_sequence.h:72, src/fse_quality.h:50
//   CompressionWorkspace::encodeHeader / DecompressionWorkspace::decodeHeader   src/workspace.cpp:95-157
// The seq/qual FSE streams are coded on the GPU; the header fields are tokenised and delta-coded
// on the host (headers.hpp).  The misc streams (readlens, n_count, n_pos,
// header fields) go through compressMiscBuffers / decompressMiscBuffers like in the reference
// (src/workspace.cpp:176-256) -- with the library's own coder (fq_misc.cpp) in place of libbsc, whose
// source is absent: the compressed misc BYTES are out of parity scope, everything in front of that
// pass (the streams themselves, cbs.original_size) is the reference's, byte for byte.
// Error behaviour:
// the reference asserts / silently returns size 0; this shim throws std::runtime_error with
// fqgpu_strerror().  Header-only; link with libfqgpu.so.
#pragma once

#include <algorithm>

#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <istream>
#include <memory>
#include <new>
#include <ostream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "../../include/fqgpu.h"
#include "headers.hpp"

namespace fqcomp28 {

using readlen_t = uint16_t;  // src/defs.h:14

/** Allocator of the buffers that cross PCIe: page-locked host memory (fqgpu_host_alloc), so that
 *  the copies to and from the GPU run at link rate and asynchronously.  The reference's
 *  FastqData / std::vector<std::byte> with another allocator: same interface, same contents. */
template <class T> struct HostAllocator {
  using value_type = T;
  HostAllocator() = default;
  template <class U> HostAllocator(const HostAllocator<U> &) {}
  T *allocate(std::size_t n) {
    void *p = fqgpu_host_alloc(n * sizeof(T));
    if (!p) throw std::bad_alloc();
    return static_cast<T *>(p);
  }
  void deallocate(T *p, std::size_t) { fqgpu_host_free(p); }
  /** resize() of a chunk or stream buffer must not sweep hundreds of megabytes with zeros that the
   *  file read / the copy from the GPU overwrites the next moment: elements are default-initialised */
  template <class U> void construct(U *p) { ::new (static_cast<void *>(p)) U; }
  template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&...a) {
    ::new (static_cast<void *>(p)) U(std::forward<A0>(a0), std::forward<A>(a)...);
  }
  template <class U> bool operator==(const HostAllocator<U> &) const { return true; }
  template <class U> bool operator!=(const HostAllocator<U> &) const { return false; }
};
using FastqData = std::vector<char, HostAllocator<char>>;            // src/defs.h:20
using stream_bytes_t = std::vector<std::byte, HostAllocator<std::byte>>;  // cbs.seq / cbs.qual
// The side buffers (record table, readlens, n_count, n_pos) stay PAGEABLE on purpose: page-locked, their
// small copies queue up in the DMA engines behind the other workers' block uploads (fqgpu_encode_block
// from four threads: 47.9 GB/s with pageable side buffers, 40-42 with page-locked ones, same box).
using RecordTable = std::vector<fqgpu_rec>;
using u16_buffer_t = std::vector<uint16_t>;

/** Non-owning - holds pointers into outside allocated data (src/defs.h:22-32) */
struct FastqRecord {
  char *seqp = nullptr, *qualp = nullptr, *headerp = nullptr;
  readlen_t length = 0, header_length = 0;
  [[nodiscard]] std::string_view header() const { return {headerp, header_length}; }
  [[nodiscard]] std::string_view seq() const { return {seqp, length}; }
  [[nodiscard]] std::string_view qual() const { return {qualp, length}; }
};

struct FastqChunk {  // src/defs.h:34-52
  FastqData raw_data;
  std::vector<FastqRecord> records;
  std::size_t tot_reads_length = 0;
  std::size_t headers_length = 0;
  unsigned idx = 0;
  void clear() {
    idx = 0; tot_reads_length = 0; headers_length = 0;
    raw_data.clear(); records.clear();
  }
};

struct cb_original_sizes_t {  // src/compressed_buffers.h:10-32
  std::vector<headers::FieldStorage::sizes> header_fields;
  uint32_t total = 0, readlens = 0, n_records = 0, n_count = 0, n_pos = 0;
  void clear() {
    total = readlens = n_records = n_count = n_pos = 0;
    for (auto &sz : header_fields) sz = {};
  }
};

struct CompressedBuffers {  // src/compressed_buffers.h:34-69
  stream_bytes_t seq, qual;
  std::vector<std::byte> readlens, compressed_readlens;
  std::vector<headers::CompressedFieldStorage> compressed_header_fields;
  std::vector<std::byte> n_count, compressed_n_count;
  std::vector<std::byte> n_pos, compressed_n_pos;
  cb_original_sizes_t original_size;
  uint32_t chunk_idx = 0;
  /** Extension, not in the reference and not in the .fqc container: the decode index of the sequence / quality
   *  stream (fqgpu_encode_index), filled by encodeChunk when the workspace was asked for it, used by decodeChunk
   *  when present.  The farm keeps it in a file beside the archive (archive.hpp: DecodeIndexFile). */
  std::vector<std::byte> decode_index[2];
  /* like the reference, clear() does NOT clear n_count / n_pos */
  virtual void clear() {
    seq.clear(); qual.clear();
    decode_index[0].clear(); decode_index[1].clear();
    readlens.clear(); compressed_readlens.clear();
    for (auto &chf : compressed_header_fields) chf.clear();
    original_size.clear();
  }
  virtual ~CompressedBuffers() = default;
};

/** memcompress / memdecompress (src/memcompress.h:5-28) over the library's own misc-stream coder
 *  (fq_misc.cpp; libbsc's bytes are out of parity scope) */
inline std::size_t memcompress(std::byte *dst, const std::byte *src, std::size_t src_size) {
  return fqgpu_memcompress(reinterpret_cast<uint8_t *>(dst), fqgpu_memcompress_bound(src_size),
                           reinterpret_cast<const uint8_t *>(src), src_size);
}
inline std::size_t memdecompress(std::byte *dst, std::size_t dst_size, const std::byte *src, std::size_t src_size) {
  const std::size_t n = fqgpu_memdecompress(reinterpret_cast<uint8_t *>(dst), dst_size,
                                            reinterpret_cast<const uint8_t *>(src), src_size);
  if (n == static_cast<std::size_t>(-1) || (src_size && n != dst_size)) throw std::runtime_error("memdecompress: malformed misc stream");
  return n;
}
/** Every misc stream of a block (everything but the two FSE streams) as f(plain, compressed,
 *  original size): the one list both directions of the misc pass walk (reference
 *  src/workspace.cpp:176-256 runs libbsc over the same streams).  A NUMERIC header field has a
 *  content stream only. */
template <class Buffers, class F> void miscStreams(Buffers &cbs, const headers::HeaderFormatSpeciciation &fmt, F &&f) {
  f(cbs.readlens, cbs.compressed_readlens, cbs.original_size.readlens);
  f(cbs.n_count, cbs.compressed_n_count, cbs.original_size.n_count);
  f(cbs.n_pos, cbs.compressed_n_pos, cbs.original_size.n_pos);
  for (std::size_t i = 0; i < fmt.n_fields(); ++i) {
    auto &plain = cbs.header_fields[i];
    auto &packed = cbs.compressed_header_fields[i];
    auto &sizes = cbs.original_size.header_fields[i];
    f(plain.content, packed.content, sizes.content);
    if (fmt.field_types[i] == headers::FieldType::STRING) {
      f(plain.isDifferentFlag, packed.isDifferentFlag, sizes.isDifferentFlag);
      f(plain.contentLength, packed.contentLength, sizes.contentLength);
    }
  }
}

/** Extension: the CRC-32 (zlib's) of a chunk's canonical bytes -- what decodeChunk lays out for it -- and their number
 *  (fqgpu_chunk_crc32); valid: one was taken */
struct ChunkDigest {
  uint32_t crc32 = 0;
  std::size_t length = 0;
  bool valid = false;
};

struct CompressedBuffersDst : CompressedBuffers {
  std::vector<headers::FieldStorageDst> header_fields;
  /** Extension, not in the .fqc container: filled by encodeChunk when the workspace was asked to (setChecksum).  The
   *  farm keeps it in a file beside the archive (archive.hpp: ChunkSumsFile). */
  ChunkDigest digest;
  void clear() override {
    CompressedBuffers::clear();
    for (auto &hf : header_fields) hf.clear();
    digest = {};
  }
};
struct CompressedBuffersSrc : CompressedBuffers {
  std::vector<headers::FieldStorageSrc> header_fields;
  struct { std::size_t n_count = 0, n_pos = 0; } index;  // src/compressed_buffers.h:90-93
  void clear() override {
    CompressedBuffers::clear();
    for (auto &hf : header_fields) hf.clear();
    index = {};
  }
};

/** FQGPU_SHIM_TRACE=1: one line per block on stderr with the milliseconds of every stage of
 *  encodeChunk (where a worker's time goes: DESIGN.md section 9) */
struct StageClock {
  bool on = std::getenv("FQGPU_SHIM_TRACE") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  std::string line;
  void lap(const char *name) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    char buf[64];
    std::snprintf(buf, sizeof(buf), " %s %.1f", name, std::chrono::duration<double, std::milli>(now - t).count());
    line += buf;
    t = now;
  }
  void done(unsigned idx) { if (on) std::fprintf(stderr, "block %u:%s\n", idx, line.c_str()); }
};

inline void fqgpuCheck(int rc, const char *what) {
  if (rc != FQGPU_OK) throw std::runtime_error(std::string(what) + ": " + fqgpu_strerror(rc));
}

/** FreqTable PODs exactly as the archive stores them (src/fse_common.hpp:147-174) */
struct DatasetMeta {
  /** used by the host's header coder for delta-ing the first header of each chunk (src/prepare.h:30) */
  std::string first_header;
  headers::HeaderFormatSpeciciation header_fmt;  // src/prepare.h:31
  std::unique_ptr<std::byte[]> ft_seq{new std::byte[FQGPU_SEQ_FT_BYTES]};
  std::unique_ptr<std::byte[]> ft_qual{new std::byte[FQGPU_QUAL_FT_BYTES]};
  DatasetMeta() = default;
  explicit DatasetMeta(std::string_view header)
      : first_header(header), header_fmt(headers::HeaderFormatSpeciciation::fromHeader(first_header)) {}
  /** DatasetMeta(const FastqChunk&) (src/prepare.h:23-27): dataset analysis on the GPU */
  explicit DatasetMeta(const FastqChunk &chunk, int device = 0)
      : first_header(chunk.records.empty() ? std::string_view() : chunk.records.front().header()) {
    if (!first_header.empty()) header_fmt = headers::HeaderFormatSpeciciation::fromHeader(first_header);
    RecordTable recs = toRecordTable(chunk);
    fqgpuCheck(fqgpu_freq_tables(device, reinterpret_cast<const uint8_t *>(chunk.raw_data.data()),
                                 chunk.raw_data.size(), recs.data(), recs.size(), ft_seq.get(),
                                 ft_qual.get(), nullptr, nullptr),
               "calculateFreqTable");
  }
  /** bytes of the metadata section of an archive (src/prepare.h:44-52) */
  [[nodiscard]] std::size_t size() const { return sizeof(readlen_t) + first_header.length() + FQGPU_SEQ_FT_BYTES + FQGPU_QUAL_FT_BYTES; }

  /** The metadata section of an archive (src/prepare.cpp:12-21 writes the same bytes): u16 header
   *  length, the header, then the two FreqTable PODs as they lie in memory */
  void appendTo(std::vector<uint8_t> &out) const {
    if (first_header.size() > 0xFFFFu) throw std::invalid_argument("first header longer than a readlen_t");
    const readlen_t hlen = static_cast<readlen_t>(first_header.size());
    const std::size_t at = out.size();
    out.resize(at + size());
    uint8_t *p = out.data() + at;
    std::memcpy(p, &hlen, sizeof(hlen));
    std::memcpy(p + sizeof(hlen), first_header.data(), hlen);
    std::memcpy(p + sizeof(hlen) + hlen, ft_seq.get(), FQGPU_SEQ_FT_BYTES);
    std::memcpy(p + sizeof(hlen) + hlen + FQGPU_SEQ_FT_BYTES, ft_qual.get(), FQGPU_QUAL_FT_BYTES);
  }
  static DatasetMeta fromBytes(const uint8_t *p, std::size_t n) {
    readlen_t hlen = 0;
    if (n < sizeof(hlen)) throw std::runtime_error("truncated dataset metadata");
    std::memcpy(&hlen, p, sizeof(hlen));
    if (n < sizeof(hlen) + hlen + FQGPU_SEQ_FT_BYTES + FQGPU_QUAL_FT_BYTES) throw std::runtime_error("truncated dataset metadata");
    DatasetMeta meta{std::string_view(reinterpret_cast<const char *>(p) + sizeof(hlen), hlen)};
    std::memcpy(meta.ft_seq.get(), p + sizeof(hlen) + hlen, FQGPU_SEQ_FT_BYTES);
    std::memcpy(meta.ft_qual.get(), p + sizeof(hlen) + hlen + FQGPU_SEQ_FT_BYTES, FQGPU_QUAL_FT_BYTES);
    return meta;
  }
  /** the same through streams, under the reference's names (src/prepare.cpp:12-41) */
  static void storeToStream(const DatasetMeta &meta, std::ostream &os) {
    std::vector<uint8_t> bytes;
    meta.appendTo(bytes);
    os.write(reinterpret_cast<const char *>(bytes.data()), static_cast<std::streamsize>(bytes.size()));
  }
  static DatasetMeta loadFromStream(std::istream &is) {
    std::vector<uint8_t> bytes(sizeof(readlen_t));
    is.read(reinterpret_cast<char *>(bytes.data()), sizeof(readlen_t));
    readlen_t hlen = 0;
    std::memcpy(&hlen, bytes.data(), sizeof(hlen));
    bytes.resize(sizeof(hlen) + hlen + FQGPU_SEQ_FT_BYTES + FQGPU_QUAL_FT_BYTES);
    is.read(reinterpret_cast<char *>(bytes.data()) + sizeof(hlen), static_cast<std::streamsize>(bytes.size() - sizeof(hlen)));
    if (!is.good()) throw std::runtime_error("truncated dataset metadata");
    return fromBytes(bytes.data(), bytes.size());
  }
  friend bool operator==(const DatasetMeta &a, const DatasetMeta &b) {
    return a.first_header == b.first_header && std::memcmp(a.ft_seq.get(), b.ft_seq.get(), FQGPU_SEQ_FT_BYTES) == 0 &&
           std::memcmp(a.ft_qual.get(), b.ft_qual.get(), FQGPU_QUAL_FT_BYTES) == 0;
  }

  static RecordTable toRecordTable(const FastqChunk &chunk) {
    RecordTable recs(chunk.records.size());
    const char *base = chunk.raw_data.data();
    for (std::size_t i = 0; i < recs.size(); ++i) {
      const FastqRecord &r = chunk.records[i];
      recs[i] = {static_cast<uint32_t>(r.seqp - base), static_cast<uint32_t>(r.qualp - base), r.length};
    }
    return recs;
  }
};

class Workspace {
public:
  static std::size_t compressBoundSequence(std::size_t n) { return fqgpu_bound_seq(n); }
  static std::size_t compressBoundQuality(std::size_t n) { return fqgpu_bound_qual(n); }

  /** Extension: every chunk this workspace encodes / decodes is also summarised where it lies on the device
   *  (fqgpu_chunk_stats, `positions` rows; taken where the digest is taken) and added to stats(), the summary of all its
   *  chunks so far (fqgpu_stats_merge).  positions 0: off, not one call more. */
  void setStats(unsigned positions) {
    stats_positions_ = positions;
    stats_.assign(fqgpu_stats_words(positions), 0);
    stats_chunk_.assign(stats_.size(), 0);
    if (positions && stats_.empty()) throw std::invalid_argument("setStats: positions must be 1 .. 65535");
    if (positions) stats_[5] = positions;  // (the empty summary of P: a worker that gets no chunk still has one to merge)
  }
  [[nodiscard]] const std::vector<uint64_t> &stats() const { return stats_; }

  /** Extension: every chunk is also searched for the probes' adapters where it lies on the device (fqgpu_chunk_probe,
   *  `positions` rows; taken where the summary is taken) and the result added to probes(), the adapter content of all its
   *  chunks so far (fqgpu_probe_merge).  nullptr: off, not one call more. */
  void setProbes(const fqgpu_probes *probes, unsigned positions) {
    probes_on_ = probes != nullptr;
    probes_.clear();
    probes_chunk_.clear();
    if (!probes) return;
    if (fqgpu_probes_check(probes) != FQGPU_OK) throw std::invalid_argument("setProbes: a probe set fqgpu_probes_check refuses");
    probe_set_ = *probes;
    probe_positions_ = positions;
    probes_.assign(fqgpu_probe_words(probes->n, positions), 0);
    probes_chunk_.assign(probes_.size(), 0);
    if (probes_.empty()) throw std::invalid_argument("setProbes: positions must be 1 .. 65535");
  }
  /** all zeros while no chunk has been taken: fqgpu_probe_merge's empty result */
  [[nodiscard]] const std::vector<uint64_t> &probes() const { return probes_; }

protected:
  /** the summary of the chunk on the handle, into stats(), and its adapter content, into probes() */
  void takeStats(const char *what) {
    if (stats_positions_) {
      fqgpuCheck(fqgpu_chunk_stats(ctx_, stats_positions_, stats_chunk_.data(), stats_chunk_.size()), what);
      fqgpuCheck(fqgpu_stats_merge(stats_.data(), stats_.size(), stats_chunk_.data(), stats_chunk_.size()), what);
    }
    if (probes_on_) {
      fqgpuCheck(fqgpu_chunk_probe(ctx_, &probe_set_, probe_positions_, probes_chunk_.data(), probes_chunk_.size(), nullptr), what);
      fqgpuCheck(fqgpu_probe_merge(probes_.data(), probes_.size(), probes_chunk_.data(), probes_chunk_.size()), what);
    }
  }
  explicit Workspace(const DatasetMeta *meta, int device)
      : meta_(meta), fmt_(meta->header_fmt), first_header_fields_(headers::fromHeader(meta->first_header, fmt_)) {
    fqgpuCheck(fqgpu_ctx_create(device, meta->ft_seq.get(), meta->ft_qual.get(), &ctx_), "Workspace");
    // one block at a time per workspace (like the reference's): one encode lane, a quarter of the scratch
    fqgpuCheck(fqgpu_ctx_set_lanes(ctx_, 1), "Workspace");
    for (const auto t : fmt_.field_types) field_types_.push_back(t == headers::FieldType::STRING ? 1 : 0);
  }
  /** every chunk codes its first header against the dataset's first header (src/workspace.cpp:90-93) */
  void startNewChunk() { prev_header_fields_ = first_header_fields_; }
  ~Workspace() { fqgpu_ctx_destroy(ctx_); }
  Workspace(const Workspace &) = delete;
  Workspace &operator=(const Workspace &) = delete;
  const DatasetMeta *const meta_;
  const headers::HeaderFormatSpeciciation fmt_;
  const headers::header_fields_t first_header_fields_;
  headers::header_fields_t prev_header_fields_;
  std::vector<uint8_t> field_types_;  // fmt_.field_types as the C ABI takes them (0 = NUMERIC, 1 = STRING)
  fqgpu_ctx *ctx_ = nullptr;

private:
  unsigned stats_positions_ = 0;
  std::vector<uint64_t> stats_, stats_chunk_;
  bool probes_on_ = false;
  fqgpu_probes probe_set_ = {};
  unsigned probe_positions_ = 0;
  std::vector<uint64_t> probes_, probes_chunk_;
};

class CompressionWorkspace : public Workspace {
public:
  explicit CompressionWorkspace(const DatasetMeta *meta, int device = 0) : Workspace(meta, device) {}

  /** Device memory for chunks of up to chunk_bytes now instead of inside the first encodeChunk
   *  (the farm calls it while it sets its workers up; the sizes assume records of 64 bytes or more) */
  void reserve(std::size_t chunk_bytes) {
    if (chunk_bytes) fqgpuCheck(fqgpu_ctx_reserve(ctx_, chunk_bytes, chunk_bytes / 64 + 1, chunk_bytes / 2 + 1), "reserve");
  }

  /** encodeChunk also leaves cbs.decode_index (extension: a decoder that has it decodes a stream from every
   *  snapshot at once; seq / qual and everything else in cbs are unchanged) */
  void setDecodeIndex(bool on, unsigned stride_symbols = 0) {
    decode_index_ = on;
    // symbols between two snapshots (a multiple of 64 Ki; 0 = the library's 1 Mi): a stride is what ONE wave decodes, so
    // a block alone takes a stride's time -- 105 ms at 1 Mi -- and the index grows as the stride shrinks (2 % of the
    // archive at 1 Mi, 8 % at 256 Ki)
    if (on && stride_symbols) fqgpuCheck(fqgpu_ctx_set_index_stride(ctx_, stride_symbols), "setDecodeIndex");
  }

  /** encodeChunk also leaves cbs.digest (extension): the chunk is digested where it lies, on the device, beside its
   *  encode and before any N -> A reaches a copy of it; off, encodeChunk makes not one call more */
  void setChecksum(bool on) { checksum_ = on; }

  /** Encodes reads into cbs, allocating memory in cbs as needed; mutates the chunk (N -> A).
   *  The chunk may come UNPARSED (records empty, as FastqReader hands it out): the GPU then finds the
   *  records, and chunk.records / the length sums are filled in from its table.  The header fields are coded on
   *  the GPU as well (fqgpu_encode_headers_*: round 3 coded them on this thread, 78 ms per 256 MiB chunk beside
   *  3 ms of GPU work); FQGPU_SHIM_HOST_HEADERS=1 keeps the host coder (headers.hpp), same bytes. */
  void encodeChunk(FastqChunk &chunk, CompressedBuffersDst &cbs) {
    StageClock clk;
    cbs.clear();
    cbs.chunk_idx = chunk.idx;
    auto *raw = reinterpret_cast<uint8_t *>(chunk.raw_data.data());
    const bool parsed = !chunk.records.empty();
    RecordTable recs;
    if (parsed) recs = DatasetMeta::toRecordTable(chunk);
    std::size_t R = 0, n_bases = 0, used = 0;
    fqgpuCheck(fqgpu_encode_begin(ctx_, raw, chunk.raw_data.size(), parsed ? recs.data() : nullptr, recs.size(),
                                  FQGPU_F_WRITE_BACK_N | (decode_index_ ? FQGPU_F_DECODE_INDEX : 0u), &R, &n_bases, &used),
               "encodeChunk");
    // From here to fqgpu_encode_end the block is in flight: copies of chunk.raw_data and of `recs` may still be queued.
    // Whatever throws in between (a chunk that ends inside a record, the header coder, a failing call) must not
    // unwind past them: the guard waits for the handle before the local table dies and the caller's page-locked
    // vectors can go back to the pin cache.
    struct InFlight {
      fqgpu_ctx *ctx;
      bool armed = true;
      ~InFlight() { if (armed) (void)fqgpu_encode_cancel(ctx); }
    } in_flight{ctx_};
    static const bool host_headers = std::getenv("FQGPU_SHIM_HOST_HEADERS") != nullptr;
    if (!host_headers)
      fqgpuCheck(fqgpu_encode_headers_begin(ctx_, field_types_.data(), fmt_.separators.data(), static_cast<unsigned>(fmt_.n_fields()),
                                            reinterpret_cast<const uint8_t *>(meta_->first_header.data()), meta_->first_header.size()),
                 "encodeChunk");
    if (checksum_) {
      fqgpuCheck(fqgpu_chunk_crc32(ctx_, &cbs.digest.crc32, &cbs.digest.length), "encodeChunk");
      cbs.digest.valid = true;
    }
    takeStats("encodeChunk");
    clk.lap("begin");
    if (!parsed) {
      recs.resize(R);
      fqgpuCheck(fqgpu_encode_records(ctx_, recs.data(), R), "encodeChunk");
      if (used != chunk.raw_data.size()) throw std::invalid_argument("encodeChunk: the chunk does not end with a complete record");
      recordViews(chunk, recs);
    }
    clk.lap("records");
    // ---- the header fields
    cbs.header_fields.resize(fmt_.n_fields());
    cbs.original_size.header_fields.resize(fmt_.n_fields());
    for (auto &field : cbs.header_fields) field.clear();
    bool on_host = host_headers;
    if (!on_host) {
      std::vector<fqgpu_field_sizes> sizes(fmt_.n_fields());
      std::size_t total = 0, bad = 0;
      const int rc = fqgpu_encode_headers_wait(ctx_, sizes.data(), &total, &bad);
      if (rc == FQGPU_E_HEADER) {
        on_host = true;  // the host coder throws the reference-side exception for that header (below)
      } else {
        fqgpuCheck(rc, "encodeChunk");
        header_stage_.resize(total);
        fqgpuCheck(fqgpu_encode_headers_end(ctx_, reinterpret_cast<uint8_t *>(header_stage_.data()), header_stage_.size()), "encodeChunk");
        const std::byte *at = header_stage_.data();
        for (std::size_t i = 0; i < fmt_.n_fields(); ++i) {
          auto &f = cbs.header_fields[i];
          f.isDifferentFlag.assign(at, at + sizes[i].isDifferentFlag); at += sizes[i].isDifferentFlag;
          f.content.assign(at, at + sizes[i].content); at += sizes[i].content;
          f.contentLength.assign(at, at + sizes[i].contentLength); at += sizes[i].contentLength;
        }
      }
    }
    if (on_host) {
      startNewChunk();
      for (const FastqRecord &r : chunk.records) headers::encodeHeader(r.header(), fmt_, prev_header_fields_, cbs.header_fields);
      if (!host_headers) throw std::logic_error("encodeChunk: the device refused a header the host coder takes");
    }
    clk.lap("headers");
    // ---- the streams, at their exact sizes
    std::size_t seq_len = 0, qual_len = 0, n_pos_len = 0;
    fqgpuCheck(fqgpu_encode_wait(ctx_, &seq_len, &qual_len, &n_pos_len), "encodeChunk");
    clk.lap("wait");
    cbs.seq.resize(seq_len);
    cbs.qual.resize(qual_len);
    cbs.readlens.resize(R * sizeof(readlen_t));
    // n_count / n_pos are appended, never cleared: what a reused CompressedBuffersDst holds in the reference
    const std::size_t cnt_at = cbs.n_count.size(), pos_at = cbs.n_pos.size();
    cbs.n_count.resize(cnt_at + R * sizeof(uint16_t));
    cbs.n_pos.resize(pos_at + n_pos_len * sizeof(uint16_t));
    fqgpuCheck(fqgpu_encode_end(ctx_, raw, reinterpret_cast<uint8_t *>(cbs.seq.data()), cbs.seq.size(), &seq_len,
                                reinterpret_cast<uint8_t *>(cbs.qual.data()), cbs.qual.size(), &qual_len,
                                reinterpret_cast<uint16_t *>(cbs.readlens.data()), reinterpret_cast<uint16_t *>(cbs.n_count.data() + cnt_at),
                                reinterpret_cast<uint16_t *>(cbs.n_pos.data() + pos_at), n_pos_len, &n_pos_len),
               "encodeChunk");
    in_flight.armed = false;
    for (int s = 0; s < 2 && decode_index_; ++s) {
      std::size_t n = 0;
      fqgpuCheck(fqgpu_encode_index(ctx_, s, nullptr, 0, &n), "encodeChunk");
      cbs.decode_index[s].resize(n);
      fqgpuCheck(fqgpu_encode_index(ctx_, s, reinterpret_cast<uint8_t *>(cbs.decode_index[s].data()), n, &n), "encodeChunk");
    }
    clk.lap("end");
    cbs.original_size.n_records = static_cast<uint32_t>(R);
    cbs.original_size.total = static_cast<uint32_t>(chunk.raw_data.size());
    compressMiscBuffers(cbs);
    clk.lap("misc");
    clk.done(chunk.idx);
  }

private:
  stream_bytes_t header_stage_;  // page-locked landing place of the header field streams
  bool decode_index_ = false, checksum_ = false;

public:
  /** The misc pass (the reference's compressMiscBuffers, src/workspace.cpp:176-213): readlens, n_count,
   *  n_pos and every header field stream through memcompress, original sizes recorded for the container */
  void compressMiscBuffers(CompressedBuffersDst &cbs) const { compressMiscBuffers(cbs, fmt_); }
  /** the same without a workspace (host-only tools and tests: no GPU involved) */
  static void compressMiscBuffers(CompressedBuffersDst &cbs, const headers::HeaderFormatSpeciciation &fmt) {
    cbs.compressed_header_fields.resize(fmt.n_fields());
    cbs.original_size.header_fields.assign(fmt.n_fields(), {});
    for (auto &packed : cbs.compressed_header_fields) packed.clear();
    miscStreams(cbs, fmt, [](const auto &plain, std::vector<std::byte> &packed, uint32_t &size) {
      size = static_cast<uint32_t>(plain.size());
      packed.resize(fqgpu_memcompress_bound(plain.size()));
      packed.resize(memcompress(packed.data(), plain.data(), plain.size()));
    });
  }

  /** chunk.records (pointers into the chunk) and the length sums from a record table */
  static void recordViews(FastqChunk &chunk, const RecordTable &recs) {
    chunk.records.resize(recs.size());
    chunk.tot_reads_length = chunk.headers_length = 0;
    char *base = chunk.raw_data.data();
    std::size_t line = 0;  // start of the record's header line
    for (std::size_t i = 0; i < recs.size(); ++i) {
      FastqRecord &r = chunk.records[i];
      r.headerp = base + line;
      r.header_length = static_cast<readlen_t>(recs[i].seq_off - 1 - line);
      r.seqp = base + recs[i].seq_off;
      r.qualp = base + recs[i].qual_off;
      r.length = static_cast<readlen_t>(recs[i].len);
      chunk.tot_reads_length += r.length;
      chunk.headers_length += r.header_length;
      line = static_cast<std::size_t>(recs[i].qual_off) + recs[i].len + 1;
    }
  }

};

/** Extension: what a selecting restore does to every read, as one value -- the steps in the order they run: the clip at the
 *  3' adapter, the poly-X tail and the sliding-window cut, the trim, then the filter that judges what is left.  nullptr: the
 *  step is off (no filter: every read that is not emptied is kept).  The pointers are not owned. */
struct Selection {
  const fqgpu_adapter *adapter = nullptr;
  const fqgpu_tail *tail = nullptr;
  const fqgpu_trim *trim = nullptr;
  const fqgpu_filter *filter = nullptr;
  /** paired restores alone (processArchivePaired): the mate overlap is analysed with this spec and summarised in
   *  PairedReport::overlap; overlap_trim: its limits stand in front of each mate's steps */
  const fqgpu_overlap *overlap = nullptr;
  bool overlap_trim = false;
  /** ... and, with `correct`, the mismatched bases inside every overlap are corrected (fqgpu_chunk_pair_correct) behind the
   *  analysis and in front of everything that judges either mate; PairedReport::correct sums its reports */
  const fqgpu_correct *correct = nullptr;
  /** ... and, with `merge`, every pair that has an insert size and whose mates both pass the selection is written as ONE read
   *  to a third output instead of the two mate files (fqgpu_chunk_pair_merge, behind the analysis and the optional
   *  correction); PairedReport::merge sums its reports.  Positional cuts (cut_front, cut_tail, crop) have no defined meaning
   *  on a merged read yet and are refused beside it */
  const fqgpu_merge *merge = nullptr;
  /** something is cut: the counters are a trim report (FarmReport::trim), not a filter report (FarmReport::filter) */
  [[nodiscard]] bool trims() const { return adapter || tail || trim; }
  /** the fqgpu_chunk_* call that serves it, by the name of its first step */
  [[nodiscard]] const char *step() const { return tail ? "tail trim" : adapter ? "clip" : trim ? "trim" : "filter"; }
  /** the words of that call's report (only a tail has more than the filter's and the trim's) */
  [[nodiscard]] unsigned reportWords() const {
    static_assert(FQGPU_FILTER_REPORT_WORDS == FQGPU_TRIM_REPORT_WORDS, "one report size for both");
    return tail ? FQGPU_TAIL_REPORT_WORDS : FQGPU_FILTER_REPORT_WORDS;
  }
  /** throws std::invalid_argument("<name>: ...") for a step its fqgpu_*_check refuses.  A selection that cuts nothing needs
   *  its filter; may_be_empty (the paired restore, which then restores both files whole): not even that. */
  void check(const std::string &name, bool may_be_empty = false) const {
    if (tail && fqgpu_tail_check(tail) != FQGPU_OK) throw std::invalid_argument(name + ": a tail fqgpu_tail_check refuses");
    if (adapter && fqgpu_adapter_check(adapter) != FQGPU_OK) throw std::invalid_argument(name + ": an adapter fqgpu_adapter_check refuses");
    if (trim && fqgpu_trim_check(trim) != FQGPU_OK) throw std::invalid_argument(name + ": a trim fqgpu_trim_check refuses");
    if ((filter || !(trims() || may_be_empty)) && fqgpu_filter_check(filter) != FQGPU_OK) throw std::invalid_argument(name + ": a filter fqgpu_filter_check refuses");
    if (overlap && fqgpu_overlap_check(overlap) != FQGPU_OK) throw std::invalid_argument(name + ": an overlap spec fqgpu_overlap_check refuses");
    if (overlap_trim && !overlap) throw std::invalid_argument(name + ": overlap_trim without an overlap spec");
    if (correct && !overlap) throw std::invalid_argument(name + ": a correction without an overlap spec");
    if (correct && fqgpu_correct_check(correct) != FQGPU_OK) throw std::invalid_argument(name + ": a correction fqgpu_correct_check refuses");
    if (merge && !overlap) throw std::invalid_argument(name + ": a merge without an overlap spec");
    if (merge && fqgpu_merge_check(merge) != FQGPU_OK) throw std::invalid_argument(name + ": a merge fqgpu_merge_check refuses");
    if (merge && trim && (trim->cut_front || trim->cut_tail || trim->crop != FQGPU_FILTER_NONE))
      throw std::invalid_argument(name + ": a merge beside cut_front, cut_tail or crop");
  }
};

class DecompressionWorkspace : public Workspace {
public:
  explicit DecompressionWorkspace(const DatasetMeta *meta, int device = 0) : Workspace(meta, device) {}

  /** Extension, the decode-side twin of CompressionWorkspace::setDecodeIndex: decodeChunk of a chunk that arrives WITHOUT
   *  decode indexes builds them on the way (fqgpu_decode_chunk_indexing: one serial decode, at the pace the format dictates
   *  anyway) and leaves them in cbs.decode_index; a chunk that arrives with its indexes is decoded from them as always.
   *  index_only: such a chunk is not restored at all -- chunk.raw_data stays empty, nothing but the indexes comes back. */
  void setBuildIndex(bool on, unsigned stride_symbols = 0, bool index_only = false) {
    build_index_ = on;
    index_only_ = on && index_only;
    if (on && stride_symbols) fqgpuCheck(fqgpu_ctx_set_index_stride(ctx_, stride_symbols), "setBuildIndex");
  }

  /** Extension: decodeChunk takes the digest of every chunk it restores (fqgpu_chunk_crc32: of the restored bytes where
   *  they lie on the device, on the device path and on the host-layout path alike); lastDigest() is that of the chunk
   *  decoded last.  Comparing it with what the writer recorded is the caller's part (process.hpp). */
  void setVerify(bool on) { verify_ = on; }
  [[nodiscard]] const ChunkDigest &lastDigest() const { return last_digest_; }
  /** Extension: decodeChunk decodes and judges everything and restores nothing -- chunk.raw_data stays empty (as with
   *  setBuildIndex(..., index_only)) */
  void setCheckOnly(bool on) {
    fqgpuCheck(fqgpu_ctx_set_check_only(ctx_, on ? 1 : 0), "setCheckOnly");
    check_only_ = on;
  }

  /** Both passes of decodeChunk (src/workspace.cpp:47-88): the first lays the chunk out
   *  (headers decoded, lengths from readlens, '+' and newlines), the second fills the sequence and quality lines.
   *  Both run on the GPU (fqgpu_decode_chunk: only the side streams go up, no skeleton).  FQGPU_SHIM_HOST_HEADERS=1
   *  keeps the host layout (headers.hpp) in front of fqgpu_decode_block_indexed; a chunk the device refuses (a header
   *  stream that runs out, a chunk too small for its records, a format it does not take) goes through the host path
   *  as well, so that the error is the host's. */
  void decodeChunk(FastqChunk &chunk, CompressedBuffersSrc &cbs) {
    last_digest_ = {};
    // (an index is built by the device path alone: FQGPU_SHIM_HOST_HEADERS does not apply to a chunk that is to get one)
    if ((!hostHeaders() || buildsIndexFor(cbs)) && decodeChunkOnDevice(chunk, cbs)) return;
    StageClock clk;
    chunk.clear();  // prepareFastqChunk (src/workspace.h:127-133)
    chunk.idx = cbs.chunk_idx;
    // (chunks of one archive differ by a record or two: room for the next ones, or every slightly longer chunk costs a
    // fresh page-locked block -- 45 ms of hipHostMalloc for 256 MiB)
    if (chunk.raw_data.capacity() < cbs.original_size.total) chunk.raw_data.reserve(cbs.original_size.total + cbs.original_size.total / 16 + 4096);
    chunk.raw_data.resize(cbs.original_size.total);
    chunk.records.resize(cbs.original_size.n_records);
    startNewChunk();
    clk.lap("resize");
    decompressMiscBuffers(cbs);
    clk.lap("misc");
    if (cbs.header_fields.size() != fmt_.n_fields()) throw std::invalid_argument("decodeChunk: header field streams do not match the format");
    if (cbs.readlens.size() < chunk.records.size() * sizeof(readlen_t)) throw std::invalid_argument("decodeChunk: readlens too short");
    char *dst = chunk.raw_data.data();
    char *const end = dst + chunk.raw_data.size();
    for (std::size_t i = 0, E = chunk.records.size(); i < E; ++i) {
      FastqRecord &r = chunk.records[i];
      std::memcpy(&r.length, cbs.readlens.data() + sizeof(readlen_t) * i, sizeof(readlen_t));
      r.headerp = dst;
      r.header_length = static_cast<readlen_t>(decodeHeaderChecked(dst, end, cbs));
      dst += r.header_length;
      if (static_cast<std::size_t>(end - dst) < 2u * r.length + 5u) throw std::out_of_range("decodeChunk: original_size.total too small");
      *dst++ = '\n';
      r.seqp = dst;  dst += r.length;  *dst++ = '\n';
      *dst++ = '+';  *dst++ = '\n';
      r.qualp = dst; dst += r.length;  *dst++ = '\n';
      chunk.tot_reads_length += r.length;
      chunk.headers_length += r.header_length;
    }
    clk.lap("headers+layout");
    RecordTable recs = DatasetMeta::toRecordTable(chunk);
    clk.lap("table");
    // (with cbs.decode_index -- an extension, empty in a reference archive -- every stream is decoded from all its
    // snapshots at once; without, by one lane from its end: the format's own pace)
    const StreamArgs s(cbs);
    fqgpuCheck(fqgpu_decode_block_indexed(ctx_, s.seq, s.seq_len, s.qual, s.qual_len, s.n_count, s.n_count_len, s.n_pos, s.n_pos_len,
                                          recs.data(), recs.size(), reinterpret_cast<uint8_t *>(chunk.raw_data.data()),
                                          chunk.raw_data.size(), s.index[0], s.index_len[0], s.index[1], s.index_len[1]),
               "decodeChunk");
    takeDigest();
    takeStats("decodeChunk");
    if (check_only_) { chunk.raw_data.clear(); chunk.records.clear(); }  // (the host layout needs the chunk; the caller gets none)
    clk.lap("gpu");
    clk.done(chunk.idx);
  }

  /** Extension: records [first, end) of the chunk into piece -- exactly the bytes decodeChunk lays out for them
   *  (fqgpu_decode_chunk_range: with the block's decode indexes only the strides that hold the range are decoded);
   *  piece.idx = cbs.chunk_idx.  A chunk the device refuses, or FQGPU_SHIM_HOST_HEADERS=1: decodeChunk, then the slice,
   *  so that the errors are the host's. */
  void decodeChunkRange(FastqChunk &piece, CompressedBuffersSrc &cbs, std::size_t first, std::size_t end) {
    if (first >= end || end > cbs.original_size.n_records) throw std::invalid_argument("decodeChunkRange: bad record range");
    std::size_t len = 0;
    if (!hostHeaders() && rangeOnDevice(cbs, first, end, &piece, &len)) return;
    decodeChunk(whole_, cbs);
    const RecordTable all = DatasetMeta::toRecordTable(whole_);
    const std::size_t lo = all[first].seq_off - 1 - whole_.records[first].header_length;
    const std::size_t hi = static_cast<std::size_t>(all[end - 1].qual_off) + all[end - 1].len + 1;
    piece.clear();
    piece.idx = cbs.chunk_idx;
    piece.raw_data.assign(whole_.raw_data.begin() + lo, whole_.raw_data.begin() + hi);
    RecordTable recs(all.begin() + first, all.begin() + end);
    for (auto &r : recs) { r.seq_off -= static_cast<uint32_t>(lo); r.qual_off -= static_cast<uint32_t>(lo); }
    CompressionWorkspace::recordViews(piece, recs);
  }
  /** The size of records [first, end) of the chunk as decodeChunkRange restores them (on the device: the layout passes
   *  only) */
  std::size_t rangeSize(CompressedBuffersSrc &cbs, std::size_t first, std::size_t end) {
    std::size_t len = 0;
    if (first < end && end <= cbs.original_size.n_records && !hostHeaders() && rangeOnDevice(cbs, first, end, nullptr, &len)) return len;
    FastqChunk piece;
    decodeChunkRange(piece, cbs, first, end);
    return piece.raw_data.size();
  }

  /** Extension: records [first, end) of the chunk as FASTA into piece.raw_data (fqgpu_decode_chunk_fasta: ">hdr\nSEQ\n"
   *  per record, from the sequence stream alone; cbs.qual is not looked at and may be empty).  piece.idx = cbs.chunk_idx,
   *  piece.records stays empty: a FASTA piece is bytes to be written.  There is no host fallback -- the host path would
   *  need the qualities -- and FQGPU_SHIM_HOST_HEADERS does not apply: a chunk the device refuses throws
   *  std::runtime_error naming the chunk and the record. */
  void decodeChunkFasta(FastqChunk &piece, CompressedBuffersSrc &cbs, std::size_t first, std::size_t end) {
    if (first >= end || end > cbs.original_size.n_records) throw std::invalid_argument("decodeChunkFasta: bad record range");
    (void)fastaOnDevice(cbs, first, end, &piece);
  }
  /** The size of records [first, end) of the chunk as decodeChunkFasta restores them (the layout passes only) */
  std::size_t fastaSize(CompressedBuffersSrc &cbs, std::size_t first, std::size_t end) {
    if (first >= end || end > cbs.original_size.n_records) throw std::invalid_argument("fastaSize: bad record range");
    return fastaOnDevice(cbs, first, end, nullptr);
  }

  /** Extension: the reads of the chunk as `sel` leaves them -- clipped, tail-trimmed, trimmed, then judged by its filter; with
   *  a filter alone the reads that pass, as the canonical FASTQ bytes decodeChunk lays out for them -- into piece.raw_data.
   *  ONE call serves a selection, named by its first step: fqgpu_chunk_tailtrim, fqgpu_chunk_clip, fqgpu_chunk_trim or
   *  fqgpu_chunk_filter; `report` receives the chunk's sel.reportWords() counters (with an adapter words 14 and 15 among
   *  them).  The chunk is decoded check-only -- nothing of it comes back -- with the block's decode indexes when present, its
   *  digest is taken first and kept for lastDigest() when setVerify is on (the digest of the WHOLE restored chunk, so the
   *  caller compares it with the writer's as always), and only the kept bytes cross the link, into a buffer of the chunk's
   *  recorded size: they are never more than the chunk, so there is no size query.  piece.idx = cbs.chunk_idx, piece.records
   *  stays empty.  There is no host fallback and FQGPU_SHIM_HOST_HEADERS does not apply: a chunk the device refuses throws
   *  std::runtime_error naming the chunk and the record. */
  void decodeChunkSelected(FastqChunk &piece, CompressedBuffersSrc &cbs, const Selection &sel, uint64_t *report) {
    StageClock clk;
    last_digest_ = {};
    sel.check("decodeChunkSelected");
    piece.clear();
    piece.idx = cbs.chunk_idx;
    stageChunk(cbs, "decodeChunkSelected", &clk);
    piece.raw_data.resize(cbs.original_size.total);
    uint8_t *const out = reinterpret_cast<uint8_t *>(piece.raw_data.data());
    const std::size_t cap = piece.raw_data.size();
    std::size_t len = 0;
    // (four calls, not fqgpu_chunk_select_marked: each runs its own kernel instantiation and fills its own report)
    const int rc = sel.tail      ? fqgpu_chunk_tailtrim(ctx_, sel.adapter, sel.tail, sel.trim, sel.filter, out, cap, &len, report, nullptr, nullptr, nullptr)
                   : sel.adapter ? fqgpu_chunk_clip(ctx_, sel.adapter, sel.trim, sel.filter, out, cap, &len, report, nullptr, nullptr)
                   : sel.trim    ? fqgpu_chunk_trim(ctx_, sel.trim, sel.filter, out, cap, &len, report, nullptr, nullptr)
                                 : fqgpu_chunk_filter(ctx_, sel.filter, out, cap, &len, report, nullptr);
    if (rc != FQGPU_OK)
      throw std::runtime_error("decodeChunkSelected: chunk " + std::to_string(cbs.chunk_idx) + ": the " + sel.step() + ": " + fqgpu_strerror(rc));
    piece.raw_data.resize(len);
    clk.lap(sel.step());
    clk.done(cbs.chunk_idx);
  }

  /** Extension (paired restores, process.hpp: processArchivePaired): the three steps a worker makes a pair of chunks of.
   *  stagePairedChunk decodes the chunk check-only, takes its digest for lastDigest() when setVerify is on and leaves it on
   *  the handle's staging block (as decodeChunkSelected does in front of its selecting call); there is no host fallback.
   *  selectMarked is fqgpu_chunk_select_limited on the chunk staged last: records [first, end) against `mark` (nullptr: none;
   *  (end - first + 7) / 8 bytes) with `limit` (nullptr: none -- then it is fqgpu_chunk_select_marked byte for byte; end - first
   *  entries) in front of the steps, any of sel's steps, or all, off; out == nullptr asks for the
   *  counters and the keep bits alone; -> the bytes written to out (at most out_cap: the chunk's recorded size is always
   *  enough).  pairNames is fqgpu_chunk_pair_names: the read ids of this handle's staged records first + i against those of
   *  `mate`'s mate_first + i, i < count -> the first i that differs, (size_t)-1 when none does.  A call the device refuses
   *  throws std::runtime_error naming the chunk. */
  void stagePairedChunk(CompressedBuffersSrc &cbs) {
    StageClock clk;
    stageChunk(cbs, "stagePairedChunk", &clk);
    staged_idx_ = cbs.chunk_idx;
    clk.done(cbs.chunk_idx);
  }
  std::size_t selectMarked(const Selection &sel, std::size_t first, std::size_t end, const uint8_t *mark, uint8_t *out, std::size_t out_cap,
                           uint64_t *report, uint8_t *keep_out, const uint16_t *limit = nullptr) {
    std::size_t len = 0;
    const int rc = fqgpu_chunk_select_limited(ctx_, sel.adapter, sel.tail, sel.trim, sel.filter, first, end, mark, limit, out, out_cap, &len, report,
                                              keep_out, nullptr, nullptr);
    if (rc != FQGPU_OK)
      throw std::runtime_error("selectMarked: chunk " + std::to_string(staged_idx_) + ", records " + std::to_string(first) + ":" +
                               std::to_string(end) + ": " + fqgpu_strerror(rc));
    return len;
  }
  std::size_t pairNames(std::size_t first, DecompressionWorkspace &mate, std::size_t mate_first, std::size_t count) {
    std::size_t mismatch = static_cast<std::size_t>(-1);
    const int rc = fqgpu_chunk_pair_names(ctx_, first, mate.ctx_, mate_first, count, &mismatch);
    if (rc != FQGPU_OK)
      throw std::runtime_error("pairNames: chunk " + std::to_string(staged_idx_) + " against chunk " + std::to_string(mate.staged_idx_) + ": " +
                               fqgpu_strerror(rc));
    return mismatch;
  }
  /** fqgpu_chunk_pair_overlap: this handle's staged records first + i (mate 1) against `mate`'s mate_first + i (mate 2),
   *  i < count -> out[0, FQGPU_OVERLAP_WORDS) and, each where not nullptr, count limits of either mate and count insert sizes */
  void pairOverlap(std::size_t first, DecompressionWorkspace &mate, std::size_t mate_first, std::size_t count, const fqgpu_overlap &spec,
                   uint64_t *out, uint16_t *limit_out, uint16_t *mate_limit_out, uint16_t *insert_out = nullptr) {
    const int rc = fqgpu_chunk_pair_overlap(ctx_, first, mate.ctx_, mate_first, count, &spec, out, FQGPU_OVERLAP_WORDS, limit_out, mate_limit_out, insert_out);
    if (rc != FQGPU_OK)
      throw std::runtime_error("pairOverlap: chunk " + std::to_string(staged_idx_) + " against chunk " + std::to_string(mate.staged_idx_) + ": " +
                               fqgpu_strerror(rc));
  }
  /** fqgpu_chunk_pair_correct: with pairOverlap's insert sizes of the same records, the mismatched bases inside every overlap
   *  corrected IN BOTH STAGED CHUNKS -> report[0, FQGPU_CORRECT_REPORT_WORDS).  Every selection, digest or summary taken
   *  afterwards sees the corrected bytes */
  void pairCorrect(std::size_t first, DecompressionWorkspace &mate, std::size_t mate_first, std::size_t count, const uint16_t *insert,
                   const fqgpu_correct &spec, uint64_t *report) {
    const int rc = fqgpu_chunk_pair_correct(ctx_, first, mate.ctx_, mate_first, count, insert, &spec, report, nullptr, nullptr);
    if (rc != FQGPU_OK)
      throw std::runtime_error("pairCorrect: chunk " + std::to_string(staged_idx_) + " against chunk " + std::to_string(mate.staged_idx_) + ": " +
                               fqgpu_strerror(rc));
  }
  /** fqgpu_chunk_pair_merge: with pairOverlap's insert sizes of the same records and the pair bits `mark` (nullptr: every
   *  pair), the mates of every marked pair that has an insert merged into one read -> the bytes written to out (at most cap:
   *  the two chunks' recorded sizes together are always enough), report[0, FQGPU_MERGE_REPORT_WORDS) and -- merged_bits not
   *  nullptr -- the bits of the merged pairs.  Both staged chunks stay as they are */
  std::size_t pairMerge(std::size_t first, DecompressionWorkspace &mate, std::size_t mate_first, std::size_t count, const uint16_t *insert,
                        const uint8_t *mark, const fqgpu_merge &spec, uint8_t *out, std::size_t cap, uint64_t *report, uint8_t *merged_bits) {
    std::size_t len = 0;
    const int rc = fqgpu_chunk_pair_merge(ctx_, first, mate.ctx_, mate_first, count, insert, mark, &spec, out, cap, &len, report, merged_bits);
    if (rc != FQGPU_OK)
      throw std::runtime_error("pairMerge: chunk " + std::to_string(staged_idx_) + " against chunk " + std::to_string(mate.staged_idx_) + ": " +
                               fqgpu_strerror(rc));
    return len;
  }

  /** The misc pass backwards (the reference's decompressMiscBuffers, src/workspace.cpp:215-256): every
   *  misc stream is restored from its compressed twin to the size the container recorded; index.n_count /
   *  index.n_pos are set to the ends of the buffers (the decoder pops from there) */
  void decompressMiscBuffers(CompressedBuffersSrc &cbs) const { decompressMiscBuffers(cbs, fmt_); }
  static void decompressMiscBuffers(CompressedBuffersSrc &cbs, const headers::HeaderFormatSpeciciation &fmt) {
    if (cbs.compressed_header_fields.size() != fmt.n_fields() || cbs.original_size.header_fields.size() != fmt.n_fields())
      throw std::invalid_argument("decodeChunk: header field streams do not match the format");
    cbs.header_fields.resize(fmt.n_fields());
    for (auto &plain : cbs.header_fields) plain.clear();
    miscStreams(cbs, fmt, [](auto &plain, const std::vector<std::byte> &packed, const uint32_t &size) {
      plain.resize(size);
      memdecompress(plain.data(), plain.size(), packed.data(), packed.size());
    });
    cbs.index.n_count = cbs.n_count.size();
    cbs.index.n_pos = cbs.n_pos.size();
  }

private:
  /** The chunk decoded check-only -- nothing of it comes back -- with the block's decode indexes when present, and its
   *  digest taken (setVerify): it is left on the handle's staging block, where the fqgpu_chunk_* calls find it.  No host
   *  fallback: a chunk the device refuses throws std::runtime_error naming the chunk and the record. */
  void stageChunk(CompressedBuffersSrc &cbs, const char *who, StageClock *clk = nullptr) {
    last_digest_ = {};
    const auto refused = [&](const std::string &what) {
      return std::runtime_error(std::string(who) + ": chunk " + std::to_string(cbs.chunk_idx) + ": " + what);
    };
    ChunkArgs a;
    if (!chunkArgs(cbs, a)) throw refused("header field streams do not match the format");
    if (clk) clk->lap("misc");
    // the check-only mode is this call's alone: a workspace that restores whole chunks elsewhere keeps doing so
    struct CheckOnly {
      fqgpu_ctx *ctx;
      bool restore;
      ~CheckOnly() { if (restore) (void)fqgpu_ctx_set_check_only(ctx, 0); }
    } mode{ctx_, !check_only_};
    fqgpuCheck(fqgpu_ctx_set_check_only(ctx_, 1), who);
    RecordTable recs(a.n_recs);
    std::size_t laid_out = 0, bad = 0;
    const StreamArgs &s = a.s;
    const int rc = fqgpu_decode_chunk(ctx_, &a.hdr, a.readlens, a.n_recs, s.seq, s.seq_len, s.qual, s.qual_len, s.n_count, s.n_count_len,
                                      s.n_pos, s.n_pos_len, s.index[0], s.index_len[0], s.index[1], s.index_len[1], nullptr,
                                      cbs.original_size.total, recs.data(), &laid_out, &bad);
    if (rc != FQGPU_OK)
      throw refused(bad == static_cast<std::size_t>(-1) ? std::string("no record named: ") + fqgpu_strerror(rc)
                                                         : "record " + std::to_string(bad) + ": " + fqgpu_strerror(rc));
    if (clk) clk->lap("gpu");
    takeDigest();
  }

  /** decodeChunk through fqgpu_decode_chunk; false: the device refused the chunk (the host path decides) */
  bool decodeChunkOnDevice(FastqChunk &chunk, CompressedBuffersSrc &cbs) {
    StageClock clk;
    const bool build = buildsIndexFor(cbs), restore = !(build && index_only_) && !check_only_;
    chunk.clear();
    chunk.idx = cbs.chunk_idx;
    if (restore) {
      if (chunk.raw_data.capacity() < cbs.original_size.total) chunk.raw_data.reserve(cbs.original_size.total + cbs.original_size.total / 16 + 4096);
      chunk.raw_data.resize(cbs.original_size.total);
    }
    clk.lap("resize");
    ChunkArgs a;
    if (!chunkArgs(cbs, a)) return false;
    clk.lap("misc");
    const std::size_t n = a.n_recs, nf = fmt_.n_fields();
    RecordTable recs(n);
    std::size_t laid_out = 0, bad = 0;
    const StreamArgs &s = a.s;
    uint8_t *raw_out = restore ? reinterpret_cast<uint8_t *>(chunk.raw_data.data()) : nullptr;
    const int rc = build ? fqgpu_decode_chunk_indexing(ctx_, &a.hdr, a.readlens, n, s.seq, s.seq_len, s.qual, s.qual_len, s.n_count,
                                                       s.n_count_len, s.n_pos, s.n_pos_len, raw_out, cbs.original_size.total, recs.data(),
                                                       &laid_out, &bad)
                         : fqgpu_decode_chunk(ctx_, &a.hdr, a.readlens, n, s.seq, s.seq_len, s.qual, s.qual_len, s.n_count, s.n_count_len,
                                              s.n_pos, s.n_pos_len, s.index[0], s.index_len[0], s.index[1], s.index_len[1], raw_out,
                                              cbs.original_size.total, recs.data(), &laid_out, &bad);
    clk.lap("gpu");
    if (!deviceTook(rc, bad, "decodeChunk")) return false;
    takeDigest();
    takeStats("decodeChunk");
    for (int k = 0; k < 2 && build; ++k) {
      std::size_t len = 0;
      fqgpuCheck(fqgpu_decode_index(ctx_, k, nullptr, 0, &len), "decodeChunk");
      cbs.decode_index[k].resize(len);
      fqgpuCheck(fqgpu_decode_index(ctx_, k, reinterpret_cast<uint8_t *>(cbs.decode_index[k].data()), len, &len), "decodeChunk");
    }
    if (!restore) {  // (no bytes to point into: the chunk names its position alone)
      clk.done(chunk.idx);
      return true;
    }
    // the stream cursors where the host decoder leaves them: every stream consumed up to the chunk's last header
    for (std::size_t i = 0; i < nf; ++i) {
      auto &f = cbs.header_fields[i];
      f.index = {};
      if (fmt_.field_types[i] == headers::FieldType::NUMERIC) {
        f.index.contentPos = n * sizeof(headers::numeric_t);
        continue;
      }
      f.index.isDifferentPos = n;
      f.index.contentLengthPos = n - static_cast<std::size_t>(std::count(f.isDifferentFlag.begin(), f.isDifferentFlag.begin() + n, std::byte{0}));
      for (std::size_t j = 0; j < f.index.contentLengthPos; ++j) f.index.contentPos += static_cast<unsigned char>(f.contentLength[j]);
    }
    CompressionWorkspace::recordViews(chunk, recs);
    clk.lap("table");
    clk.done(chunk.idx);
    return true;
  }

  bool build_index_ = false, index_only_ = false, verify_ = false, check_only_ = false;
  ChunkDigest last_digest_;
  unsigned staged_idx_ = 0;  // the chunk stagePairedChunk staged last (for messages)
  /** the digest of the chunk the handle has just restored */
  void takeDigest() {
    if (!verify_) return;
    fqgpuCheck(fqgpu_chunk_crc32(ctx_, &last_digest_.crc32, &last_digest_.length), "decodeChunk");
    last_digest_.valid = true;
  }
  /** setBuildIndex is on and this chunk came without indexes */
  bool buildsIndexFor(const CompressedBuffersSrc &cbs) const {
    return build_index_ && cbs.decode_index[0].empty() && cbs.decode_index[1].empty();
  }

  /** FQGPU_SHIM_HOST_HEADERS=1: the host coder lays the chunks out */
  static bool hostHeaders() {
    static const bool host_headers = std::getenv("FQGPU_SHIM_HOST_HEADERS") != nullptr;
    return host_headers;
  }

  /** the coded streams of cbs (misc buffers decompressed) as the C ABI's decode calls take them */
  struct StreamArgs {
    const uint8_t *seq = nullptr, *qual = nullptr;
    const uint16_t *n_count = nullptr, *n_pos = nullptr;
    std::size_t seq_len = 0, qual_len = 0, n_count_len = 0, n_pos_len = 0;
    const uint8_t *index[2] = {nullptr, nullptr};
    std::size_t index_len[2] = {0, 0};
    StreamArgs() = default;
    explicit StreamArgs(const CompressedBuffersSrc &cbs)
        : seq(reinterpret_cast<const uint8_t *>(cbs.seq.data())), qual(reinterpret_cast<const uint8_t *>(cbs.qual.data())),
          n_count(reinterpret_cast<const uint16_t *>(cbs.n_count.data())), n_pos(reinterpret_cast<const uint16_t *>(cbs.n_pos.data())),
          seq_len(cbs.seq.size()), qual_len(cbs.qual.size()), n_count_len(cbs.index.n_count / sizeof(uint16_t)),
          n_pos_len(cbs.index.n_pos / sizeof(uint16_t)),
          index{reinterpret_cast<const uint8_t *>(cbs.decode_index[0].data()), reinterpret_cast<const uint8_t *>(cbs.decode_index[1].data())},
          index_len{cbs.decode_index[0].size(), cbs.decode_index[1].size()} {}
  };
  /** a chunk as the device's chunk decodes take it; sizes / streams hold what hdr points to */
  struct ChunkArgs {
    std::vector<fqgpu_field_sizes> sizes;
    std::vector<const uint8_t *> streams;
    fqgpu_header_streams hdr;
    const uint16_t *readlens;
    std::size_t n_recs;
    StreamArgs s;
  };
  /** the misc pass, then cbs as the device takes it; false: streams that do not match the format (the host path throws) */
  bool chunkArgs(CompressedBuffersSrc &cbs, ChunkArgs &a) const {
    decompressMiscBuffers(cbs);
    const std::size_t n = cbs.original_size.n_records, nf = fmt_.n_fields();
    if (cbs.header_fields.size() != nf || cbs.readlens.size() < n * sizeof(readlen_t)) return false;
    a.sizes.resize(nf);
    a.streams.resize(3 * nf);
    for (std::size_t i = 0; i < nf; ++i) {
      const auto &f = cbs.header_fields[i];
      a.sizes[i] = {static_cast<uint32_t>(f.isDifferentFlag.size()), static_cast<uint32_t>(f.content.size()),
                    static_cast<uint32_t>(f.contentLength.size())};
      a.streams[3 * i] = reinterpret_cast<const uint8_t *>(f.isDifferentFlag.data());
      a.streams[3 * i + 1] = reinterpret_cast<const uint8_t *>(f.content.data());
      a.streams[3 * i + 2] = reinterpret_cast<const uint8_t *>(f.contentLength.data());
    }
    a.hdr = fqgpu_header_streams{field_types_.data(), fmt_.separators.data(), static_cast<unsigned>(nf),
                                 reinterpret_cast<const uint8_t *>(meta_->first_header.data()), meta_->first_header.size(),
                                 a.sizes.data(), a.streams.data()};
    a.readlens = reinterpret_cast<const uint16_t *>(cbs.readlens.data());
    a.n_recs = n;
    a.s = StreamArgs(cbs);
    return true;
  }
  /** What a chunk decode's return code means.  Throws where the host path would end the same way: a damaged sequence /
   *  quality stream (no record named), a runtime failure, an overflow (the size was asked for first).  false: the device
   *  refused the chunk (the host path decides) */
  static bool deviceTook(int rc, std::size_t bad, const char *where) {
    if ((rc == FQGPU_E_CORRUPT && bad == static_cast<std::size_t>(-1)) || rc == FQGPU_E_HIP || rc == FQGPU_E_NOMEM ||
        rc == FQGPU_E_NO_DEVICE || rc == FQGPU_E_OVERFLOW)
      fqgpuCheck(rc, where);
    return rc == FQGPU_OK;
  }

  /** fqgpu_decode_chunk_range: the size query (*len), then, with a piece, the decode into it.  false: the device
   *  refused the chunk (the host path decides) */
  bool rangeOnDevice(CompressedBuffersSrc &cbs, std::size_t first, std::size_t end, FastqChunk *piece, std::size_t *len) {
    StageClock clk;
    ChunkArgs a;
    if (!chunkArgs(cbs, a)) return false;
    clk.lap("misc");
    const auto call = [&](uint8_t *out, std::size_t cap, fqgpu_rec *recs) {
      std::size_t bad = 0;
      const StreamArgs &s = a.s;
      const int rc = fqgpu_decode_chunk_range(ctx_, &a.hdr, a.readlens, a.n_recs, s.seq, s.seq_len, s.qual, s.qual_len, s.n_count,
                                              s.n_count_len, s.n_pos, s.n_pos_len, s.index[0], s.index_len[0], s.index[1],
                                              s.index_len[1], cbs.original_size.total, first, end, out, cap, len, recs, &bad);
      return deviceTook(rc, bad, "decodeChunkRange");
    };
    if (!call(nullptr, 0, nullptr)) return false;
    clk.lap("gpu size");
    if (!piece) return true;
    piece->clear();
    piece->idx = cbs.chunk_idx;
    piece->raw_data.resize(*len);
    RecordTable recs(end - first);
    if (!call(reinterpret_cast<uint8_t *>(piece->raw_data.data()), piece->raw_data.size(), recs.data())) return false;
    clk.lap("gpu");
    CompressionWorkspace::recordViews(*piece, recs);
    clk.done(cbs.chunk_idx);
    return true;
  }

  /** fqgpu_decode_chunk_fasta: the size query, then, with a piece, the decode into it; returns the size.  Every refusal
   *  throws. */
  std::size_t fastaOnDevice(CompressedBuffersSrc &cbs, std::size_t first, std::size_t end, FastqChunk *piece) {
    StageClock clk;
    ChunkArgs a;
    const auto refused = [&](const std::string &what) {
      return std::runtime_error("decodeChunkFasta: chunk " + std::to_string(cbs.chunk_idx) + ": " + what);
    };
    if (!chunkArgs(cbs, a)) throw refused("header field streams do not match the format");
    clk.lap("misc");
    std::size_t len = 0;
    const auto call = [&](uint8_t *out, std::size_t cap) {
      std::size_t bad = 0;
      const StreamArgs &s = a.s;
      const int rc = fqgpu_decode_chunk_fasta(ctx_, &a.hdr, a.readlens, a.n_recs, s.seq, s.seq_len, s.n_count, s.n_count_len, s.n_pos,
                                              s.n_pos_len, s.index[0], s.index_len[0], cbs.original_size.total, first, end, out, cap,
                                              &len, nullptr, &bad);
      if (rc == FQGPU_OK) return;
      throw refused(bad == static_cast<std::size_t>(-1) ? std::string("no record named: ") + fqgpu_strerror(rc)
                                                         : "record " + std::to_string(bad) + ": " + fqgpu_strerror(rc));
    };
    // a whole chunk is smaller as FASTA than its recorded FASTQ size: one call; a range asks for its size first
    const bool whole = piece && first == 0 && end == a.n_recs;
    if (!whole) call(nullptr, 0);
    clk.lap("gpu size");
    if (!piece) return len;
    piece->clear();
    piece->idx = cbs.chunk_idx;
    piece->raw_data.resize(whole ? cbs.original_size.total : len);
    call(reinterpret_cast<uint8_t *>(piece->raw_data.data()), piece->raw_data.size());
    piece->raw_data.resize(len);
    clk.lap("gpu");
    clk.done(cbs.chunk_idx);
    return len;
  }

  /** decodeHeader with the output bound checked: near the end of the chunk the header goes through
   *  a local buffer, since the field decoders may write up to FIELDLEN_MAX bytes per field */
  unsigned decodeHeaderChecked(char *dst, char *end, CompressedBuffersSrc &cbs) {
    const std::size_t worst = 1 + fmt_.n_fields() * (headers::FIELDLEN_MAX + 1);
    if (static_cast<std::size_t>(end - dst) >= worst) return headers::decodeHeader(dst, fmt_, prev_header_fields_, cbs.header_fields);
    tail_.resize(worst);
    const unsigned n = headers::decodeHeader(tail_.data(), fmt_, prev_header_fields_, cbs.header_fields);
    if (static_cast<std::size_t>(end - dst) < n) throw std::out_of_range("decodeChunk: original_size.total too small");
    std::memcpy(dst, tail_.data(), n);
    // string fields of the previous header must point at bytes that stay: re-anchor them in dst
    headers::header_fields_t anchored = headers::fromHeader(std::string_view(dst, n), fmt_);
    for (std::size_t i = 0; i < anchored.size(); ++i)
      if (fmt_.field_types[i] == headers::FieldType::STRING) prev_header_fields_[i] = anchored[i];
    return n;
  }
  std::vector<char> tail_;
  FastqChunk whole_;  // decodeChunkRange on the host path: the whole chunk, sliced
};

/** The host parser (FastqReader::parseRecords, src/fastq_io.cpp:67-125) on top of fqgpu_parse_fastq: fills
 *  chunk.records; returns the bytes up to the end of the last complete record */
inline std::size_t parseRecords(FastqChunk &chunk) {
  const auto *raw = reinterpret_cast<const uint8_t *>(chunk.raw_data.data());
  const long n = fqgpu_parse_fastq(raw, chunk.raw_data.size(), nullptr, 0);
  if (n < 0) throw std::invalid_argument("malformed FASTQ block");
  RecordTable recs(static_cast<std::size_t>(n));
  fqgpu_parse_fastq(raw, chunk.raw_data.size(), recs.data(), recs.size());
  CompressionWorkspace::recordViews(chunk, recs);
  return recs.empty() ? 0 : static_cast<std::size_t>(recs.back().qual_off) + recs.back().len + 1;
}

}  // namespace fqcomp28
