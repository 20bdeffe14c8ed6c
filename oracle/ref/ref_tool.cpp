// oracle/ref/ref_tool.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// A driver over the reference's own classes, compiled together with the reference's unmodified
// sources (oracle/Makefile, target `ref`) into oracle/_ref/ref_tool.  The tests run it to pin the
// oracle (oracle/fqc_oracle.c, oracle/headers_oracle.py) and the HIP path to what the reference's
// compiled code does.  Built with asserts on: the reference's asserts are its input contract, and
// an abort is how it refuses an input.
//
//   ref_tool parse IN RECS_OUT
//       FastqReader::parseRecords on the bytes of IN.  RECS_OUT: five little-endian u32 per record
//       (header offset, header length, sequence offset, quality offset, read length).  stdout:
//       "used U records N bases B headers H".
//   ref_tool bounds N...
//       one line "N compressBoundSequence(N) compressBoundQuality(N)" per argument.
//   ref_tool analyze IN OUTDIR
//       DatasetMeta(chunk) of the whole records of IN: first_header.bin, field_types.bin (one byte
//       per field, 'N' numeric or 'S' string), separators.bin, seq_ft.bin and qual_ft.bin (the two
//       FreqTable structs as the reference stores them in an archive).
//   ref_tool encode IN OUTDIR [--tables-from SAMPLE | --seq-ft F --qual-ft F] [--first-header TEXT]
//       CompressionWorkspace::encodeChunk on the whole records of IN.  Tables: of IN itself, of the
//       whole records of SAMPLE, or the two struct files.  OUTDIR gets seq.bin, qual.bin,
//       readlens.bin, n_count.bin, n_pos.bin, raw_after.bin (the chunk after N replacement),
//       field_K.flags.bin / field_K.content.bin / field_K.lengths.bin (every header field before the
//       misc coder), sizes.bin (u32 chunk bytes, u32 records), and what `analyze` writes.
//   ref_tool decode DIR OUT
//       packs the plain misc buffers of such a directory with memcompress, runs
//       DecompressionWorkspace::decodeChunk and writes the restored chunk to OUT.
//   ref_tool write-archive IN ARCHIVE BLOCK_BYTES [SAMPLE_BYTES]
//   ref_tool read-archive ARCHIVE OUT
//       the chunk loops of the reference's processReads / processArchiveParts with one thread.
//   ref_tool shim-sizes TABLE_LOG MAX_SYMBOL
//       the values of the shim's four size macros (oracle/ref/shim/common/fse.h).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "archive.h"
#include "compressed_buffers.h"
#include "defs.h"
#include "fastq_io.h"
#include "memcompress.h"
#include "prepare.h"
#include "workspace.h"

using namespace fqcomp28;

namespace {

std::vector<char> readFile(const std::string &path) {
  std::ifstream is(path, std::ios::binary);
  if (!is) throw std::runtime_error("cannot read " + path);
  return std::vector<char>(std::istreambuf_iterator<char>(is), std::istreambuf_iterator<char>());
}

void writeFile(const std::string &path, const void *data, std::size_t n) {
  std::ofstream os(path, std::ios::binary);
  os.write(static_cast<const char *>(data), static_cast<std::streamsize>(n));
  if (!os) throw std::runtime_error("cannot write " + path);
}

void writeBytes(const std::string &path, const std::vector<std::byte> &v) { writeFile(path, v.data(), v.size()); }

std::vector<std::byte> readBytes(const std::string &path) {
  const auto c = readFile(path);
  std::vector<std::byte> v(c.size());
  if (!c.empty()) std::memcpy(v.data(), c.data(), c.size());
  return v;
}

/** the whole records of a file as one chunk: what readNextChunk hands on, the cut-off tail dropped */
void loadChunk(const std::string &path, FastqChunk &chunk) {
  chunk.clear();
  chunk.raw_data = readFile(path);
  const std::size_t used = FastqReader::parseRecords(chunk);
  chunk.raw_data.resize(used); /* shrinking: the record pointers stay valid */
}

void writeMeta(const std::string &dir, const DatasetMeta &meta) {
  writeFile(dir + "/first_header.bin", meta.first_header.data(), meta.first_header.size());
  std::string types;
  for (const auto t : meta.header_fmt.field_types) types += t == headers::FieldType::NUMERIC ? 'N' : 'S';
  writeFile(dir + "/field_types.bin", types.data(), types.size());
  writeFile(dir + "/separators.bin", meta.header_fmt.separators.data(), meta.header_fmt.separators.size());
  writeFile(dir + "/seq_ft.bin", meta.ft_seq.get(), sizeof(*meta.ft_seq));
  writeFile(dir + "/qual_ft.bin", meta.ft_qual.get(), sizeof(*meta.ft_qual));
}

template <class FT> std::unique_ptr<FT> loadTable(const std::string &path) {
  const auto bytes = readFile(path);
  if (bytes.size() != sizeof(FT)) throw std::runtime_error(path + ": not a frequency table struct");
  auto ft = std::make_unique<FT>();
  std::memcpy(static_cast<void *>(ft.get()), bytes.data(), sizeof(FT));
  return ft;
}

int cmdParse(const std::string &in, const std::string &out) {
  FastqChunk chunk;
  chunk.raw_data = readFile(in);
  const std::size_t used = FastqReader::parseRecords(chunk);
  std::vector<uint32_t> table;
  const char *beg = chunk.raw_data.data();
  for (const auto &r : chunk.records) {
    table.push_back(static_cast<uint32_t>(r.headerp - beg));
    table.push_back(r.header_length);
    table.push_back(static_cast<uint32_t>(r.seqp - beg));
    table.push_back(static_cast<uint32_t>(r.qualp - beg));
    table.push_back(r.length);
  }
  writeFile(out, table.data(), table.size() * sizeof(uint32_t));
  std::printf("used %zu records %zu bases %zu headers %zu\n", used, chunk.records.size(), chunk.tot_reads_length,
              chunk.headers_length);
  return 0;
}

int cmdBounds(int argc, char **argv) {
  for (int i = 0; i < argc; ++i) {
    const std::size_t n = std::strtoull(argv[i], nullptr, 10);
    std::printf("%zu %zu %zu\n", n, Workspace::compressBoundSequence(n), Workspace::compressBoundQuality(n));
  }
  return 0;
}

int cmdAnalyze(const std::string &in, const std::string &dir) {
  FastqChunk chunk;
  loadChunk(in, chunk);
  const DatasetMeta meta(chunk);
  writeMeta(dir, meta);
  return 0;
}

int cmdEncode(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string in = argv[0], dir = argv[1];
  std::string sample, seq_ft, qual_ft, first_header;
  bool have_first_header = false;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    if (i + 1 >= argc) return 2;
    if (a == "--tables-from") sample = argv[++i];
    else if (a == "--seq-ft") seq_ft = argv[++i];
    else if (a == "--qual-ft") qual_ft = argv[++i];
    else if (a == "--first-header") first_header = argv[++i], have_first_header = true;
    else return 2;
  }
  if (seq_ft.empty() != qual_ft.empty() || (!sample.empty() && !seq_ft.empty())) return 2;

  FastqChunk chunk;
  loadChunk(in, chunk);
  if (chunk.records.empty()) throw std::runtime_error("no whole record in " + in);

  DatasetMeta meta(have_first_header ? std::string_view(first_header) : chunk.records.front().header());
  if (!seq_ft.empty()) {
    meta.ft_seq = loadTable<FSE_Sequence::FreqTableT>(seq_ft);
    meta.ft_qual = loadTable<FSE_Quality::FreqTableT>(qual_ft);
  } else if (!sample.empty()) {
    FastqChunk s;
    loadChunk(sample, s);
    meta.ft_seq = FSE_Sequence::calculateFreqTable(s);
    meta.ft_qual = FSE_Quality::calculateFreqTable(s);
  } else {
    meta.ft_seq = FSE_Sequence::calculateFreqTable(chunk);
    meta.ft_qual = FSE_Quality::calculateFreqTable(chunk);
  }

  CompressionWorkspace wksp(&meta);
  CompressedBuffersDst cbs;
  wksp.encodeChunk(chunk, cbs);
  if (cbs.seq.empty() || cbs.qual.empty()) { /* endChunk() == 0: the stream did not fit its bound */
    std::fprintf(stderr, "ref_tool: a stream overflowed its bound\n");
    return 3;
  }

  writeMeta(dir, meta);
  writeBytes(dir + "/seq.bin", cbs.seq);
  writeBytes(dir + "/qual.bin", cbs.qual);
  writeBytes(dir + "/readlens.bin", cbs.readlens);
  writeBytes(dir + "/n_count.bin", cbs.n_count);
  writeBytes(dir + "/n_pos.bin", cbs.n_pos);
  writeFile(dir + "/raw_after.bin", chunk.raw_data.data(), chunk.raw_data.size());
  for (std::size_t i = 0; i < cbs.header_fields.size(); ++i) {
    const std::string stem = dir + "/field_" + std::to_string(i);
    writeBytes(stem + ".flags.bin", cbs.header_fields[i].isDifferentFlag);
    writeBytes(stem + ".content.bin", cbs.header_fields[i].content);
    writeBytes(stem + ".lengths.bin", cbs.header_fields[i].contentLength);
  }
  const uint32_t sizes[2] = {cbs.original_size.total, cbs.original_size.n_records};
  writeFile(dir + "/sizes.bin", sizes, sizeof(sizes));
  return 0;
}

void pack(std::vector<std::byte> &dst, const std::vector<std::byte> &src, uint32_t &original) {
  original = static_cast<uint32_t>(src.size());
  dst.resize(src.size() + 28);
  dst.resize(memcompress(dst.data(), src.data(), src.size()));
}

int cmdDecode(const std::string &dir, const std::string &out) {
  const auto fh = readFile(dir + "/first_header.bin");
  DatasetMeta meta(std::string_view(fh.data(), fh.size()));
  meta.ft_seq = loadTable<FSE_Sequence::FreqTableT>(dir + "/seq_ft.bin");
  meta.ft_qual = loadTable<FSE_Quality::FreqTableT>(dir + "/qual_ft.bin");

  CompressedBuffersSrc cbs;
  cbs.clear();
  cbs.chunk_idx = 0;
  const auto sizes = readFile(dir + "/sizes.bin");
  if (sizes.size() != 2 * sizeof(uint32_t)) throw std::runtime_error("sizes.bin: two u32 expected");
  std::memcpy(&cbs.original_size.total, sizes.data(), sizeof(uint32_t));
  std::memcpy(&cbs.original_size.n_records, sizes.data() + sizeof(uint32_t), sizeof(uint32_t));
  cbs.seq = readBytes(dir + "/seq.bin");
  cbs.qual = readBytes(dir + "/qual.bin");
  pack(cbs.compressed_readlens, readBytes(dir + "/readlens.bin"), cbs.original_size.readlens);
  pack(cbs.compressed_n_count, readBytes(dir + "/n_count.bin"), cbs.original_size.n_count);
  pack(cbs.compressed_n_pos, readBytes(dir + "/n_pos.bin"), cbs.original_size.n_pos);
  const std::size_t n_fields = meta.header_fmt.n_fields();
  cbs.original_size.header_fields.resize(n_fields);
  cbs.header_fields.resize(n_fields);
  cbs.compressed_header_fields.resize(n_fields);
  for (std::size_t i = 0; i < n_fields; ++i) {
    const std::string stem = dir + "/field_" + std::to_string(i);
    auto &c = cbs.compressed_header_fields[i];
    auto &o = cbs.original_size.header_fields[i];
    pack(c.isDifferentFlag, readBytes(stem + ".flags.bin"), o.isDifferentFlag);
    pack(c.content, readBytes(stem + ".content.bin"), o.content);
    pack(c.contentLength, readBytes(stem + ".lengths.bin"), o.contentLength);
  }

  DecompressionWorkspace wksp(&meta);
  FastqChunk chunk;
  wksp.decodeChunk(chunk, cbs);
  writeFile(out, chunk.raw_data.data(), chunk.raw_data.size());
  return 0;
}

int cmdWriteArchive(const std::string &fastq_path, const std::string &archive_path, std::size_t block_bytes,
                    std::size_t sample_bytes) {
  Archive out(archive_path, fastq_path, sample_bytes);
  FastqReader in(fastq_path, block_bytes);
  /* one workspace and ONE set of buffers for all blocks, as a worker thread of the reference has them: its
   * CompressedBuffersDst::clear() leaves n_count / n_pos alone, so they grow from block to block */
  CompressionWorkspace coder(&out.meta());
  CompressedBuffersDst block;
  FastqChunk records;
  while (in.readNextChunk(records)) {
    coder.encodeChunk(records, block);
    out.writeBlock(block);
  }
  out.writeIndex();
  out.flush();
  return 0;
}

int cmdReadArchive(const std::string &archive_path, const std::string &fastq_path) {
  Archive in(archive_path);
  FastqWriter out(fastq_path);
  DecompressionWorkspace coder(&in.meta());
  CompressedBuffersSrc block;
  FastqChunk records;
  while (in.readBlock(block)) {
    coder.decodeChunk(records, block);
    out.writeChunk(records);
  }
  out.flush();
  return 0;
}

int cmdShimSizes(unsigned log, unsigned max_symbol) {
  std::printf("ctable_u32 %zu dtable_u32 %zu ctable_wksp_bytes %zu dtable_wksp_bytes %zu dtable_wksp_u32 %zu\n",
              static_cast<std::size_t>(FSE_CTABLE_SIZE_U32(log, max_symbol)),
              static_cast<std::size_t>(FSE_DTABLE_SIZE_U32(log)),
              static_cast<std::size_t>(FSE_BUILD_CTABLE_WORKSPACE_SIZE(max_symbol, log)),
              static_cast<std::size_t>(FSE_BUILD_DTABLE_WKSP_SIZE(log, max_symbol)),
              static_cast<std::size_t>(FSE_BUILD_DTABLE_WKSP_SIZE_U32(log, max_symbol)));
  return 0;
}

int usage() {
  std::fprintf(stderr, "usage: ref_tool parse|bounds|analyze|encode|decode|write-archive|read-archive|shim-sizes ...\n");
  return 2;
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2) return usage();
  const std::string cmd = argv[1];
  const int n = argc - 2;
  char **a = argv + 2;
  try {
    if (cmd == "parse" && n == 2) return cmdParse(a[0], a[1]);
    if (cmd == "bounds" && n >= 1) return cmdBounds(n, a);
    if (cmd == "analyze" && n == 2) return cmdAnalyze(a[0], a[1]);
    if (cmd == "encode") {
      const int rc = cmdEncode(n, a);
      return rc == 2 ? usage() : rc;
    }
    if (cmd == "decode" && n == 2) return cmdDecode(a[0], a[1]);
    if (cmd == "write-archive" && (n == 3 || n == 4))
      return cmdWriteArchive(a[0], a[1], std::strtoull(a[2], nullptr, 10),
                             n == 4 ? std::strtoull(a[3], nullptr, 10) : mbToBytes(128));
    if (cmd == "read-archive" && n == 2) return cmdReadArchive(a[0], a[1]);
    if (cmd == "shim-sizes" && n == 2)
      return cmdShimSizes(static_cast<unsigned>(std::atoi(a[0])), static_cast<unsigned>(std::atoi(a[1])));
  } catch (const std::exception &e) {
    /* the reference's other way of refusing: invalid_argument, narrow_cast, system_error */
    std::fprintf(stderr, "ref_tool: exception: %s\n", e.what());
    return 4;
  }
  return usage();
}
