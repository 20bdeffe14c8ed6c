// process.hpp -- the reference's block pipeline (src/process.cpp:32-105) over the GPU workspaces:
// N worker threads, each owning chunk + buffers + workspace (src/process.cpp:49-54, 95-98), pull
// whole blocks from a reader, code them, and hand them to a writer; blocks land in the archive in
// the order they claim their space and the index records chunk_idx (src/archive.h:85-89).  Reader,
// archive and writer (archive.hpp) move the bytes OUTSIDE their locks, and a failing worker stops
// the farm instead of leaving the others waiting (the reference's ordered writer would wait forever).
//
// What is new against the reference is only where a worker's workspace lives: worker t of T uses
// GPU devices[t mod G] (blocks are independent given the tables, every GPU holds a
// replica of them, no collective, no peer traffic).  With T > G several workers share a GPU; each
// has its own handle (own streams, own staging block in HBM), so worker A's H2D copy, worker B's
// kernels and worker C's D2H copy overlap on the device -- the chunk and stream buffers are
// page-locked (workspace.hpp: HostAllocator), the copies asynchronous (api.hip: fqgpu_encode_block).
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <optional>
#include <thread>
#include <type_traits>

#include "archive.hpp"

namespace fqcomp28 {

struct Settings {  // the part of src/settings.h:36-50 this path needs, plus the device list
  unsigned n_threads = 1;
  std::size_t reading_chunk_size = std::size_t(256) << 20;  // -R, MiB
  std::size_t sample_chunk_size = std::size_t(128) << 20;   // -S, MiB
  std::vector<int> devices = {0};
  /** The reference never clears cbs.n_count / cbs.n_pos (src/compressed_buffers.h:58-68), so block k
   *  of a worker carries the N tables of all its earlier blocks in front (decode pops
   *  from the end, so both forms decode everywhere).  Default: fresh tables per block -- the
   *  accumulation makes misc-stream work grow quadratically with the number of blocks. */
  bool accumulate_n_buffers = false;
  /** Workers that may be inside the source (reading a chunk) at once; 0 = a quarter of the workers, at least two.
   *  Sixteen workers that all read 256 MiB at the same moment share the host's memory bandwidth, finish together, then
   *  share the PCIe link, then the page cache: every stage waits for the slowest of sixteen.  Through a gate the first
   *  chunks are on the GPU while the others are still being read and the stages overlap from the first block on
   *  (FQGPU_FARM_READ_GATE overrides; a value of n_threads or more = no gate). */
  unsigned read_gate = 0;
  /** Extension: compress also writes `<archive>.fqx`, the decode indexes of every block (archive.hpp: DecodeIndexFile;
   *  about 2 % of the archive's size); decompress uses the file whenever it lies beside the archive. */
  bool decode_index = false;
  unsigned index_stride = 0;  // symbols between two snapshots of a decode index (multiple of 64 Ki; 0 = 1 Mi)
  /** Extension: decompress of an archive WITHOUT a usable `<archive>.fqx` builds one while it restores (one serial pass,
   *  at the pace the format dictates anyway: DecompressionWorkspace::setBuildIndex); every later restore and every
   *  --records query then runs at the indexed pace.  With a usable file nothing is built. */
  bool build_index = false;
  bool index_only = false;  // ... and nothing is restored (processArchiveIndex sets it)
  /** Extension: compress also writes `<archive>.fqs`, the CRC-32 of every chunk (archive.hpp: ChunkSumsFile); decompress
   *  verifies every restored chunk against the file whenever a usable one lies beside the archive. */
  bool checksum = false;
  bool verify = false;      // decompressFarm: the workspaces take every restored chunk's digest (the sink compares it)
  bool check_only = false;  // ... and nothing is restored (processArchiveCheck sets both)
  /** Extension: rows of the read summary every worker takes of its chunks where they lie on the device (Workspace::setStats;
   *  1 .. 65535); the report carries the merged result.  0: none.  compressFarm and processArchiveCheck look at it. */
  unsigned stats_positions = 0;
  /** Extension: the adapters every worker also searches its chunks for, where the summary is taken and with its rows
   *  (Workspace::setProbes; needs stats_positions); the report carries the merged adapter content.  Empty: none. */
  std::optional<fqgpu_probes> probes;
};

struct InputStats {  // src/report.h
  std::size_t seq = 0, header = 0, n_records = 0, raw = 0;
  InputStats &operator+=(const InputStats &o) { seq += o.seq; header += o.header; n_records += o.n_records; raw += o.raw; return *this; }
};
struct CompressedStats {
  std::size_t seq = 0, qual = 0, misc = 0, n_blocks = 0;
  CompressedStats &operator+=(const CompressedStats &o) { seq += o.seq; qual += o.qual; misc += o.misc; n_blocks += o.n_blocks; return *this; }
};
struct FarmReport {
  InputStats in;
  CompressedStats out;
  double seconds = 0;          // wall clock over the worker threads (tables and handles built before)
  std::vector<unsigned> blocks_per_worker;
  // decode indexes: blocks decoded from one and the bytes read (index_built false), or blocks given one and the bytes written
  std::size_t indexed_blocks = 0, index_bytes = 0;
  bool index_built = false;
  // chunk sums: "written" (compress), "used" / "none" / "unusable" (decompress, check); blocks whose digest was compared
  // and held; the whole file's CRC-32 (written, or as the sums file records it)
  const char *sums = "none";
  std::size_t verified_blocks = 0;
  uint32_t file_crc32 = 0;
  uint64_t archive_bytes_read = 0;  // processArchiveFasta: what was read of the archive file (the quality streams are not)
  std::vector<uint64_t> stats;      // the read summary of every chunk, merged (fqgpu_stats_words(set.stats_positions) words; empty: none taken)
  std::vector<uint64_t> probes;     // the adapter content of every chunk, merged (fqgpu_probe_words words; empty: set.probes was not given)
  std::vector<uint64_t> filter;     // processArchiveSelected with a filter alone: the chunks' filter reports, added word by word (FQGPU_FILTER_REPORT_WORDS; empty: none)
  std::vector<uint64_t> trim;       // processArchiveSelected with anything that cuts: the chunks' trim reports, added word by word (Selection::reportWords; empty: none)
};

namespace detail {
/** the workers' summaries, and their adapter content, into the report */
template <class Workspaces> void mergeStats(FarmReport &rep, const Workspaces &wksp, unsigned positions) {
  if (!positions) return;
  rep.stats.assign(fqgpu_stats_words(positions), 0);
  rep.stats[5] = positions;
  for (const auto &w : wksp) fqgpuCheck(fqgpu_stats_merge(rep.stats.data(), rep.stats.size(), w->stats().data(), w->stats().size()), "stats");
  for (const auto &w : wksp) {
    const std::vector<uint64_t> &p = w->probes();
    if (p.empty()) continue;
    if (rep.probes.empty()) rep.probes.assign(p.size(), 0);
    if (p[0]) fqgpuCheck(fqgpu_probe_merge(rep.probes.data(), rep.probes.size(), p.data(), p.size()), "probes");  // (a worker without a chunk has nothing)
  }
}
/** the report's probe set: nullptr unless a summary is taken as well */
inline const fqgpu_probes *probesOf(const Settings &set) { return set.stats_positions && set.probes ? &*set.probes : nullptr; }
inline std::size_t miscBytes(const CompressedBuffersDst &cbs) {
  std::size_t n = cbs.compressed_readlens.size() + cbs.compressed_n_count.size() + cbs.compressed_n_pos.size();
  for (const auto &f : cbs.compressed_header_fields) n += f.isDifferentFlag.size() + f.content.size() + f.contentLength.size();
  return n;
}
/** runs body(t) on n threads; a worker that throws calls on_failure() (which must make the sources
 *  of work run dry, so that the others finish their block and stop: nobody waits for anybody here);
 *  the first exception is rethrown after all have joined */
template <class Body, class OnFailure> void runWorkers(unsigned n, Body &&body, OnFailure &&on_failure) {
  std::vector<std::thread> threads;
  std::vector<std::exception_ptr> errors(n);
  threads.reserve(n);
  for (unsigned t = 0; t < n; ++t)
    threads.emplace_back([&, t] {
      try { body(t); } catch (...) { errors[t] = std::current_exception(); on_failure(); }
    });
  for (auto &th : threads) th.join();
  for (auto &e : errors) if (e) std::rethrow_exception(e);
}
template <class Body> void runWorkers(unsigned n, Body &&body) { runWorkers(n, body, [] {}); }

/** at most `slots` holders at a time (C++17: no std::counting_semaphore) */
class Gate {
public:
  explicit Gate(unsigned slots) : free_(slots) {}
  class Pass {
  public:
    explicit Pass(Gate &g) : g_(g) {
      std::unique_lock<std::mutex> lock(g_.m_);
      g_.cv_.wait(lock, [&] { return g_.free_ > 0; });
      --g_.free_;
    }
    ~Pass() {
      { const std::lock_guard<std::mutex> lock(g_.m_); ++g_.free_; }
      g_.cv_.notify_one();
    }
    Pass(const Pass &) = delete;
    Pass &operator=(const Pass &) = delete;
  private:
    Gate &g_;
  };
private:
  std::mutex m_;
  std::condition_variable cv_;
  unsigned free_;
};
}  // namespace detail

/** The compression farm: `next_chunk(chunk)` and `write_block(cbs)` are called concurrently from
 *  the workers and must be thread-safe (FastqReader::readNextChunk and Archive::writeBlock are);
 *  `stop()` is called when a worker fails and must make next_chunk return false from then on. */
template <class Source, class Sink, class Stop>
FarmReport compressFarm(const DatasetMeta &meta, Source &&next_chunk, Sink &&write_block, Stop &&stop, const Settings &set) {
  const unsigned T = std::max(1u, set.n_threads);
  if (set.devices.empty()) throw std::invalid_argument("compressFarm: no device");
  // every worker builds its workspace first (256 + 8192 tables on its GPU: the reference does the
  // same once per thread, src/workspace.h:62-64); the clock starts when all are ready
  // ... and so are its buffers: device scratch for chunks of the reading size, page-locked chunk and
  // stream buffers (half a second of hipMalloc / hipHostMalloc per worker that would otherwise sit
  // inside its first block)
  // (declared BEFORE the workspaces: locals die in reverse order, so the handles -- whose destruction waits for
  // everything they have queued -- go first and the page-locked buffers return to the pin cache after that)
  std::vector<FastqChunk> chunks(T);
  std::vector<CompressedBuffersDst> buffers(T);
  std::vector<std::unique_ptr<CompressionWorkspace>> wksp(T);
  detail::runWorkers(T, [&](unsigned t) {
    wksp[t] = std::make_unique<CompressionWorkspace>(&meta, set.devices[t % set.devices.size()]);
    wksp[t]->reserve(set.reading_chunk_size);
    wksp[t]->setDecodeIndex(set.decode_index, set.index_stride);
    wksp[t]->setChecksum(set.checksum);
    wksp[t]->setStats(set.stats_positions);
    wksp[t]->setProbes(detail::probesOf(set), set.stats_positions);
    chunks[t].raw_data.reserve(set.reading_chunk_size);
    buffers[t].seq.reserve(set.reading_chunk_size / 8 + (1u << 20));
    buffers[t].qual.reserve(set.reading_chunk_size / 3 + (1u << 20));
  });
  std::vector<InputStats> istats(T);
  std::vector<CompressedStats> cstats(T);
  FarmReport rep;
  rep.blocks_per_worker.assign(T, 0);
  unsigned gate_slots = set.read_gate ? set.read_gate : std::max(2u, T / 4);
  if (const char *e = std::getenv("FQGPU_FARM_READ_GATE")) gate_slots = std::max(1, std::atoi(e));
  detail::Gate read_gate(std::min(gate_slots, T));
  const auto t0 = std::chrono::steady_clock::now();
  detail::runWorkers(T, [&](unsigned t) {
    FastqChunk &chunk = chunks[t];
    CompressedBuffersDst &cbs = buffers[t];
    for (;;) {
      StageClock clk;
      {
        const detail::Gate::Pass pass(read_gate);
        if (!next_chunk(chunk)) break;
      }
      clk.lap("read");
      if (!set.accumulate_n_buffers) { cbs.n_count.clear(); cbs.n_pos.clear(); }
      wksp[t]->encodeChunk(chunk, cbs);  // (an unparsed chunk has its records found on the GPU: the sums are known afterwards)
      clk.lap("encodeChunk");
      istats[t].seq += chunk.tot_reads_length;
      istats[t].header += chunk.headers_length;
      istats[t].n_records += chunk.records.size();
      istats[t].raw += chunk.raw_data.size();
      cstats[t].seq += cbs.seq.size();
      cstats[t].qual += cbs.qual.size();
      cstats[t].misc += detail::miscBytes(cbs);
      cstats[t].n_blocks++;
      rep.blocks_per_worker[t]++;
      write_block(cbs);
      clk.lap("write");
      clk.done(chunk.idx);
    }
  }, stop);
  rep.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (unsigned t = 0; t < T; ++t) { rep.in += istats[t]; rep.out += cstats[t]; }
  detail::mergeStats(rep, wksp, set.stats_positions);
  return rep;
}
template <class Source, class Sink>
FarmReport compressFarm(const DatasetMeta &meta, Source &&next_chunk, Sink &&write_block, const Settings &set) {
  std::atomic<bool> stopped{false};
  return compressFarm(meta, [&](FastqChunk &c) { return !stopped.load() && next_chunk(c); }, write_block, [&] { stopped.store(true); }, set);
}

/** processReads (src/process.cpp:32-82): file in, archive out */
inline FarmReport processReads(const path_t &mates1, const path_t &archive_path, const Settings &set) {
  Archive archive(archive_path, mates1, set.sample_chunk_size, set.devices.at(0));
  FastqReader reader(mates1, set.reading_chunk_size);
  std::unique_ptr<DecodeIndexFile> sidecar;
  if (set.decode_index) {
    sidecar = std::make_unique<DecodeIndexFile>(DecodeIndexFile::pathFor(archive_path), PosFile::Mode::Create);
  } else {  // what an earlier archive of this name left behind is not this one's
    std::error_code ec;
    std::filesystem::remove(DecodeIndexFile::pathFor(archive_path), ec);
  }
  ChunkSumsFile sums;
  {  // what an earlier archive of this name left behind is not this one's
    std::error_code ec;
    std::filesystem::remove(ChunkSumsFile::pathFor(archive_path), ec);
  }
  FarmReport rep = compressFarm(
      archive.meta(), [&](FastqChunk &c) { return reader.readNextChunk(c); },
      [&](const CompressedBuffersDst &cbs) {
        archive.writeBlock(cbs);
        if (sidecar) sidecar->put(cbs);
        if (set.checksum) {
          if (!cbs.digest.valid || cbs.digest.length >= (uint64_t(1) << 32)) throw std::logic_error("no digest was taken of chunk " + std::to_string(cbs.chunk_idx));
          sums.put(cbs.chunk_idx, {cbs.digest.crc32, static_cast<uint32_t>(cbs.digest.length), cbs.original_size.n_records});
        }
      },
      [&] { reader.abort(); }, set);
  archive.writeIndex();
  archive.flush();
  if (sidecar) sidecar->close(DecodeIndexFile::identityOf(archive_path));
  if (set.checksum) {
    sums.write(archive_path);
    rep.sums = "written";
    rep.file_crc32 = sums.fileCrc32();
  }
  return rep;
}

/** The decompression farm (src/process.cpp:84-105): `next_block(cbs)` / `write_chunk(chunk)` thread-safe;
 *  `stop()`: a worker has failed, next_block must return false from now on */
template <class Source, class Sink, class Stop>
FarmReport decompressFarm(const DatasetMeta &meta, Source &&next_block, Sink &&write_chunk, Stop &&stop, const Settings &set) {
  const unsigned T = std::max(1u, set.n_threads);
  if (set.devices.empty()) throw std::invalid_argument("decompressFarm: no device");
  std::vector<std::unique_ptr<DecompressionWorkspace>> wksp(T);
  detail::runWorkers(T, [&](unsigned t) {
    wksp[t] = std::make_unique<DecompressionWorkspace>(&meta, set.devices[t % set.devices.size()]);
    wksp[t]->setBuildIndex(set.build_index, set.index_stride, set.index_only);
    wksp[t]->setVerify(set.verify);
    if (set.check_only) wksp[t]->setCheckOnly(true);
    wksp[t]->setStats(set.stats_positions);
    wksp[t]->setProbes(detail::probesOf(set), set.stats_positions);
  });
  std::vector<InputStats> istats(T);
  FarmReport rep;
  rep.blocks_per_worker.assign(T, 0);
  const auto t0 = std::chrono::steady_clock::now();
  detail::runWorkers(T, [&](unsigned t) {
    CompressedBuffersSrc cbs;
    FastqChunk chunk;
    for (;;) {
      StageClock clk;
      if (!next_block(cbs)) break;
      clk.lap("read");
      wksp[t]->decodeChunk(chunk, cbs);
      clk.lap("decodeChunk");
      istats[t].raw += chunk.raw_data.size();
      istats[t].n_records += cbs.original_size.n_records;
      rep.blocks_per_worker[t]++;
      // (a sink that also takes the block's buffers sees the decode indexes the workspace built; one that takes a digest
      // too, what setVerify made of the restored chunk)
      if constexpr (std::is_invocable_v<Sink &, const FastqChunk &, const CompressedBuffersSrc &, const ChunkDigest &>)
        write_chunk(chunk, cbs, wksp[t]->lastDigest());
      else if constexpr (std::is_invocable_v<Sink &, const FastqChunk &, const CompressedBuffersSrc &>) write_chunk(chunk, cbs);
      else write_chunk(chunk);
      clk.lap("write");
      clk.done(chunk.idx);
    }
  }, stop);
  rep.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (unsigned t = 0; t < T; ++t) rep.in += istats[t];
  detail::mergeStats(rep, wksp, set.stats_positions);
  return rep;
}
template <class Source, class Sink>
FarmReport decompressFarm(const DatasetMeta &meta, Source &&next_block, Sink &&write_chunk, const Settings &set) {
  std::atomic<bool> stopped{false};
  return decompressFarm(meta, [&](CompressedBuffersSrc &c) { return !stopped.load() && next_block(c); }, write_chunk, [&] { stopped.store(true); }, set);
}

namespace detail {
/** The archive's decode index file and what was used of it, the `.fqx` counterpart of ChunkVerifier: opened if one lies
 *  beside the archive and was written for it (another archive's is reported on stderr and not used), asked by the workers
 *  block by block, and at the end it says what it gave. */
class IndexSidecar {
public:
  explicit IndexSidecar(const path_t &archive_path) {
    const path_t p = DecodeIndexFile::pathFor(archive_path);
    if (!std::filesystem::exists(p)) return;
    file_ = std::make_unique<DecodeIndexFile>(p, PosFile::Mode::Read);
    if (!file_->belongsTo(DecodeIndexFile::identityOf(archive_path))) {
      std::fprintf(stderr, "%s was written for another archive: not used\n", p.string().c_str());
      file_.reset();
    }
  }
  [[nodiscard]] bool on() const { return file_ != nullptr; }
  /** thread-safe: the block's indexes into cbs.decode_index, counted; false: there is no usable file, or it has no entry for
   *  the chunk, which is then decoded without.  seq_only (the FASTA farm): the entry is checked as a whole, but the quality
   *  index has no use there, is dropped and not counted. */
  bool get(CompressedBuffersSrc &cbs, bool seq_only = false) {
    if (!file_ || !file_->get(cbs)) return false;
    if (seq_only) cbs.decode_index[1].clear();
    blocks_.fetch_add(1);
    bytes_.fetch_add(cbs.decode_index[0].size() + cbs.decode_index[1].size());
    return true;
  }
  void report(FarmReport &rep) const {
    rep.indexed_blocks = blocks_.load();
    rep.index_bytes = bytes_.load();
  }

private:
  std::unique_ptr<DecodeIndexFile> file_;
  std::atomic<std::size_t> blocks_{0}, bytes_{0};
};
}  // namespace detail

namespace detail {
/** The archive's chunk sums file and what became of it.  strict (the `t` command, whose only job is checking): a file
 *  that exists and cannot be used -- damaged, unclosed, written for another archive or for another number of blocks --
 *  is an error, and so is, once every chunk has held, an archive of another size than the recorded one.  Otherwise it is reported on stderr and NOT used: an optional file
 *  beside a good archive must never keep it from being restored (an archive whose size differs is still verified chunk
 *  by chunk: the file is its own). */
class ChunkVerifier {
public:
  ChunkVerifier(const path_t &archive_path, std::size_t n_blocks, bool strict) {
    const path_t p = ChunkSumsFile::pathFor(archive_path);
    if (!std::filesystem::exists(p)) {
      if (strict) std::fprintf(stderr, "%s: no chunk sums file: the streams are decoded, nothing is compared\n", archive_path.string().c_str());
      return;
    }
    std::string why;
    try {
      sums_ = std::make_unique<ChunkSumsFile>(p);
      const DecodeIndexFile::Identity id = DecodeIndexFile::identityOf(archive_path);
      if (!sums_->belongsTo(id)) why = "was written for another archive";
      else if (sums_->size() != n_blocks) why = "holds " + std::to_string(sums_->size()) + " chunks, the archive " + std::to_string(n_blocks);
      else if (sums_->archiveSize() != id.size) {  // (reported now; the chunks tell more, so they are still compared)
        size_differs_ = archive_path.string() + ": the archive has " + std::to_string(id.size) + " bytes, its chunk sums file recorded " +
                        std::to_string(sums_->archiveSize());
        std::fprintf(stderr, "%s\n", size_differs_.c_str());
      }
    } catch (const std::runtime_error &e) {
      why = e.what();
    }
    if (!why.empty()) {
      if (strict) throw std::runtime_error(p.string() + ": " + why);
      std::fprintf(stderr, "%s: %s: not used\n", p.string().c_str(), why.c_str());
      sums_.reset();
      state_ = "unusable";
      return;
    }
    state_ = "used";
  }
  [[nodiscard]] bool on() const { return sums_ != nullptr; }
  /** thread-safe; throws when the restored chunk is not the one the writer digested */
  void check(const CompressedBuffersSrc &cbs, const ChunkDigest &d) {
    if (!sums_) return;
    const ChunkSumsFile::Sum &want = sums_->at(cbs.chunk_idx);
    if (!d.valid || d.crc32 != want.crc32 || d.length != want.length || cbs.original_size.n_records != want.n_records) {
      char buf[256];
      std::snprintf(buf, sizeof(buf), "checksum of chunk %u does not hold: restored crc32 %08x, %zu bytes, %u records; recorded crc32 %08x, %u bytes, %u records",
                    cbs.chunk_idx, d.crc32, d.length, cbs.original_size.n_records, want.crc32, want.length, want.n_records);
      throw std::runtime_error(buf);
    }
    verified_.fetch_add(1);
  }
  void report(FarmReport &rep, bool strict = false) const {
    if (strict && !size_differs_.empty()) throw std::runtime_error(size_differs_);
    rep.sums = state_;
    rep.verified_blocks = verified_.load();
    if (sums_) rep.file_crc32 = sums_->fileCrc32();
  }

private:
  std::unique_ptr<ChunkSumsFile> sums_;
  const char *state_ = "none";
  std::string size_differs_;
  std::atomic<std::size_t> verified_{0};
};

/** A decode index file in the making: `<archive>.fqx.part` until every block's indexes are in it, then closed for the
 *  archive and renamed over whatever `<archive>.fqx` was; a build that does not get there leaves no file (FastqWriter
 *  works the same way) and the old one untouched. */
class DecodeIndexBuilder {
public:
  explicit DecodeIndexBuilder(const path_t &archive_path)
      : archive_(archive_path), final_(DecodeIndexFile::pathFor(archive_path)), part_(final_.string() + ".part"),
        file_(std::make_unique<DecodeIndexFile>(part_, PosFile::Mode::Create)) {}
  ~DecodeIndexBuilder() {
    if (done_) return;
    file_.reset();
    std::error_code ec;
    std::filesystem::remove(part_, ec);
  }
  /** thread-safe */
  void put(const CompressedBuffersSrc &cbs) {
    if (cbs.decode_index[0].empty() || cbs.decode_index[1].empty())
      throw std::runtime_error("no decode index was built for chunk " + std::to_string(cbs.chunk_idx));
    file_->put(cbs);
    blocks_.fetch_add(1);
    bytes_.fetch_add(cbs.decode_index[0].size() + cbs.decode_index[1].size());
  }
  void finish(FarmReport &rep) {
    file_->close(DecodeIndexFile::identityOf(archive_));
    file_.reset();
    std::filesystem::rename(part_, final_);
    done_ = true;
    rep.index_built = true;
    rep.indexed_blocks = blocks_.load();
    rep.index_bytes = bytes_.load();
  }

private:
  path_t archive_, final_, part_;
  std::unique_ptr<DecodeIndexFile> file_;
  std::atomic<std::size_t> blocks_{0}, bytes_{0};
  bool done_ = false;
};

/** The ordered hand-out loop of the restores whose unit of work is a numbered item -- a piece, a block, a pair of chunks:
 *  processArchiveRange, processArchiveFasta, processArchiveSelected, processArchivePaired.  It comes in two steps because the
 *  output is opened between them: detail::pieceFarm(name, n_items, set, make) readies the workers, run(body, abort, block_of)
 *  is the loop.  What every such restore relies on:
 *   - Worker count: T = max(1, min(set.n_threads, max(n_items, 1))).  The report's blocks_per_worker has max(1, set.n_threads)
 *     entries, of which only the first T are ever counted.
 *   - Device check: an empty set.devices throws std::invalid_argument("<name>: no device") from pieceFarm, that is before the
 *     caller has created any output file.  Worker t uses set.devices[t % set.devices.size()].
 *   - Start-up: make(t, device) builds worker t's state -- its workspace or workspaces, buffers and accumulators, of any type,
 *     movable or not; the helper knows nothing of it -- and the T of them are built concurrently.  The clock starts only when
 *     all exist (workers()[0] may then serve the caller before the loop: processArchiveRange sizes its edge pieces with it).
 *   - Hand-out: the items 0 .. n_items - 1 are handed out by ONE atomic counter, in increasing order, and a worker takes a new
 *     one only while nobody has failed.  OrderedPieceWriter's freedom from deadlock rests on this and on the next but one
 *     point: whoever waits in a writer waits for items that are already taken.
 *   - body(state, item, clk, in) does one item, adds what it wrote to `in` and says whether to go on.  When it returns false,
 *     or an OrderedPieceWriter::Aborted escapes it, the worker leaves quietly: somebody else has failed and says why.
 *   - When anything else escapes it, the stop flag is set and abort() is called, which must release everybody who waits in a
 *     writer (a FastqWriter has no waiters: nothing to do).  The others finish their item or are released, and leave.  After
 *     all have joined, the first exception by worker index is rethrown (runWorkers' rule); the caller's writers die without a
 *     flush(), so neither `<out>` nor `<out>.part` remains.
 *   - Per-item clock: every item gets a fresh StageClock, closed with block_of(item), the number of the block the item came
 *     from (FQGPU_SHIM_TRACE=1 prints the body's laps under it).
 *   - report(), called after the writers' flush(), gives blocks_per_worker, the workers' `in` added up and seconds, which so
 *     runs from "all workers ready" to "writers flushed". */
template <class State> class PieceFarm {
public:
  template <class Make> PieceFarm(const std::string &name, std::size_t n_items, const Settings &set, Make &&make)
      : n_items_(n_items), blocks_(std::max(1u, set.n_threads), 0) {
    if (set.devices.empty()) throw std::invalid_argument(name + ": no device");
    const unsigned T = std::max(1u, std::min<unsigned>(set.n_threads, static_cast<unsigned>(std::max<std::size_t>(n_items, 1))));
    workers_.resize(T);
    in_.resize(T);
    runWorkers(T, [&](unsigned t) { workers_[t].reset(new State(make(t, set.devices[t % set.devices.size()]))); });
    t0_ = std::chrono::steady_clock::now();
  }
  [[nodiscard]] const std::vector<std::unique_ptr<State>> &workers() const { return workers_; }
  template <class Body, class Abort, class BlockOf> void run(Body &&body, Abort &&abort, BlockOf &&block_of) {
    std::atomic<std::size_t> next{0};
    std::atomic<bool> stopped{false};
    runWorkers(static_cast<unsigned>(workers_.size()), [&](unsigned t) {
      for (;;) {
        const std::size_t item = next.fetch_add(1);
        if (stopped.load() || item >= n_items_) break;
        StageClock clk;
        try {
          if (!body(*workers_[t], item, clk, in_[t])) break;
        } catch (const OrderedPieceWriter::Aborted &) {
          break;
        }
        blocks_[t]++;
        clk.done(static_cast<unsigned>(block_of(item)));
      }
    }, [&] { stopped.store(true); abort(); });
  }
  /** items that are blocks, or units numbered as their blocks are */
  template <class Body, class Abort> void run(Body &&body, Abort &&abort) { run(body, abort, [](std::size_t item) { return item; }); }
  [[nodiscard]] FarmReport report() const {
    FarmReport rep;
    rep.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0_).count();
    rep.blocks_per_worker = blocks_;
    for (const InputStats &in : in_) rep.in += in;
    return rep;
  }

private:
  std::size_t n_items_;
  std::vector<unsigned> blocks_;
  std::vector<std::unique_ptr<State>> workers_;
  std::vector<InputStats> in_;
  std::chrono::steady_clock::time_point t0_;
};
/** the farm whose worker state is what make(t, device) returns */
template <class Make> auto pieceFarm(const std::string &name, std::size_t n_items, const Settings &set, Make &&make) {
  return PieceFarm<std::invoke_result_t<Make &, unsigned, int>>(name, n_items, set, make);
}

/** A restoring worker's state: its workspace, the block it has read and the piece it makes of it. */
struct RestoreWorker {
  DecompressionWorkspace wksp;
  CompressedBuffersSrc cbs;
  FastqChunk piece;
  RestoreWorker(const DatasetMeta &meta, int device, bool verify = false) : wksp(&meta, device) { wksp.setVerify(verify); }
};
}  // namespace detail

/** processArchiveParts (src/process.cpp:84-105): archive in, file out (chunks in original order).  set.build_index: an
 *  archive without a usable decode index file gets one on the way (and the report says so); with one, it is used as always
 *  and nothing is built. */
inline FarmReport processArchiveParts(const path_t &archive_path, const path_t &mates1_out, const Settings &set) {
  Archive archive(archive_path);
  const std::vector<uint64_t> chunk_at = archive.chunkOffsets();
  FastqWriter writer(mates1_out, chunk_at);
  detail::IndexSidecar sidecar(archive_path);
  std::unique_ptr<detail::DecodeIndexBuilder> builder;
  detail::ChunkVerifier verifier(archive_path, chunk_at.size() - 1, false);
  Settings farm = set;
  farm.build_index = set.build_index && !sidecar.on();
  farm.index_only = false;
  farm.verify = verifier.on();
  farm.check_only = false;
  farm.stats_positions = 0;
  if (farm.build_index) builder = std::make_unique<detail::DecodeIndexBuilder>(archive_path);
  FarmReport rep = decompressFarm(
      archive.meta(),
      [&](CompressedBuffersSrc &cbs) {
        if (!archive.readBlock(cbs)) return false;
        sidecar.get(cbs);
        return true;
      },
      [&](const FastqChunk &chunk, const CompressedBuffersSrc &cbs, const ChunkDigest &digest) {
        verifier.check(cbs, digest);  // (before the chunk reaches the file)
        writer.writeChunk(chunk);
        if (builder) builder->put(cbs);
      },
      [&] { archive.abort(); }, farm);
  writer.flush();
  sidecar.report(rep);
  verifier.report(rep);
  if (builder) builder->finish(rep);
  return rep;
}

/** Extension: `t` -- every block decoded and judged, every chunk's digest compared with the archive's chunk sums file,
 *  nothing restored and no file written.  With set.stats_positions (`s`) every chunk is also summarised where its decode
 *  left it, and the report carries the archive's read summary; everything else is the same.  Uses the decode index file when it lies there (the indexed pace).  Without a
 *  chunk sums file the streams are still decoded (rep.sums "none", nothing compared); with one that cannot be used the
 *  command fails: checking is all it does. */
inline FarmReport processArchiveCheck(const path_t &archive_path, const Settings &set) {
  Archive archive(archive_path);
  detail::IndexSidecar sidecar(archive_path);
  detail::ChunkVerifier verifier(archive_path, archive.chunkOffsets().size() - 1, true);
  Settings farm = set;
  farm.build_index = farm.index_only = false;
  farm.verify = verifier.on();
  farm.check_only = true;
  FarmReport rep = decompressFarm(
      archive.meta(),
      [&](CompressedBuffersSrc &cbs) {
        if (!archive.readBlock(cbs)) return false;
        sidecar.get(cbs);
        return true;
      },
      [&](const FastqChunk &, const CompressedBuffersSrc &cbs, const ChunkDigest &digest) { verifier.check(cbs, digest); },
      [&] { archive.abort(); }, farm);
  sidecar.report(rep);
  verifier.report(rep, true);
  return rep;
}

/** Extension: `x` -- the decode index file of an existing archive, and nothing else: every block is walked once from its
 *  streams' ends, only its indexes come back from the device, no FASTQ is written.  Always builds afresh: a stale,
 *  foreign, unclosed or damaged `<archive>.fqx` is not opened and is replaced when the last block has succeeded. */
inline FarmReport processArchiveIndex(const path_t &archive_path, const Settings &set) {
  Archive archive(archive_path);
  detail::DecodeIndexBuilder builder(archive_path);
  Settings farm = set;
  farm.build_index = farm.index_only = true;
  farm.stats_positions = 0;
  FarmReport rep = decompressFarm(
      archive.meta(),
      [&](CompressedBuffersSrc &cbs) {
        return archive.readBlock(cbs);  // (without decode indexes: readBlock clears the buffers)
      },
      [&](const FastqChunk &, const CompressedBuffersSrc &cbs) { builder.put(cbs); }, [&] { archive.abort(); }, farm);
  builder.finish(rep);
  return rep;
}

/** Extension: a part of one chunk to restore -- records [first, end) of block `block` (whole: all of them) */
struct RangePiece {
  std::size_t block = 0, first = 0, end = 0;
  bool whole = false;
};
/** Records [a, b) of an archive (numbered from 0 across it, in input order) as pieces of the blocks they overlap, in
 *  order; counts: records per block (Archive::recordCounts).  Throws std::invalid_argument unless a < b <= the total. */
inline std::vector<RangePiece> planRecordRange(const std::vector<uint32_t> &counts, std::size_t a, std::size_t b) {
  std::size_t total = 0;
  for (const uint32_t n : counts) total += n;
  if (a >= b || b > total)
    throw std::invalid_argument("records " + std::to_string(a) + ":" + std::to_string(b) + ": not a range of the archive's " +
                                std::to_string(total) + " records");
  std::vector<RangePiece> pieces;
  std::size_t at = 0;  // first record of block k
  for (std::size_t k = 0; k < counts.size() && at < b; at += counts[k], ++k) {
    const std::size_t lo = std::max(a, at), hi = std::min(b, at + counts[k]);
    if (lo >= hi) continue;
    pieces.push_back(RangePiece{k, lo - at, hi - at, lo == at && hi == at + counts[k]});
  }
  return pieces;
}

/** Extension: `d --records A:B` -- records [a, b) of the archive into a file of their own.  Only the blocks that
 *  overlap the range are read and decoded: the middle ones whole (decodeChunk), the one or two at the edges through
 *  decodeChunkRange (with the block's decode index, only the strides that hold the range).  The pieces' sizes are
 *  known before the farm starts -- a whole block's from its first word, an edge piece's from the layout passes
 *  (rangeSize) -- so FastqWriter places them as they finish.  b = SIZE_MAX: to the last record. */
inline FarmReport processArchiveRange(const path_t &archive_path, const path_t &mates1_out, std::size_t a, std::size_t b,
                                      const Settings &set) {
  Archive archive(archive_path);
  const std::vector<uint32_t> counts = archive.recordCounts();
  if (b == SIZE_MAX) {
    b = 0;
    for (const uint32_t n : counts) b += n;
  }
  const std::vector<RangePiece> pieces = planRecordRange(counts, a, b);
  const std::vector<uint64_t> chunk_at = archive.chunkOffsets();
  detail::IndexSidecar sidecar(archive_path);
  auto farm = detail::pieceFarm("processArchiveRange", pieces.size(), set,
                                [&](unsigned, int device) { return detail::RestoreWorker(archive.meta(), device); });
  std::vector<uint64_t> out_at(pieces.size() + 1, 0);
  for (std::size_t p = 0; p < pieces.size(); ++p) {
    const RangePiece &pc = pieces[p];
    std::size_t size = chunk_at[pc.block + 1] - chunk_at[pc.block];
    if (!pc.whole) {
      CompressedBuffersSrc cbs;
      archive.readBlockAt(pc.block, cbs);
      size = farm.workers()[0]->wksp.rangeSize(cbs, pc.first, pc.end);
    }
    out_at[p + 1] = out_at[p] + size;
  }
  FastqWriter writer(mates1_out, out_at);
  farm.run([&](detail::RestoreWorker &w, std::size_t p, StageClock &clk, InputStats &in) {
    const RangePiece &pc = pieces[p];
    archive.readBlockAt(pc.block, w.cbs);
    sidecar.get(w.cbs);
    clk.lap("read");
    if (pc.whole) w.wksp.decodeChunk(w.piece, w.cbs);
    else w.wksp.decodeChunkRange(w.piece, w.cbs, pc.first, pc.end);
    clk.lap("decode");
    w.piece.idx = static_cast<unsigned>(p);  // (the writer places pieces, not chunks)
    in.raw += w.piece.raw_data.size();
    in.n_records += w.piece.records.size();
    writer.writeChunk(w.piece);
    clk.lap("write");
    return true;
  }, [] {}, [&](std::size_t p) { return pieces[p].block; });  // (the sizes are known: nobody waits in this writer)
  writer.flush();
  FarmReport rep = farm.report();
  sidecar.report(rep);
  return rep;
}

/** Extension: `d --fasta [--records A:B]` -- the sequences alone, as FASTA (">hdr\nSEQ\n" per record, the header line
 *  as in the FASTQ but for its first byte).  Serves the whole archive (a = 0, b = SIZE_MAX) and a record range alike, as
 *  planRecordRange pieces that all go through decodeChunkFasta.  The quality streams are neither read from the archive
 *  (readBlockAt without them) nor uploaded nor decoded; of a usable `<archive>.fqx` only the sequence indexes are passed
 *  down.  Never builds an index and never verifies against `.fqs` (the sums describe FASTQ bytes): rep.sums "none".
 *  FASTA sizes are not recorded in the archive, so the pieces go through OrderedPieceWriter: handed out in order, placed
 *  by the sizes published so far. */
inline FarmReport processArchiveFasta(const path_t &archive_path, const path_t &fasta_out, std::size_t a, std::size_t b,
                                      const Settings &set) {
  Archive archive(archive_path);
  const std::vector<uint32_t> counts = archive.recordCounts();
  if (b == SIZE_MAX) {
    b = 0;
    for (const uint32_t n : counts) b += n;
  }
  const std::vector<RangePiece> pieces = planRecordRange(counts, a, b);
  detail::IndexSidecar sidecar(archive_path);
  auto farm = detail::pieceFarm("processArchiveFasta", pieces.size(), set,
                                [&](unsigned, int device) { return detail::RestoreWorker(archive.meta(), device); });
  const uint64_t read_before = archive.bytesRead();
  OrderedPieceWriter writer(fasta_out, pieces.size());
  farm.run([&](detail::RestoreWorker &w, std::size_t p, StageClock &clk, InputStats &in) {
    const RangePiece &pc = pieces[p];
    archive.readBlockAt(pc.block, w.cbs, false);
    sidecar.get(w.cbs, true);
    clk.lap("read");
    w.wksp.decodeChunkFasta(w.piece, w.cbs, pc.first, pc.end);
    clk.lap("decode");
    in.raw += w.piece.raw_data.size();
    in.n_records += pc.end - pc.first;
    writer.writePiece(p, w.piece.raw_data.data(), w.piece.raw_data.size());
    clk.lap("write");
    return true;
  }, [&] { writer.abort(); }, [&](std::size_t p) { return pieces[p].block; });
  writer.flush();
  FarmReport rep = farm.report();
  sidecar.report(rep);
  rep.archive_bytes_read = archive.bytesRead() - read_before;
  return rep;
}

/** Extension: `d` with any of the filter, trim, adapter, poly and window options -- the reads as `sel` leaves them, in input
 *  order: clipped at the 3' adapter, their poly-X tail and everything from a sliding-window quality drop on taken, trimmed,
 *  then judged by the filter (each step nullptr: off; no filter: every read that is not emptied is kept; a selection that
 *  cuts nothing needs its filter and writes the passing reads as the bytes a plain restore writes for them).  Every block is
 *  decoded on the device and selected there (decodeChunkSelected); only the kept bytes come down and reach the file.  A
 *  usable `<archive>.fqx` is used, and with a usable `<archive>.fqs` every chunk is verified before any of it is written: the
 *  digest is of the WHOLE restored chunk, as the writer took it.  Never builds an index.  The kept sizes are known only after
 *  the decode, so the blocks go through OrderedPieceWriter as the FASTA pieces do: handed out in order, placed by the sizes
 *  published so far; a failed run leaves neither `<out>` nor `<out>.part`.  rep.in counts what was written.  The chunks'
 *  reports, added word by word, go to rep.filter (what was read and why it was dropped) when nothing is cut, else to rep.trim:
 *  the same and what was cut, with an adapter words 14 and 15 (the reads in which it was found, the bases it took), with a
 *  tail FQGPU_TAIL_REPORT_WORDS words (then the reads with a poly tail, its bases, the reads the window cut, its bases). */
inline FarmReport processArchiveSelected(const path_t &archive_path, const path_t &mates1_out, const Selection &sel, const Settings &set) {
  sel.check("processArchiveSelected");
  Archive archive(archive_path);
  const std::size_t n_blocks = archive.chunkOffsets().size() - 1;
  detail::IndexSidecar sidecar(archive_path);
  detail::ChunkVerifier verifier(archive_path, n_blocks, false);
  struct Worker : detail::RestoreWorker {
    using RestoreWorker::RestoreWorker;
    uint64_t report[FQGPU_TAIL_REPORT_WORDS], sum[FQGPU_TAIL_REPORT_WORDS] = {};  // (the longest of the reports)
  };
  const unsigned W = sel.reportWords();
  auto farm = detail::pieceFarm("processArchiveSelected", n_blocks, set,
                                [&](unsigned, int device) { return Worker(archive.meta(), device, verifier.on()); });
  OrderedPieceWriter writer(mates1_out, n_blocks);
  farm.run([&](Worker &w, std::size_t k, StageClock &clk, InputStats &in) {
    archive.readBlockAt(k, w.cbs);
    sidecar.get(w.cbs);
    clk.lap("read");
    w.wksp.decodeChunkSelected(w.piece, w.cbs, sel, w.report);
    clk.lap("decode");
    verifier.check(w.cbs, w.wksp.lastDigest());  // (before anything of the chunk reaches the file)
    for (unsigned i = 0; i < W; ++i) w.sum[i] += w.report[i];
    in.raw += w.piece.raw_data.size();
    in.n_records += static_cast<std::size_t>(w.report[1]);
    writer.writePiece(k, w.piece.raw_data.data(), w.piece.raw_data.size());
    clk.lap("write");
    return true;
  }, [&] { writer.abort(); });
  writer.flush();
  FarmReport rep = farm.report();
  std::vector<uint64_t> &sum = sel.trims() ? rep.trim : rep.filter;
  sum.assign(W, 0);
  for (const auto &w : farm.workers())
    for (unsigned i = 0; i < W; ++i) sum[i] += w->sum[i];
  sidecar.report(rep);
  verifier.report(rep);
  return rep;
}

namespace detail {
/** Bits [from, from + count) of src -- bit i & 7 of byte i >> 3, the keep bits' layout -- as `count` bits from bit 0 of dst,
 *  which has (count + 7) / 8 bytes; the bits of its last byte behind them are zero. */
inline void sliceBits(const uint8_t *src, std::size_t from, std::size_t count, uint8_t *dst) {
  std::memset(dst, 0, (count + 7) / 8);
  for (std::size_t i = 0; i < count; ++i)
    if ((src[(from + i) >> 3] >> ((from + i) & 7)) & 1u) dst[i >> 3] |= static_cast<uint8_t>(1u << (i & 7));
}
/** The other way: `count` bits from bit 0 of src become the bits [at, at + count) of dst; its other bits stay. */
inline void placeBits(const uint8_t *src, std::size_t count, uint8_t *dst, std::size_t at) {
  for (std::size_t i = 0; i < count; ++i) {
    const uint8_t bit = static_cast<uint8_t>(1u << ((at + i) & 7));
    if ((src[i >> 3] >> (i & 7)) & 1u) dst[(at + i) >> 3] |= bit;
    else dst[(at + i) >> 3] &= static_cast<uint8_t>(~bit);
  }
}
}  // namespace detail

/** Extension: reports of fqgpu_chunk_pair_correct add word by word -- a piece's into its worker's, a worker's into the run's.
 *  dst: empty (it becomes src's size, zeros) or FQGPU_CORRECT_REPORT_WORDS words; src: that many, else std::logic_error. */
inline void addCorrectReport(std::vector<uint64_t> &dst, const uint64_t *src, std::size_t src_words) {
  if (dst.empty()) dst.assign(FQGPU_CORRECT_REPORT_WORDS, 0);
  if (!src || src_words != FQGPU_CORRECT_REPORT_WORDS || dst.size() != FQGPU_CORRECT_REPORT_WORDS)
    throw std::logic_error("addCorrectReport: not a correction's report");
  for (std::size_t i = 0; i < src_words; ++i) dst[i] += src[i];
}

/** Extension: reports of fqgpu_chunk_pair_merge add word by word, as the correction's do.  dst: empty (it becomes
 *  FQGPU_MERGE_REPORT_WORDS zeros) or that many words; src: that many, else std::logic_error. */
inline void addMergeReport(std::vector<uint64_t> &dst, const uint64_t *src, std::size_t src_words) {
  if (dst.empty()) dst.assign(FQGPU_MERGE_REPORT_WORDS, 0);
  if (!src || src_words != FQGPU_MERGE_REPORT_WORDS || dst.size() != FQGPU_MERGE_REPORT_WORDS)
    throw std::logic_error("addMergeReport: not a merge's report");
  for (std::size_t i = 0; i < src_words; ++i) dst[i] += src[i];
}

/** Extension: a part of a paired restore's work unit -- the mates of the records [at, at + end - first) of the unit are the
 *  records [first, end) of block `block` of archive 2 */
struct MatePiece {
  std::size_t block = 0, first = 0, end = 0, at = 0;
};
/** The mates of a unit that holds the records [a, b) of archive 1, as pieces of the blocks of archive 2 (counts2: its
 *  records per block) in order: planRecordRange with every piece's place in the unit.  Throws as planRecordRange does. */
inline std::vector<MatePiece> planMateUnit(const std::vector<uint32_t> &counts2, std::size_t a, std::size_t b) {
  std::vector<std::size_t> start2(counts2.size() + 1, 0);
  for (std::size_t k = 0; k < counts2.size(); ++k) start2[k + 1] = start2[k] + counts2[k];
  std::vector<MatePiece> pieces;
  for (const RangePiece &pc : planRecordRange(counts2, a, b)) pieces.push_back(MatePiece{pc.block, pc.first, pc.end, start2[pc.block] + pc.first - a});
  return pieces;
}

/** Extension: what a paired restore did -- a FarmReport per mate (in: what was written; trim: the chunks' marked reports,
 *  FQGPU_TAIL_REPORT_WORDS words added word by word; index, sums and verified as in a single restore, mate 2's counted per
 *  DECODE) and the pairs: both mates kept, dropped because mate 1 alone failed, mate 2 alone, both, and -- with a merge --
 *  merged into one read: pairs = kept + merged + the three dropped counts.  In mate1.trim and mate2.trim a merged pair shows
 *  under dropped_unmarked (word 20), for its bit is taken out of both mates' marks.  decodes2: chunk decodes of archive 2 (its
 *  number of chunks when the two archives are cut at the same records). */
struct PairedReport {
  FarmReport mate1, mate2;
  uint64_t pairs = 0, kept = 0, dropped_mate1_only = 0, dropped_mate2_only = 0, dropped_both = 0, merged = 0;
  std::size_t blocks1 = 0, blocks2 = 0, decodes2 = 0;
  std::vector<uint64_t> overlap;  // with Selection::overlap: the units' summaries merged (FQGPU_OVERLAP_WORDS; an archive without records: zeros)
  std::vector<uint64_t> correct;  // with Selection::correct: the pieces' reports added word by word (FQGPU_CORRECT_REPORT_WORDS)
  std::vector<uint64_t> merge;    // with Selection::merge: the pieces' reports added word by word (FQGPU_MERGE_REPORT_WORDS)
};

/** Extension: `d <in1.fqc> <out1.fastq> --mate <in2.fqc> <out2.fastq>` -- two archives whose records are mates restored in
 *  step: record i of both outputs are mates, and a pair is written only if BOTH mates pass.  Every step of `sel`
 *  (processArchiveSelected) applies to both mates, but that mate 2 is clipped at adapter2 instead of sel.adapter; each of the
 *  five may be nullptr: with all of them nullptr both files are restored whole and only the read ids are checked.
 *  The two archives need the same number of records and nothing else: their chunks are cut by bytes, so a chunk of archive 1
 *  -- the work unit, handed out in order -- holds the records [A, B) and planMateUnit(counts2, A, B) names the one to
 *  three chunks of archive 2 that hold their mates.  A worker owns one workspace per archive, both on its device, and needs
 *  no other worker: (1) chunk k of archive 1 decoded check-only, its digest taken; (2) a size query over it for its keep
 *  bits K1; (3) for every piece (j, lo, hi): chunk j of archive 2 decoded check-only, its digest taken, the read ids of the
 *  piece compared with their mates' (fqgpu_chunk_pair_names: a mismatch ends the run), the piece selected against the
 *  matching slice of K1 -- its output is appended to the unit's piece of file 2, its keep bits to K; (4) chunk k selected
 *  against K; (5) both pieces go to their OrderedPieceWriter as piece k.  A chunk of archive 2 that straddles a boundary of
 *  archive 1 is decoded by two workers (rep.decodes2 counts); with archives cut at the same records every chunk is decoded
 *  once.  With sel.overlap the mate overlap of every piece is analysed behind the id check (fqgpu_chunk_pair_overlap) and its
 *  summary merged into rep.overlap; with sel.overlap_trim as well the limits stand in front of each mate's steps, and the
 *  order inside a unit changes, because mate 1 cannot be judged before its mates are staged: step (2) is left out and per
 *  piece, behind the overlap, mate 1's records [at, at + count) are judged as a size query with their limits -- those keep
 *  bits are the piece's mark --, then the piece of mate 2 is judged and gathered with its limits; step (4) takes mate 1's
 *  limits too.  No chunk is decoded more often than without.  With sel.correct every piece is corrected directly behind its
 *  overlap (fqgpu_chunk_pair_correct with the piece's insert sizes), in front of everything that judges either mate, for it
 *  changes qualities and N counts: the unit takes the order just described -- its condition is "limits or correction", the
 *  limit pointers stay nullptr unless overlap_trim is on --, mate 1's chunk stays staged for the unit and collects every
 *  piece's corrections before its final gather, and a chunk of archive 2 that two workers decode is patched by each in its
 *  own range only.  The digests are taken at staging, before any correction; rep.correct sums the pieces' reports.
 *  With sel.merge (and `merged_out`, the third output) the unit takes that by-piece order too -- its condition is "limits,
 *  correction or merge" -- and per piece, behind the overlap and the optional correction: mate 1's range is judged as a size
 *  query (the piece's mark), mate 2's piece is judged as a SIZE QUERY with that mark (the pair bits `keep`: both mates pass,
 *  exactly as without a merge), fqgpu_chunk_pair_merge takes `keep` as its mark, appends the merged reads -- built from the
 *  staged, untrimmed, possibly corrected mates -- to the unit's merged piece and says which pairs it merged, and mate 2 is
 *  gathered with keep & ~merged, whose bits go into K: a merged pair is in neither mate file.  Mate 2's piece is judged twice;
 *  no chunk is decoded more often than without.  A third OrderedPieceWriter writes the merged piece as piece `unit`, so the
 *  merged file does not depend on how many workers there are; rep.merge sums the pieces' reports, rep.merged is its word 2.
 *  Each archive's `.fqx` is used and its `.fqs` verified as in a single restore; a failed run leaves neither output
 *  nor a `.part` file.  Throws before any output is opened when the archives' record totals differ. */
inline PairedReport processArchivePaired(const path_t &archive1_path, const path_t &out1, const path_t &archive2_path, const path_t &out2,
                                         const fqgpu_adapter *adapter2, const Selection &sel, const Settings &set,
                                         const path_t &merged_out = path_t()) {
  const std::string name("processArchivePaired");
  if (static_cast<bool>(sel.merge) != !merged_out.empty()) throw std::invalid_argument(name + ": a merge and a merged output come together");
  Selection sel2 = sel;
  sel2.adapter = adapter2;
  sel.check(name, true);
  sel2.check(name, true);
  Archive archive1(archive1_path), archive2(archive2_path);
  const std::vector<uint32_t> counts1 = archive1.recordCounts(), counts2 = archive2.recordCounts();
  const std::size_t n1 = counts1.size(), n2 = counts2.size();
  std::vector<std::size_t> start1(n1 + 1, 0);  // the first record of every chunk, numbered across the archive
  for (std::size_t k = 0; k < n1; ++k) start1[k + 1] = start1[k] + counts1[k];
  std::size_t total2 = 0;
  for (const uint32_t c : counts2) total2 += c;
  if (start1[n1] != total2)
    throw std::runtime_error(name + ": " + archive1_path.string() + " holds " + std::to_string(start1[n1]) + " records, " +
                             archive2_path.string() + " " + std::to_string(total2) + ": not the two files of one paired run");
  detail::IndexSidecar sidecar1(archive1_path), sidecar2(archive2_path);
  detail::ChunkVerifier verifier1(archive1_path, n1, false), verifier2(archive2_path, n2, false);
  constexpr unsigned W = FQGPU_TAIL_REPORT_WORDS;
  struct Worker {  // one workspace per archive, both on the worker's device; `in`, blocks and sums of mate 2 (mate 1's `in` and blocks are the farm's)
    detail::RestoreWorker m1, m2;
    std::vector<uint8_t> k1, k, mark, keep;
    std::vector<uint16_t> limit1, limit2;         // with an overlap spec: the unit's limits of mate 1, the piece's of mate 2
    std::vector<uint64_t> overlap, overlap_sum;   // ... the piece's summary, the worker's
    std::vector<uint16_t> insert;                 // with a correction: the piece's insert sizes
    uint64_t correct[FQGPU_CORRECT_REPORT_WORDS];  // ... the piece's report
    std::vector<uint64_t> correct_sum;             // ... the worker's (empty until its first piece)
    std::vector<uint8_t> merged_bits, merged_piece;  // with a merge: the piece's merged pairs, the unit's merged reads
    uint64_t merge[FQGPU_MERGE_REPORT_WORDS];        // ... the piece's report
    std::vector<uint64_t> merge_sum;                 // ... the worker's (empty until its first piece)
    uint64_t report[W], sum1[W] = {}, sum2[W] = {};
    InputStats in2;
    unsigned decodes2 = 0;
  };
  auto farm = detail::pieceFarm(name, n1, set, [&](unsigned, int device) {
    return Worker{{archive1.meta(), device, verifier1.on()}, {archive2.meta(), device, verifier2.on()}};
  });
  OrderedPieceWriter writer1(out1, n1), writer2(out2, n1);
  std::unique_ptr<OrderedPieceWriter> writer_merged(sel.merge ? new OrderedPieceWriter(merged_out, n1) : nullptr);
  farm.run([&](Worker &w, std::size_t unit, StageClock &clk, InputStats &in1) {
    DecompressionWorkspace &w1 = w.m1.wksp, &w2 = w.m2.wksp;
    CompressedBuffersSrc &cbs1 = w.m1.cbs, &cbs2 = w.m2.cbs;
    FastqChunk &piece1 = w.m1.piece, &piece2 = w.m2.piece;
    const std::size_t A = start1[unit], n = counts1[unit];
    piece1.clear();
    piece2.clear();
    piece1.idx = piece2.idx = static_cast<unsigned>(unit);
    std::size_t len1 = 0, len2 = 0, len_merged = 0;
    if (n) {
      archive1.readBlockAt(unit, cbs1);
      sidecar1.get(cbs1);
      clk.lap("read");
      w1.stagePairedChunk(cbs1);
      verifier1.check(cbs1, w1.lastDigest());  // (before anything of the chunk reaches the file)
      const bool limited = sel.overlap && sel.overlap_trim;  // the limits stand in front of each mate's steps
      const bool by_piece = limited || sel.correct || sel.merge;  // mate 1 is then judged piece by piece, behind the piece's overlap
      w.k1.assign((n + 7) / 8, 0);
      if (!by_piece) (void)w1.selectMarked(sel, 0, n, nullptr, nullptr, 0, w.report, w.k1.data());
      clk.lap("mate 1");
      w.k.assign((n + 7) / 8, 0);
      if (sel.overlap) {
        w.limit1.assign(n, 0);
        w.overlap.assign(FQGPU_OVERLAP_WORDS, 0);
        if (w.overlap_sum.empty()) w.overlap_sum.assign(FQGPU_OVERLAP_WORDS, 0);
      }
      for (const MatePiece &pc : planMateUnit(counts2, A, A + n)) {
        archive2.readBlockAt(pc.block, cbs2);
        sidecar2.get(cbs2);
        w2.stagePairedChunk(cbs2);
        verifier2.check(cbs2, w2.lastDigest());
        w.decodes2++;
        const std::size_t count = pc.end - pc.first, at = pc.at;
        const std::size_t differs = w1.pairNames(at, w2, pc.first, count);
        if (differs != static_cast<std::size_t>(-1))
          throw std::runtime_error(name + ": record " + std::to_string(A + at + differs) + ": the read ids of the two mates differ (chunk " +
                                   std::to_string(unit) + " of " + archive1_path.string() + ", chunk " + std::to_string(pc.block) + " of " +
                                   archive2_path.string() + ")");
        w.mark.resize((count + 7) / 8);
        w.keep.assign((count + 7) / 8, 0);
        if (sel.overlap) {
          w.limit2.assign(count, 0);
          const bool inserts = sel.correct || sel.merge;
          if (inserts) w.insert.assign(count, 0);
          w1.pairOverlap(at, w2, pc.first, count, *sel.overlap, w.overlap.data(), w.limit1.data() + at, w.limit2.data(),
                         inserts ? w.insert.data() : nullptr);
          if (fqgpu_overlap_merge(w.overlap_sum.data(), w.overlap_sum.size(), w.overlap.data(), w.overlap.size()) != FQGPU_OK)
            throw std::logic_error(name + ": overlap summaries of different specs");
          if (sel.correct) {  // (in front of everything that judges either mate)
            w1.pairCorrect(at, w2, pc.first, count, w.insert.data(), *sel.correct, w.correct);
            addCorrectReport(w.correct_sum, w.correct, FQGPU_CORRECT_REPORT_WORDS);
          }
        }
        if (by_piece) (void)w1.selectMarked(sel, at, at + count, nullptr, nullptr, 0, w.report, w.mark.data(), limited ? w.limit1.data() + at : nullptr);
        else detail::sliceBits(w.k1.data(), at, count, w.mark.data());
        if (sel.merge) {  // the pairs whose mates both pass; those of them that have an insert are merged and leave the mark
          (void)w2.selectMarked(sel2, pc.first, pc.end, w.mark.data(), nullptr, 0, w.report, w.keep.data(), limited ? w.limit2.data() : nullptr);
          const std::size_t cap = cbs1.original_size.total + cbs2.original_size.total;  // (fqgpu_chunk_pair_merge's bound)
          w.merged_piece.resize(len_merged + cap);
          w.merged_bits.assign((count + 7) / 8, 0);
          len_merged += w1.pairMerge(at, w2, pc.first, count, w.insert.data(), w.keep.data(), *sel.merge, w.merged_piece.data() + len_merged, cap,
                                     w.merge, w.merged_bits.data());
          addMergeReport(w.merge_sum, w.merge, FQGPU_MERGE_REPORT_WORDS);
          for (std::size_t i = 0; i < w.mark.size(); ++i) w.mark[i] = static_cast<uint8_t>(w.keep[i] & ~w.merged_bits[i]);
        }
        piece2.raw_data.resize(len2 + cbs2.original_size.total);  // (what is kept of a chunk is never more than the chunk)
        len2 += w2.selectMarked(sel2, pc.first, pc.end, w.mark.data(), reinterpret_cast<uint8_t *>(piece2.raw_data.data()) + len2,
                                cbs2.original_size.total, w.report, w.keep.data(), limited ? w.limit2.data() : nullptr);
        for (unsigned i = 0; i < W; ++i) w.sum2[i] += w.report[i];
        detail::placeBits(w.keep.data(), count, w.k.data(), at);
      }
      clk.lap("mate 2");
      piece1.raw_data.resize(cbs1.original_size.total);
      len1 = w1.selectMarked(sel, 0, n, w.k.data(), reinterpret_cast<uint8_t *>(piece1.raw_data.data()), piece1.raw_data.size(), w.report, nullptr,
                             limited ? w.limit1.data() : nullptr);
      for (unsigned i = 0; i < W; ++i) w.sum1[i] += w.report[i];
      in1.n_records += static_cast<std::size_t>(w.report[1]);
      w.in2.n_records += static_cast<std::size_t>(w.report[1]);
      clk.lap("gather 1");
    }
    piece1.raw_data.resize(len1);
    piece2.raw_data.resize(len2);
    in1.raw += len1;
    w.in2.raw += len2;
    writer1.writePiece(unit, piece1.raw_data.data(), len1);
    writer2.writePiece(unit, piece2.raw_data.data(), len2);
    if (writer_merged) writer_merged->writePiece(unit, w.merged_piece.data(), len_merged);
    clk.lap("write");
    return true;
  }, [&] { writer1.abort(); writer2.abort(); if (writer_merged) writer_merged->abort(); });
  writer1.flush();
  writer2.flush();
  if (writer_merged) writer_merged->flush();
  PairedReport rep;
  rep.mate1 = farm.report();
  rep.mate2.seconds = rep.mate1.seconds;
  rep.mate2.blocks_per_worker.assign(rep.mate1.blocks_per_worker.size(), 0);
  rep.mate1.trim.assign(W, 0);
  rep.mate2.trim.assign(W, 0);
  if (sel.overlap) rep.overlap.assign(FQGPU_OVERLAP_WORDS, 0);
  if (sel.correct) rep.correct.assign(FQGPU_CORRECT_REPORT_WORDS, 0);
  if (sel.merge) rep.merge.assign(FQGPU_MERGE_REPORT_WORDS, 0);
  for (std::size_t t = 0; t < farm.workers().size(); ++t) {
    const Worker &w = *farm.workers()[t];
    if (!w.overlap_sum.empty() && fqgpu_overlap_merge(rep.overlap.data(), rep.overlap.size(), w.overlap_sum.data(), w.overlap_sum.size()) != FQGPU_OK)
      throw std::logic_error(name + ": overlap summaries of different specs");
    if (!w.correct_sum.empty()) addCorrectReport(rep.correct, w.correct_sum.data(), w.correct_sum.size());
    if (!w.merge_sum.empty()) addMergeReport(rep.merge, w.merge_sum.data(), w.merge_sum.size());
    rep.mate2.in += w.in2;
    rep.mate2.blocks_per_worker[t] = w.decodes2;
    rep.decodes2 += w.decodes2;
    for (unsigned i = 0; i < W; ++i) {
      rep.mate1.trim[i] += w.sum1[i];
      rep.mate2.trim[i] += w.sum2[i];
    }
  }
  sidecar1.report(rep.mate1);
  sidecar2.report(rep.mate2);
  verifier1.report(rep.mate1);
  verifier2.report(rep.mate2);
  rep.blocks1 = n1;
  rep.blocks2 = n2;
  rep.pairs = start1[n1];
  rep.kept = rep.mate1.trim[1];
  rep.merged = sel.merge ? rep.merge[2] : 0;     // (a merged pair passes in both mates and is in neither mark)
  rep.dropped_mate1_only = rep.mate2.trim[20] - rep.merged;  // mate 2 passes, its mark -- mate 1's verdict -- says no
  rep.dropped_mate2_only = rep.mate1.trim[20] - rep.merged;
  rep.dropped_both = rep.pairs - rep.kept - rep.merged - rep.dropped_mate1_only - rep.dropped_mate2_only;
  return rep;
}

/** Extension: the report file of a mate overlap summary (fqgpu_chunk_pair_overlap, merged) -- text, tab-separated, integers
 *  only, a pure function of the summary and the spec: the spec's three numbers, the eight summary words by name, then
 *  "insert", I and the pairs for every non-empty row; with a correction (`correct` and its summed report `cw`), and only then,
 *  six more lines behind the last row: good_q, bad_q, pairs_corrected, bases_corrected_1, bases_corrected_2, n_resolved; with
 *  a merge (`merge` and its summed report `mw`), and only then, nine more behind those: min_len, floor_q, pairs_merged,
 *  bases_merged, bytes_merged, merged_overlap_bases (the merge's word 5: "overlap_bases" is the summary's line), places_disagree,
 *  places_n, pairs_too_short.  Written as `<path>.part` and renamed when it is complete. */
inline std::string overlapReportText(const std::vector<uint64_t> &w, const fqgpu_overlap &spec, const fqgpu_correct *correct = nullptr,
                                     const std::vector<uint64_t> &cw = {}, const fqgpu_merge *merge = nullptr,
                                     const std::vector<uint64_t> &mw = {}) {
  if (w.size() != FQGPU_OVERLAP_WORDS) throw std::logic_error("writeOverlapReport: not an overlap summary");
  if (correct && cw.size() != FQGPU_CORRECT_REPORT_WORDS) throw std::logic_error("writeOverlapReport: not a correction's report");
  if (merge && mw.size() != FQGPU_MERGE_REPORT_WORDS) throw std::logic_error("writeOverlapReport: not a merge's report");
  std::string out = "#fqgpu-overlap 1\n";
  const auto line = [&](const char *name, uint64_t v) { out += name; out += '\t'; out += std::to_string(v); out += '\n'; };
  line("min_overlap", spec.min_overlap);
  line("max_mism", spec.max_mism);
  line("max_err_pct", spec.max_err_pct);
  const char *names[8] = {"pairs", "pairs_overlapped", "pairs_read_through", "bases_behind_1", "bases_behind_2", "pairs_not_analysed", "mismatches",
                          "overlap_bases"};
  for (int i = 0; i < 8; ++i) line(names[i], w[i]);
  for (std::size_t r = 0; r < FQGPU_OVERLAP_ROWS; ++r)
    if (w[16 + r]) { out += "insert\t"; out += std::to_string(r); out += '\t'; out += std::to_string(w[16 + r]); out += '\n'; }
  if (correct) {  // behind the last row: the correction's two numbers and what it did
    line("good_q", correct->good_q);
    line("bad_q", correct->bad_q);
    line("pairs_corrected", cw[2]);
    line("bases_corrected_1", cw[3]);
    line("bases_corrected_2", cw[4]);
    line("n_resolved", cw[5]);
  }
  if (merge) {  // behind the correction's lines: the merge's two numbers and what it did
    line("min_len", merge->min_len);
    line("floor_q", merge->floor_q);
    line("pairs_merged", mw[2]);
    line("bases_merged", mw[3]);
    line("bytes_merged", mw[4]);
    line("merged_overlap_bases", mw[5]);
    line("places_disagree", mw[6]);
    line("places_n", mw[7]);
    line("pairs_too_short", mw[11]);
  }
  return out;
}
inline void writeOverlapReport(const path_t &path, const std::vector<uint64_t> &w, const fqgpu_overlap &spec, const fqgpu_correct *correct = nullptr,
                               const std::vector<uint64_t> &cw = {}, const fqgpu_merge *merge = nullptr, const std::vector<uint64_t> &mw = {}) {
  const std::string out = overlapReportText(w, spec, correct, cw, merge, mw);
  const path_t part = path.string() + ".part";
  std::FILE *f = std::fopen(part.string().c_str(), "wb");
  const bool ok = f && std::fwrite(out.data(), 1, out.size(), f) == out.size();
  if ((f && std::fclose(f) != 0) || !ok) {
    std::error_code ec;
    std::filesystem::remove(part, ec);
    throw std::runtime_error("cannot write " + part.string());
  }
  std::filesystem::rename(part, path);
}

namespace detail {
/** the report of the summary `w`, `more` behind it */
inline void writeStatsReportText(const path_t &path, const std::vector<uint64_t> &w, const std::string &more) {
  if (w.size() < 176 || w.size() != fqgpu_stats_words(static_cast<unsigned>(w[5]))) throw std::logic_error("writeStatsReport: not a read summary");
  const std::size_t rows = static_cast<std::size_t>(w[5]) + 1;
  const uint64_t *len = w.data() + 176, *base = len + rows, *qual = base + 5 * rows;
  std::string out = "#fqgpu-stats 1\n";
  const auto num = [&](uint64_t v) { out += std::to_string(v); };
  const char *names[6] = {"records", "bases", "min_len", "max_len", "reads_with_n", "positions"};
  for (int i = 0; i < 6; ++i) { out += names[i]; out += '\t'; num(w[i]); out += '\n'; }
  const auto hist = [&](const char *tag, const uint64_t *h, std::size_t n) {
    for (std::size_t i = 0; i < n; ++i)
      if (h[i]) { out += tag; out += '\t'; num(i); out += '\t'; num(h[i]); out += '\n'; }
  };
  hist("len", len, rows);
  hist("mq", w.data() + 8, 64);
  hist("gc", w.data() + 72, 101);
  std::size_t used = 0;  // rows 0 .. used - 1 are written
  for (std::size_t r = 0; r < rows; ++r) {
    bool any = false;
    for (int c = 0; c < 5; ++c) any = any || base[5 * r + c];
    for (int c = 0; c < 64; ++c) any = any || qual[64 * r + c];
    if (any) used = r + 1;
  }
  const auto table = [&](const char *tag, const uint64_t *t, std::size_t cols) {
    for (std::size_t r = 0; r < used; ++r) {
      out += tag; out += '\t'; num(r);
      for (std::size_t c = 0; c < cols; ++c) { out += '\t'; num(t[cols * r + c]); }
      out += '\n';
    }
  };
  table("base", base, 5);
  table("qual", qual, 64);
  out += more;
  const path_t part = path.string() + ".part";
  std::FILE *f = std::fopen(part.string().c_str(), "wb");
  const bool ok = f && std::fwrite(out.data(), 1, out.size(), f) == out.size();
  if ((f && std::fclose(f) != 0) || !ok) {
    std::error_code ec;
    std::filesystem::remove(part, ec);
    throw std::runtime_error("cannot write " + part.string());
  }
  std::filesystem::rename(part, path);
}
}  // namespace detail
/** Extension: the report file of a read summary (fqgpu_chunk_stats) -- text, tab-separated, integers only, a pure function
 *  of the summary -- written as `<path>.part` and renamed when it is complete. */
inline void writeStatsReport(const path_t &path, const std::vector<uint64_t> &w) { detail::writeStatsReportText(path, w, std::string()); }
/** Extension: the same report followed by the lines of an adapter content result `p` (fqgpu_chunk_probe) for the probe set
 *  `set`, whose probes have the names `names`: per probe "probe", its number, name, sequence, min_overlap, max_err_pct and the
 *  table's four counters, the same for "any" with "-" in the probe's places, then "probepos", the table and the row for every
 *  non-zero cell.  An empty `p` (no chunk was taken) counts as a result of zeros. */
inline void writeStatsReport(const path_t &path, const std::vector<uint64_t> &w, const std::vector<uint64_t> &p, const fqgpu_probes &set,
                             const std::vector<std::string> &names) {
  const unsigned n = set.n;
  const std::size_t rows = static_cast<std::size_t>(w.size() > 5 ? w[5] : 0) + 1, stride = 8 + rows;
  if (names.size() != n || (!p.empty() && (p.size() != fqgpu_probe_words(n, static_cast<unsigned>(rows - 1)) || (p[0] && (p[2] != n || p[3] != rows - 1)))))
    throw std::logic_error("writeStatsReport: not an adapter content result of these probes");
  const auto word = [&](std::size_t t, std::size_t i) -> uint64_t { return p.empty() ? 0 : p[8 + t * stride + i]; };
  std::string out;
  const auto num = [&](uint64_t v) { out += std::to_string(v); };
  for (unsigned t = 0; t <= n; ++t) {
    out += "probe\t";
    if (t < n) {
      const fqgpu_adapter &a = set.probe[t];
      num(t); out += '\t'; out += names[t]; out += '\t'; out.append(reinterpret_cast<const char *>(a.seq), a.len); out += '\t';
      num(a.min_overlap); out += '\t'; num(a.max_err_pct);
    } else {
      out += "any\t-\t-\t-\t-";
    }
    for (unsigned c = 0; c < 4; ++c) { out += '\t'; num(word(t, c)); }
    out += '\n';
  }
  for (unsigned t = 0; t <= n; ++t)
    for (std::size_t r = 0; r < rows; ++r)
      if (const uint64_t v = word(t, 8 + r)) {
        out += "probepos\t";
        if (t < n) num(t); else out += "any";
        out += '\t'; num(r); out += '\t'; num(v); out += '\n';
      }
  detail::writeStatsReportText(path, w, out);
}
/** total Phred of a read summary / its bases (0 without bases) */
inline double statsMeanQuality(const std::vector<uint64_t> &w) {
  const std::size_t rows = static_cast<std::size_t>(w[5]) + 1;
  const uint64_t *qual = w.data() + 176 + 6 * rows;
  uint64_t sum = 0;
  for (std::size_t r = 0; r < rows; ++r)
    for (unsigned q = 0; q < 64; ++q) sum += qual[64 * r + q] * q;
  return w[1] ? static_cast<double>(sum) / static_cast<double>(w[1]) : 0.0;
}
}  // namespace fqcomp28
