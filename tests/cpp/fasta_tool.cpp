// The host pieces of the FASTA restore (fqcomp28_amd/csrc/archive.hpp), for tests/test_fasta_host.py -- no GPU:
//   fasta_tool writer <out> <seed> ok|throw|abort
//        OrderedPieceWriter from 4 threads: 40 pieces of pseudo-random sizes (some empty), handed out in order, delivered in
//        scrambled completion order.  Byte i of piece k is (131 k + 7 i) mod 256.
//        ok:    prints "sizes s0 s1 ..." and "written <bytes>"; the file is the pieces' concatenation.
//        throw: the worker of piece 7 throws instead of delivering; the farm's failure hook aborts the writer.
//        abort: the worker of piece 7 holds its piece back until the main thread has called abort().
//        Both print "released <n>": the waiters that abort() let go with OrderedPieceWriter::Aborted; no file stays.
//   fasta_tool skipqual <in.fqc>
//        per block: readBlockAt(k, cb) and readBlockAt(k, cb, false) -- "block <k> extent <bytes a full read took> qual <bytes of
//        the quality stream> skipped <bytes the second read took> same <1: every field but qual equal, qual empty>"
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

using namespace fqcomp28;

namespace {
constexpr std::size_t N_PIECES = 40, HELD = 7;

std::vector<std::size_t> pieceSizes(uint64_t seed) {
  std::vector<std::size_t> sizes(N_PIECES);
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
  for (auto &s : sizes) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    s = (x >> 33) % 5 == 0 ? 0 : static_cast<std::size_t>((x >> 40) % 200000);
  }
  return sizes;
}
std::vector<char> pieceBytes(std::size_t k, std::size_t n) {
  std::vector<char> b(n);
  for (std::size_t i = 0; i < n; ++i) b[i] = static_cast<char>((131 * k + 7 * i) & 0xFF);
  return b;
}

int writer(const path_t &out, uint64_t seed, const std::string &mode) {
  const std::vector<std::size_t> sizes = pieceSizes(seed);
  std::atomic<std::size_t> next{0}, released{0};
  std::atomic<bool> stopped{false}, abort_called{false};
  bool failed = false;
  uint64_t written = 0;
  {
    OrderedPieceWriter w(out, N_PIECES);
    std::thread aborter;
    if (mode == "abort")
      aborter = std::thread([&] {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        w.abort();
        abort_called.store(true);
      });
    try {
      detail::runWorkers(4, [&](unsigned) {
        for (;;) {
          const std::size_t k = next.fetch_add(1);
          if (stopped.load() || k >= N_PIECES) break;
          const std::vector<char> b = pieceBytes(k, sizes[k]);
          // scrambled completion: a later piece is often ready before an earlier one
          std::this_thread::sleep_for(std::chrono::microseconds(((k * 2654435761u) >> 7) % 3000));
          if (k == HELD && mode == "throw") {
            std::this_thread::sleep_for(std::chrono::milliseconds(50));  // (the others are waiting by now)
            throw std::runtime_error("piece 7 could not be decoded");
          }
          if (k == HELD && mode == "abort")
            while (!abort_called.load()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
          try {
            w.writePiece(k, b.data(), b.size());
          } catch (const OrderedPieceWriter::Aborted &) {
            released.fetch_add(1);
            break;
          }
        }
      }, [&] { stopped.store(true); w.abort(); });
      w.flush();
      written = w.bytes();
    } catch (const std::exception &e) {
      failed = true;
      std::printf("failed: %s\n", e.what());
    }
    if (aborter.joinable()) aborter.join();
  }
  if (mode == "ok") {
    if (failed) return 1;
    std::printf("sizes");
    for (const std::size_t s : sizes) std::printf(" %zu", s);
    std::printf("\nwritten %llu\n", static_cast<unsigned long long>(written));
    return 0;
  }
  std::printf("released %zu\n", released.load());
  return failed ? 0 : 1;  // (these two modes must not get to a file)
}

int skipqual(const path_t &in) {
  Archive a(in);
  const auto &fmt = a.meta().header_fmt;
  for (std::size_t k = 0; k < a.nBlocks(); ++k) {
    CompressedBuffersSrc full, part;
    const uint64_t r0 = a.bytesRead();
    a.readBlockAt(k, full);
    const uint64_t r1 = a.bytesRead();
    a.readBlockAt(k, part, false);
    const uint64_t r2 = a.bytesRead();
    bool same = part.qual.empty() && full.chunk_idx == part.chunk_idx && full.original_size.total == part.original_size.total &&
                full.original_size.n_records == part.original_size.n_records;
    std::vector<std::string> f, p;
    std::vector<uint32_t> fo, po;
    const auto collect = [&](CompressedBuffersSrc &cb, std::vector<std::string> &bytes, std::vector<uint32_t> &orig) {
      blockfmt::blockFields(cb, fmt, [&](uint32_t *o, auto &data) {
        if (static_cast<const void *>(&data) == static_cast<const void *>(&cb.qual)) return;
        bytes.emplace_back(reinterpret_cast<const char *>(data.data()), data.size());
        orig.push_back(o ? *o : 0u);
      });
    };
    collect(full, f, fo);
    collect(part, p, po);
    same = same && f == p && fo == po;
    std::printf("block %zu extent %llu qual %zu skipped %llu same %d\n", k, static_cast<unsigned long long>(r1 - r0), full.qual.size(),
                static_cast<unsigned long long>(r2 - r1), same ? 1 : 0);
  }
  return 0;
}
}  // namespace

int main(int argc, char **argv) {
  try {
    if (argc == 5 && !strcmp(argv[1], "writer")) return writer(argv[2], std::strtoull(argv[3], nullptr, 10), argv[4]);
    if (argc == 3 && !strcmp(argv[1], "skipqual")) return skipqual(argv[2]);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "fasta_tool: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: fasta_tool writer <out> <seed> ok|throw|abort | skipqual <in.fqc>\n");
  return 2;
}
