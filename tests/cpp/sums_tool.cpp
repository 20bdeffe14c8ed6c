// Host-only exerciser of the chunk sums file (fqcomp28_amd/csrc/archive.hpp: ChunkSumsFile) -- no GPU call:
//   sums_tool write <archive> <n> <seed>   n pseudo-random chunk sums, put in a scrambled order, written to <archive>.fqs
//                                          for that archive (any file); prints every field
//   sums_tool read <file.fqs>              prints every field of the file the same way; a file that is not a complete,
//                                          undamaged one: "refused: <message>", exit 1
//   sums_tool belongs <archive>            "own" / "foreign" (the identity of <archive>.fqs against the archive's), and
//                                          whether the archive still has the recorded size
// tests/test_checksum_host.py drives it, also under AddressSanitizer and UBSan, against a Python reading of the layout.
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstdlib>

using namespace fqcomp28;

static void print(const ChunkSumsFile &f) {
  std::printf("n %zu\n", f.size());
  for (std::size_t i = 0; i < f.size(); ++i) std::printf("chunk %zu %u %u %u\n", i, f.at(i).crc32, f.at(i).length, f.at(i).n_records);
  std::printf("file %u %llu\n", f.fileCrc32(), (unsigned long long)f.fileLength());
  std::printf("archive %llu %llu\n", (unsigned long long)f.archiveSize(), (unsigned long long)f.archiveHash());
}

int main(int argc, char **argv) {
  try {
    if (argc == 5 && std::string(argv[1]) == "write") {
      const std::size_t n = std::strtoull(argv[3], nullptr, 10);
      uint64_t s = std::strtoull(argv[4], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
      const auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return static_cast<uint32_t>(s >> 16); };
      std::vector<ChunkSumsFile::Sum> sums(n);
      for (auto &x : sums) x = {next(), next() % (300u << 20), next() % 2000000u};
      if (n > 2) sums[1].length = 0xFFFFFFFFu;  // (lengths up to the container's limit)
      ChunkSumsFile f;
      for (std::size_t k = 0; k < n; ++k) {  // any order
        const std::size_t i = (k * 7 + 3) % n;
        f.put(static_cast<uint32_t>(i), sums[i]);
      }
      for (std::size_t i = 0; i < n; ++i) f.put(static_cast<uint32_t>(i), sums[i]);  // (n not coprime with 7: fill the rest)
      f.write(argv[2]);
      print(f);
      return 0;
    }
    if (argc == 3 && std::string(argv[1]) == "read") {
      try {
        const ChunkSumsFile f{path_t(argv[2])};
        print(f);
      } catch (const std::runtime_error &e) {
        std::printf("refused: %s\n", e.what());
        return 1;
      }
      return 0;
    }
    if (argc == 3 && std::string(argv[1]) == "belongs") {
      const ChunkSumsFile f{ChunkSumsFile::pathFor(argv[2])};
      const auto id = DecodeIndexFile::identityOf(argv[2]);
      std::printf("%s %s\n", f.belongsTo(id) ? "own" : "foreign", f.archiveSize() == id.size ? "same-size" : "other-size");
      return 0;
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "sums_tool: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: sums_tool write <archive> <n> <seed> | read <file.fqs> | belongs <archive>\n");
  return 2;
}
