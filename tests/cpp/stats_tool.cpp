// stats_tool -- the host side of the read summaries without a GPU (tests/test_stats_host.py):
//   stats_tool report <words.bin> <report.tsv>   writeStatsReport of a summary stored as little-endian u64 words; prints
//                                                its mean quality
//   stats_tool merge <dst.bin> <src.bin> ...     fqgpu_stats_merge of the files from left to right into the first, which is
//                                                written back; prints the return code of every merge
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

using namespace fqcomp28;

static std::vector<uint64_t> load(const char *path) {
  std::ifstream f(path, std::ios::binary);
  const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<uint64_t> w(bytes.size() / 8);
  std::memcpy(w.data(), bytes.data(), w.size() * 8);
  return w;
}

int main(int argc, char **argv) {
  try {
    if (argc == 4 && !strcmp(argv[1], "report")) {
      const std::vector<uint64_t> w = load(argv[2]);
      writeStatsReport(argv[3], w);
      std::printf("%.6f\n", statsMeanQuality(w));
      return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "merge")) {
      std::vector<uint64_t> dst = load(argv[2]);
      for (int i = 3; i < argc; ++i) {
        const std::vector<uint64_t> src = load(argv[i]);
        std::printf("%d\n", fqgpu_stats_merge(dst.data(), dst.size(), src.data(), src.size()));
      }
      std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(dst.data()), static_cast<std::streamsize>(dst.size() * 8));
      return 0;
    }
  } catch (const std::exception &e) {
    std::printf("refused: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: stats_tool report <words.bin> <report.tsv> | merge <dst.bin> <src.bin> ...\n");
  return 2;
}
