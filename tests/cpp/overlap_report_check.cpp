// The host logic of the mate overlap (fqcomp28_amd/csrc/process.hpp, fq_host.cpp), for a build with -fsanitize=address,undefined:
// the merge of the pieces' summaries into a worker's and of the workers' into the run's, and the report's text.
//   overlap_report_check merge <seed>   -> "ok": pieces of drawn counters dealt to drawn workers, merged as processArchivePaired
//                                          merges them, against the plain sum; what the merge refuses, and that it then
//                                          leaves dst alone
//   overlap_report_check text <min_overlap> <max_mism> <max_err_pct> <word>,<word>,... [<row>:<count> ...]
//                                       -> the report's text for a summary with these eight words and rows on stdout
//   overlap_report_check file <path>    -> writes a small report to <path> (through <path>.part) and prints it
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace fqcomp28;

static std::vector<uint64_t> summary_of(const char *words, char **rows, int n_rows, uint64_t fingerprint) {
  std::vector<uint64_t> w(FQGPU_OVERLAP_WORDS, 0);
  std::size_t i = 0;
  for (const char *p = words; *p && i < 8;) {
    w[i++] = std::strtoull(p, nullptr, 10);
    while (*p && *p != ',') ++p;
    if (*p) ++p;
  }
  for (int r = 0; r < n_rows; ++r) {
    char *colon = nullptr;
    const unsigned long row = std::strtoul(rows[r], &colon, 10);
    if (!colon || *colon != ':' || row >= FQGPU_OVERLAP_ROWS) throw std::invalid_argument("expected <row>:<count>");
    w[16 + row] = std::strtoull(colon + 1, nullptr, 10);
  }
  w[8] = fingerprint;
  return w;
}

int main(int argc, char **argv) {
  try {
    if (argc == 3 && !std::strcmp(argv[1], "merge")) {
      std::mt19937_64 rng(std::strtoull(argv[2], nullptr, 10));
      for (int round = 0; round < 200; ++round) {
        const unsigned n_workers = 1 + rng() % 5, n_pieces = rng() % 40;
        const uint64_t fp = 1 + rng() % 0xFFFFFFFFull;
        std::vector<std::vector<uint64_t>> worker(n_workers);  // (empty until the worker's first unit, as in the farm)
        std::vector<uint64_t> want(FQGPU_OVERLAP_WORDS, 0);
        for (unsigned p = 0; p < n_pieces; ++p) {
          std::vector<uint64_t> piece(FQGPU_OVERLAP_WORDS, 0);
          piece[0] = 1 + rng() % 5000;
          for (unsigned i = 1; i < 8; ++i) piece[i] = rng() % 100000;
          piece[8] = fp;
          for (int k = 0; k < 20; ++k) piece[16 + rng() % FQGPU_OVERLAP_ROWS] += rng() % 50;
          for (std::size_t i = 0; i < piece.size(); ++i) want[i] += piece[i];
          std::vector<uint64_t> &sum = worker[rng() % n_workers];
          if (sum.empty()) sum.assign(FQGPU_OVERLAP_WORDS, 0);
          if (fqgpu_overlap_merge(sum.data(), sum.size(), piece.data(), piece.size()) != FQGPU_OK) { std::printf("a piece is refused\n"); return 1; }
        }
        want[8] = n_pieces ? fp : 0;
        std::vector<uint64_t> run(FQGPU_OVERLAP_WORDS, 0);
        for (const auto &sum : worker)
          if (!sum.empty() && fqgpu_overlap_merge(run.data(), run.size(), sum.data(), sum.size()) != FQGPU_OK) { std::printf("a worker is refused\n"); return 1; }
        if (run != want) { std::printf("round %d: the merged summary is not the sum\n", round); return 1; }
        // what is refused leaves dst as it is
        std::vector<uint64_t> other(FQGPU_OVERLAP_WORDS, 0), before = run;
        other[0] = 1;
        other[8] = fp + 1;
        if (n_pieces && fqgpu_overlap_merge(run.data(), run.size(), other.data(), other.size()) != FQGPU_E_ARG) { std::printf("another spec is taken\n"); return 1; }
        if (fqgpu_overlap_merge(run.data(), run.size() - 1, other.data(), other.size()) != FQGPU_E_ARG ||
            fqgpu_overlap_merge(run.data(), run.size(), other.data(), other.size() - 1) != FQGPU_E_ARG ||
            fqgpu_overlap_merge(nullptr, run.size(), other.data(), other.size()) != FQGPU_E_ARG ||
            fqgpu_overlap_merge(run.data(), run.size(), nullptr, other.size()) != FQGPU_E_ARG) { std::printf("a bad length or a NULL is taken\n"); return 1; }
        if (run != before) { std::printf("a refused merge wrote to dst\n"); return 1; }
      }
      std::printf("ok\n");
      return 0;
    }
    if (argc >= 6 && !std::strcmp(argv[1], "text")) {
      const fqgpu_overlap spec = {static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 10)), static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10)),
                                  static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10)), {0, 0, 0, 0, 0}};
      const std::string text = overlapReportText(summary_of(argv[5], argv + 6, argc - 6, 7), spec);
      std::fwrite(text.data(), 1, text.size(), stdout);
      return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "file")) {
      const fqgpu_overlap spec = {30, 5, 20, {0, 0, 0, 0, 0}};
      char row_a[] = "40:2", row_b[] = "1023:1";
      char *rows[2] = {row_a, row_b};
      const std::vector<uint64_t> w = summary_of("10,3,2,7,8,1,4,160", rows, 2, 7);
      writeOverlapReport(argv[2], w, spec);
      const std::string text = overlapReportText(w, spec);
      std::fwrite(text.data(), 1, text.size(), stdout);
      bool refused = false;
      try { writeOverlapReport(argv[2], std::vector<uint64_t>(5, 0), spec); } catch (const std::logic_error &) { refused = true; }
      return refused ? 0 : 1;
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "overlap_report_check: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: overlap_report_check merge <seed> | text <min_overlap> <max_mism> <max_err_pct> <words> [<row>:<count> ...] | file <path>\n");
  return 2;
}
