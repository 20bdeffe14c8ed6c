// The host logic of the overlap correction (fqcomp28_amd/csrc/process.hpp, workspace.hpp, fq_host.cpp), for a build with
// -fsanitize=address,undefined: the report's text with and without a correction, the word-by-word sum of the pieces' reports
// into a worker's and of the workers' into the run's, and what Selection::check refuses.
//   correct_report_check text <words> <good_q> <bad_q> <cwords> [<row>:<count> ...]
//                                       -> the overlap report (spec 30, 5, 20) of a summary with these eight words and rows,
//                                          with the correction's six lines for the eight words <cwords>; <good_q> 0: without
//                                          a correction, through the old signature
//   correct_report_check sum <seed>     -> "ok": pieces of drawn reports dealt to drawn workers, added as processArchivePaired
//                                          adds them, against the plain sum; what the sum refuses
//   correct_report_check selection      -> "ok": Selection::check with a correction
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace fqcomp28;

static std::vector<uint64_t> words_of(const char *words, std::size_t size) {
  std::vector<uint64_t> w(size, 0);
  std::size_t i = 0;
  for (const char *p = words; *p && i < 8;) {
    w[i++] = std::strtoull(p, nullptr, 10);
    while (*p && *p != ',') ++p;
    if (*p) ++p;
  }
  return w;
}

template <class F> static bool refuses(F &&f, const char *what) {
  try {
    f();
  } catch (const std::invalid_argument &e) {
    return std::strstr(e.what(), what) != nullptr;
  }
  return false;
}

int main(int argc, char **argv) {
  try {
    if (argc >= 6 && !std::strcmp(argv[1], "text")) {
      const fqgpu_overlap spec = {30, 5, 20, {0, 0, 0, 0, 0}};
      std::vector<uint64_t> w = words_of(argv[2], FQGPU_OVERLAP_WORDS);
      for (int r = 6; r < argc; ++r) {
        char *colon = nullptr;
        const unsigned long row = std::strtoul(argv[r], &colon, 10);
        if (!colon || *colon != ':' || row >= FQGPU_OVERLAP_ROWS) throw std::invalid_argument("expected <row>:<count>");
        w[16 + row] = std::strtoull(colon + 1, nullptr, 10);
      }
      const fqgpu_correct c = {static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10)), static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10)),
                               {0, 0, 0, 0, 0, 0}};
      const std::string text = c.good_q ? overlapReportText(w, spec, &c, words_of(argv[5], FQGPU_CORRECT_REPORT_WORDS)) : overlapReportText(w, spec);
      std::fwrite(text.data(), 1, text.size(), stdout);
      if (c.good_q) {  // a correction without its eight words is a logic error, and nullptr gives the old bytes whatever comes with it
        bool refused = false;
        try { (void)overlapReportText(w, spec, &c, std::vector<uint64_t>(7, 0)); } catch (const std::logic_error &) { refused = true; }
        if (!refused || overlapReportText(w, spec, nullptr, std::vector<uint64_t>(3, 1)) != overlapReportText(w, spec)) return 1;
      }
      return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "sum")) {
      std::mt19937_64 rng(std::strtoull(argv[2], nullptr, 10));
      for (int round = 0; round < 200; ++round) {
        const unsigned n_workers = 1 + rng() % 5, n_pieces = rng() % 40;
        std::vector<std::vector<uint64_t>> worker(n_workers);  // (empty until the worker's first piece, as in the farm)
        std::vector<uint64_t> want(FQGPU_CORRECT_REPORT_WORDS, 0);
        for (unsigned p = 0; p < n_pieces; ++p) {
          uint64_t piece[FQGPU_CORRECT_REPORT_WORDS];
          for (uint64_t &v : piece) v = rng() % 100000;
          for (unsigned i = 0; i < FQGPU_CORRECT_REPORT_WORDS; ++i) want[i] += piece[i];
          addCorrectReport(worker[rng() % n_workers], piece, FQGPU_CORRECT_REPORT_WORDS);
        }
        std::vector<uint64_t> run(FQGPU_CORRECT_REPORT_WORDS, 0);
        for (const auto &sum : worker)
          if (!sum.empty()) addCorrectReport(run, sum.data(), sum.size());
        if (run != want) { std::printf("round %d: the summed report is not the sum\n", round); return 1; }
        const std::vector<uint64_t> before = run;
        int refused = 0;
        try { addCorrectReport(run, want.data(), FQGPU_CORRECT_REPORT_WORDS - 1); } catch (const std::logic_error &) { refused++; }
        try { addCorrectReport(run, nullptr, FQGPU_CORRECT_REPORT_WORDS); } catch (const std::logic_error &) { refused++; }
        std::vector<uint64_t> odd(3, 0);
        try { addCorrectReport(odd, want.data(), FQGPU_CORRECT_REPORT_WORDS); } catch (const std::logic_error &) { refused++; }
        if (refused != 3 || run != before) { std::printf("a bad length or a NULL is taken\n"); return 1; }
      }
      std::printf("ok\n");
      return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "selection")) {
      const fqgpu_overlap o = {30, 5, 20, {0, 0, 0, 0, 0}};
      const fqgpu_correct good = {30, 14, {0, 0, 0, 0, 0, 0}}, equal = {30, 30, {0, 0, 0, 0, 0, 0}}, zero = {0, 0, {0, 0, 0, 0, 0, 0}},
                          high = {64, 14, {0, 0, 0, 0, 0, 0}}, reserved = {30, 14, {0, 0, 0, 0, 0, 1}}, widest = {63, 62, {0, 0, 0, 0, 0, 0}},
                          narrowest = {1, 0, {0, 0, 0, 0, 0, 0}};
      Selection sel;
      sel.overlap = &o;
      for (const fqgpu_correct *c : {&good, &widest, &narrowest}) {
        sel.correct = c;
        sel.check("check", true);  // (throws when it refuses)
        sel.overlap_trim = !sel.overlap_trim;
      }
      for (const fqgpu_correct *c : {&equal, &zero, &high, &reserved}) {
        sel.correct = c;
        if (!refuses([&] { sel.check("check", true); }, "check: a correction fqgpu_correct_check refuses")) { std::printf("a bad spec is taken\n"); return 1; }
      }
      Selection alone;
      alone.correct = &good;
      if (!refuses([&] { alone.check("check", true); }, "check: a correction without an overlap spec")) { std::printf("a correction without an overlap is taken\n"); return 1; }
      Selection plain;  // (nothing new is asked of a selection without one)
      plain.overlap = &o;
      plain.check("check", true);
      std::printf("ok\n");
      return 0;
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "correct_report_check: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: correct_report_check text <words> <good_q> <bad_q> <cwords> [<row>:<count> ...] | sum <seed> | selection\n");
  return 2;
}
