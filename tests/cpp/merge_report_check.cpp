// The host logic of the mate merge (fqcomp28_amd/csrc/process.hpp, workspace.hpp, fq_host.cpp), for a build with
// -fsanitize=address,undefined: the report's text with and without a merge, the word-by-word sum of the pieces' reports into
// a worker's and of the workers' into the run's, and what Selection::check refuses.
//   merge_report_check text <words> <good_q> <bad_q> <cwords> <min_len> <floor_q> <mwords> [<row>:<count> ...]
//                                     -> the overlap report (spec 30, 5, 20) of a summary with these eight words and rows, with
//                                        the correction's six lines for the eight words <cwords> (<good_q> 0: without one) and
//                                        the merge's nine lines for the sixteen words <mwords>; <min_len> 0: without a merge,
//                                        through the old signature
//   merge_report_check sum <seed>     -> "ok": pieces of drawn reports dealt to drawn workers, added as processArchivePaired
//                                        adds them, against the plain sum; what the sum refuses
//   merge_report_check selection      -> "ok": Selection::check with a merge
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace fqcomp28;

static std::vector<uint64_t> words_of(const char *words, std::size_t size, std::size_t given) {
  std::vector<uint64_t> w(size, 0);
  std::size_t i = 0;
  for (const char *p = words; *p && i < given;) {
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
    if (argc >= 9 && !std::strcmp(argv[1], "text")) {
      const fqgpu_overlap spec = {30, 5, 20, {0, 0, 0, 0, 0}};
      std::vector<uint64_t> w = words_of(argv[2], FQGPU_OVERLAP_WORDS, 8);
      for (int r = 9; r < argc; ++r) {
        char *colon = nullptr;
        const unsigned long row = std::strtoul(argv[r], &colon, 10);
        if (!colon || *colon != ':' || row >= FQGPU_OVERLAP_ROWS) throw std::invalid_argument("expected <row>:<count>");
        w[16 + row] = std::strtoull(colon + 1, nullptr, 10);
      }
      const fqgpu_correct c = {static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10)), static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10)),
                               {0, 0, 0, 0, 0, 0}};
      const std::vector<uint64_t> cw = words_of(argv[5], FQGPU_CORRECT_REPORT_WORDS, FQGPU_CORRECT_REPORT_WORDS);
      const fqgpu_merge m = {static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10)), static_cast<uint32_t>(std::strtoul(argv[6], nullptr, 10)),
                             {0, 0, 0, 0, 0, 0}};
      const std::vector<uint64_t> mw = words_of(argv[8], FQGPU_MERGE_REPORT_WORDS, FQGPU_MERGE_REPORT_WORDS);
      const fqgpu_correct *const cp = c.good_q ? &c : nullptr;
      const std::string old_text = cp ? overlapReportText(w, spec, cp, cw) : overlapReportText(w, spec);
      const std::string text = m.min_len ? overlapReportText(w, spec, cp, cw, &m, mw) : old_text;
      std::fwrite(text.data(), 1, text.size(), stdout);
      if (m.min_len) {  // a merge without its sixteen words is a logic error, and nullptr gives the old bytes whatever comes with it
        bool refused = false;
        try { (void)overlapReportText(w, spec, cp, cw, &m, std::vector<uint64_t>(FQGPU_MERGE_REPORT_WORDS - 1, 0)); } catch (const std::logic_error &) { refused = true; }
        if (!refused || overlapReportText(w, spec, cp, cw, nullptr, std::vector<uint64_t>(3, 1)) != old_text) return 1;
        if (text.compare(0, old_text.size(), old_text) != 0) return 1;  // (the merge's lines stand behind everything else)
      }
      return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "sum")) {
      std::mt19937_64 rng(std::strtoull(argv[2], nullptr, 10));
      for (int round = 0; round < 200; ++round) {
        const unsigned n_workers = 1 + rng() % 5, n_pieces = rng() % 40;
        std::vector<std::vector<uint64_t>> worker(n_workers);  // (empty until the worker's first piece, as in the farm)
        std::vector<uint64_t> want(FQGPU_MERGE_REPORT_WORDS, 0);
        for (unsigned p = 0; p < n_pieces; ++p) {
          uint64_t piece[FQGPU_MERGE_REPORT_WORDS];
          for (uint64_t &v : piece) v = rng() % 100000;
          for (unsigned i = 0; i < FQGPU_MERGE_REPORT_WORDS; ++i) want[i] += piece[i];
          addMergeReport(worker[rng() % n_workers], piece, FQGPU_MERGE_REPORT_WORDS);
        }
        std::vector<uint64_t> run(FQGPU_MERGE_REPORT_WORDS, 0);
        for (const auto &sum : worker)
          if (!sum.empty()) addMergeReport(run, sum.data(), sum.size());
        if (run != want) { std::printf("round %d: the summed report is not the sum\n", round); return 1; }
        const std::vector<uint64_t> before = run;
        int refused = 0;
        try { addMergeReport(run, want.data(), FQGPU_MERGE_REPORT_WORDS - 1); } catch (const std::logic_error &) { refused++; }
        try { addMergeReport(run, nullptr, FQGPU_MERGE_REPORT_WORDS); } catch (const std::logic_error &) { refused++; }
        try { addMergeReport(run, want.data(), FQGPU_CORRECT_REPORT_WORDS); } catch (const std::logic_error &) { refused++; }
        std::vector<uint64_t> odd(FQGPU_CORRECT_REPORT_WORDS, 0);
        try { addMergeReport(odd, want.data(), FQGPU_MERGE_REPORT_WORDS); } catch (const std::logic_error &) { refused++; }
        if (refused != 4 || run != before) { std::printf("a bad length or a NULL is taken\n"); return 1; }
      }
      std::printf("ok\n");
      return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "selection")) {
      const fqgpu_overlap o = {30, 5, 20, {0, 0, 0, 0, 0}};
      const fqgpu_correct correct = {30, 14, {0, 0, 0, 0, 0, 0}};
      const fqgpu_merge good = {2, 1, {0, 0, 0, 0, 0, 0}}, widest = {63, 1023, {0, 0, 0, 0, 0, 0}}, lowest = {0, 1, {0, 0, 0, 0, 0, 0}},
                        floor64 = {64, 1, {0, 0, 0, 0, 0, 0}}, len0 = {2, 0, {0, 0, 0, 0, 0, 0}}, len1024 = {2, 1024, {0, 0, 0, 0, 0, 0}},
                        reserved = {2, 1, {0, 0, 0, 0, 0, 1}};
      Selection sel;
      sel.overlap = &o;
      for (const fqgpu_merge *m : {&good, &widest, &lowest}) {
        sel.merge = m;
        sel.check("check", true);  // (throws when it refuses)
        sel.overlap_trim = !sel.overlap_trim;
        sel.correct = sel.correct ? nullptr : &correct;
      }
      for (const fqgpu_merge *m : {&floor64, &len0, &len1024, &reserved}) {
        sel.merge = m;
        if (!refuses([&] { sel.check("check", true); }, "check: a merge fqgpu_merge_check refuses")) { std::printf("a bad spec is taken\n"); return 1; }
      }
      Selection alone;
      alone.merge = &good;
      if (!refuses([&] { alone.check("check", true); }, "check: a merge without an overlap spec")) { std::printf("a merge without an overlap is taken\n"); return 1; }
      // positional cuts beside a merge; the quality trims are no positional cuts
      const fqgpu_trim none = {0, 0, 0, 0, FQGPU_FILTER_NONE, {0, 0, 0}}, quality = {0, 0, 20, 20, FQGPU_FILTER_NONE, {0, 0, 0}},
                       front = {1, 0, 0, 0, FQGPU_FILTER_NONE, {0, 0, 0}}, back = {0, 1, 0, 0, FQGPU_FILTER_NONE, {0, 0, 0}},
                       crop = {0, 0, 0, 0, 100, {0, 0, 0}};
      Selection cut;
      cut.overlap = &o;
      cut.merge = &good;
      for (const fqgpu_trim *t : {&none, &quality}) {
        cut.trim = t;
        cut.check("check", true);
      }
      for (const fqgpu_trim *t : {&front, &back, &crop}) {
        cut.trim = t;
        if (!refuses([&] { cut.check("check", true); }, "check: a merge beside cut_front, cut_tail or crop")) { std::printf("a positional cut beside a merge is taken\n"); return 1; }
        cut.merge = nullptr;
        cut.check("check", true);  // (without the merge the cut is what it was)
        cut.merge = &good;
      }
      Selection plain;  // (nothing new is asked of a selection without one)
      plain.overlap = &o;
      plain.correct = &correct;
      plain.trim = &crop;
      plain.check("check", true);
      std::printf("ok\n");
      return 0;
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "merge_report_check: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: merge_report_check text <words> <good_q> <bad_q> <cwords> <min_len> <floor_q> <mwords> [<row>:<count> ...] | sum <seed> | selection\n");
  return 2;
}
