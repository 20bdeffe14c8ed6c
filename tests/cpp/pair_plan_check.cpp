// The host arithmetic of a paired restore (fqcomp28_amd/csrc/process.hpp): the mates of a work unit as pieces of archive 2's
// blocks (planMateUnit), and the two bit helpers that carry keep bits between the calls (detail::sliceBits, detail::placeBits).
//   pair_plan_check plan <counts1> <counts2>   (comma-separated records per block) -> per unit "unit k a b" and, for each of its
//                                              pieces, "piece block first end at"
//   pair_plan_check bits <seed>                -> "ok": both helpers against a bit-by-bit restatement on drawn lengths and places
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace fqcomp28;

static std::vector<uint32_t> counts_of(const char *list) {
  std::vector<uint32_t> v;
  for (const char *p = list; *p;) {
    v.push_back(static_cast<uint32_t>(std::strtoul(p, nullptr, 10)));
    while (*p && *p != ',') ++p;
    if (*p) ++p;
  }
  return v;
}

int main(int argc, char **argv) {
  try {
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
      const std::vector<uint32_t> c1 = counts_of(argv[2]), c2 = counts_of(argv[3]);
      std::size_t a = 0;
      for (std::size_t k = 0; k < c1.size(); a += c1[k], ++k) {
        std::printf("unit %zu %zu %zu\n", k, a, a + c1[k]);
        for (const MatePiece &pc : planMateUnit(c2, a, a + c1[k])) std::printf("piece %zu %zu %zu %zu\n", pc.block, pc.first, pc.end, pc.at);
      }
      return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "bits")) {
      std::mt19937_64 rng(std::strtoull(argv[2], nullptr, 10));
      const auto bit = [](const std::vector<uint8_t> &v, std::size_t i) { return (v[i >> 3] >> (i & 7)) & 1u; };
      for (int round = 0; round < 2000; ++round) {
        const std::size_t n = 1 + rng() % 300, from = rng() % n, count = rng() % (n - from + 1);
        std::vector<uint8_t> src((n + 7) / 8), dst((count + 7) / 8 + 1, 0xA5);
        for (auto &b : src) b = static_cast<uint8_t>(rng());
        detail::sliceBits(src.data(), from, count, dst.data());
        for (std::size_t i = 0; i < 8 * ((count + 7) / 8); ++i)
          if (bit(dst, i) != (i < count ? bit(src, from + i) : 0u)) { std::printf("sliceBits: n %zu from %zu count %zu bit %zu\n", n, from, count, i); return 1; }
        if (dst.back() != 0xA5) { std::printf("sliceBits writes behind its bytes\n"); return 1; }
        // the slice put back at another place of a block of drawn bits
        std::vector<uint8_t> into((n + 7) / 8 + 1), before;
        for (auto &b : into) b = static_cast<uint8_t>(rng());
        before = into;
        const std::size_t at = rng() % (n - count + 1);
        detail::placeBits(dst.data(), count, into.data(), at);
        for (std::size_t i = 0; i < 8 * into.size(); ++i)
          if (bit(into, i) != (i >= at && i < at + count ? bit(src, from + i - at) : bit(before, i))) { std::printf("placeBits: n %zu at %zu count %zu bit %zu\n", n, at, count, i); return 1; }
      }
      std::printf("ok\n");
      return 0;
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "pair_plan_check: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: pair_plan_check plan <counts1> <counts2> | bits <seed>\n");
  return 2;
}
