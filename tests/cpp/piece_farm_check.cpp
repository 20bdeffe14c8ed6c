// The ordered hand-out loop of the restores (fqcomp28_amd/csrc/process.hpp: detail::pieceFarm), for
// tests/test_piece_farm_host.py -- no GPU: the worker state holds no workspace.
//   piece_farm_check <out> <seed> ok|throw|nodevice
//        One OrderedPieceWriter, 40 items of pseudo-random sizes (some empty), n_threads = 4 over devices = {0}; byte i of
//        item k is (131 k + 7 i) mod 256 and the items complete in scrambled order.
//        ok:       every item ran once, blocks_per_worker has 4 entries that sum to 40; prints "sizes s0 s1 ..." and
//                  "written <bytes>" (the file is for the caller to compare).  Then n_threads = 8 over 3 items: 8 entries, at
//                  most 3 of them non-zero; then 0 items: the body never runs, nothing throws.
//        throw:    item 7 throws once the others wait behind it.  The exception that arrives must be item 7's; prints
//                  "failed: <what>" and "started <highest item that was started>" (at most 7 + 3: the caller checks).
//        nodevice: devices = {} -- std::invalid_argument naming the farm, before the state factory ran; prints "refused: <what>".
//        Exit 0: everything the program checks itself held; 1: something did not (said on stderr).
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <chrono>
#include <cstdio>
#include <string>
#include <thread>

using namespace fqcomp28;

namespace {
constexpr std::size_t N_ITEMS = 40, THROWS = 7;

std::vector<std::size_t> itemSizes(uint64_t seed, std::size_t n) {
  std::vector<std::size_t> sizes(n);
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
  for (auto &s : sizes) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    s = (x >> 33) % 5 == 0 ? 0 : static_cast<std::size_t>((x >> 40) % 200000);
  }
  return sizes;
}

struct Worker {  // no workspace: what the farm hands to the body, and what the body leaves for the merge
  unsigned t;
  int device;
  std::vector<char> bytes;
  std::size_t items = 0;
};

struct Run {  // (filled as far as the farm got when it throws)
  FarmReport rep;
  std::vector<std::atomic<int>> ran;  // how often every item's body was started
  std::atomic<std::size_t> made{0};   // worker states built
};

bool fail(const std::string &what) {
  std::fprintf(stderr, "piece_farm_check: %s\n", what.c_str());
  return false;
}

/** n items through a farm of n_threads into `out`; item `throws` (none: SIZE_MAX) throws instead of delivering */
void farmRun(Run &r, const path_t &out, const std::vector<std::size_t> &sizes, unsigned n_threads, std::vector<int> devices, std::size_t throws) {
  Settings set;
  set.n_threads = n_threads;
  set.devices = std::move(devices);
  const std::size_t n = sizes.size();
  r.ran = std::vector<std::atomic<int>>(n);
  for (auto &c : r.ran) c.store(0);
  r.made.store(0);
  auto farm = detail::pieceFarm("pieceFarmCheck", n, set, [&](unsigned t, int device) {
    r.made.fetch_add(1);
    return Worker{t, device, {}};
  });
  OrderedPieceWriter writer(out, n);
  farm.run([&](Worker &w, std::size_t k, StageClock &clk, InputStats &in) {
    r.ran[k].fetch_add(1);
    w.bytes.resize(sizes[k]);
    for (std::size_t i = 0; i < sizes[k]; ++i) w.bytes[i] = static_cast<char>((131 * k + 7 * i) & 0xFF);
    // scrambled completion: a later item is often ready before an earlier one
    std::this_thread::sleep_for(std::chrono::microseconds(((k * 2654435761u) >> 7) % 3000));
    clk.lap("make");
    if (k == throws) {
      std::this_thread::sleep_for(std::chrono::milliseconds(50));  // (the others are waiting by now)
      throw std::runtime_error("item " + std::to_string(k) + " could not be decoded");
    }
    in.raw += sizes[k];
    in.n_records++;
    w.items++;
    writer.writePiece(k, w.bytes.data(), w.bytes.size());
    clk.lap("write");
    return true;
  }, [&] { writer.abort(); });
  writer.flush();
  r.rep = farm.report();
  std::size_t items = 0;
  for (const auto &w : farm.workers()) {
    if (w->device != 0 || w->items != r.rep.blocks_per_worker[w->t]) throw std::logic_error("a worker's state is not the one its factory made");
    items += w->items;
  }
  if (items != n) throw std::logic_error("the workers' states count " + std::to_string(items) + " items");
}

bool noFile(const path_t &out) {
  return !std::filesystem::exists(out) && !std::filesystem::exists(path_t(out.string() + ".part"));
}

bool ok(const path_t &out, uint64_t seed) {
  const std::vector<std::size_t> sizes = itemSizes(seed, N_ITEMS);
  Run r;
  farmRun(r, out, sizes, 4, {0}, SIZE_MAX);
  std::size_t total = 0, blocks = 0;
  for (const std::size_t s : sizes) total += s;
  for (const auto &c : r.ran)
    if (c.load() != 1) return fail("an item ran " + std::to_string(c.load()) + " times");
  for (const unsigned b : r.rep.blocks_per_worker) blocks += b;
  if (r.made != 4 || r.rep.blocks_per_worker.size() != 4 || blocks != N_ITEMS) return fail("40 items over 4 workers: blocks_per_worker is not 4 entries that sum to 40");
  if (r.rep.in.raw != total || r.rep.in.n_records != N_ITEMS || r.rep.seconds <= 0) return fail("the report does not add up the workers' input stats");
  if (std::filesystem::exists(path_t(out.string() + ".part"))) return fail("a .part file is left");
  std::printf("sizes");
  for (const std::size_t s : sizes) std::printf(" %zu", s);
  std::printf("\nwritten %llu\n", static_cast<unsigned long long>(std::filesystem::file_size(out)));

  // more workers asked for than items: T = 3, the report still has n_threads entries
  const path_t few = out.string() + ".few", none = out.string() + ".none";
  Run f;
  farmRun(f, few, itemSizes(seed + 1, 3), 8, {0}, SIZE_MAX);
  std::size_t nonzero = 0, sum = 0;
  for (const unsigned b : f.rep.blocks_per_worker) { nonzero += b != 0; sum += b; }
  if (f.made != 3 || f.rep.blocks_per_worker.size() != 8 || nonzero > 3 || sum != 3) return fail("3 items, n_threads 8: not 8 entries with at most 3 non-zero");
  for (const auto &c : f.ran)
    if (c.load() != 1) return fail("3 items, n_threads 8: an item did not run once");
  // no items: one worker, whose body never runs; an empty file
  Run z;
  farmRun(z, none, {}, 4, {0}, SIZE_MAX);
  if (z.made != 1 || z.rep.blocks_per_worker != std::vector<unsigned>(4, 0) || z.rep.in.raw != 0) return fail("0 items: the body ran, or the report is not empty");
  if (!std::filesystem::exists(none) || std::filesystem::file_size(none) != 0) return fail("0 items: no empty file");
  std::filesystem::remove(few);
  std::filesystem::remove(none);
  return true;
}

bool throws(const path_t &out, uint64_t seed) {
  Run r;
  try {
    farmRun(r, out, itemSizes(seed, N_ITEMS), 4, {0}, THROWS);
    return fail("item 7 threw and the farm returned");
  } catch (const OrderedPieceWriter::Aborted &e) {
    return fail(std::string("a released waiter's exception reached the caller: ") + e.what());
  } catch (const std::runtime_error &e) {
    std::printf("failed: %s\n", e.what());
    if (std::string(e.what()) != "item 7 could not be decoded") return fail("not item 7's exception");
  }
  if (!noFile(out)) return fail("the failed run left a file");
  // handed out in order, and each of the other three workers waits in the writer with at most one item behind the one that
  // never came: nothing above 7 + 3 can have been started
  std::size_t highest = 0;
  for (std::size_t k = 0; k < N_ITEMS; ++k)
    if (r.ran[k].load()) highest = k;
  std::printf("started %zu\n", highest);
  if (r.ran[THROWS].load() != 1 || highest > THROWS + 3) return fail("an item above 10 was started");
  return true;
}

bool nodevice(const path_t &out) {
  Run r;
  try {
    farmRun(r, out, itemSizes(1, N_ITEMS), 4, {}, SIZE_MAX);
    return fail("no device and the farm ran");
  } catch (const std::invalid_argument &e) {
    std::printf("refused: %s\n", e.what());
    if (std::string(e.what()) != "pieceFarmCheck: no device") return fail("not the farm's refusal");
  }
  if (r.made.load() != 0) return fail("a farm without a device built a worker's state");
  if (!noFile(out)) return fail("a farm without a device created a file");
  return true;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: piece_farm_check <out> <seed> ok|throw|nodevice\n");
    return 2;
  }
  const std::string mode = argv[3];
  const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
  try {
    if (mode == "ok") return ok(argv[1], seed) ? 0 : 1;
    if (mode == "throw") return throws(argv[1], seed) ? 0 : 1;
    if (mode == "nodevice") return nodevice(argv[1]) ? 0 : 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "piece_farm_check: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "piece_farm_check: unknown mode %s\n", mode.c_str());
  return 2;
}
