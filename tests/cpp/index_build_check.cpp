// Host check of the decode index file a decode builds (process.hpp: detail::DecodeIndexBuilder over archive.hpp's
// DecodeIndexFile): written to `<archive>.fqx.part`, closed for the archive and renamed, it reads back (belongsTo, get);
// a build that is given up leaves no file and the old one untouched; a finished one replaces the old one.  No GPU.
//   index_build_check <directory>
#include "../../fqcomp28_amd/csrc/process.hpp"

#include <cstdio>
#include <fstream>

using namespace fqcomp28;

namespace {
int failures = 0;
void expect(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}

std::vector<std::byte> pattern(std::size_t n, unsigned seed) {
  std::vector<std::byte> v(n);
  for (std::size_t i = 0; i < n; ++i) v[i] = static_cast<std::byte>((i * 131u + seed * 17u + (i >> 8)) & 0xFFu);
  return v;
}

CompressedBuffersSrc chunk(unsigned idx, std::size_t ns, std::size_t nq) {
  CompressedBuffersSrc cbs;
  cbs.chunk_idx = idx;
  cbs.decode_index[0] = pattern(ns, idx);
  cbs.decode_index[1] = pattern(nq, idx + 100);
  return cbs;
}

std::string slurp(const path_t &p) {
  std::ifstream f(p, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: index_build_check <directory>\n"); return 2; }
  const path_t dir(argv[1]), arc = dir / "a.fqc", side = DecodeIndexFile::pathFor(arc), part = path_t(side.string() + ".part");
  { std::ofstream f(arc, std::ios::binary); const auto body = pattern(100000, 7); f.write(reinterpret_cast<const char *>(body.data()), body.size()); }
  const std::size_t sizes[4][2] = {{32, 32}, {32 + 3 * 528, 32 + 3 * 16400}, {32 + 528, 32 + 16400}, {32 + 7 * 528, 32 + 7 * 16400}};
  try {
    // 1. a build that is given up: no file, and none under the final name
    {
      detail::DecodeIndexBuilder b(arc);
      b.put(chunk(2, sizes[2][0], sizes[2][1]));
      expect(std::filesystem::exists(part), "the build works in <archive>.fqx.part");
    }
    expect(!std::filesystem::exists(part) && !std::filesystem::exists(side), "a build given up leaves no file");
    // 2. a finished build, chunks in any order: reads back
    FarmReport rep;
    {
      detail::DecodeIndexBuilder b(arc);
      for (unsigned idx : {3u, 0u, 2u, 1u}) b.put(chunk(idx, sizes[idx][0], sizes[idx][1]));
      b.finish(rep);
    }
    expect(std::filesystem::exists(side) && !std::filesystem::exists(part), "finish renames the part file");
    expect(rep.index_built && rep.indexed_blocks == 4, "the report counts the blocks");
    std::size_t total = 0;
    for (const auto &s : sizes) total += s[0] + s[1];
    expect(rep.index_bytes == total, "the report counts the bytes");
    {
      const DecodeIndexFile f(side, PosFile::Mode::Read);
      expect(f.belongsTo(DecodeIndexFile::identityOf(arc)), "the file belongs to its archive");
      for (unsigned idx = 0; idx < 4; ++idx) {
        CompressedBuffersSrc got;
        got.chunk_idx = idx;
        const CompressedBuffersSrc want = chunk(idx, sizes[idx][0], sizes[idx][1]);
        expect(f.get(got), "get finds the chunk");
        expect(got.decode_index[0] == want.decode_index[0] && got.decode_index[1] == want.decode_index[1], "get returns what was put");
      }
      CompressedBuffersSrc none;
      none.chunk_idx = 4;
      expect(!f.get(none), "a chunk the file does not hold");
    }
    // 3. a later build that fails leaves the finished file as it was; a block without indexes is refused
    const std::string before = slurp(side);
    {
      detail::DecodeIndexBuilder b(arc);
      b.put(chunk(0, 64, 64));
      bool refused = false;
      try { b.put(chunk(1, 0, 0)); } catch (const std::runtime_error &) { refused = true; }
      expect(refused, "a block without decode indexes is refused");
    }
    expect(slurp(side) == before && !std::filesystem::exists(part), "a failed build leaves the old file untouched");
    // 4. a later build that finishes replaces it -- also a file that is no decode index file at all
    { std::ofstream f(side, std::ios::binary | std::ios::trunc); f << "FQX"; }
    {
      detail::DecodeIndexBuilder b(arc);
      b.put(chunk(0, 96, 160));
      b.finish(rep);
    }
    {
      const DecodeIndexFile f(side, PosFile::Mode::Read);
      CompressedBuffersSrc got;
      got.chunk_idx = 0;
      expect(f.belongsTo(DecodeIndexFile::identityOf(arc)) && f.get(got) && got.decode_index[1].size() == 160, "the new file replaces the old one");
      got.chunk_idx = 1;
      expect(!f.get(got), "... entirely");
    }
    // 5. the archive changes: the file is no longer its own
    { std::ofstream f(arc, std::ios::binary | std::ios::app); f << "x"; }
    expect(!DecodeIndexFile(side, PosFile::Mode::Read).belongsTo(DecodeIndexFile::identityOf(arc)), "another archive: not its file");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "index_build_check: %s\n", e.what());
    return 1;
  }
  if (!failures) std::printf("index_build_check ok\n");
  return failures ? 1 : 0;
}
