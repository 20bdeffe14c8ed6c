// Command-line face of fqcomp28_amd/csrc/headers.hpp for the CPU tests (tests/test_headers.py,
// tests/test_headers_families_host.py):
//   headers_tool fmt '<header>'   ->  "types N S ...", "seps <code> ..."  (exit 3 + message if refused)
//   headers_tool code <fastq> [<first header>]
//                                 ->  per field "field <i> <N|S> <flags hex> <content hex> <lengths hex>"
//                                     (empty stream = "-"), then "roundtrip ok <n headers>"
//   headers_tool decode <file>    ->  the headers decoded from given streams, one a line, then "decoded ok <n headers>".
//                                     The file: the first header, the number of records, then per field three lines of
//                                     hex (flags, content, lengths; empty stream = "-")
// `code`: every header of the file is coded against the dataset's first header (without one: the file's first, a chunk
// start), then decoded back.  A header or a stream the coder throws on: "refused at <record>: <what>", exit 3.
#include "../../fqcomp28_amd/csrc/headers.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

using namespace fqcomp28::headers;

static void hex(const std::vector<std::byte> &v) {
  if (v.empty()) { std::printf(" -"); return; }
  std::printf(" ");
  for (std::byte b : v) std::printf("%02x", static_cast<unsigned>(b));
}

static std::vector<std::byte> unhex(const std::string &s) {
  std::vector<std::byte> v;
  if (s == "-") return v;
  auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
  for (std::size_t i = 0; i + 1 < s.size(); i += 2) v.push_back(static_cast<std::byte>(nib(s[i]) * 16 + nib(s[i + 1])));
  return v;
}

static int decode_given(const char *path) {
  std::ifstream ifs(path, std::ios::binary);
  std::string first, line;
  if (!std::getline(ifs, first) || !std::getline(ifs, line)) return 2;
  const std::size_t n = std::strtoull(line.c_str(), nullptr, 10);
  std::size_t r = 0;
  try {
    const auto fmt = HeaderFormatSpeciciation::fromHeader(first);
    header_fields_t prev = fromHeader(first, fmt);
    std::vector<FieldStorageSrc> src(fmt.n_fields());
    std::size_t room = 1;
    for (auto &f : src) {
      std::vector<std::byte> *parts[3] = {&f.isDifferentFlag, &f.content, &f.contentLength};
      for (auto *p : parts) {
        if (!std::getline(ifs, line)) return 2;
        *p = unhex(line);
      }
      room += FIELDLEN_MAX + 1;
    }
    // (string values of a decoded header are views into it: every header keeps its own bytes)
    std::vector<std::vector<char>> out(n, std::vector<char>(room));
    std::vector<unsigned> len(n);
    for (; r < n; ++r) len[r] = decodeHeader(out[r].data(), fmt, prev, src);
    for (r = 0; r < n; ++r) std::printf("%.*s\n", (int)len[r], out[r].data());
    std::printf("decoded ok %zu\n", n);
    return 0;
  } catch (const std::exception &e) {
    std::printf("refused at %zu: %s\n", r, e.what());
    return 3;
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "decode") return decode_given(argv[2]);
  std::size_t at = 0;  // the header being coded
  try {
    if (mode == "fmt") {
      const auto fmt = HeaderFormatSpeciciation::fromHeader(argv[2]);
      std::printf("types");
      for (FieldType t : fmt.field_types) std::printf(" %c", t == FieldType::NUMERIC ? 'N' : 'S');
      std::printf("\nseps");
      for (char c : fmt.separators) std::printf(" %d", static_cast<int>(static_cast<unsigned char>(c)));
      std::printf("\n");
      return 0;
    }
    if (mode != "code") return 2;
    std::ifstream ifs(argv[2], std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    std::vector<std::string_view> hdrs;  // every fourth line
    for (std::size_t pos = 0, line = 0; pos < text.size(); ++line) {
      std::size_t nl = text.find('\n', pos);
      if (nl == std::string::npos) nl = text.size();
      if (line % 4 == 0) hdrs.emplace_back(text.data() + pos, nl - pos);
      pos = nl + 1;
    }
    if (hdrs.empty()) return 2;
    const std::string_view first_header = argc > 3 ? std::string_view(argv[3]) : hdrs.front();
    const auto fmt = HeaderFormatSpeciciation::fromHeader(first_header);
    const header_fields_t first = fromHeader(first_header, fmt);
    std::vector<FieldStorageDst> dst(fmt.n_fields());
    header_fields_t prev = first;
    for (; at < hdrs.size(); ++at) encodeHeader(hdrs[at], fmt, prev, dst);
    for (std::size_t i = 0; i < dst.size(); ++i) {
      std::printf("field %zu %c", i, fmt.field_types[i] == FieldType::NUMERIC ? 'N' : 'S');
      hex(dst[i].isDifferentFlag); hex(dst[i].content); hex(dst[i].contentLength);
      std::printf("\n");
    }
    std::vector<FieldStorageSrc> src(fmt.n_fields());
    for (std::size_t i = 0; i < dst.size(); ++i) {
      src[i].isDifferentFlag = dst[i].isDifferentFlag;
      src[i].content = dst[i].content;
      src[i].contentLength = dst[i].contentLength;
    }
    prev = first;
    std::vector<char> out(text.size() + fmt.n_fields() * (FIELDLEN_MAX + 1) + 1);
    char *p = out.data();
    for (std::string_view h : hdrs) {
      const unsigned n = decodeHeader(p, fmt, prev, src);
      if (std::string_view(p, n) != h) { std::printf("mismatch: '%.*s' != '%.*s'\n", (int)n, p, (int)h.size(), h.data()); return 1; }
      p += n;
    }
    for (const auto &f : src)
      if (f.index.isDifferentPos != f.isDifferentFlag.size() || f.index.contentPos != f.content.size() ||
          f.index.contentLengthPos != f.contentLength.size()) { std::printf("streams not consumed\n"); return 1; }
    std::printf("roundtrip ok %zu\n", hdrs.size());
    return 0;
  } catch (const std::exception &e) {
    std::printf("refused at %zu: %s\n", at, e.what());
    return 3;
  }
}
