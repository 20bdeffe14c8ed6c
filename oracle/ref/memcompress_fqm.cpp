// oracle/ref/memcompress_fqm.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The two functions the reference declares in src/memcompress.h, over the project's own misc
// coder (fqcomp28_amd/csrc/fq_misc.cpp) in place of libbsc, exactly as the product's
// workspace.hpp binds them.  With them the reference's Workspace and Archive write and read the
// misc blocks fqc_tool does, so archives can cross between the two programs.
#include <cstddef>
#include <cstdint>
#include <stdexcept>

#include "fqgpu.h"
#include "memcompress.h"

namespace fqcomp28 {

std::size_t memcompress(std::byte *dst, const std::byte *src, std::size_t src_size) {
  // the reference sizes dst as src_size + 28 (extra_csize_misc, src/workspace.h), the coder's bound
  return fqgpu_memcompress(reinterpret_cast<uint8_t *>(dst), fqgpu_memcompress_bound(src_size),
                           reinterpret_cast<const uint8_t *>(src), src_size);
}

std::size_t memdecompress(std::byte *dst, std::size_t dst_size, const std::byte *src, std::size_t src_size) {
  const std::size_t n = fqgpu_memdecompress(reinterpret_cast<uint8_t *>(dst), dst_size,
                                            reinterpret_cast<const uint8_t *>(src), src_size);
  if (n == static_cast<std::size_t>(-1) || (src_size && n != dst_size))
    throw std::runtime_error("memdecompress: malformed misc stream");
  return n;
}

} // namespace fqcomp28
