// C ABI of libfqgpu.so (include/fqgpu.h): handle and buffer management around the
// kernels of tables.hip / encode.hip / decode.hip.  Host code only.
#include "fqgpu_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

// The encode lanes use up to 16 streams (two per block in flight: sequence and quality pipelines).  ROCm maps streams onto
// GPU_MAX_HW_QUEUES hardware queues (default 4) and kernels of streams that share a queue
// run back to back; ask for 16 before the runtime initialises (one per stream of 8 lanes;
// 24 helps blocks of 16 MiB and less by a fifth and costs 256 MiB blocks 2 %; 32 collapses processes
// with many handles).  This touches the host process's environment, so it is narrow and can be
// switched off.  A count below 16 is RAISED to 16: launchers and job schedulers write HIP's default
// of 4 into the environment of every command, which is no choice anyone made about this library, and
// the default lanes then ran their nine streams on four queues (DESIGN.md sections 6 and 8).  A count
// of 16 or more, and a value that is no number, stay as they are: the library never lowers a count
// and never writes one above 16.  It has no effect once HIP is initialised, and FQGPU_KEEP_HW_QUEUES=1
// in the environment makes the library leave the variable alone ("Environment").
__attribute__((constructor)) static void fq_ask_for_hw_queues() {
  if (getenv("FQGPU_KEEP_HW_QUEUES")) return;
  if (const char *have = getenv("GPU_MAX_HW_QUEUES")) {
    char *end = nullptr;
    const long n = strtol(have, &end, 10);
    if (end == have || *end != 0 || n < 1 || n >= 16) return;  // no number, none the rule names, or enough already
  }
  setenv("GPU_MAX_HW_QUEUES", "16", 1);
}

// ------------------------------------------------------------------ errors
static thread_local char g_hip_msg[256] = "";

int fq_hip_error(hipError_t e, const char *file, int line) {
  snprintf(g_hip_msg, sizeof(g_hip_msg), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
  if (getenv("FQGPU_VERBOSE")) fprintf(stderr, "fqgpu: %s\n", g_hip_msg);
  return (e == hipErrorOutOfMemory) ? FQGPU_E_NOMEM
         : (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? FQGPU_E_NO_DEVICE
                                                                 : FQGPU_E_HIP;
}

extern "C" const char *fqgpu_strerror(int code) {
  switch (code) {
  case FQGPU_OK: return "ok";
  case FQGPU_E_OVERFLOW: return "compressed stream exceeds the reference capacity bound";
  case FQGPU_E_SHORT_READ: return "read shorter than 3 bases (undefined in the reference coder)";
  case FQGPU_E_CORRUPT: return "corrupt stream (end mark / leftover bits / N table)";
  case FQGPU_E_ARG: return "bad argument or symbol outside the model alphabet";
  case FQGPU_E_NO_DEVICE: return "no usable MI355X / HIP device (there is no CPU fallback)";
  case FQGPU_E_NOMEM: return "out of device or host memory";
  case FQGPU_E_HIP: return g_hip_msg[0] ? g_hip_msg : "HIP runtime error";
  case FQGPU_E_HEADER: return "read header the field coder cannot code (numeric field not an int32 / string field of 255 or more bytes)";
  default: return "unknown fqgpu error";
  }
}

extern "C" const char *fqgpu_version(void) { return "fqgpu 0.1 (gfx950)"; }

extern "C" int fqgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Workspace::compressBoundSequence / compressBoundQuality (reference src/workspace.h:21-35)
extern "C" size_t fqgpu_bound_seq(size_t n) {
  if (n < 1024) return (size_t)1024 * FQGPU_SEQ_MODELS;
  return n / 4 + 1024;
}
extern "C" size_t fqgpu_bound_qual(size_t n) {
  const size_t a = (size_t)1024 * FQGPU_QUAL_MODELS, b = n * 7 / 8 + 1024;
  return a > b ? a : b;
}

static int use_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FQGPU_E_NO_DEVICE;
  if (device < 0 || device >= n) return FQGPU_E_NO_DEVICE;
  FQ_HIP(hipSetDevice(device));
  return FQGPU_OK;
}

// ------------------------------------------------------------------ pinned host memory
// A 64-byte header in front of the block says how it was allocated (pinned, or plain heap when
// there is no usable device: host-only tools and tests) and how large it is.
//
// hipHostFree waits until the DEVICE is idle (measured: 1.25 s behind a 1.6 s decode kernel of
// another thread, 6 ms on an idle device): a worker that lets a buffer grow stalls behind every
// other worker's kernels, and four decoding workers of the block farm ran two at a time because of
// it.  So freed pinned blocks go back to a cache by size class (sizes are rounded up to 1/8 of their
// power of two: at most 12.5 % more) and are handed out again; only what exceeds the cache limit
// (FQGPU_PINNED_CACHE_MB, default 8192) is really freed.  Blocks below 64 KiB are not pinned at all:
// they never carry a stream, and a farm makes thousands of them.
namespace {
struct HostHdr { uint64_t magic, pinned, size, pad[5]; };  // size: bytes of the whole block, header included
constexpr uint64_t HOST_MAGIC = 0x46514850494E4E44ull;
constexpr size_t PIN_MIN = 64 << 10;
struct PinCache {
  std::mutex mutex;
  std::multimap<size_t, void *> blocks;  // block size -> free pinned block
  size_t bytes = 0;
};
// (never destroyed: fqgpu_host_free is called from the destructors of the callers' own statics at exit)
PinCache &pin_cache() {
  static PinCache *c = new PinCache;
  return *c;
}
size_t pin_class(size_t bytes) {  // rounded up to a multiple of 1/8 of the largest power of two below it
  size_t step = 1;
  while ((step << 4) <= bytes) step <<= 1;
  return (bytes + step - 1) & ~(step - 1);
}
size_t pin_cache_limit() {
  static const size_t limit = [] {
    const char *e = getenv("FQGPU_PINNED_CACHE_MB");
    return (size_t)(e ? strtoull(e, nullptr, 10) : 8192ull) << 20;
  }();
  return limit;
}
}  // namespace
extern "C" void *fqgpu_host_alloc(size_t bytes) {
  void *p = nullptr;
  size_t total = bytes + sizeof(HostHdr);
  bool pinned = false;
  if (total >= PIN_MIN) {
    total = pin_class(total);
    {
      PinCache &pc = pin_cache();
      std::lock_guard<std::mutex> lock(pc.mutex);
      auto it = pc.blocks.find(total);
      if (it != pc.blocks.end()) { p = it->second; pc.blocks.erase(it); pc.bytes -= total; pinned = true; }
    }
    if (!p) {
      int n = 0;
      const bool gpu = hipGetDeviceCount(&n) == hipSuccess && n > 0;
      // Portable: the cache is process-wide, a block pinned while one device was current may be handed to a worker of another
      pinned = gpu && hipHostMalloc(&p, total, hipHostMallocPortable) == hipSuccess;
      if (!pinned) { (void)hipGetLastError(); p = nullptr; }
    }
  }
  if (!p) {
    total = (total + 63) & ~(size_t)63;
    p = aligned_alloc(64, total);
    if (!p) return nullptr;
  }
  HostHdr *h = static_cast<HostHdr *>(p);
  h->magic = HOST_MAGIC;
  h->pinned = pinned ? 1 : 0;
  h->size = total;
  return h + 1;
}
extern "C" void fqgpu_host_free(void *p) {
  if (!p) return;
  HostHdr *h = static_cast<HostHdr *>(p) - 1;
  if (h->magic != HOST_MAGIC) return;  // not ours
  h->magic = 0;
  if (!h->pinned) { free(h); return; }
  const size_t total = h->size;
  {
    PinCache &pc = pin_cache();
    std::lock_guard<std::mutex> lock(pc.mutex);
    if (pc.bytes + total <= pin_cache_limit()) {
      pc.blocks.emplace(total, h);
      pc.bytes += total;
      return;
    }
  }
  (void)hipHostFree(h);  // (waits for the device)
}
// gives the cached pinned blocks back to the system (waits for the device); returns the bytes freed
extern "C" size_t fqgpu_host_trim(void) {
  std::multimap<size_t, void *> drop;
  size_t bytes;
  {
    PinCache &pc = pin_cache();
    std::lock_guard<std::mutex> lock(pc.mutex);
    drop.swap(pc.blocks);
    bytes = pc.bytes;
    pc.bytes = 0;
  }
  for (auto &kv : drop) (void)hipHostFree(kv.second);
  return bytes;
}

// ------------------------------------------------------------------ kernel timing
// Spans = pairs of HIP events recorded on the stream the kernels run on.  Spans accumulate
// from fqgpu_ctx_enable_timing(ctx, 1) until they are read; fqgpu_ctx_last_timing sums them
// per label (total device time and number of launches of every kernel group).
struct KernelTimer {
  bool on = false;
  std::string only;  // if not empty: only spans of this label get events (fqgpu_ctx_timing_only)
  static constexpr size_t SKIPPED = (size_t)-2;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  struct Span { const char *name; size_t b, e; };
  std::vector<Span> spans;
  hipEvent_t get(size_t *idx) {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    *idx = used;
    return pool[used++];
  }
};

void fq_timer_span_begin(fqgpu_ctx *ctx, const char *name, hipStream_t st) {
  KernelTimer *t = ctx->timer;
  if (!t || !t->on) return;
  if (!t->only.empty() && t->only != name) {  // an open span without events, closed by its span_end
    t->spans.push_back({name, KernelTimer::SKIPPED, (size_t)-1});
    return;
  }
  size_t i;
  hipEvent_t e = t->get(&i);
  if (!e) return;
  (void)hipEventRecord(e, st);
  t->spans.push_back({name, i, (size_t)-1});
}
void fq_timer_span_end(fqgpu_ctx *ctx, hipStream_t st) {
  KernelTimer *t = ctx->timer;
  if (!t || !t->on || t->spans.empty()) return;
  // the matching begin is the last open span (launch code nests nothing across streams)
  for (size_t k = t->spans.size(); k-- > 0;) {
    if (t->spans[k].e == (size_t)-1) {
      if (t->spans[k].b == KernelTimer::SKIPPED) { t->spans.erase(t->spans.begin() + (long)k); return; }
      size_t i;
      hipEvent_t e = t->get(&i);
      if (!e) return;
      (void)hipEventRecord(e, st);
      t->spans[k].e = i;
      return;
    }
  }
}

extern "C" int fqgpu_ctx_enable_timing(fqgpu_ctx *ctx, int on) {
  if (!ctx) return FQGPU_E_ARG;
  if (!ctx->timer) ctx->timer = new (std::nothrow) KernelTimer();
  if (!ctx->timer) return FQGPU_E_NOMEM;
  ctx->timer->on = on != 0;
  if (on) { ctx->timer->used = 0; ctx->timer->spans.clear(); }
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_timing_only(fqgpu_ctx *ctx, const char *name) {
  if (!ctx) return FQGPU_E_ARG;
  if (!ctx->timer) ctx->timer = new (std::nothrow) KernelTimer();
  if (!ctx->timer) return FQGPU_E_NOMEM;
  ctx->timer->only = name ? name : "";
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_last_timing(fqgpu_ctx *ctx, fqgpu_timing *out) {
  if (!ctx || !out || !ctx->timer) return FQGPU_E_ARG;
  KernelTimer *t = ctx->timer;
  memset(out, 0, sizeof(*out));
  int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  float first_to_last = 0;
  for (const KernelTimer::Span &sp : t->spans) {
    if (sp.e == (size_t)-1) continue;
    float ms = 0, span_end = 0;
    FQ_HIP(hipEventElapsedTime(&ms, t->pool[sp.b], t->pool[sp.e]));
    FQ_HIP(hipEventElapsedTime(&span_end, t->pool[t->spans[0].b], t->pool[sp.e]));
    if (span_end > first_to_last) first_to_last = span_end;
    int k = 0;
    for (; k < out->n_kernels; k++) if (strcmp(out->kernel_name[k], sp.name) == 0) break;
    if (k == out->n_kernels) {
      if (k == 32) continue;
      out->kernel_name[k] = sp.name;
      out->n_kernels++;
    }
    out->kernel_ms[k] += ms;
    out->kernel_calls[k] += 1;
  }
  out->total_ms = first_to_last;
  return FQGPU_OK;
}

// ------------------------------------------------------------------ encode lanes
// Blocks take the lanes in turn -- unless the handle keeps coding the SAME few blocks (no more of them than lanes): then
// a block goes back to the lane of its last encode.  Its encodes are ordered anyway (same streams, same result words: ev_encoded),
// and on its own lane that order costs nothing, where the rotation sends the next encode to another lane that must also finish
// ANOTHER block's encode first: the chains of unrelated blocks get coupled and every step ends in a partial barrier -- four blocks
// coded over and over on six lanes ran at 56-58 GB/s against 69 on their own four.  With more blocks than lanes the rotation
// stays: a fixed assignment (sixteen blocks: 3 3 3 3 2 2) leaves two lanes idle at the end of a batch.
// `b` is only compared with the blocks coded last, never followed (it may be gone); nullptr: reserving, lanes in turn.
EncLane *fq_next_lane(fqgpu_ctx *ctx, size_t n_bases, fqgpu_dblock *b) {
  const unsigned n = fq_lanes_for(ctx, n_bases);
  unsigned pick = n;
  if (b) {
    unsigned distinct = 0;
    bool seen = false;
    for (unsigned i = 0; i < FQ_RECENT_BLOCKS; i++) {
      const void *p = ctx->recent[i];
      if (!p) continue;
      bool first = true;
      for (unsigned j = 0; j < i; j++) first = first && ctx->recent[j] != p;
      distinct += first;
      seen = seen || p == b;
    }
    ctx->recent[ctx->recent_at++ % FQ_RECENT_BLOCKS] = b;
    if (seen && distinct <= n && b->home_lane >= 0 && (unsigned)b->home_lane < n) pick = (unsigned)b->home_lane;
  }
  if (pick == n) {
    pick = ctx->next_lane % n;
    ctx->next_lane++;
  }
  if (b) b->home_lane = (int)pick;
  EncLane &l = ctx->lanes[pick];
  if (!l.st_seq) {
    // Both pipelines at the same priority: while the sequence chains were serial their stream
    // ran at high priority; with every kernel a throughput kernel that costs 2 % (measured).
    if (hipStreamCreateWithFlags(&l.st_seq, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&l.st_qual, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&l.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming) != hipSuccess)
      return nullptr;
  }
  return &l;
}

// ------------------------------------------------------------------ the handle's scratch, one enumeration
// Every device scratch buffer a handle owns, as f(owner, name, pointer, bytes allocated): the DevBuf lists of the scratch
// structs (fqgpu_internal.h: FQ_SCRATCH_BUFS) and the staging block's arrays (FQ_DBLOCK_BUFS).  fqgpu_ctx_destroy frees what
// these visit and fqgpu_ctx_fill_scratch fills it: one walk for both.
template <class F> static void ctx_each_devbuf(fqgpu_ctx *ctx, F &&f) {  // f(owner, name, DevBuf &)
  for (int i = 0; i < FQ_MAX_LANES; i++) {
    EncLane &l = ctx->lanes[i];
    fq_each_buf(l, [&](const char *n, DevBuf &b) { f("lane", n, b); });
    for (int s = 0; s < 2; s++) fq_each_buf(l.enc[s], [&](const char *n, DevBuf &b) { f("lane.enc", n, b); });
  }
  fq_each_buf(*ctx, [&](const char *n, DevBuf &b) { f("ctx", n, b); });
  fq_each_buf(ctx->hp_parse, [&](const char *n, DevBuf &b) { f("hp_parse", n, b); });
  fq_each_buf(ctx->hp_hdr, [&](const char *n, DevBuf &b) { f("hp_hdr", n, b); });
  fq_each_buf(ctx->hp_chunk, [&](const char *n, DevBuf &b) { f("hp_chunk", n, b); });
  fq_each_buf(ctx->crc, [&](const char *n, DevBuf &b) { f("crc", n, b); });
  fq_each_buf(ctx->stats, [&](const char *n, DevBuf &b) { f("stats", n, b); });
  fq_each_buf(ctx->select, [&](const char *n, DevBuf &b) { f("select", n, b); });
}

// The scratch buffers whose content is state ON PURPOSE: fqgpu_ctx_fill_scratch leaves them alone.  Every other scratch word
// is written before it is read within one call ("Scratch that carries state").
static const struct { const char *owner, *name, *why; } kScratchState[] = {
    {"lane", "rscan", "k_record_scan's tickets and epoch-stamped status words count on from launch to launch (zeroed when allocated and every 2^24 launches)"},
    {"crc", "tab", "the CRC multiplier tables are built once per handle (CrcScratch::tab_built)"},
};
static bool scratch_is_state(const char *owner, const char *name) {
  for (const auto &e : kScratchState)
    if (!strcmp(e.owner, owner) && !strcmp(e.name, name)) return true;
  return false;
}

static void free_lane(EncLane &l) {  // (its DevBufs: ctx_each_devbuf)
  hipEvent_t evs[] = {l.ev_fork, l.ev_join};
  for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
  hipStream_t sts[] = {l.st_seq, l.st_qual};
  for (hipStream_t q : sts) if (q) (void)hipStreamDestroy(q);
  l = EncLane();
}

// ------------------------------------------------------------------ record validation (host)
static int check_recs(const fqgpu_rec *recs, size_t n_recs, size_t raw_len, size_t *n_bases) {
  size_t tot = 0;
  for (size_t i = 0; i < n_recs; i++) {
    const fqgpu_rec &r = recs[i];
    if (r.len > 65535u) return FQGPU_E_ARG;  // readlen_t is u16 (src/defs.h:14)
    if ((size_t)r.seq_off + r.len > raw_len || (size_t)r.qual_off + r.len > raw_len) return FQGPU_E_ARG;
    if (r.len < 3) return FQGPU_E_SHORT_READ;
    tot += r.len;
  }
  if (tot >= 0xFFF00000ull) return FQGPU_E_ARG;  // block sizes are u32 in the reference too
  *n_bases = tot;
  return FQGPU_OK;
}

// ------------------------------------------------------------------ frequency tables
struct FtLayout {
  int n_models, alpha;
  size_t norm_bytes, logs_off, maxlog_off, total;
};
static FtLayout ft_layout(int stream) {
  FtLayout l;
  l.n_models = stream ? FQGPU_QUAL_MODELS : FQGPU_SEQ_MODELS;
  l.alpha = stream ? FQGPU_QUAL_ALPHA : FQGPU_SEQ_ALPHA;
  l.norm_bytes = (size_t)l.n_models * l.alpha * 2;
  l.logs_off = l.norm_bytes;
  l.maxlog_off = l.logs_off + (size_t)l.n_models * 4;
  l.total = l.maxlog_off + 4;
  return l;
}

// counts (device) -> FreqTable POD (host)
static int normalize_to_host(hipStream_t st, const uint32_t *counts_dev, int stream, void *ft_out) {
  const FtLayout l = ft_layout(stream);
  uint8_t *dev = fq_dev_alloc<uint8_t>(l.total + 8);
  if (!dev) return FQGPU_E_NOMEM;
  int rc = FQGPU_OK;
  uint32_t err = 0;
  do {
    if (hipMemsetAsync(dev, 0, l.total + 8, st) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    uint32_t *err_dev = reinterpret_cast<uint32_t *>(dev + ((l.total + 3) & ~(size_t)3));
    rc = fq_normalize_counts(st, counts_dev, l.n_models, l.alpha, reinterpret_cast<int16_t *>(dev),
                             reinterpret_cast<uint32_t *>(dev + l.logs_off),
                             reinterpret_cast<uint32_t *>(dev + l.maxlog_off), err_dev);
    if (rc) break;
    if (hipMemcpyAsync(ft_out, dev, l.total, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&err, err_dev, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    if (err) rc = FQGPU_E_ARG;
  } while (0);
  (void)hipFree(dev);
  return rc;
}

extern "C" int fqgpu_tables_from_counts(int device, const uint32_t *seq_counts, const uint32_t *qual_counts,
                                        void *seq_ft_out, void *qual_ft_out) {
  int rc = use_device(device);
  if (rc) return rc;
  if (!seq_counts || !qual_counts || !seq_ft_out || !qual_ft_out) return FQGPU_E_ARG;
  const size_t ns = (size_t)FQGPU_SEQ_MODELS * FQGPU_SEQ_ALPHA, nq = (size_t)FQGPU_QUAL_MODELS * FQGPU_QUAL_ALPHA;
  uint32_t *dev = fq_dev_alloc<uint32_t>(ns + nq);
  if (!dev) return FQGPU_E_NOMEM;
  hipStream_t st = nullptr;
  if (hipMemcpy(dev, seq_counts, ns * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dev + ns, qual_counts, nq * 4, hipMemcpyHostToDevice) != hipSuccess) rc = FQGPU_E_HIP;
  if (!rc) rc = normalize_to_host(st, dev, 0, seq_ft_out);
  if (!rc) rc = normalize_to_host(st, dev + ns, 1, qual_ft_out);
  (void)hipFree(dev);
  return rc;
}

extern "C" int fqgpu_freq_tables(int device, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs,
                                 size_t n_recs, void *seq_ft_out, void *qual_ft_out,
                                 uint32_t *seq_counts_out, uint32_t *qual_counts_out) {
  int rc = use_device(device);
  if (rc) return rc;
  if (!raw || !recs || !seq_ft_out || !qual_ft_out) return FQGPU_E_ARG;
  // the histogram pass itself accepts reads of any length (src/fse_sequence.cpp:145-169)
  size_t n_bases = 0;
  unsigned min_len = 0xFFFFFFFFu;
  for (size_t i = 0; i < n_recs; i++) {
    if ((size_t)recs[i].seq_off + recs[i].len > raw_len || (size_t)recs[i].qual_off + recs[i].len > raw_len)
      return FQGPU_E_ARG;
    n_bases += recs[i].len;
    if (recs[i].len < min_len || recs[i].len > 65535u) min_len = recs[i].len > 65535u ? 0u : recs[i].len;
  }
  const size_t ns = (size_t)FQGPU_SEQ_MODELS * FQGPU_SEQ_ALPHA, nq = (size_t)FQGPU_QUAL_MODELS * FQGPU_QUAL_ALPHA;
  uint8_t *raw_dev = fq_dev_alloc<uint8_t>(raw_len + 64);
  fqgpu_rec *recs_dev = fq_dev_alloc<fqgpu_rec>(n_recs + 1);
  uint32_t *cnt = fq_dev_alloc<uint32_t>(ns + nq + 1);
  hipStream_t st = nullptr;
  uint32_t err = 0;
  if (!raw_dev || !recs_dev || !cnt) rc = FQGPU_E_NOMEM;
  do {
    if (rc) break;
    if (hipMemcpy(raw_dev, raw, raw_len, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(recs_dev, recs, n_recs * sizeof(fqgpu_rec), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(cnt + ns + nq, 0, 4) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    if ((rc = fq_build_freq_tables(device, st, raw_dev, recs_dev, n_recs, cnt, cnt + ns, n_bases, min_len))) break;
    if (hipMemcpy(&err, cnt + ns + nq, 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    if (err) { rc = FQGPU_E_ARG; break; }  // quality above Q63: the reference throws (src/fse_quality.cpp:88); a base byte outside ACGTN
    if (seq_counts_out && hipMemcpy(seq_counts_out, cnt, ns * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    if (qual_counts_out && hipMemcpy(qual_counts_out, cnt + ns, nq * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = FQGPU_E_HIP; break; }
    if ((rc = normalize_to_host(st, cnt, 0, seq_ft_out))) break;
    if ((rc = normalize_to_host(st, cnt + ns, 1, qual_ft_out))) break;
  } while (0);
  if (raw_dev) (void)hipFree(raw_dev);
  if (recs_dev) (void)hipFree(recs_dev);
  if (cnt) (void)hipFree(cnt);
  return rc;
}

// ------------------------------------------------------------------ handle
static void free_tables(DevTables &t) {
  void *ps[] = {t.norm, t.logs, t.log_prefix, t.ct, t.ct_off, t.dt, t.dt_off, t.next1, t.next2, t.reset_mask,
                t.seq_pow[0], t.seq_pow[1], t.seq_pow[2], t.seq_pow[3]};
  for (void *p : ps) if (p) (void)hipFree(p);
  t = DevTables();
}

static int upload_tables(fqgpu_ctx *ctx, int stream, const void *ft) {
  const FtLayout l = ft_layout(stream);
  DevTables &t = ctx->tab[stream];
  const uint8_t *p = static_cast<const uint8_t *>(ft);
  const uint32_t *logs = reinterpret_cast<const uint32_t *>(p + l.logs_off);
  const int16_t *norm = reinterpret_cast<const int16_t *>(p);
  uint32_t max_log = 0;
  for (int i = 0; i < l.n_models; i++) {
    if (logs[i] < 5 || logs[i] > 12) return FQGPU_E_ARG;  // FSE_MIN_TABLELOG .. FSE_MAX_TABLELOG
    if (logs[i] > max_log) max_log = logs[i];
    // every entry -1 or more, and the entries sum to 2^log with -1 counted as 1: refused here, before a kernel runs.
    // (k_build_tables counts an entry below -1 as 0 and would pass [-2, 2^log, 0, 0]; and behind its own refusal of a
    // sum the transition-table kernels would still walk that context's unbuilt tables.)
    uint32_t sum = 0;
    for (int s = 0; s < l.alpha; s++) {
      const int n = norm[(size_t)i * l.alpha + s];
      if (n < -1) return FQGPU_E_ARG;
      sum += n == -1 ? 1u : (uint32_t)n;
    }
    if (sum != (1u << logs[i])) return FQGPU_E_ARG;
  }
  t.max_log = max_log;
  t.norm = fq_dev_alloc<int16_t>((size_t)l.n_models * l.alpha);
  t.logs = fq_dev_alloc<uint32_t>(l.n_models);
  uint32_t *err_dev = fq_dev_alloc<uint32_t>(1);
  if (!t.norm || !t.logs || !err_dev) return FQGPU_E_NOMEM;
  FQ_HIP(hipMemcpyAsync(t.norm, p, l.norm_bytes, hipMemcpyHostToDevice, ctx->stream));
  FQ_HIP(hipMemcpyAsync(t.logs, logs, (size_t)l.n_models * 4, hipMemcpyHostToDevice, ctx->stream));
  FQ_HIP(hipMemsetAsync(err_dev, 0, 4, ctx->stream));
  int rc = fq_build_tables(ctx->stream, t, l.n_models, l.alpha, err_dev);
  uint32_t err = 0;
  if (!rc) {
    FQ_HIP(hipMemcpyAsync(&err, err_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    FQ_HIP(hipStreamSynchronize(ctx->stream));
    if (err) rc = FQGPU_E_ARG;  // counts of a context do not sum to 2^log
  }
  (void)hipFree(err_dev);
  return rc;
}

extern "C" int fqgpu_ctx_create(int device, const void *seq_ft, const void *qual_ft, fqgpu_ctx **out) {
  if (!out) return FQGPU_E_ARG;
  *out = nullptr;
  int rc = use_device(device);
  if (rc) return rc;
  if (!seq_ft || !qual_ft) return FQGPU_E_ARG;
  fqgpu_ctx *ctx = new (std::nothrow) fqgpu_ctx();
  if (!ctx) return FQGPU_E_NOMEM;
  ctx->device = device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->n_cus = (unsigned)cus;
  }
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return FQGPU_E_HIP;
  }
  rc = fq_probe_lds_atomic_order(ctx->stream, &ctx->lds_atomics_ordered);
  if (!rc) rc = fq_encode_init_device();
  if (getenv("FQGPU_NO_LDS_ATOMIC_RANK")) ctx->lds_atomics_ordered = false;  // force the ballot kernel
  if (getenv("FQGPU_SLOT_PARTITION")) ctx->tile_sorted = false;  // the slot-based partition/gather (same bits, for comparisons)
  if (const char *e = getenv("FQGPU_SETFUNC_WGS")) ctx->setfunc_wgs = (unsigned)atoi(e);  // experiments: same bits
  if (const char *e = getenv("FQGPU_SEQ_GROUP")) ctx->seq_group = (unsigned)atoi(e);  // experiments
  if (const char *e = getenv("FQGPU_SEQ_GROUP_MIN")) ctx->seq_group_min = (unsigned)atoi(e);
  if (const char *e = getenv("FQGPU_SEQ_CAND_CAP")) ctx->seq_cand_cap = std::min((unsigned)atoi(e), 64u);
  if (const char *e = getenv("FQGPU_SEQ_CAND_PREFIX")) ctx->seq_cand_prefix = std::max((unsigned)atoi(e), 1u);
  if (!rc) rc = upload_tables(ctx, 0, seq_ft);
  if (!rc) rc = upload_tables(ctx, 1, qual_ft);
  if (rc) { fqgpu_ctx_destroy(ctx); return rc; }
  *out = ctx;
  return FQGPU_OK;
}

#ifdef FQGPU_EXPERIMENTS
void fq_ts_prof_dump();
#endif

extern "C" void fqgpu_ctx_destroy(fqgpu_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)fqgpu_sync(ctx);
#ifdef FQGPU_EXPERIMENTS
  fq_ts_prof_dump();
#endif
  free_tables(ctx->tab[0]);
  free_tables(ctx->tab[1]);
  ctx_each_devbuf(ctx, [](const char *, const char *, DevBuf &b) { b.release(); });
  ctx->hp_hdr.release_host();
  ctx->hp_chunk.release_host();
  ctx->crc.release_host();
  ctx->stats.release_host();
  ctx->select.release_host();
  for (int i = 0; i < FQ_MAX_LANES; i++) free_lane(ctx->lanes[i]);
  fqgpu_dblock_destroy(ctx->hp.block);
  if (ctx->hp_ev_h2d) (void)hipEventDestroy(ctx->hp_ev_h2d);
  if (ctx->hp_result) (void)hipHostFree(ctx->hp_result);
  if (ctx->timer) {
    for (hipEvent_t e : ctx->timer->pool) (void)hipEventDestroy(e);
    delete ctx->timer;
  }
  if (ctx->dec_stream2) (void)hipStreamDestroy(ctx->dec_stream2);
  if (ctx->dec_fork) (void)hipEventDestroy(ctx->dec_fork);
  if (ctx->dec_join) (void)hipEventDestroy(ctx->dec_join);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

extern "C" int fqgpu_ctx_set_chain_params(fqgpu_ctx *ctx, unsigned segment, unsigned flags) {
  if (!ctx) return FQGPU_E_ARG;
  if (segment) {
    if (segment < 2 || segment > (1u << 24)) return FQGPU_E_ARG;
    ctx->seg_len = segment;
  }
  ctx->seq_generic = (flags & FQGPU_CHAIN_SEQ_GENERIC) ? 1 : 0;
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_set_seq_group(fqgpu_ctx *ctx, unsigned max_segments, unsigned min_groups) {
  if (!ctx) return FQGPU_E_ARG;
  ctx->seq_group = max_segments ? max_segments : 8u;
  ctx->seq_group_min = min_groups ? min_groups : 16u;
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_set_seq_handover(fqgpu_ctx *ctx, unsigned cap, unsigned prefix_segments) {
  if (!ctx || cap > 64) return FQGPU_E_ARG;
  ctx->seq_cand_cap = cap;
  ctx->seq_cand_prefix = prefix_segments ? prefix_segments : 1u;
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_set_seq_segment(fqgpu_ctx *ctx, unsigned symbols) {
  if (!ctx) return FQGPU_E_ARG;
  ctx->seq_segment = symbols;
  if (symbols) {  // the power tables for this segment length (encode.hip rounds it the same way), before any encode uses them
    int rc = use_device(ctx->device);
    if (!rc) rc = fqgpu_sync(ctx);
    if (rc) return rc;
    const unsigned S = (unsigned)std::min((((size_t)symbols + 1023) / 1024) * 1024, (size_t)1 << 30);
    if ((rc = fq_seq_pow_ensure(ctx->stream, ctx->tab[0], FQGPU_SEQ_MODELS, S))) return rc;
    FQ_HIP(hipStreamSynchronize(ctx->stream));
  }
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_set_index_stride(fqgpu_ctx *ctx, unsigned symbols) {
  if (!ctx || symbols == 0 || symbols > (1u << 30)) return FQGPU_E_ARG;
  ctx->index_stride = (symbols + 65535u) & ~65535u;  // whole partition tiles of both streams
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_index_bytes(const fqgpu_dblock *b, int stream, size_t *bytes) {
  if (!b || !bytes || stream < 0 || stream > 1) return FQGPU_E_ARG;
  *bytes = b->index_bytes[stream];
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_fetch_index(fqgpu_ctx *ctx, const fqgpu_dblock *b, int stream, void *out, size_t cap) {
  if (!ctx || !b || !out || stream < 0 || stream > 1 || cap < b->index_bytes[stream]) return FQGPU_E_ARG;
  int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  if (b->index_bytes[stream]) FQ_HIP(hipMemcpy(out, b->index[stream], b->index_bytes[stream], hipMemcpyDeviceToHost));
  return FQGPU_OK;
}

// an index for this block's stream: its header must describe the block; room for it on the device.  (The decode checks
// that every stride consumes exactly the bits between two snapshots; the states in a snapshot are taken as they are:
// a container that stores an index protects it with a checksum -- archive.hpp's DecodeIndexFile does.)
// the header of a decode index of a block of n_bases symbols, if it describes the index's size
static int index_header(int stream, size_t n_bases, const void *data, size_t len, FqIndexHeader *out) {
  const unsigned B = stream ? FQGPU_QUAL_MODELS : FQGPU_SEQ_MODELS;
  FqIndexHeader h;
  if (len < sizeof(h)) return FQGPU_E_CORRUPT;
  memcpy(&h, data, sizeof(h));
  if (h.magic != FQ_INDEX_MAGIC || h.stream != (uint32_t)stream || h.stride == 0 || (h.stride & 65535u) ||
      h.n_sym != n_bases || h.n_snap != fq_index_n_snap(h.n_sym, h.stride) || len != fq_index_bytes(h.n_snap, B))
    return FQGPU_E_CORRUPT;
  if (out) *out = h;
  return FQGPU_OK;
}

static int index_accept(fqgpu_dblock *b, int stream, const void *data, size_t len) {
  const int rc = index_header(stream, b->n_bases, data, len, nullptr);
  return rc ? rc : b->index[stream].grow(len + 64);
}

extern "C" int fqgpu_dblock_load_index(fqgpu_ctx *ctx, fqgpu_dblock *b, int stream, const void *data, size_t len) {
  if (!ctx || !b || stream < 0 || stream > 1 || (!data && len)) return FQGPU_E_ARG;
  int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  if (len == 0) { b->index_bytes[stream] = 0; return FQGPU_OK; }
  if ((rc = index_accept(b, stream, data, len))) return rc;
  FQ_HIP(hipMemcpy(b->index[stream], data, len, hipMemcpyHostToDevice));
  b->index_bytes[stream] = len;
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_set_lanes(fqgpu_ctx *ctx, unsigned lanes) {
  if (!ctx || lanes > FQ_MAX_LANES) return FQGPU_E_ARG;  // (0: by block size)
  int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  ctx->n_lanes = lanes;
  ctx->next_lane = 0;
  for (EncLane &l : ctx->lanes) l.forget_diag();  // blocks land on other lanes from here on: no lane answers for an earlier encode
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_dump_tables(fqgpu_ctx *ctx, int stream, unsigned model, uint32_t *ctable_out,
                                     size_t ctable_cap_words, uint32_t *dtable_out, size_t dtable_cap_words) {
  if (!ctx || stream < 0 || stream > 1) return FQGPU_E_ARG;
  const FtLayout l = ft_layout(stream);
  if (model >= (unsigned)l.n_models) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  const DevTables &t = ctx->tab[stream];
  uint32_t lg = 0, co = 0, dof = 0;
  FQ_HIP(hipMemcpy(&lg, t.logs + model, 4, hipMemcpyDeviceToHost));
  FQ_HIP(hipMemcpy(&co, t.ct_off + model, 4, hipMemcpyDeviceToHost));
  FQ_HIP(hipMemcpy(&dof, t.dt_off + model, 4, hipMemcpyDeviceToHost));
  const size_t cw = 1 + ((size_t)1 << (lg - 1)) + 2 * (size_t)l.alpha, dw = 1 + ((size_t)1 << lg);
  if (ctable_out) {
    if (ctable_cap_words < cw) return FQGPU_E_ARG;
    FQ_HIP(hipMemcpy(ctable_out, t.ct + co, cw * 4, hipMemcpyDeviceToHost));
  }
  if (dtable_out) {
    if (dtable_cap_words < dw) return FQGPU_E_ARG;
    FQ_HIP(hipMemcpy(dtable_out, t.dt + dof, dw * 4, hipMemcpyDeviceToHost));
    for (size_t k = 1; k < dw; k++) dtable_out[k] = FQ_DENTRY_TO_ZSTD(dtable_out[k]);  // the device keeps the walk's arrangement
  }
  return FQGPU_OK;
}

// ------------------------------------------------------------------ device-resident blocks
extern "C" void fqgpu_dblock_destroy(fqgpu_dblock *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  fq_dblock_each_buf(*b, [](const char *, auto &a) { (void)a.release(); });
  if (b->ev_encoded) (void)hipEventDestroy(b->ev_encoded);
  delete b;
}

// A block of the handle's device that holds nothing but its result words; every error path of its maker is a plain return.
// nullptr: no memory.
struct DblockDestroy { void operator()(fqgpu_dblock *b) const { fqgpu_dblock_destroy(b); } };
typedef std::unique_ptr<fqgpu_dblock, DblockDestroy> DblockPtr;
static DblockPtr dblock_new(fqgpu_ctx *ctx) {
  DblockPtr b(new (std::nothrow) fqgpu_dblock());
  if (!b) return b;
  b->device = ctx->device;
  b->owner = ctx;
  if (b->result.grow(1)) b.reset();
  return b;
}

// stream / side-stream arrays of a caller's block whose n_recs, n_bases and n_pos_cap are set: exactly what they must hold
static int alloc_block_outputs(fqgpu_dblock *b) {
  b->seq_cap = fqgpu_bound_seq(b->n_bases);
  b->qual_cap = fqgpu_bound_qual(b->n_bases);
  if (b->seq.grow(b->seq_cap + 64) || b->qual.grow(b->qual_cap + 64) || b->readlens.grow(b->n_recs) || b->n_count.grow(b->n_recs) ||
      b->n_pos.grow(b->n_pos_cap + 16))
    return FQGPU_E_NOMEM;
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_create(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs,
                                   size_t n_recs, fqgpu_dblock **out) {
  if (!ctx || !raw || !recs || !out || !n_recs) return FQGPU_E_ARG;
  *out = nullptr;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  size_t n_bases = 0;
  if ((rc = check_recs(recs, n_recs, raw_len, &n_bases))) return rc;
  // number of N bases = entries of n_pos (the reference grows the vector as it goes)
  size_t n_n = 0;
  for (size_t i = 0; i < n_recs; i++) {
    const uint8_t *s = raw + recs[i].seq_off, *e = s + recs[i].len;
    while ((s = static_cast<const uint8_t *>(memchr(s, 'N', (size_t)(e - s)))) != nullptr) { n_n++; s++; }
  }
  DblockPtr b = dblock_new(ctx);
  if (!b) return FQGPU_E_NOMEM;
  b->raw_len = raw_len; b->n_recs = n_recs; b->n_bases = n_bases;
  b->n_pos_cap = n_n;
  if (b->raw.grow(raw_len + 64) || b->recs.grow(n_recs) || alloc_block_outputs(b.get())) return FQGPU_E_NOMEM;
  FQ_HIP(hipMemcpyAsync(b->raw, raw, raw_len, hipMemcpyHostToDevice, ctx->stream));
  FQ_HIP(hipMemcpyAsync(b->recs, recs, n_recs * sizeof(fqgpu_rec), hipMemcpyHostToDevice, ctx->stream));
  FQ_HIP(hipMemsetAsync(b->result, 0, sizeof(BlockResult), ctx->stream));
  FQ_HIP(hipStreamSynchronize(ctx->stream));
  *out = b.release();
  return FQGPU_OK;
}

int fq_parse_on_device(hipStream_t st, const uint8_t *raw_dev, size_t raw_len, DevBuf &scan_tmp,
                       DevArray<fqgpu_rec> &recs, size_t *n_recs, size_t *n_bases, size_t *n_n);

// Raw block in, record table built on the GPU (parse.hip): replaces FastqReader::parseRecords
// (reference src/fastq_io.cpp:67-125) for callers that hand over unparsed chunks.
extern "C" int fqgpu_dblock_create_from_raw(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, fqgpu_dblock **out) {
  if (!ctx || !raw || !out || !raw_len) return FQGPU_E_ARG;
  *out = nullptr;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  DblockPtr b = dblock_new(ctx);
  if (!b || b->raw.grow(raw_len + 64)) return FQGPU_E_NOMEM;
  FQ_HIP(hipMemsetAsync(b->raw + raw_len, 0, 64, ctx->stream));
  FQ_HIP(hipMemcpyAsync(b->raw, raw, raw_len, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = fq_parse_on_device(ctx->stream, b->raw, raw_len, ctx->scan_tmp, b->recs, &b->n_recs, &b->n_bases, &b->n_pos_cap))) return rc;
  // the block ends with the last complete record (partial tail ignored like the reference)
  fqgpu_rec last;
  FQ_HIP(hipMemcpy(&last, b->recs + (b->n_recs - 1), sizeof(last), hipMemcpyDeviceToHost));
  b->raw_len = (size_t)last.qual_off + last.len + 1;
  if ((rc = alloc_block_outputs(b.get()))) return rc;
  FQ_HIP(hipMemsetAsync(b->result, 0, sizeof(BlockResult), ctx->stream));
  FQ_HIP(hipStreamSynchronize(ctx->stream));
  *out = b.release();
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_records(fqgpu_ctx *ctx, const fqgpu_dblock *b, fqgpu_rec *recs_out, size_t cap,
                                    size_t *n_recs, size_t *raw_len) {
  if (!ctx || !b) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  if (n_recs) *n_recs = b->n_recs;
  if (raw_len) *raw_len = b->raw_len;
  if (recs_out) {
    const size_t n = cap < b->n_recs ? cap : b->n_recs;
    FQ_HIP(hipMemcpy(recs_out, b->recs, n * sizeof(fqgpu_rec), hipMemcpyDeviceToHost));
  }
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_encode(fqgpu_ctx *ctx, fqgpu_dblock *b, unsigned flags) {
  if (!ctx || !b || b->device != ctx->device) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  b->launched(1);
  return fq_encode_launch(ctx, b, flags);
}

extern "C" int fqgpu_dblock_wipe(fqgpu_ctx *ctx, fqgpu_dblock *b) {
  if (!ctx || !b || b->device != ctx->device) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  return fq_wipe_launch(ctx, b);
}

extern "C" int fqgpu_sync(fqgpu_ctx *ctx) {
  if (!ctx) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  for (int i = 0; i < FQ_MAX_LANES; i++) {
    if (ctx->lanes[i].st_seq) FQ_HIP(hipStreamSynchronize(ctx->lanes[i].st_seq));
    if (ctx->lanes[i].st_qual) FQ_HIP(hipStreamSynchronize(ctx->lanes[i].st_qual));
  }
  if (ctx->stream) FQ_HIP(hipStreamSynchronize(ctx->stream));
  return FQGPU_OK;
}

// Reads the device result block; call after fqgpu_sync.  Encode results also set the
// stream sizes a later decode of this block uses.
static int pull_result(fqgpu_dblock *b, bool from_encode) {
  FQ_HIP(hipMemcpy(&b->host_result, b->result, sizeof(BlockResult), hipMemcpyDeviceToHost));
  b->result_pulled = true;
  const BlockResult &r = b->host_result;
  if (r.s[1].bad_symbol || r.s[0].bad_symbol) return FQGPU_E_ARG;
  if (from_encode) {
    if (r.s[0].overflow || r.s[1].overflow) return FQGPU_E_OVERFLOW;
    b->seq_len = (size_t)r.s[0].len;
    b->qual_len = (size_t)r.s[1].len;
    b->n_pos_len = (size_t)r.n_pos_len;
  } else if (r.s[0].corrupt || r.s[1].corrupt) {
    return FQGPU_E_CORRUPT;
  }
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_status(const fqgpu_dblock *b, size_t *seq_len, size_t *qual_len, size_t *n_pos_len,
                                   size_t *n_bases) {
  if (!b) return FQGPU_E_ARG;
  fqgpu_dblock *mb = const_cast<fqgpu_dblock *>(b);
  (void)hipSetDevice(b->device);
  // The lanes run on non-blocking streams: a copy on the null stream is not ordered behind them.
  // An operation still in flight is waited for here (its sizes would otherwise read zero or stale).
  int rc = FQGPU_OK;
  if (b->last_op && !b->result_pulled && b->owner && (rc = fqgpu_sync(b->owner))) return rc;
  rc = b->last_op ? pull_result(mb, b->last_op == 1) : FQGPU_OK;
  if (seq_len) *seq_len = b->seq_len;
  if (qual_len) *qual_len = b->qual_len;
  if (n_pos_len) *n_pos_len = b->n_pos_len;
  if (n_bases) *n_bases = b->n_bases;
  return rc;
}

extern "C" int fqgpu_dblock_longest_chain(const fqgpu_dblock *b, unsigned *seq_segments, unsigned *qual_segments) {
  if (!b) return FQGPU_E_ARG;
  (void)hipSetDevice(b->device);
  BlockResult tmp;
  FQ_HIP(hipMemcpy(&tmp, b->result, sizeof(tmp), hipMemcpyDeviceToHost));
  if (seq_segments) *seq_segments = tmp.s[0].refixed;
  if (qual_segments) *qual_segments = tmp.s[1].refixed;
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_seq_handover(const fqgpu_dblock *b, unsigned *handed_over, unsigned *kept) {
  if (!b) return FQGPU_E_ARG;
  (void)hipSetDevice(b->device);
  if (b->last_op && !b->result_pulled && b->owner) {
    const int rc = fqgpu_sync(b->owner);
    if (rc) return rc;
  }
  BlockResult tmp;
  FQ_HIP(hipMemcpy(&tmp, b->result, sizeof(tmp), hipMemcpyDeviceToHost));
  if (handed_over) *handed_over = tmp.seq_groups_handed;
  if (kept) *kept = tmp.seq_groups_kept;
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_decode_forms(const fqgpu_ctx *ctx, unsigned *forms, unsigned *qual_chains, unsigned *qual_strides, unsigned *n_cus) {
  if (!ctx) return FQGPU_E_ARG;
  if (forms) *forms = ctx->dec_forms;
  if (qual_chains) *qual_chains = ctx->dec_qual_chains;
  if (qual_strides) *qual_strides = ctx->dec_qual_strides;
  if (n_cus) *n_cus = ctx->n_cus;
  return FQGPU_OK;
}

// The lane whose scratch still holds the quality segments of b's last encode, and their number: the guards and the refusals
// of both segment diagnostics
static int diag_lane(fqgpu_ctx *ctx, const fqgpu_dblock *b, const EncLane **lane_out, uint32_t *n_out) {
  if (int rc = fqgpu_sync(ctx)) return rc;
  // the classes lie in the scratch of the lane that coded the block: the handle's own lane, and only while no later encode has
  // gone through it and it has not been reset (free_lane, fqgpu_ctx_set_lanes)
  if (b->owner != ctx || !b->diag_stamp || b->home_lane < 0 || b->home_lane >= FQ_MAX_LANES) return FQGPU_E_ARG;
  const EncLane &lane = ctx->lanes[b->home_lane];
  if (lane.diag_stamp != b->diag_stamp || !lane.diag_cls || !lane.diag_anchor || !lane.diag_n_segs) return FQGPU_E_ARG;
  FQ_HIP(hipMemcpy(n_out, lane.diag_n_segs, 4, hipMemcpyDeviceToHost));
  *lane_out = &lane;
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_qual_segment_classes(fqgpu_ctx *ctx, const fqgpu_dblock *b, size_t counts[4]) {
  if (!ctx || !b || !counts) return FQGPU_E_ARG;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  const EncLane *lane = nullptr;
  uint32_t n = 0;
  if (int rc = diag_lane(ctx, b, &lane, &n)) return rc;
  if (!n) return FQGPU_OK;
  uint8_t *cls = static_cast<uint8_t *>(malloc(n));
  if (!cls) return FQGPU_E_NOMEM;
  const hipError_t he = hipMemcpy(cls, lane->diag_cls, n, hipMemcpyDeviceToHost);
  if (he == hipSuccess)
    for (uint32_t i = 0; i < n; i++) counts[cls[i] == 1 ? 0 : cls[i] == 0xFF ? 2 : cls[i] == 0 ? 3 : 1]++;
  free(cls);
  return he == hipSuccess ? FQGPU_OK : fq_hip_error(he, __FILE__, __LINE__);
}

extern "C" int fqgpu_dblock_qual_segments(fqgpu_ctx *ctx, const fqgpu_dblock *b, uint8_t *cls_out, uint32_t *anchor_out,
                                          uint32_t *ctx_out, size_t cap, size_t *n_out) {
  if (!ctx || !b || !n_out || (cap && (!cls_out || !anchor_out || !ctx_out))) return FQGPU_E_ARG;
  *n_out = 0;
  const EncLane *lane = nullptr;
  uint32_t n = 0;
  if (int rc = diag_lane(ctx, b, &lane, &n)) return rc;
  *n_out = n;
  if (n > cap) return FQGPU_E_OVERFLOW;  // (*n_out says how many there are)
  if (!n) return FQGPU_OK;
  constexpr unsigned B = FQGPU_QUAL_MODELS;
  uint32_t *seg_base = static_cast<uint32_t *>(malloc((size_t)(B + 1) * 4));
  if (!seg_base) return FQGPU_E_NOMEM;
  hipError_t he = hipMemcpy(seg_base, lane->diag_n_segs - B, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost);
  if (he == hipSuccess) he = hipMemcpy(cls_out, lane->diag_cls, n, hipMemcpyDeviceToHost);
  if (he == hipSuccess) he = hipMemcpy(anchor_out, lane->diag_anchor, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (he == hipSuccess)
    for (unsigned c = 0; c < B; c++)
      for (uint32_t s = seg_base[c]; s < seg_base[c + 1] && s < n; s++) ctx_out[s] = c;
  free(seg_base);
  return he == hipSuccess ? FQGPU_OK : fq_hip_error(he, __FILE__, __LINE__);
}

extern "C" int fqgpu_dblock_fetch(fqgpu_ctx *ctx, const fqgpu_dblock *b, uint8_t *seq_out, uint8_t *qual_out,
                                  uint16_t *readlens_out, uint16_t *n_count_out, uint16_t *n_pos_out,
                                  uint8_t *raw_out) {
  if (!ctx || !b) return FQGPU_E_ARG;
  int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  // sizes of an encode nobody has asked the status of yet
  if (b->last_op && !b->result_pulled && (rc = pull_result(const_cast<fqgpu_dblock *>(b), b->last_op == 1))) return rc;
  if (seq_out && b->seq_len) FQ_HIP(hipMemcpy(seq_out, b->seq, b->seq_len, hipMemcpyDeviceToHost));
  if (qual_out && b->qual_len) FQ_HIP(hipMemcpy(qual_out, b->qual, b->qual_len, hipMemcpyDeviceToHost));
  if (readlens_out) FQ_HIP(hipMemcpy(readlens_out, b->readlens, b->n_recs * 2, hipMemcpyDeviceToHost));
  if (n_count_out) FQ_HIP(hipMemcpy(n_count_out, b->n_count, b->n_recs * 2, hipMemcpyDeviceToHost));
  if (n_pos_out && b->n_pos_len) FQ_HIP(hipMemcpy(n_pos_out, b->n_pos, b->n_pos_len * 2, hipMemcpyDeviceToHost));
  if (raw_out) FQ_HIP(hipMemcpy(raw_out, b->raw, b->raw_len, hipMemcpyDeviceToHost));
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_load_streams(fqgpu_ctx *ctx, fqgpu_dblock *b, const uint8_t *seq, size_t seq_len,
                                         const uint8_t *qual, size_t qual_len, const uint16_t *n_count,
                                         const uint16_t *n_pos, size_t n_pos_len) {
  if (!ctx || !b || !seq || !qual || !n_count || (!n_pos && n_pos_len)) return FQGPU_E_ARG;
  int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  // foreign streams may be larger than what this block's own encode would need
  // (seq_cap / qual_cap stay the capacities a later re-encode of this block is judged against)
  if (b->seq.grow(seq_len + 64) || b->qual.grow(qual_len + 64) || b->n_pos.grow(n_pos_len + 16)) return FQGPU_E_NOMEM;
  if (n_pos_len > b->n_pos_cap) b->n_pos_cap = n_pos_len;
  FQ_HIP(hipMemset(b->seq + seq_len, 0, 16));  // the bit reader loads whole dwords
  FQ_HIP(hipMemset(b->qual + qual_len, 0, 16));
  FQ_HIP(hipMemcpy(b->seq, seq, seq_len, hipMemcpyHostToDevice));
  FQ_HIP(hipMemcpy(b->qual, qual, qual_len, hipMemcpyHostToDevice));
  FQ_HIP(hipMemcpy(b->n_count, n_count, b->n_recs * 2, hipMemcpyHostToDevice));
  if (n_pos_len) FQ_HIP(hipMemcpy(b->n_pos, n_pos, n_pos_len * 2, hipMemcpyHostToDevice));
  b->seq_len = seq_len; b->qual_len = qual_len; b->n_pos_len = n_pos_len;
  b->drop_results();  // the result block no longer describes these streams, and an index belongs to the streams it was made for
  return FQGPU_OK;
}

static int dblocks_decode(fqgpu_ctx *ctx, fqgpu_dblock *const *blocks, size_t n_blocks, bool build_index) {
  if (!ctx || (!blocks && n_blocks)) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  for (size_t i = 0; i < n_blocks; i++)
    if (!blocks[i] || blocks[i]->device != ctx->device) return FQGPU_E_ARG;
  // blocks that come straight out of an encode: wait for it and take over its stream sizes
  bool synced = false;
  for (size_t i = 0; i < n_blocks; i++) {
    fqgpu_dblock *b = blocks[i];
    if (b->last_op == 1 && !b->result_pulled) {
      if (!synced && (rc = fqgpu_sync(ctx))) return rc;
      synced = true;
      if ((rc = pull_result(b, true))) return rc;
    }
    if (!b->seq_len || !b->qual_len) return FQGPU_E_ARG;
  }
  for (size_t i = 0; i < n_blocks; i++) blocks[i]->launched(2);
  return fq_decode_launch(ctx, blocks, n_blocks, nullptr, build_index);
}

extern "C" int fqgpu_dblocks_decode(fqgpu_ctx *ctx, fqgpu_dblock *const *blocks, size_t n_blocks) {
  return dblocks_decode(ctx, blocks, n_blocks, false);
}

// The same decode by the indexing walk: every block is left with both decode indexes.  Waits for the batch (a block whose
// streams turn out corrupt keeps no index); the blocks' status is reported by fqgpu_dblock_status as after fqgpu_dblocks_decode.
extern "C" int fqgpu_dblocks_decode_indexing(fqgpu_ctx *ctx, fqgpu_dblock *const *blocks, size_t n_blocks) {
  int rc = dblocks_decode(ctx, blocks, n_blocks, true);
  if (rc) {
    for (size_t i = 0; blocks && i < n_blocks; i++)
      if (blocks[i]) blocks[i]->index_bytes[0] = blocks[i]->index_bytes[1] = 0;
    return rc;
  }
  if ((rc = fqgpu_sync(ctx))) return rc;
  for (size_t i = 0; i < n_blocks; i++) {
    const int brc = pull_result(blocks[i], false);
    if (brc) blocks[i]->index_bytes[0] = blocks[i]->index_bytes[1] = 0;
    if (brc && brc != FQGPU_E_CORRUPT && brc != FQGPU_E_ARG) return brc;  // (a HIP error; the block's own verdict is its status)
  }
  return FQGPU_OK;
}

// ------------------------------------------------------------------ host-pointer convenience calls
// The two calls below stage through one device block the handle keeps between calls: a worker
// that codes chunk after chunk (reference src/process.cpp:49-54) pays hipMalloc only while its
// chunks are still growing.
// One rule of growth for the staging block: an eighth more than is needed.
template <class A> static bool hp_room(A &a, size_t need) { return a.grow(need, need / 8) == FQGPU_OK; }

static int hp_block_acquire(fqgpu_ctx *ctx, size_t raw_len, size_t n_recs, size_t n_bases, size_t seq_cap,
                            size_t qual_cap, size_t n_pos_cap, fqgpu_dblock **out) {
  if (!ctx->hp.block && !(ctx->hp.block = dblock_new(ctx).release())) return FQGPU_E_NOMEM;
  fqgpu_dblock *b = ctx->hp.block;
  const bool ok = hp_room(b->raw, raw_len + 64) && hp_room(b->recs, n_recs) && hp_room(b->seq, seq_cap + 64) &&
                  hp_room(b->qual, qual_cap + 64) && hp_room(b->readlens, n_recs) && hp_room(b->n_count, n_recs) &&
                  hp_room(b->n_pos, n_pos_cap + 16);
  if (!ok) {  // leave nothing half-sized behind
    fqgpu_dblock_destroy(b);
    ctx->hp.block = nullptr;
    ctx->hp.clear();
    return FQGPU_E_NOMEM;
  }
  b->raw_len = raw_len; b->n_recs = n_recs; b->n_bases = n_bases;
  b->seq_cap = seq_cap; b->qual_cap = qual_cap; b->n_pos_cap = n_pos_cap;
  ctx->hp.clear();
  *out = b;
  return FQGPU_OK;
}

extern "C" int fqgpu_ctx_fill_scratch(fqgpu_ctx *ctx, unsigned char byte, size_t *n_buffers, size_t *n_bytes) {
  if (!ctx || ctx->hp.pending || ctx->hp_hdr.pending) return FQGPU_E_ARG;
  int rc = fqgpu_sync(ctx);  // (selects the device)
  if (rc) return rc;
  size_t bufs = 0, bytes = 0;
  hipError_t he = hipSuccess;
  for (EncLane &l : ctx->lanes) l.forget_diag();  // the segment classes of earlier encodes are about to be overwritten
  auto fill = [&](void *p, size_t n) {
    if (!p || !n || he != hipSuccess) return;
    if ((he = hipMemsetAsync(p, byte, n, ctx->stream)) != hipSuccess) return;
    bufs++;
    bytes += n;
  };
  ctx_each_devbuf(ctx, [&](const char *owner, const char *name, DevBuf &b) {
    if (!scratch_is_state(owner, name)) fill(b.p, b.cap);
  });
  if (ctx->hp.block) fq_dblock_each_buf(*ctx->hp.block, [&](const char *, auto &a) { fill(a.p, a.bytes()); });
  ctx->hp.clear();  // no chunk to digest, no index, no result
  FQ_HIP(he);
  FQ_HIP(hipStreamSynchronize(ctx->stream));
  if (n_buffers) *n_buffers = bufs;
  if (n_bytes) *n_bytes = bytes;
  return FQGPU_OK;
}

// Everything a block of this shape will need -- the staging block of the host-pointer calls and the
// scratch of every encode lane -- allocated now: the first block of a worker otherwise pays half a
// second of hipMalloc (2.3 GB of scratch per 256 MiB block and lane) inside its timed loop.
extern "C" int fqgpu_ctx_reserve(fqgpu_ctx *ctx, size_t raw_len, size_t n_recs, size_t n_bases) {
  if (!ctx || !raw_len || !n_recs || !n_bases || n_bases >= 0xFFF00000ull) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  if ((rc = fqgpu_sync(ctx))) return rc;
  fqgpu_dblock *b = nullptr;
  if ((rc = hp_block_acquire(ctx, raw_len, n_recs, n_bases, fqgpu_bound_seq(n_bases), fqgpu_bound_qual(n_bases), n_bases / 64 + 1024, &b))) return rc;
  if ((rc = ctx->hp_parse.cnt.reserve((raw_len / 4096 + 2) * 4)) || (rc = ctx->hp_parse.base.reserve((raw_len / 4096 + 3) * 4)) ||
      (rc = ctx->hp_parse.nl_pos.reserve((n_recs * 4 + 8) * 4)))
    return rc;
  const unsigned first = ctx->next_lane;
  for (unsigned l = 0; l < fq_lanes_for(ctx, n_bases) && !rc; l++) rc = fq_encode_reserve(ctx, b);
  ctx->next_lane = first;
  return rc;
}

// Waits for everything the handle has queued before an error return: the caller's buffers (page-locked
// vectors that go back to the pin cache, where another thread may pick them up) must not be read or
// written by a copy that is still in flight.
static int hp_fail(fqgpu_ctx *ctx, int rc) {
  ctx->hp.clear();
  (void)fqgpu_sync(ctx);
  return rc;
}
#define FQ_HIP_HP(call)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) return hp_fail(ctx, fq_hip_error(e_, __FILE__, __LINE__));          \
  } while (0)

// caller_seq_cap / caller_qual_cap: capacities the overflow rule is judged against (0: the reference's bounds)
static int hp_encode_begin(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs, size_t n_recs,
                           unsigned flags, size_t caller_seq_cap, size_t caller_qual_cap, size_t *n_recs_out,
                           size_t *n_bases_out, size_t *used_len) {
  if (!ctx || !raw || !raw_len || (recs && !n_recs)) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  ctx->hp.pending = false;  // (a block begun and never collected is dropped: fqgpu_sync below waits for it)
  ctx->hp_hdr.pending = ctx->hp_hdr.collected = false;
  size_t n_bases = 0, n_n = 0, used = raw_len;
  if (recs && (rc = check_recs(recs, n_recs, raw_len, &n_bases))) return rc;
  if ((rc = fqgpu_sync(ctx))) return rc;
  fqgpu_dblock *b = nullptr;
  // the raw buffer first: without a record table the other sizes are known only after the device has counted the lines
  if ((rc = hp_block_acquire(ctx, raw_len, recs ? n_recs : 0, n_bases, 0, 0, 0, &b))) return rc;
  if (!ctx->hp_ev_h2d) FQ_HIP(hipEventCreateWithFlags(&ctx->hp_ev_h2d, hipEventDisableTiming));
  if (!ctx->hp_result) FQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&ctx->hp_result), sizeof(BlockResult), hipHostMallocPortable));
  FQ_HIP_HP(hipMemsetAsync(b->raw + raw_len, 0, 64, ctx->stream));
  FQ_HIP_HP(hipMemcpyAsync(b->raw, raw, raw_len, hipMemcpyHostToDevice, ctx->stream));
  if (!recs) {
    if ((rc = fq_parse_count(ctx->stream, b->raw, raw_len, ctx->hp_parse, &n_recs))) return hp_fail(ctx, rc);
    if (!hp_room(b->recs, n_recs)) return hp_fail(ctx, FQGPU_E_NOMEM);
    if ((rc = fq_parse_records(ctx->stream, b->raw, raw_len, ctx->hp_parse, b->recs, n_recs, &n_bases, &n_n, &used))) return hp_fail(ctx, rc);
  }
  // The reference's capacities are the ones the overflow rule is judged against.  n_pos: the device
  // parser counted the N's; with a caller's table the worst case (every base an N) is provided for.
  if ((rc = hp_block_acquire(ctx, used, n_recs, n_bases, caller_seq_cap ? caller_seq_cap : fqgpu_bound_seq(n_bases),
                             caller_qual_cap ? caller_qual_cap : fqgpu_bound_qual(n_bases), recs ? n_bases : n_n, &b)))
    return hp_fail(ctx, rc);
  if (recs) FQ_HIP_HP(hipMemcpyAsync(b->recs, recs, n_recs * sizeof(fqgpu_rec), hipMemcpyHostToDevice, ctx->stream));
  FQ_HIP_HP(hipEventRecord(ctx->hp_ev_h2d, ctx->stream));
  b->launched(1);
  hipStream_t st = nullptr;
  // (the device copy of raw is scratch here: its N's are patched on the host by fqgpu_encode_end)
  if ((rc = fq_encode_launch(ctx, b, flags & ~FQGPU_F_WRITE_BACK_N, ctx->hp_ev_h2d, &st))) return hp_fail(ctx, rc);
  FQ_HIP_HP(hipMemcpyAsync(ctx->hp_result, b->result, sizeof(BlockResult), hipMemcpyDeviceToHost, st));
  ctx->hp.pending = true;
  ctx->hp.flags = flags;
  ctx->hp.done = st;
  ctx->hp.used = used;
  ctx->hp.crc_what = 1;
  if (n_recs_out) *n_recs_out = n_recs;
  if (n_bases_out) *n_bases_out = n_bases;
  if (used_len) *used_len = used;
  return FQGPU_OK;
}

extern "C" int fqgpu_encode_begin(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs, size_t n_recs,
                                  unsigned flags, size_t *n_recs_out, size_t *n_bases_out, size_t *used_len) {
  return hp_encode_begin(ctx, raw, raw_len, recs, n_recs, flags, 0, 0, n_recs_out, n_bases_out, used_len);
}

extern "C" int fqgpu_encode_records(fqgpu_ctx *ctx, fqgpu_rec *recs_out, size_t cap) {
  if (!ctx || !recs_out || !ctx->hp.pending || !ctx->hp.block || cap < ctx->hp.block->n_recs) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  // on the handle's copy stream: the table was built (or uploaded) there; the lanes' kernels are not waited for
  FQ_HIP(hipMemcpyAsync(recs_out, ctx->hp.block->recs, ctx->hp.block->n_recs * sizeof(fqgpu_rec), hipMemcpyDeviceToHost, ctx->stream));
  FQ_HIP(hipStreamSynchronize(ctx->stream));
  return FQGPU_OK;
}

// waits for the block in flight and reads its result block; the block stays pending
static int hp_collect(fqgpu_ctx *ctx) {
  fqgpu_dblock *b = ctx->hp.block;
  if (b->result_pulled) return FQGPU_OK;
  FQ_HIP_HP(hipStreamSynchronize(ctx->hp.done));
  b->host_result = *ctx->hp_result;
  b->result_pulled = true;
  const BlockResult &r = b->host_result;
  if (r.s[0].bad_symbol || r.s[1].bad_symbol) return hp_fail(ctx, FQGPU_E_ARG);
  if (r.s[0].overflow || r.s[1].overflow) return hp_fail(ctx, FQGPU_E_OVERFLOW);
  b->seq_len = (size_t)r.s[0].len; b->qual_len = (size_t)r.s[1].len; b->n_pos_len = (size_t)r.n_pos_len;
  return FQGPU_OK;
}

extern "C" int fqgpu_encode_wait(fqgpu_ctx *ctx, size_t *seq_len, size_t *qual_len, size_t *n_pos_len) {
  if (!ctx || !ctx->hp.pending || !ctx->hp.block) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  if ((rc = hp_collect(ctx))) return rc;
  if (seq_len) *seq_len = ctx->hp.block->seq_len;
  if (qual_len) *qual_len = ctx->hp.block->qual_len;
  if (n_pos_len) *n_pos_len = ctx->hp.block->n_pos_len;
  return FQGPU_OK;
}

extern "C" int fqgpu_encode_cancel(fqgpu_ctx *ctx) {
  if (!ctx) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  ctx->hp.clear();
  ctx->hp_hdr.pending = ctx->hp_hdr.collected = false;
  return fqgpu_sync(ctx);
}

// The header fields of the block in flight (headers.hip), on the handle's copy stream -- where the chunk arrived and
// its record table was uploaded or built -- beside the lane's encode kernels.
extern "C" int fqgpu_encode_headers_begin(fqgpu_ctx *ctx, const uint8_t *field_types, const char *separators, unsigned n_fields,
                                          const uint8_t *first_header, size_t first_header_len) {
  if (!ctx || !ctx->hp.pending || !ctx->hp.block || ctx->hp_hdr.pending || !field_types || !first_header || (n_fields > 1 && !separators))
    return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  const fqgpu_dblock *b = ctx->hp.block;
  if ((rc = fq_headers_launch(ctx->stream, b->raw, ctx->hp.used, b->recs, b->n_recs, b->n_bases, field_types, separators, n_fields,
                              first_header, first_header_len, ctx->hp_hdr)))
    return rc == FQGPU_E_ARG ? rc : hp_fail(ctx, rc);
  ctx->hp_hdr.pending = true;
  ctx->hp_hdr.collected = false;
  return FQGPU_OK;
}

extern "C" int fqgpu_encode_headers_wait(fqgpu_ctx *ctx, fqgpu_field_sizes *sizes, size_t *total_bytes, size_t *bad_record) {
  if (!ctx || !ctx->hp_hdr.pending) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  HdrScratch &hs = ctx->hp_hdr;
  if (!hs.collected) {
    FQ_HIP_HP(hipStreamSynchronize(ctx->stream));
    hs.collected = true;
  }
  const HdrResult &r = *hs.host_res;
  if (r.first_error != ~0ull) {
    if ((r.first_error & 0xFFu) == 3u || r.total > hs.bound) return FQGPU_E_ARG;  // a record table whose headers overlap: not this chunk's
    if (bad_record) *bad_record = (size_t)(r.first_error >> 8);
    return FQGPU_E_HEADER;
  }
  for (unsigned i = 0; sizes && i < hs.n_fields; i++) sizes[i] = {r.size[3 * i], r.size[3 * i + 1], r.size[3 * i + 2]};
  if (total_bytes) *total_bytes = (size_t)r.total;
  return FQGPU_OK;
}

extern "C" int fqgpu_encode_headers_end(fqgpu_ctx *ctx, uint8_t *out, size_t out_cap) {
  if (!ctx || !ctx->hp_hdr.pending || !out) return FQGPU_E_ARG;
  size_t total = 0;
  int rc = fqgpu_encode_headers_wait(ctx, nullptr, &total, nullptr);
  if (rc) return rc;
  if (out_cap < total) return FQGPU_E_ARG;
  HdrScratch &hs = ctx->hp_hdr;
  FQ_HIP_HP(hipMemcpyAsync(out, hs.out.p, total, hipMemcpyDeviceToHost, ctx->stream));
  FQ_HIP_HP(hipStreamSynchronize(ctx->stream));
  hs.pending = hs.collected = false;
  return FQGPU_OK;
}

extern "C" int fqgpu_encode_end(fqgpu_ctx *ctx, uint8_t *raw, uint8_t *seq_out, size_t seq_cap, size_t *seq_len,
                                uint8_t *qual_out, size_t qual_cap, size_t *qual_len, uint16_t *readlens_out,
                                uint16_t *n_count_out, uint16_t *n_pos_out, size_t n_pos_cap, size_t *n_pos_len) {
  if (!ctx || !ctx->hp.pending || !ctx->hp.block) return FQGPU_E_ARG;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  if (!seq_out || !qual_out || !seq_len || !qual_len) return hp_fail(ctx, FQGPU_E_ARG);
  fqgpu_dblock *b = ctx->hp.block;
  hipStream_t st = ctx->hp.done;
  const size_t n_recs = b->n_recs;
  if ((rc = hp_collect(ctx))) return rc;
  ctx->hp.pending = false;
  if (b->seq_len > seq_cap || b->qual_len > qual_cap) return FQGPU_E_OVERFLOW;
  if (n_pos_out && b->n_pos_len > n_pos_cap) return FQGPU_E_ARG;
  // N -> A on the host needs the N tables even if the caller does not want them
  std::vector<uint16_t> tmp_cnt, tmp_pos;
  const bool patch = raw && (ctx->hp.flags & FQGPU_F_WRITE_BACK_N) && b->n_pos_len;
  uint16_t *cnt_h = n_count_out, *pos_h = n_pos_out;
  if (patch && !cnt_h) { tmp_cnt.resize(n_recs); cnt_h = tmp_cnt.data(); }
  if (patch && !pos_h) { tmp_pos.resize(b->n_pos_len); pos_h = tmp_pos.data(); }
  std::vector<fqgpu_rec> tmp_recs;
  if (patch) tmp_recs.resize(n_recs);
  // (the side buffers -- record table, readlens, n_count, n_pos -- are best left PAGEABLE: as page-locked
  // buffers their small copies queue up in the DMA engines behind the other workers' 256 MiB uploads;
  // four threads: 47.9 GB/s with pageable, 40-42 with page-locked side buffers, same box)
  FQ_HIP_HP(hipMemcpyAsync(seq_out, b->seq, b->seq_len, hipMemcpyDeviceToHost, st));
  FQ_HIP_HP(hipMemcpyAsync(qual_out, b->qual, b->qual_len, hipMemcpyDeviceToHost, st));
  if (readlens_out) FQ_HIP_HP(hipMemcpyAsync(readlens_out, b->readlens, n_recs * 2, hipMemcpyDeviceToHost, st));
  if (cnt_h) FQ_HIP_HP(hipMemcpyAsync(cnt_h, b->n_count, n_recs * 2, hipMemcpyDeviceToHost, st));
  if (pos_h && b->n_pos_len) FQ_HIP_HP(hipMemcpyAsync(pos_h, b->n_pos, b->n_pos_len * 2, hipMemcpyDeviceToHost, st));
  if (patch) FQ_HIP_HP(hipMemcpyAsync(tmp_recs.data(), b->recs, n_recs * sizeof(fqgpu_rec), hipMemcpyDeviceToHost, st));
  FQ_HIP_HP(hipStreamSynchronize(st));
  if (patch) {  // replaceAndEncodeNs (src/fse_sequence.cpp:35-51): deltas to the previous N, the first one absolute
    size_t at = 0;
    for (size_t r = 0; r < n_recs; r++) {
      uint8_t *s = raw + tmp_recs[r].seq_off;
      unsigned pos = 0;
      for (unsigned k = cnt_h[r]; k > 0; k--) { pos += pos_h[at++]; s[pos] = 'A'; }
    }
  }
  *seq_len = b->seq_len;
  *qual_len = b->qual_len;
  if (n_pos_len) *n_pos_len = b->n_pos_len;
  return FQGPU_OK;
}

// The staging block's decode index of stream s: its size to *len and, if there is an `out` and anything to bring, its bytes
// (cap < *len: FQGPU_E_ARG) -- behind the stream `st`, or with a synchronous copy (st = nullptr).  *he: what the copy said.
static int hp_index_fetch(fqgpu_ctx *ctx, int stream, uint8_t *out, size_t cap, size_t *len, hipStream_t st, hipError_t *he) {
  const fqgpu_dblock *b = ctx->hp.block;
  *he = hipSuccess;
  *len = b->index_bytes[stream];
  if (!out || !*len) return FQGPU_OK;
  if (cap < *len) return FQGPU_E_ARG;
  const int rc = use_device(ctx->device);
  if (rc) return rc;
  if (!st) *he = hipMemcpy(out, b->index[stream], *len, hipMemcpyDeviceToHost);
  else if ((*he = hipMemcpyAsync(out, b->index[stream], *len, hipMemcpyDeviceToHost, st)) == hipSuccess) *he = hipStreamSynchronize(st);
  return FQGPU_OK;
}

// The decode index of the block fqgpu_encode_begin coded with FQGPU_F_DECODE_INDEX: after fqgpu_encode_wait or _end,
// until the handle's next host-pointer call.
extern "C" int fqgpu_encode_index(fqgpu_ctx *ctx, int stream, uint8_t *out, size_t cap, size_t *len) {
  if (!ctx || !ctx->hp.block || stream < 0 || stream > 1 || !len) return FQGPU_E_ARG;
  if (ctx->hp.block->last_op != 1 || !ctx->hp.block->result_pulled) return FQGPU_E_ARG;
  hipError_t he;
  const int rc = hp_index_fetch(ctx, stream, out, cap, len, ctx->hp.done, &he);
  if (rc) return rc;
  FQ_HIP(he);
  return FQGPU_OK;
}

// Host-pointer encode, one block per call, as asynchronous as one call can be: the inputs go up on
// the handle's copy stream, the lane's kernels wait for that event (not for the host), the result
// block lands in page-locked memory behind the last kernel, and the streams come down with their
// exact sizes on the stream the encode ran on.  The host waits twice: for the sizes, for the
// streams.  With page-locked caller buffers (fqgpu_host_alloc; the shim's chunk and stream vectors
// use it) every copy runs at link rate and several worker threads -- one handle each, like the
// reference's one workspace per thread (src/process.cpp:49-54) -- overlap their copies with each
// other's kernels.  Pageable buffers work too, at the rate of the runtime's staging copies.
// N -> A write-back happens on the HOST from n_count / n_pos (a few thousand bytes to touch)
// instead of copying the whole raw block back over PCIe.
extern "C" int fqgpu_encode_block(fqgpu_ctx *ctx, uint8_t *raw, size_t raw_len, const fqgpu_rec *recs,
                                  size_t n_recs, uint8_t *seq_out, size_t seq_cap, size_t *seq_len,
                                  uint8_t *qual_out, size_t qual_cap, size_t *qual_len,
                                  uint16_t *readlens_out, uint16_t *n_count_out, uint16_t *n_pos_out,
                                  size_t n_pos_cap, size_t *n_pos_len, unsigned flags) {
  if (!ctx || !raw || !recs || !n_recs || !seq_out || !qual_out || !seq_len || !qual_len) return FQGPU_E_ARG;
  if (!seq_cap || !qual_cap) return FQGPU_E_ARG;
  // the caller's capacities are the ones the overflow rule is judged against
  int rc = hp_encode_begin(ctx, raw, raw_len, recs, n_recs, flags, seq_cap, qual_cap, nullptr, nullptr, nullptr);
  if (rc) return rc;
  return fqgpu_encode_end(ctx, raw, seq_out, seq_cap, seq_len, qual_out, qual_cap, qual_len, readlens_out, n_count_out, n_pos_out,
                          n_pos_cap, n_pos_len);
}

// The coded streams of one block as the host-pointer decodes take them; index: the decode indexes (NULL / 0: none)
struct DecStreams {
  const uint8_t *seq;  size_t seq_len;
  const uint8_t *qual; size_t qual_len;
  const uint16_t *n_count; size_t n_count_len;
  const uint16_t *n_pos;   size_t n_pos_len;
  const uint8_t *index[2]; size_t index_len[2];
  bool build_index = false;  // decode by the indexing walk: the staging block is left with both indexes (index / index_len: none)
  bool seq_only = false;     // fqgpu_decode_chunk_fasta: no quality stream, no quality index; records are placed as FASTA
  bool ok() const {
    return seq && n_count && seq_len && (seq_only ? !build_index : qual && qual_len) && (index[0] || !index_len[0]) &&
           (index[1] || !index_len[1]);
  }
  int n_streams() const { return seq_only ? 1 : 2; }
};

// The staging block for a decode of these streams, once the handle is idle
static int hp_decode_acquire(fqgpu_ctx *ctx, size_t raw_len, size_t n_recs, size_t n_bases, const DecStreams &s, fqgpu_dblock **b) {
  const int rc = fqgpu_sync(ctx);
  if (rc) return rc;
  const size_t seq_cap = s.seq_len > fqgpu_bound_seq(n_bases) ? s.seq_len : fqgpu_bound_seq(n_bases);
  const size_t qual_cap = s.seq_only ? 0 : s.qual_len > fqgpu_bound_qual(n_bases) ? s.qual_len : fqgpu_bound_qual(n_bases);
  return hp_block_acquire(ctx, raw_len, n_recs, n_bases, seq_cap, qual_cap, s.n_pos_len, b);
}

// The common part of the host-pointer decodes, once the staging block holds the layout: uploads the streams, decodes
// (plan != NULL: its strides and window alone) and, when the kernels are through, copies back len bytes of the block from
// offset skip (out == NULL: nothing of the block) and, recs_out != NULL, the records [first, first + n_out) with their
// offsets relative to skip.  s.seq_only: the sequence stream alone goes up and is decoded.
static int hp_decode_staged(fqgpu_ctx *ctx, fqgpu_dblock *b, const DecStreams &s, const FqStridePlan *plan, uint8_t *out, size_t skip,
                            size_t len, fqgpu_rec *recs_out, size_t first, size_t n_out) {
  int rc;
  const size_t n_recs = b->n_recs;
  hipStream_t st = ctx->stream;
  FQ_HIP_HP(hipMemsetAsync(b->seq + s.seq_len, 0, 16, st));  // the bit reader loads whole dwords
  FQ_HIP_HP(hipMemcpyAsync(b->seq, s.seq, s.seq_len, hipMemcpyHostToDevice, st));
  if (!s.seq_only) {
    FQ_HIP_HP(hipMemsetAsync(b->qual + s.qual_len, 0, 16, st));
    FQ_HIP_HP(hipMemcpyAsync(b->qual, s.qual, s.qual_len, hipMemcpyHostToDevice, st));
  }
  // the reference pops from the END of n_count (src/fse_sequence.cpp:115-126)
  FQ_HIP_HP(hipMemcpyAsync(b->n_count, s.n_count + (s.n_count_len - n_recs), n_recs * 2, hipMemcpyHostToDevice, st));
  if (s.n_pos_len) FQ_HIP_HP(hipMemcpyAsync(b->n_pos, s.n_pos, s.n_pos_len * 2, hipMemcpyHostToDevice, st));
  for (int k = 0; k < s.n_streams(); k++)  // (hp_block_acquire has dropped whatever index the staging block held)
    if (s.index[k] && s.index_len[k]) {
      if ((rc = index_accept(b, k, s.index[k], s.index_len[k]))) return hp_fail(ctx, rc);
      FQ_HIP_HP(hipMemcpyAsync(b->index[k], s.index[k], s.index_len[k], hipMemcpyHostToDevice, st));
      b->index_bytes[k] = s.index_len[k];
    }
  b->seq_len = s.seq_len; b->qual_len = s.seq_only ? 0 : s.qual_len; b->n_pos_len = s.n_pos_len;
  b->launched(2);
  fqgpu_dblock *one[1] = {b};
  if ((rc = fq_decode_launch(ctx, one, 1, plan, s.build_index, s.seq_only ? FQ_DEC_SEQ : FQ_DEC_BOTH))) return hp_fail(ctx, rc);
  if (!ctx->hp_result) FQ_HIP_HP(hipHostMalloc(reinterpret_cast<void **>(&ctx->hp_result), sizeof(BlockResult), hipHostMallocPortable));
  // The copies back are issued only when the kernels are through: a copy that waits in a DMA
  // engine's queue for a 13 s decode kernel holds that engine, and the uploads of the next workers'
  // blocks queue up behind it (measured in the block farm: four decoding workers ran two and two,
  // the third worker's fifth hipMemcpyAsync returning after 12.8 s).
  FQ_HIP_HP(hipStreamSynchronize(st));
  FQ_HIP_HP(hipMemcpyAsync(ctx->hp_result, b->result, sizeof(BlockResult), hipMemcpyDeviceToHost, st));
  if (out) FQ_HIP_HP(hipMemcpyAsync(out, b->raw + skip, len, hipMemcpyDeviceToHost, st));
  if (recs_out) FQ_HIP_HP(hipMemcpyAsync(recs_out, b->recs + first, n_out * sizeof(fqgpu_rec), hipMemcpyDeviceToHost, st));
  FQ_HIP_HP(hipStreamSynchronize(st));
  for (size_t i = 0; recs_out && skip && i < n_out; i++) {
    recs_out[i].seq_off -= (uint32_t)skip;
    if (!s.seq_only) recs_out[i].qual_off -= (uint32_t)skip;  // (a FASTA record has no quality line: 0)
  }
  b->host_result = *ctx->hp_result;
  b->result_pulled = true;
  const int verdict = b->host_result.s[0].bad_symbol || b->host_result.s[1].bad_symbol ? FQGPU_E_ARG
                      : b->host_result.s[0].corrupt || b->host_result.s[1].corrupt     ? FQGPU_E_CORRUPT
                                                                                         : FQGPU_OK;
  if (s.build_index) {
    if (verdict) b->index_bytes[0] = b->index_bytes[1] = 0;
    ctx->hp.index_built = !verdict;
  }
  if (!verdict && !plan && !s.seq_only) {  // a whole block, restored: fqgpu_chunk_crc32 may digest it
    ctx->hp.crc_what = 2;
    ctx->hp.crc_len = b->raw_len;
  }
  return verdict;
}

static int hp_decode(fqgpu_ctx *ctx, const DecStreams &s, const fqgpu_rec *recs, size_t n_recs, uint8_t *raw_out, size_t raw_len) {
  if (ctx) ctx->hp.end_digest();  // (whatever becomes of this decode, the chunk before it is no longer what the handle answers for)
  if (!ctx || !s.ok() || !recs || !raw_out) return FQGPU_E_ARG;
  if (s.n_count_len < n_recs) return FQGPU_E_CORRUPT;
  int rc = use_device(ctx->device);
  if (rc) return rc;
  size_t n_bases = 0;
  if ((rc = check_recs(recs, n_recs, raw_len, &n_bases))) return rc;
  fqgpu_dblock *b = nullptr;
  if ((rc = hp_decode_acquire(ctx, raw_len, n_recs, n_bases, s, &b))) return rc;
  // raw_out holds the skeleton the first decode pass laid out (headers, newlines, '+')
  // everything on the handle's stream (the decode kernels run there too): no host wait in between
  hipStream_t st = ctx->stream;
  FQ_HIP_HP(hipMemcpyAsync(b->raw, raw_out, raw_len, hipMemcpyHostToDevice, st));
  FQ_HIP_HP(hipMemcpyAsync(b->recs, recs, n_recs * sizeof(fqgpu_rec), hipMemcpyHostToDevice, st));
  return hp_decode_staged(ctx, b, s, nullptr, raw_out, 0, raw_len, nullptr, 0, n_recs);
}

extern "C" int fqgpu_decode_block(fqgpu_ctx *ctx, const uint8_t *seq, size_t seq_len, const uint8_t *qual,
                                  size_t qual_len, const uint16_t *n_count, size_t n_count_len,
                                  const uint16_t *n_pos, size_t n_pos_len, const fqgpu_rec *recs,
                                  size_t n_recs, uint8_t *raw_out, size_t raw_len) {
  return hp_decode(ctx, {seq, seq_len, qual, qual_len, n_count, n_count_len, n_pos, n_pos_len, {nullptr, nullptr}, {0, 0}}, recs, n_recs,
                   raw_out, raw_len);
}

// The same with the decode index the block's encode left (FQGPU_F_DECODE_INDEX, fqgpu_encode_index): each stream is
// decoded from every snapshot at once instead of by one lane from its end.
extern "C" int fqgpu_decode_block_indexed(fqgpu_ctx *ctx, const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                                          const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                                          const fqgpu_rec *recs, size_t n_recs, uint8_t *raw_out, size_t raw_len,
                                          const uint8_t *seq_index, size_t seq_index_len, const uint8_t *qual_index, size_t qual_index_len) {
  return hp_decode(ctx, {seq, seq_len, qual, qual_len, n_count, n_count_len, n_pos, n_pos_len, {seq_index, qual_index},
                         {seq_index_len, qual_index_len}},
                   recs, n_recs, raw_out, raw_len);
}

// The front of the chunk decodes: the arguments both refuse, the pass over readlens -- *n_bases and, rec_start != NULL, the
// encode index of every record's first symbol (n_recs + 1 entries) --, the header streams into the handle's stage.
static int chunk_front(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs, const DecStreams &s,
                       size_t raw_len, std::vector<uint32_t> *rec_start, size_t *n_bases) {
  if (!ctx || !hdr || !readlens || !n_recs || !s.ok() || (s.n_pos_len && !s.n_pos)) return FQGPU_E_ARG;
  if (raw_len >= ((size_t)1 << 32) || n_recs >= ((size_t)1 << 32)) return FQGPU_E_ARG;
  if (rec_start) rec_start->resize(n_recs + 1);
  size_t tot = 0;
  for (size_t r = 0; r < n_recs; r++) {
    if (readlens[r] < 3) return FQGPU_E_SHORT_READ;  // as check_recs
    if (rec_start) (*rec_start)[r] = (uint32_t)tot;
    tot += readlens[r];
  }
  if (tot >= 0xFFF00000ull) return FQGPU_E_ARG;
  if (rec_start) (*rec_start)[n_recs] = (uint32_t)tot;
  *n_bases = tot;
  const int rc = use_device(ctx->device);
  return rc ? rc : fq_chunk_prepare(hdr, readlens, n_recs, raw_len, ctx->hp_chunk);
}

// What the layout passes found, in the host decoder's order: the first record it throws on, then an n_count too short
static int layout_verdict(unsigned long long bad, unsigned long long total, size_t raw_len, size_t n_count_len, size_t n_recs,
                          size_t *bad_record) {
  if (bad != ~0ull) {  // (the decode kernels are never launched on a bad layout)
    *bad_record = (size_t)bad;
    return FQGPU_E_CORRUPT;
  }
  if (total > raw_len) return FQGPU_E_CORRUPT;  // (reported with its record above; kept as a guard)
  return n_count_len < n_recs ? FQGPU_E_CORRUPT : FQGPU_OK;
}

// Both passes of decodeChunk on the device (decode_headers.hip, then the decode above): only the side streams go up.
// s.build_index: by the indexing walk, raw_out may be NULL (nothing of the chunk comes back); so it may on a handle that only checks.
static int decode_chunk(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs, const DecStreams &s,
                        uint8_t *raw_out, size_t raw_len, fqgpu_rec *recs_out, size_t *laid_out_len, size_t *bad_record) {
  const size_t n_count_len = s.n_count_len;
  if (ctx) ctx->hp.end_digest(s.build_index);  // (as hp_decode: also a call that is refused for its arguments ends the last chunk's digest)
  if (bad_record) *bad_record = (size_t)-1;
  if (laid_out_len) *laid_out_len = 0;
  if ((!raw_out && !s.build_index && !(ctx && ctx->check_only)) || !laid_out_len || !bad_record) return FQGPU_E_ARG;
  size_t n_bases = 0;
  int rc = chunk_front(ctx, hdr, readlens, n_recs, s, raw_len, nullptr, &n_bases);
  if (rc) return rc;
  fqgpu_dblock *b = nullptr;
  if ((rc = hp_decode_acquire(ctx, raw_len, n_recs, n_bases, s, &b))) return rc;
  unsigned long long bad = 0, total = 0;
  if ((rc = fq_chunk_layout(ctx->stream, ctx->hp_chunk, b->raw, b->recs, nullptr, true, &bad, &total, nullptr))) return hp_fail(ctx, rc);
  if ((rc = layout_verdict(bad, total, raw_len, n_count_len, n_recs, bad_record))) return rc;
  *laid_out_len = (size_t)total;
  if (total < raw_len) FQ_HIP_HP(hipMemsetAsync(b->raw + total, 0, raw_len - total, ctx->stream));
  rc = hp_decode_staged(ctx, b, s, nullptr, raw_out, 0, raw_len, recs_out, 0, n_recs);
  if (!rc) ctx->hp.crc_len = (size_t)total;  // (zeros behind the last record are no part of the chunk)
  return rc;
}

extern "C" int fqgpu_decode_chunk(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                                  const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                                  const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                                  const uint8_t *seq_index, size_t seq_index_len, const uint8_t *qual_index, size_t qual_index_len,
                                  uint8_t *raw_out, size_t raw_len, fqgpu_rec *recs_out, size_t *laid_out_len, size_t *bad_record) {
  return decode_chunk(ctx, hdr, readlens, n_recs, {seq, seq_len, qual, qual_len, n_count, n_count_len, n_pos, n_pos_len,
                                                   {seq_index, qual_index}, {seq_index_len, qual_index_len}},
                      raw_out, raw_len, recs_out, laid_out_len, bad_record);
}

// fqgpu_decode_chunk from the streams alone, by the indexing walk: the chunk's decode indexes stay on the staging block
// for fqgpu_decode_index.
extern "C" int fqgpu_decode_chunk_indexing(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                                           const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                                           const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                                           uint8_t *raw_out, size_t raw_len, fqgpu_rec *recs_out, size_t *laid_out_len,
                                           size_t *bad_record) {
  return decode_chunk(ctx, hdr, readlens, n_recs, {seq, seq_len, qual, qual_len, n_count, n_count_len, n_pos, n_pos_len,
                                                   {nullptr, nullptr}, {0, 0}, true},
                      raw_out, raw_len, recs_out, laid_out_len, bad_record);
}

// The decode index fqgpu_decode_chunk_indexing built, until the handle's next host-pointer call.
extern "C" int fqgpu_decode_index(fqgpu_ctx *ctx, int stream, uint8_t *out, size_t cap, size_t *len) {
  if (len) *len = 0;
  if (!ctx || !ctx->hp.block || stream < 0 || stream > 1 || !len || !ctx->hp.index_built) return FQGPU_E_ARG;
  hipError_t he;
  int rc = hp_index_fetch(ctx, stream, out, cap, len, nullptr, &he);
  if (!rc && he != hipSuccess) rc = FQGPU_E_HIP;
  if (rc) *len = 0;
  return rc;
}

// fqgpu_decode_chunk_range's plan for the records [first, end) of a chunk.  rs: rec_start (n + 1 entries, strictly
// increasing: every read has 3 bases or more).  With both decode indexes (ix != NULL, each with a snapshot) stream s
// decodes its strides k_lo[s] .. k_hi[s] -- the ones that hold a symbol of [rs[first], rs[end]), the rule of
// fq_decode_launch -- and [w0, w1) are the records those strides write to: a stride of encode indices [e_lo, e_hi) walks
// from the record of symbol e_hi - 1 down to the record of symbol e_lo.  Without (*indexed = false), the window is the
// whole chunk and the streams are walked whole.  n_streams = 1: the sequence stream alone, by its index alone.
static FqStridePlan range_plan(const uint32_t *rs, size_t n, size_t first, size_t end, const FqIndexHeader *ix, int n_streams,
                               bool *indexed) {
  FqStridePlan p = {{0, 0}, {0, 0}, 0, (unsigned)n, rs};
  *indexed = ix && ix[0].n_snap && (n_streams < 2 || ix[1].n_snap);
  if (!*indexed) return p;
  const auto record_of = [&](uint64_t e) { return (size_t)(std::upper_bound(rs, rs + n, (uint32_t)e) - rs) - 1; };
  const uint64_t s0 = rs[first], s1 = rs[end];
  uint64_t lo = s0, hi = s1;
  for (int s = 0; s < n_streams; s++) {
    const uint64_t stride = ix[s].stride;
    p.k_lo[s] = (unsigned)(s0 / stride);
    p.k_hi[s] = (unsigned)((s1 - 1) / stride);
    lo = std::min(lo, p.k_lo[s] * stride);
    hi = std::max(hi, std::min<uint64_t>((p.k_hi[s] + 1) * stride, ix[s].n_sym));
  }
  p.w0 = (unsigned)record_of(lo);
  p.w1 = (unsigned)record_of(hi - 1) + 1;
  return p;
}

// Records [first, end) of a chunk (include/fqgpu.h): the layout passes of fqgpu_decode_chunk over the whole chunk, the
// write pass for a window of records, the walk over the strides that hold the range (or over the whole streams), the
// N pass for the window, and the range's bytes and record table back.  s.seq_only: the same with FASTA records and the
// sequence stream alone.
static int decode_chunk_range(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                              const DecStreams &s, size_t raw_len, size_t first, size_t end, uint8_t *out, size_t out_cap,
                              size_t *out_len, fqgpu_rec *recs_out, size_t *bad_record) {
  const size_t n_count_len = s.n_count_len;
  if (bad_record) *bad_record = (size_t)-1;
  if (out_len) *out_len = 0;
  if (ctx) ctx->hp.end_digest();  // (a range is never digested)
  if (!out_len || !bad_record || first >= end || end > n_recs) return FQGPU_E_ARG;
  std::vector<uint32_t> rs;
  size_t n_bases = 0;
  int rc = chunk_front(ctx, hdr, readlens, n_recs, s, raw_len, &rs, &n_bases);
  if (rc) return rc;
  // (a damaged index is reported as fqgpu_decode_chunk reports it: behind the layout's verdict)
  FqIndexHeader ix[2];
  int index_rc = FQGPU_OK;
  bool have_index = true;
  for (int k = 0; k < s.n_streams(); k++) {
    if (s.index_len[k] && (rc = index_header(k, n_bases, s.index[k], s.index_len[k], &ix[k])) && !index_rc) index_rc = rc;
    have_index = have_index && s.index_len[k];
  }
  bool indexed;
  const FqStridePlan plan = range_plan(rs.data(), n_recs, first, end, !index_rc && have_index ? ix : nullptr, s.n_streams(), &indexed);
  // the size query has no staging block: nothing is written, nothing goes up
  fqgpu_dblock *b = nullptr;
  if ((rc = out ? hp_decode_acquire(ctx, raw_len, n_recs, n_bases, s, &b) : fqgpu_sync(ctx))) return rc;
  const unsigned q[4] = {plan.w0, (unsigned)first, (unsigned)end, plan.w1};
  unsigned long long bad = 0, total = 0, at[4];
  if ((rc = fq_chunk_layout(ctx->stream, ctx->hp_chunk, b ? b->raw : nullptr, b ? b->recs : nullptr, q, b != nullptr, &bad, &total, at,
                            s.seq_only)))
    return hp_fail(ctx, rc);
  if ((rc = layout_verdict(bad, total, raw_len, n_count_len, n_recs, bad_record))) return rc;
  if (index_rc) return index_rc;
  const size_t len = (size_t)(at[2] - at[1]), skip = (size_t)(at[1] - at[0]);  // the range's bytes, where they start in the window
  *out_len = len;
  if (!out) return FQGPU_OK;
  if (out_cap < len) return FQGPU_E_OVERFLOW;
  rc = hp_decode_staged(ctx, b, s, indexed ? &plan : nullptr, out, skip, len, recs_out, first, end - first);
  ctx->hp.end_digest();  // (without indexes the whole chunk was decoded; it still is a range that was asked for)
  return rc;
}

extern "C" int fqgpu_decode_chunk_range(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                                        const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                                        const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                                        const uint8_t *seq_index, size_t seq_index_len, const uint8_t *qual_index,
                                        size_t qual_index_len, size_t raw_len, size_t first, size_t end, uint8_t *out, size_t out_cap,
                                        size_t *out_len, fqgpu_rec *recs_out, size_t *bad_record) {
  return decode_chunk_range(ctx, hdr, readlens, n_recs, {seq, seq_len, qual, qual_len, n_count, n_count_len, n_pos, n_pos_len,
                                                         {seq_index, qual_index}, {seq_index_len, qual_index_len}},
                            raw_len, first, end, out, out_cap, out_len, recs_out, bad_record);
}

// The same range as FASTA, from the sequence stream alone (include/fqgpu.h): the chunk is judged on its FASTQ layout, the
// records are placed as ">hdr\nSEQ\n", and no quality byte is asked for, uploaded or decoded.
extern "C" int fqgpu_decode_chunk_fasta(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                                        const uint8_t *seq, size_t seq_len, const uint16_t *n_count, size_t n_count_len,
                                        const uint16_t *n_pos, size_t n_pos_len, const uint8_t *seq_index, size_t seq_index_len,
                                        size_t raw_len, size_t first, size_t end, uint8_t *out, size_t out_cap, size_t *out_len,
                                        fqgpu_rec *recs_out, size_t *bad_record) {
  if (bad_record) *bad_record = (size_t)-1;
  if (out_len) *out_len = 0;
  if (const int rc = use_device(ctx ? ctx->device : 0)) return rc;  // (no device: said before any argument is looked at)
  return decode_chunk_range(ctx, hdr, readlens, n_recs, {seq, seq_len, nullptr, 0, n_count, n_count_len, n_pos, n_pos_len,
                                                         {seq_index, nullptr}, {seq_index_len, 0}, false, true},
                            raw_len, first, end, out, out_cap, out_len, recs_out, bad_record);
}

// ------------------------------------------------------------------ CRC-32 of a chunk in HBM (crc.hip)
extern "C" int fqgpu_ctx_set_check_only(fqgpu_ctx *ctx, int on) {
  if (!ctx) return FQGPU_E_ARG;
  ctx->check_only = on != 0;
  return FQGPU_OK;
}

// The two fronts of the calls on a chunk in HBM (digest, summary, filter, trim), behind their argument checks.
// The chunk on the staging block, on the handle's copy stream: the chunk in flight arrived there and its record table was
// uploaded or built there, so the call runs beside the lane's encode kernels and waits for none of them; after a decode
// the stream is idle.  FQGPU_E_ARG: no chunk there.
static int staged_block(const fqgpu_ctx *ctx, const fqgpu_dblock **b) {
  if (!ctx->hp.block || !ctx->hp.crc_what) return FQGPU_E_ARG;
  *b = ctx->hp.block;
  return FQGPU_OK;
}

// A caller's block behind its last operation, which may still write its raw block (a decode, an encode with
// FQGPU_F_WRITE_BACK_N).  FQGPU_E_ARG: no block, or one of another device.
static int settled_block(fqgpu_ctx *ctx, const fqgpu_dblock *b) {
  if (!b || b->device != ctx->device) return FQGPU_E_ARG;
  int rc;
  if ((rc = fqgpu_sync(ctx)) || (b->owner && b->owner != ctx && (rc = fqgpu_sync(b->owner)))) return rc;
  return FQGPU_OK;
}

// What the drivers take (FqChunkView): a block's whole chunk, or `count` of its records from `first` on.  FQGPU_E_ARG: no
// record, or a range that does not lie inside the table.
static FqChunkView chunk_view(const fqgpu_dblock *b) { return {b->raw, b->raw_len, b->recs, b->n_recs, false}; }
static int range_view(const fqgpu_dblock *b, size_t first, size_t count, FqChunkView *v) {
  if (count == 0 || first >= b->n_recs || count > b->n_recs - first) return FQGPU_E_ARG;  // (no sum that could overflow)
  *v = {b->raw, b->raw_len, b->recs + first, count, first != 0};
  return FQGPU_OK;
}

extern "C" int fqgpu_chunk_crc32(fqgpu_ctx *ctx, uint32_t *crc, size_t *len) {
  if (crc) *crc = 0;
  if (len) *len = 0;
  int rc = use_device(ctx ? ctx->device : 0);
  if (rc) return rc;
  const fqgpu_dblock *b = nullptr;
  if (!ctx || !crc || !len) return FQGPU_E_ARG;
  if ((rc = staged_block(ctx, &b))) return rc;
  uint32_t c = 0;
  size_t n = ctx->hp.crc_len;
  rc = ctx->hp.crc_what == 1 ? fq_crc_canonical(ctx, ctx->stream, chunk_view(b), &c, &n)
                             : fq_crc_bytes(ctx, ctx->stream, b->raw, n, &c);
  if (rc) return rc;
  *crc = c;
  *len = n;
  return FQGPU_OK;
}

extern "C" int fqgpu_dblock_crc32(fqgpu_ctx *ctx, const fqgpu_dblock *b, uint32_t *crc, size_t *len) {
  if (crc) *crc = 0;
  if (len) *len = 0;
  int rc = use_device(ctx ? ctx->device : 0);
  if (rc) return rc;
  if (!ctx || !crc || !len) return FQGPU_E_ARG;
  if ((rc = settled_block(ctx, b))) return rc;
  uint32_t c = 0;
  size_t n = 0;
  if ((rc = fq_crc_canonical(ctx, ctx->stream, chunk_view(b), &c, &n))) return rc;
  *crc = c;
  *len = n;
  return FQGPU_OK;
}

// ------------------------------------------------------------------ read summary of a chunk in HBM (stats.hip)
// The two calls (b: the caller's block; staged: the chunk on the staging block): no device is said before any argument is
// looked at; an `out` that is large enough is zeroed before anything else can fail.
static int stats_call(fqgpu_ctx *ctx, const fqgpu_dblock *b, bool staged, unsigned positions, uint64_t *out, size_t cap_words) {
  if (const int rc = use_device(ctx ? ctx->device : 0)) return rc;
  const size_t words = fqgpu_stats_words(positions);
  if (!ctx || !out || !words) return FQGPU_E_ARG;
  if (cap_words < words) return FQGPU_E_OVERFLOW;
  memset(out, 0, words * sizeof(uint64_t));
  if (const int rc = staged ? staged_block(ctx, &b) : settled_block(ctx, b)) return rc;
  return fq_stats_chunk(ctx, ctx->stream, chunk_view(b), positions, out);
}

extern "C" int fqgpu_chunk_stats(fqgpu_ctx *ctx, unsigned positions, uint64_t *out, size_t cap_words) {
  return stats_call(ctx, nullptr, true, positions, out, cap_words);
}

extern "C" int fqgpu_dblock_stats(fqgpu_ctx *ctx, const fqgpu_dblock *b, unsigned positions, uint64_t *out, size_t cap_words) {
  return stats_call(ctx, b, false, positions, out, cap_words);
}

// ------------------------------------------------------------------ adapter content of a chunk in HBM (select.hip)
// The two calls (b, staged: as stats_call): no device is said before any argument is looked at; an `out` that is large
// enough is zeroed before anything else can fail.
static int probe_call(fqgpu_ctx *ctx, const fqgpu_dblock *b, bool staged, const fqgpu_probes *p, unsigned positions, uint64_t *out,
                      size_t cap_words, uint16_t *places_out) {
  if (const int rc = use_device(ctx ? ctx->device : 0)) return rc;
  if (!ctx || !out || fqgpu_probes_check(p) != FQGPU_OK) return FQGPU_E_ARG;
  const size_t words = fqgpu_probe_words(p->n, positions);
  if (!words) return FQGPU_E_ARG;
  if (cap_words < words) return FQGPU_E_OVERFLOW;
  memset(out, 0, words * sizeof(uint64_t));
  if (const int rc = staged ? staged_block(ctx, &b) : settled_block(ctx, b)) return rc;
  return fq_probe_chunk(ctx, ctx->stream, chunk_view(b), p, positions, out, places_out);
}

extern "C" int fqgpu_chunk_probe(fqgpu_ctx *ctx, const fqgpu_probes *p, unsigned positions, uint64_t *out, size_t cap_words,
                                 uint16_t *places_out) {
  return probe_call(ctx, nullptr, true, p, positions, out, cap_words, places_out);
}

extern "C" int fqgpu_dblock_probe(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_probes *p, unsigned positions, uint64_t *out,
                                  size_t cap_words, uint16_t *places_out) {
  return probe_call(ctx, b, false, p, positions, out, cap_words, places_out);
}

// ------------------------------------------------------------------ the selection: the reads of a chunk in HBM clipped, trimmed, judged, marked, limited (select.hip)
// THE front of the twelve selection calls (b, staged: as stats_call), and the order of what a caller can observe:
//   1. no device is said before any argument is looked at;
//   2. *out_len and the report are zeroed before anything else can fail;
//   3. the specs are checked, FQGPU_E_ARG;
//   4. the chunk is found, staged or settled;
//   5. a family with a range checks [first, end) against the table.
// Between 3 and 4 the job is NORMALISED, so that fq_select_chunk looks at none of this again: a NULL trim beside an adapter, a
// tail or a range is one that cuts nothing, a NULL filter one that keeps everything; a tail that is NULL or has both rules
// off is no tail -- the clip's kernels, words 16 .. 19 zero -- unless the places are asked for: then k_tail_find runs with
// nothing to do, and the results are the clip's all the same; the windows go with the trim and the places with the tail.
struct SelectFamily {
  bool need_trim, need_filter;  // a NULL one is refused (a filter call has no trim at all, and takes none)
  bool range;                   // the records [first, end) of the table, handed to the driver as a table of their own
};
constexpr SelectFamily kFilterCall = {false, true, false}, kTrimCall = {true, false, false}, kRangeCall = {false, false, true};

static int select_call(fqgpu_ctx *ctx, const fqgpu_dblock *b, bool staged, const SelectFamily &fam, FqSelectJob job, size_t first, size_t end,
                       FqSelectOut o) {
  if (const int rc = use_device(ctx ? ctx->device : 0)) return rc;
  if (o.out_len) *o.out_len = 0;
  if (o.report) memset(o.report, 0, o.report_words * sizeof(uint64_t));
  static const fqgpu_trim none = {0u, 0u, 0u, 0u, FQGPU_FILTER_NONE, {0u, 0u, 0u}};
  static const fqgpu_tail off = {0u, 0u, 0u, 0u, 0u, 0u, {0u, 0u}};
  static const fqgpu_filter all = {0u, FQGPU_FILTER_NONE, FQGPU_FILTER_NONE, 0u, 0u, 0u, {0u, 0u}};
  if (job.tail && fqgpu_tail_check(job.tail) != FQGPU_OK) return FQGPU_E_ARG;
  if (!job.tail || !(job.tail->poly_bases || job.tail->window_len)) job.tail = o.places && (job.adapter || job.trim || fam.range) ? &off : nullptr;
  if ((job.adapter || job.tail || fam.range) && !job.trim) job.trim = &none;
  if (!ctx || !o.out_len || !o.report || (job.adapter && fqgpu_adapter_check(job.adapter) != FQGPU_OK) ||
      ((job.trim || fam.need_trim) && fqgpu_trim_check(job.trim) != FQGPU_OK) ||
      ((job.filter || fam.need_filter) && fqgpu_filter_check(job.filter) != FQGPU_OK))
    return FQGPU_E_ARG;
  if (!job.filter) job.filter = &all;
  if (!job.trim) o.win = nullptr;
  if (!job.tail) o.places = nullptr;
  job.span = fam.range ? "select_marked" : job.tail ? "tailtrim" : job.adapter ? "clip" : job.trim ? "trim" : "filter";
  if (const int rc = staged ? staged_block(ctx, &b) : settled_block(ctx, b)) return rc;
  FqChunkView v = chunk_view(b);
  if (fam.range && (first >= end || range_view(b, first, end - first, &v) != FQGPU_OK)) return FQGPU_E_ARG;
  return fq_select_chunk(ctx, ctx->stream, v, job, o);
}

extern "C" int fqgpu_chunk_filter(fqgpu_ctx *ctx, const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len,
                                  uint64_t *report, uint8_t *keep_out) {
  return select_call(ctx, nullptr, true, kFilterCall, {nullptr, nullptr, nullptr, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_FILTER_REPORT_WORDS, keep_out});
}

extern "C" int fqgpu_dblock_filter(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_filter *f, uint8_t *out, size_t out_cap,
                                   size_t *out_len, uint64_t *report, uint8_t *keep_out) {
  return select_call(ctx, b, false, kFilterCall, {nullptr, nullptr, nullptr, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_FILTER_REPORT_WORDS, keep_out});
}

extern "C" int fqgpu_chunk_trim(fqgpu_ctx *ctx, const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len,
                                uint64_t *report, uint8_t *keep_out, uint32_t *win_out) {
  return select_call(ctx, nullptr, true, kTrimCall, {nullptr, nullptr, t, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_TRIM_REPORT_WORDS, keep_out, win_out});
}

extern "C" int fqgpu_dblock_trim(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out,
                                 size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out) {
  return select_call(ctx, b, false, kTrimCall, {nullptr, nullptr, t, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_TRIM_REPORT_WORDS, keep_out, win_out});
}

// (a clip call without an adapter is the trim call)
extern "C" int fqgpu_chunk_clip(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out,
                                size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out) {
  return select_call(ctx, nullptr, true, kTrimCall, {a, nullptr, t, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_TRIM_REPORT_WORDS, keep_out, win_out});
}

extern "C" int fqgpu_dblock_clip(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_trim *t, const fqgpu_filter *f,
                                 uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out) {
  return select_call(ctx, b, false, kTrimCall, {a, nullptr, t, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_TRIM_REPORT_WORDS, keep_out, win_out});
}

extern "C" int fqgpu_chunk_tailtrim(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t, const fqgpu_filter *f,
                                    uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out,
                                    uint16_t *places_out) {
  return select_call(ctx, nullptr, true, kTrimCall, {a, x, t, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_TAIL_REPORT_WORDS, keep_out, win_out, places_out});
}

extern "C" int fqgpu_dblock_tailtrim(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t,
                                     const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report,
                                     uint8_t *keep_out, uint32_t *win_out, uint16_t *places_out) {
  return select_call(ctx, b, false, kTrimCall, {a, x, t, f}, 0, 0,
                     {out, out_cap, out_len, report, FQGPU_TAIL_REPORT_WORDS, keep_out, win_out, places_out});
}

// The marked and the limited calls (a paired restore's selection): every one of a, x, t, f may be NULL; the range's mark and
// its per-record limits (the limited calls'; k_select_limit) travel in the job.
extern "C" int fqgpu_chunk_select_marked(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t, const fqgpu_filter *f,
                                         size_t first, size_t end, const uint8_t *mark_in, uint8_t *out, size_t out_cap, size_t *out_len,
                                         uint64_t *report, uint8_t *keep_out, uint32_t *win_out, uint16_t *places_out) {
  return select_call(ctx, nullptr, true, kRangeCall, {a, x, t, f, mark_in}, first, end,
                     {out, out_cap, out_len, report, FQGPU_TAIL_REPORT_WORDS, keep_out, win_out, places_out});
}

extern "C" int fqgpu_dblock_select_marked(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t,
                                          const fqgpu_filter *f, size_t first, size_t end, const uint8_t *mark_in, uint8_t *out, size_t out_cap,
                                          size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out, uint16_t *places_out) {
  return select_call(ctx, b, false, kRangeCall, {a, x, t, f, mark_in}, first, end,
                     {out, out_cap, out_len, report, FQGPU_TAIL_REPORT_WORDS, keep_out, win_out, places_out});
}

extern "C" int fqgpu_chunk_select_limited(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t, const fqgpu_filter *f,
                                          size_t first, size_t end, const uint8_t *mark_in, const uint16_t *limit_in, uint8_t *out,
                                          size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out,
                                          uint16_t *places_out) {
  return select_call(ctx, nullptr, true, kRangeCall, {a, x, t, f, mark_in, limit_in}, first, end,
                     {out, out_cap, out_len, report, FQGPU_TAIL_REPORT_WORDS, keep_out, win_out, places_out});
}

extern "C" int fqgpu_dblock_select_limited(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t,
                                           const fqgpu_filter *f, size_t first, size_t end, const uint8_t *mark_in, const uint16_t *limit_in,
                                           uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out,
                                           uint32_t *win_out, uint16_t *places_out) {
  return select_call(ctx, b, false, kRangeCall, {a, x, t, f, mark_in, limit_in}, first, end,
                     {out, out_cap, out_len, report, FQGPU_TAIL_REPORT_WORDS, keep_out, win_out, places_out});
}

// ------------------------------------------------------------------ the calls on two chunks in HBM (pair.hip)
// The two sides of a pair call at rest, as views of `count` records from first_a and first_b on; every call below goes through
// here, behind its own argument checks (no device is said before any argument is looked at, then what the call zeroes, then
// its specs, FQGPU_E_ARG).  staged: the chunks staged on the two handles -- both non-NULL, on one device, each with a chunk
// --, every stream of both waited for; else two blocks of ctx_a's device, each settled: ctx_a's streams and its owner's waited
// for.  Then the ranges against the tables.  distinct: the sides must be two chunks -- the calls that CHANGE them.  One
// kernel on ctx_a's stream follows.  Every FQGPU_E_ARG of a call, from here or from its driver, leaves the call's report as
// it was zeroed and its per-pair arrays zeroed, and the correcting calls' chunks untouched.
static int pair_sides(bool staged, fqgpu_ctx *ctx_a, fqgpu_ctx *ctx_b, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb,
                      size_t first_b, size_t count, bool distinct, FqChunkView *a, FqChunkView *b) {
  int rc;
  if (staged) {
    if (!ctx_b || (distinct && ctx_a == ctx_b) || ctx_a->device != ctx_b->device) return FQGPU_E_ARG;
    if ((rc = staged_block(ctx_a, &ba)) || (rc = staged_block(ctx_b, &bb)) || (rc = fqgpu_sync(ctx_a)) || (rc = fqgpu_sync(ctx_b))) return rc;
  } else {
    if (distinct && ba == bb) return FQGPU_E_ARG;
    if ((rc = settled_block(ctx_a, ba)) || (rc = settled_block(ctx_a, bb))) return rc;
  }
  if ((rc = range_view(ba, first_a, count, a)) || (rc = range_view(bb, first_b, count, b))) return rc;
  return FQGPU_OK;
}
// the tail of a pair call: its per-pair arrays zeroed on FQGPU_E_ARG
static int pair_result(int rc, size_t count, std::initializer_list<uint16_t *> arrays) {
  if (rc == FQGPU_E_ARG && count)
    for (uint16_t *p : arrays)
      if (p) memset(p, 0, count * sizeof(uint16_t));
  return rc;
}

static int names_call(bool staged, fqgpu_ctx *ctx_a, fqgpu_ctx *ctx_b, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb,
                      size_t first_b, size_t count, size_t *mismatch) {
  if (mismatch) *mismatch = (size_t)-1;
  if (const int rc = use_device(ctx_a ? ctx_a->device : 0)) return rc;
  if (!ctx_a || !mismatch) return FQGPU_E_ARG;
  FqChunkView a, b;
  if (const int rc = pair_sides(staged, ctx_a, ctx_b, ba, first_a, bb, first_b, count, false, &a, &b)) return rc;
  return fq_pair_names(ctx_a, ctx_a->stream, a, b, mismatch);
}

extern "C" int fqgpu_chunk_pair_names(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, size_t *mismatch) {
  return names_call(true, ctx_a, ctx_b, nullptr, first_a, nullptr, first_b, count, mismatch);
}

extern "C" int fqgpu_dblock_pair_names(fqgpu_ctx *ctx, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b,
                                       size_t count, size_t *mismatch) {
  return names_call(false, ctx, nullptr, ba, first_a, bb, first_b, count, mismatch);
}

// The overlap calls: too little room is said before anything is written.
static int overlap_call(bool staged, fqgpu_ctx *ctx_a, fqgpu_ctx *ctx_b, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b,
                        size_t count, const fqgpu_overlap *o, uint64_t *out, size_t cap_words, uint16_t *limit_a_out, uint16_t *limit_b_out,
                        uint16_t *insert_out) {
  if (const int rc = use_device(ctx_a ? ctx_a->device : 0)) return rc;
  if (out && cap_words < FQGPU_OVERLAP_WORDS) return FQGPU_E_OVERFLOW;
  const auto run = [&]() -> int {
    if (!out) return FQGPU_E_ARG;
    memset(out, 0, FQGPU_OVERLAP_WORDS * sizeof(uint64_t));
    if (!ctx_a || fqgpu_overlap_check(o) != FQGPU_OK) return FQGPU_E_ARG;
    FqChunkView a, b;
    if (const int rc = pair_sides(staged, ctx_a, ctx_b, ba, first_a, bb, first_b, count, false, &a, &b)) return rc;
    return fq_pair_overlap(ctx_a, ctx_a->stream, a, b, o, out, limit_a_out, limit_b_out, insert_out);
  };
  return pair_result(run(), count, {limit_a_out, limit_b_out, insert_out});
}

extern "C" int fqgpu_chunk_pair_overlap(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, const fqgpu_overlap *o,
                                        uint64_t *out, size_t cap_words, uint16_t *limit_a_out, uint16_t *limit_b_out, uint16_t *insert_out) {
  return overlap_call(true, ctx_a, ctx_b, nullptr, first_a, nullptr, first_b, count, o, out, cap_words, limit_a_out, limit_b_out, insert_out);
}

extern "C" int fqgpu_dblock_pair_overlap(fqgpu_ctx *ctx, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b,
                                         size_t count, const fqgpu_overlap *o, uint64_t *out, size_t cap_words, uint16_t *limit_a_out,
                                         uint16_t *limit_b_out, uint16_t *insert_out) {
  return overlap_call(false, ctx, nullptr, ba, first_a, bb, first_b, count, o, out, cap_words, limit_a_out, limit_b_out, insert_out);
}

// The correcting calls: the two sides must be two chunks, for these calls CHANGE them (pair.hip, k_pair_correct).
static int correct_call(bool staged, fqgpu_ctx *ctx_a, fqgpu_ctx *ctx_b, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b,
                        size_t count, const uint16_t *insert_in, const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out,
                        uint16_t *fixed_b_out) {
  if (const int rc = use_device(ctx_a ? ctx_a->device : 0)) return rc;
  const auto run = [&]() -> int {
    if (!report) return FQGPU_E_ARG;
    memset(report, 0, FQGPU_CORRECT_REPORT_WORDS * sizeof(uint64_t));
    if (!ctx_a || !insert_in || fqgpu_correct_check(c) != FQGPU_OK) return FQGPU_E_ARG;
    FqChunkView a, b;
    if (const int rc = pair_sides(staged, ctx_a, ctx_b, ba, first_a, bb, first_b, count, true, &a, &b)) return rc;
    return fq_pair_correct(ctx_a, ctx_a->stream, a, b, insert_in, c, report, fixed_a_out, fixed_b_out);
  };
  return pair_result(run(), count, {fixed_a_out, fixed_b_out});
}

extern "C" int fqgpu_chunk_pair_correct(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, const uint16_t *insert_in,
                                        const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out, uint16_t *fixed_b_out) {
  return correct_call(true, ctx_a, ctx_b, nullptr, first_a, nullptr, first_b, count, insert_in, c, report, fixed_a_out, fixed_b_out);
}

extern "C" int fqgpu_dblock_pair_correct(fqgpu_ctx *ctx, fqgpu_dblock *ba, size_t first_a, fqgpu_dblock *bb, size_t first_b, size_t count,
                                         const uint16_t *insert_in, const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out,
                                         uint16_t *fixed_b_out) {
  return correct_call(false, ctx, nullptr, ba, first_a, bb, first_b, count, insert_in, c, report, fixed_a_out, fixed_b_out);
}

// The merging calls: nothing is patched, so the two sides may be one chunk.  `out` is written behind the verdict alone.
static int merge_call(bool staged, fqgpu_ctx *ctx_a, fqgpu_ctx *ctx_b, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b,
                      size_t count, const uint16_t *insert_in, const uint8_t *mark_in, const fqgpu_merge *m, uint8_t *out, size_t out_cap,
                      size_t *out_len, uint64_t *report, uint8_t *merged_out) {
  if (const int rc = use_device(ctx_a ? ctx_a->device : 0)) return rc;
  const auto run = [&]() -> int {
    if (!report || !out_len) return FQGPU_E_ARG;
    if (!ctx_a || !insert_in || fqgpu_merge_check(m) != FQGPU_OK) return FQGPU_E_ARG;
    FqChunkView a, b;
    if (const int rc = pair_sides(staged, ctx_a, ctx_b, ba, first_a, bb, first_b, count, false, &a, &b)) return rc;
    return fq_pair_merge(ctx_a, ctx_a->stream, a, b, insert_in, mark_in, m, out, out_cap, out_len, report, merged_out);
  };
  const int rc = run();
  if (rc == FQGPU_E_ARG) {
    if (out_len) *out_len = 0;
    if (report) memset(report, 0, FQGPU_MERGE_REPORT_WORDS * sizeof(uint64_t));
    if (merged_out && count) memset(merged_out, 0, (count + 7) / 8);
  }
  return rc;
}

extern "C" int fqgpu_chunk_pair_merge(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, const uint16_t *insert_in,
                                      const uint8_t *mark_in, const fqgpu_merge *m, uint8_t *out, size_t out_cap, size_t *out_len,
                                      uint64_t *report, uint8_t *merged_out) {
  return merge_call(true, ctx_a, ctx_b, nullptr, first_a, nullptr, first_b, count, insert_in, mark_in, m, out, out_cap, out_len, report, merged_out);
}

extern "C" int fqgpu_dblock_pair_merge(fqgpu_ctx *ctx, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b, size_t count,
                                       const uint16_t *insert_in, const uint8_t *mark_in, const fqgpu_merge *m, uint8_t *out, size_t out_cap,
                                       size_t *out_len, uint64_t *report, uint8_t *merged_out) {
  return merge_call(false, ctx, nullptr, ba, first_a, bb, first_b, count, insert_in, mark_in, m, out, out_cap, out_len, report, merged_out);
}
