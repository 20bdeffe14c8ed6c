/*
 * fqgpu.h -- C ABI of the MI355X-native FASTQ block entropy coder.
 *
 * This is the drop-in boundary for ONE hot path of iam28th/fqcomp28: the
 * per-block context-modelled FSE coding of bases and quality scores.  The
 * reference has no FFI layer; the seam is its block codec
 *     CompressionWorkspace::encodeChunk(FastqChunk&, CompressedBuffersDst&)    src/workspace.h:69
 *     DecompressionWorkspace::decodeChunk(FastqChunk&, CompressedBuffersSrc&)  src/workspace.h:112
 *     FSE_{Sequence,Quality}::calculateFreqTable(const FastqChunk&)            src/fse_sequence.h:72, src/fse_quality.h:50
 * and each entry point below names the reference code it replaces.  The C++
 * shim that keeps the reference's Workspace/CompressedBuffers surface on top of
 * this ABI is fqcomp28_amd/csrc/workspace.hpp; INTEGRATION.md shows the patch a
 * maintainer of the reference would apply.
 *
 * Conventions: plain pointers and sizes, little-endian integers, no exceptions
 * across the boundary; every function returns FQGPU_OK (0) or a negative
 * FQGPU_E_* code.  Pointers are HOST memory unless the name ends in _dev.
 * A handle is not re-entrant (like a reference Workspace, src/process.cpp:49-54);
 * different handles are independent and may live on different GPUs.
 * There is NO CPU fallback: every call fails with FQGPU_E_NO_DEVICE without a GPU.
 */
#ifndef FQGPU_H
#define FQGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQGPU_SEQ_MODELS 256   /* FSE_Sequence::N_MODELS,  src/fse_sequence.h:66 */
#define FQGPU_SEQ_ALPHA 4      /* FSE_Sequence::ALPHABET_SIZE, :36 */
#define FQGPU_QUAL_MODELS 8192 /* FSE_Quality::N_MODELS,   src/fse_quality.h:31 */
#define FQGPU_QUAL_ALPHA 64    /* FSE_Quality::ALPHABET_SIZE, :22 */
#define FQGPU_SEQ_FT_BYTES 3076     /* sizeof(FreqTable<256,4>),   src/fse_common.hpp:147-174 */
#define FQGPU_QUAL_FT_BYTES 1081348 /* sizeof(FreqTable<8192,64>) */

enum {
  FQGPU_OK = 0,
  FQGPU_E_OVERFLOW = -1,   /* stream does not fit the reference capacity rule: endChunk()==0, src/fse_common.hpp:85-90 */
  FQGPU_E_SHORT_READ = -2, /* a read shorter than 3: undefined in the reference (src/fse_quality.cpp:11-12) */
  FQGPU_E_CORRUPT = -3,    /* decode: end mark missing / stream not fully consumed (BIT_endOfDStream, src/fse_common.hpp:141) */
  FQGPU_E_ARG = -4,        /* bad argument, quality above Q63 (src/fse_quality.cpp:88 throws), a sequence byte that is
                            * neither A, C, G, T nor N (base2bits_arr holds UINT_MAX there, src/fse_sequence.cpp:6-14), bad table */
  FQGPU_E_NO_DEVICE = -5,  /* no usable GPU / HIP runtime error: the product path has no CPU fallback */
  FQGPU_E_NOMEM = -6,
  FQGPU_E_HIP = -7,
  FQGPU_E_HEADER = -8      /* a read header the field coder cannot code: a NUMERIC field without digits or outside int32, a
                            * changing STRING field of 255 or more bytes (asserts in the reference: src/headers.cpp:20,83,117) */
};

/* FastqRecord reduced to what this path needs (src/defs.h:22-32): byte offsets
 * of the sequence and quality lines inside the raw block, and their length. */
typedef struct {
  uint32_t seq_off, qual_off, len;
} fqgpu_rec;

typedef struct fqgpu_ctx fqgpu_ctx;

/* ---- lifecycle ------------------------------------------------------- */
int fqgpu_device_count(void);
const char *fqgpu_strerror(int code);
const char *fqgpu_version(void);

/* Workspace::compressBoundSequence / compressBoundQuality (src/workspace.h:21-35) */
size_t fqgpu_bound_seq(size_t total_bases);
size_t fqgpu_bound_qual(size_t total_bases);

/* ---- dataset analysis (replaces FSE_Sequence::calculateFreqTable
 * src/fse_sequence.cpp:145-169, FSE_Quality::calculateFreqTable
 * src/fse_quality.cpp:69-97 and makeNormalizedFreqTable src/fse_common.hpp:179-200).
 * Histograms the parsed sample block on the GPU and normalises every context
 * into the reference's FreqTable POD layout (what DatasetMeta dumps into the
 * archive, src/prepare.cpp:18-20).  seq_counts_out / qual_counts_out are
 * optional (NULL) dumps of the raw u32 counts [256][4] / [8192][64]. */
int fqgpu_freq_tables(int device, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs,
                      size_t n_recs, void *seq_ft_out, void *qual_ft_out,
                      uint32_t *seq_counts_out, uint32_t *qual_counts_out);
/* Same, from raw counts already on the host (normalisation only, on the GPU). */
int fqgpu_tables_from_counts(int device, const uint32_t *seq_counts, const uint32_t *qual_counts,
                             void *seq_ft_out, void *qual_ft_out);

/* ---- workspace (replaces the SequenceEncoder/QualityEncoder/…Decoder ctors,
 * src/fse_common.hpp:46-71,107-127: 256 + 8192 CTables and DTables are built on
 * the device from the FreqTable PODs).  One per (host thread, GPU). */
int fqgpu_ctx_create(int device, const void *seq_ft, const void *qual_ft, fqgpu_ctx **out);
void fqgpu_ctx_destroy(fqgpu_ctx *ctx);
/* Tuning knobs of the state-chain kernels; results never depend on them.
 * segment: nominal length, in symbols, of the pieces a context's chain is cut into at
 * single-state ("reset") symbols (0 keeps the default).  flags: FQGPU_CHAIN_SEQ_GENERIC
 * runs the sequence stream through the same reset-cut kernel instead of the segment-function
 * kernels (sequence tables have no single-state symbols: every chain is then walked by one lane). */
#define FQGPU_CHAIN_SEQ_GENERIC 1u
int fqgpu_ctx_set_chain_params(fqgpu_ctx *ctx, unsigned segment, unsigned flags);
/* Segment length, in symbols, of the sequence chain kernels: every chain is cut into segments
 * whose exact entry states come from per-segment state functions (0 = default: 4096, 2048 or 1024 by block size; rounded up
 * to a multiple of 1024).  Results never depend on it. */
int fqgpu_ctx_set_seq_segment(fqgpu_ctx *ctx, unsigned symbols);
/* A wave of the segment-function kernel walks up to max_segments consecutive segments in one go
 * (the state sets keep shrinking along the way; 1..16, 0 = default 8), as long as the chain still
 * splits into min_groups such groups (0 = default 16, the waves of a workgroup).  Results never
 * depend on it. */
int fqgpu_ctx_set_seq_group(fqgpu_ctx *ctx, unsigned max_segments, unsigned min_groups);
/* Hand-over of collapsed groups (tables of log <= 11): a wave of the segment-function kernel that is down to at most `cap`
 * distinct states behind the first `prefix_segments` segments of a group (0 = 1) leaves the rest of the group to a kernel
 * that walks one lane per remaining state.  cap 1..64; 0 hands nothing over.  Results never depend on it. */
int fqgpu_ctx_set_seq_handover(fqgpu_ctx *ctx, unsigned cap, unsigned prefix_segments);
/* Allocates now what blocks of up to this shape will need (staging block of the host-pointer calls,
 * scratch of every encode lane): a worker calls it while it builds its workspace, so that its
 * first block does not pay for the allocations.  Optional; everything grows on demand. */
int fqgpu_ctx_reserve(fqgpu_ctx *ctx, size_t raw_len, size_t n_recs, size_t n_bases);
/* Number of blocks the handle keeps in flight (encode lanes, 1..8; 0 = the default: four, six for
 * blocks of less than 48 M symbols): each fqgpu_dblock_encode goes to the next lane (own HIP streams
 * and scratch). */
int fqgpu_ctx_set_lanes(fqgpu_ctx *ctx, unsigned lanes);
/* Test hook: copies the device-built tables of one context out in zstd's memory
 * layout (FSE_CTable / FSE_DTable u32 words).  stream: 0 = sequence, 1 = quality. */
int fqgpu_ctx_dump_tables(fqgpu_ctx *ctx, int stream, unsigned model, uint32_t *ctable_out,
                          size_t ctable_cap_words, uint32_t *dtable_out, size_t dtable_cap_words);

/* ---- block encode (replaces the seq/qual part of
 * CompressionWorkspace::encodeChunk, src/workspace.cpp:14-45, i.e.
 * prepareBuffersForEncoding :159-174, startChunk, the per-record
 * replaceAndEncodeNs + SequenceEncoder::encodeRecord + QualityEncoder::encodeRecord
 * loop :25-31, and endChunk).  seq_out/qual_out receive bytes bit-identical to
 * cbs.seq / cbs.qual; readlens_out (n_recs u16) = cbs.readlens; n_count_out
 * (n_recs u16) and n_pos_out (one u16 per N) are what a FRESH CompressedBuffersDst
 * would hold.  seq_cap/qual_cap are the reference capacities (fqgpu_bound_*):
 * exceeding them returns FQGPU_E_OVERFLOW instead of the reference's silent 0.
 * flags: FQGPU_F_WRITE_BACK_N also rewrites N -> A inside `raw` like the reference. */
#define FQGPU_F_WRITE_BACK_N 1u
/* EXTENSION (not part of the reference format): the encode also leaves a
 * decode index per stream -- every `stride` symbols the bit position of the stream, the decoder
 * state of every context and the bytes the context model needs -- so that a decoder can start
 * in the middle of a block.  With both indexes present fqgpu_dblocks_decode runs one lane per
 * (block, stream, stride) instead of one per (block, stream); the streams themselves are the
 * reference's, byte for byte, with or without the index. */
#define FQGPU_F_DECODE_INDEX 2u
int fqgpu_encode_block(fqgpu_ctx *ctx, uint8_t *raw, size_t raw_len, const fqgpu_rec *recs,
                       size_t n_recs, uint8_t *seq_out, size_t seq_cap, size_t *seq_len,
                       uint8_t *qual_out, size_t qual_cap, size_t *qual_len,
                       uint16_t *readlens_out, uint16_t *n_count_out, uint16_t *n_pos_out,
                       size_t n_pos_cap, size_t *n_pos_len, unsigned flags);

/* The same encode in two halves, so that the caller can work while the GPU does (the shim's
 * encodeChunk codes the block's headers in between: src/workspace.cpp:25-31 does both in one
 * per-record loop), and with the record table built on the GPU when the caller has none:
 *   fqgpu_encode_begin    uploads the chunk (recs == NULL: finds its records on the device --
 *                         FastqReader::parseRecords, src/fastq_io.cpp:67-125, which the reference runs
 *                         under the reader mutex, :29-52 -- a trailing partial record is ignored),
 *                         starts the encode and returns; *used_len = bytes up to the last complete record
 *   fqgpu_encode_records  the record table of the block in flight (n_recs entries), without waiting
 *                         for the encode
 *   fqgpu_encode_wait     waits for the encode and reports the sizes of what it produced, so that the
 *                         caller can size its buffers exactly (optional)
 *   fqgpu_encode_end      waits, delivers exactly what fqgpu_encode_block delivers; `raw` may be NULL
 *                         (no N -> A write-back).  Capacities below the stream sizes: FQGPU_E_OVERFLOW.
 *   fqgpu_encode_cancel   drops the block in flight: waits until no copy or kernel of it touches the
 *                         caller's buffers any more (a caller that unwinds between begin and end calls
 *                         this before it lets go of the chunk and the stream buffers)
 * One block in flight per handle (a block begun and never ended is dropped by the next begin); every
 * other call on the handle waits for it. */
int fqgpu_encode_begin(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs, size_t n_recs,
                       unsigned flags, size_t *n_recs_out, size_t *n_bases_out, size_t *used_len);
int fqgpu_encode_records(fqgpu_ctx *ctx, fqgpu_rec *recs_out, size_t cap);
int fqgpu_encode_wait(fqgpu_ctx *ctx, size_t *seq_len, size_t *qual_len, size_t *n_pos_len);
int fqgpu_encode_cancel(fqgpu_ctx *ctx);
int fqgpu_encode_end(fqgpu_ctx *ctx, uint8_t *raw, uint8_t *seq_out, size_t seq_cap, size_t *seq_len,
                     uint8_t *qual_out, size_t qual_cap, size_t *qual_len, uint16_t *readlens_out,
                     uint16_t *n_count_out, uint16_t *n_pos_out, size_t n_pos_cap, size_t *n_pos_len);

/* ---- header fields of the block in flight, coded on the device (replaces the per-record calls of
 * CompressionWorkspace::encodeHeader, src/workspace.cpp:95-126, over FieldStorageDst::storeString /
 * storeNumeric, src/headers.cpp:76-91, 110-120).  The chunk is on the device already and every field is
 * coded against the SAME field of the header in front, which is input: all records at once.
 * Between fqgpu_encode_begin and fqgpu_encode_end / _cancel, in any order with _records / _wait:
 *   fqgpu_encode_headers_begin  field_types[i]: 0 = NUMERIC, 1 = STRING (headers::FieldType, src/headers.h:12);
 *                               separators[i] behind field i (n_fields - 1 of them): HeaderFormatSpeciciation,
 *                               src/headers.h:28-41; first_header: the dataset's first header, '@' included,
 *                               against which the chunk's first header is coded (Workspace::startNewChunk,
 *                               src/workspace.cpp:90-93).  Queues the work and returns.
 *   fqgpu_encode_headers_wait   sizes[i] = FieldStorage sizes of field i; *total_bytes = their sum.
 *                               FQGPU_E_HEADER: *bad_record = the first record whose header cannot be coded
 *   fqgpu_encode_headers_end    out: per field, in order, isDifferentFlag | content | contentLength, the bytes
 *                               the reference's FieldStorageDst holds after the chunk's last header */
#define FQGPU_HDR_MAX_FIELDS 64
typedef struct {
  uint32_t isDifferentFlag, content, contentLength;  /* = FieldStorage::sizes, src/headers.h:60-64 */
} fqgpu_field_sizes;
int fqgpu_encode_headers_begin(fqgpu_ctx *ctx, const uint8_t *field_types, const char *separators, unsigned n_fields,
                               const uint8_t *first_header, size_t first_header_len);
int fqgpu_encode_headers_wait(fqgpu_ctx *ctx, fqgpu_field_sizes *sizes, size_t *total_bytes, size_t *bad_record);
int fqgpu_encode_headers_end(fqgpu_ctx *ctx, uint8_t *out, size_t out_cap);

/* ---- block decode (replaces the second pass of
 * DecompressionWorkspace::decodeChunk, src/workspace.cpp:84-87:
 * SequenceDecoder::decodeRecord src/fse_sequence.cpp:114-143 and
 * QualityDecoder::decodeRecord src/fse_quality.cpp:55-67, records last->first).
 * raw_out is the block skeleton laid out by the first pass (:62-80); only the
 * sequence and quality line bytes are written. */
int fqgpu_decode_block(fqgpu_ctx *ctx, const uint8_t *seq, size_t seq_len, const uint8_t *qual,
                       size_t qual_len, const uint16_t *n_count, size_t n_count_len,
                       const uint16_t *n_pos, size_t n_pos_len, const fqgpu_rec *recs,
                       size_t n_recs, uint8_t *raw_out, size_t raw_len);
/* Extension (nothing in the reference): the same decode with the sidecar the block's encode left when it ran with
 * FQGPU_F_DECODE_INDEX -- fqgpu_encode_index(stream 0 / 1) after fqgpu_encode_wait or _end hands it out, *len alone
 * when out is NULL.  The streams are unchanged; with its index a stream is decoded from every snapshot (one per
 * Mi symbols) at once instead of by one lane from its end.  An index that does not describe the block, or between
 * whose snapshots the strides do not consume exactly the stream's bits, is FQGPU_E_CORRUPT (the states inside a
 * snapshot are taken as they are: store an index under a checksum); length 0 = no index for that stream. */
int fqgpu_encode_index(fqgpu_ctx *ctx, int stream, uint8_t *out, size_t cap, size_t *len);
int fqgpu_decode_block_indexed(fqgpu_ctx *ctx, const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                               const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                               const fqgpu_rec *recs, size_t n_recs, uint8_t *raw_out, size_t raw_len,
                               const uint8_t *seq_index, size_t seq_index_len, const uint8_t *qual_index, size_t qual_index_len);

/* ---- device-resident block farm ---------------------------------------
 * Blocks stay in HBM: a "dblock" owns device copies of one raw block, its
 * record table and its coded streams.  Used by the pipeline shim to overlap
 * H2D/D2H with coding, by bench.py (timed region starts with inputs resident)
 * and by the many-blocks decode path, where all blocks of a batch are decoded
 * by ONE launch (the format gives a decoder no parallelism inside a stream:
 * SURVEY.md 7.3). */
typedef struct fqgpu_dblock fqgpu_dblock;
int fqgpu_dblock_create(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, const fqgpu_rec *recs,
                        size_t n_recs, fqgpu_dblock **out);
/* Same from an UNPARSED chunk: the record table is built on the GPU (newline scan + 4-line
 * grouping), replacing FastqReader::parseRecords (src/fastq_io.cpp:67-125), which the reference
 * runs serially under the reader mutex (src/fastq_io.cpp:29-52).  A trailing partial record is
 * ignored like the reference's carry-over; malformed input returns FQGPU_E_ARG. */
int fqgpu_dblock_create_from_raw(fqgpu_ctx *ctx, const uint8_t *raw, size_t raw_len, fqgpu_dblock **out);
/* record table / size of a block (any pointer may be NULL; at most cap records are copied) */
int fqgpu_dblock_records(fqgpu_ctx *ctx, const fqgpu_dblock *b, fqgpu_rec *recs_out, size_t cap,
                         size_t *n_recs, size_t *raw_len);
void fqgpu_dblock_destroy(fqgpu_dblock *b);
/* asynchronous on the handle's stream; sizes are valid after fqgpu_sync() */
int fqgpu_dblock_encode(fqgpu_ctx *ctx, fqgpu_dblock *b, unsigned flags);
/* wipes the sequence/quality bytes of the device raw block (decode target) */
int fqgpu_dblock_wipe(fqgpu_ctx *ctx, fqgpu_dblock *b);
/* decodes every block of the batch from its own device-resident streams */
int fqgpu_dblocks_decode(fqgpu_ctx *ctx, fqgpu_dblock *const *blocks, size_t n_blocks);
/* Extension: extends fqgpu_dblocks_decode for blocks that have no decode index (archives written without
 * FQGPU_F_DECODE_INDEX, by another writer of the format, or whose sidecar is lost).  Decodes every block from its own
 * streams exactly as fqgpu_dblocks_decode does without an index -- an index already loaded on a block is ignored and
 * replaced -- and, on the way, leaves both decode indexes on the block (stride: fqgpu_ctx_set_index_stride), byte for
 * byte what the block's encode with FQGPU_F_DECODE_INDEX leaves: fqgpu_dblock_index_bytes / _fetch_index hand them out,
 * a following fqgpu_dblocks_decode uses them.  (The bytes in front of a snapshot are taken from the restored block:
 * an index from fqgpu_dblock_encode WITH FQGPU_F_WRITE_BACK_N holds 'A' where this one holds 'N'; both seed the model
 * alike.)  Unlike fqgpu_dblocks_decode the call waits for the batch.  Returns the codes of fqgpu_dblocks_decode; a block
 * with a damaged stream reports FQGPU_E_CORRUPT through fqgpu_dblock_status as there and keeps no index (index_bytes 0
 * for both streams); a block of at most `stride` symbols gets the 32-byte header alone. */
int fqgpu_dblocks_decode_indexing(fqgpu_ctx *ctx, fqgpu_dblock *const *blocks, size_t n_blocks);
int fqgpu_sync(fqgpu_ctx *ctx);
/* status/sizes of the last encode/decode of this block.  If that operation is still in flight the
 * call waits for the block's handle first (the lanes run on non-blocking streams), so it never
 * reports stale or zero sizes; fqgpu_dblock_fetch and fqgpu_dblocks_decode do the same. */
int fqgpu_dblock_status(const fqgpu_dblock *b, size_t *seq_len, size_t *qual_len,
                        size_t *n_pos_len, size_t *n_bases);
/* diagnostics of the last encode (after fqgpu_sync): the longest run of symbols one lane
 * had to walk serially, per stream (the latency floor of the chain kernels) */
int fqgpu_dblock_longest_chain(const fqgpu_dblock *b, unsigned *seq_steps, unsigned *qual_steps);
/* diagnostics of the last encode (waits for it): segment groups of the sequence chains that were handed over
 * (fqgpu_ctx_set_seq_handover) and groups that were not; both 0 where nothing may be handed over */
int fqgpu_dblock_seq_handover(const fqgpu_dblock *b, unsigned *handed_over, unsigned *kept);
/* diagnostics of the last encode of this block: how many segments of the quality chains
 * (src/fse_quality.cpp:19-52 cut into segments of S symbols) the chain kernels took as
 * counts[0] transparent (a symbol with one table cell inside: the state behind it is known),
 * [1] anchored (a symbol with <= 64 cells: one walk per candidate), [2] uniform (S times one symbol:
 * a power of one transition), [3] opaque (the full entry-state -> exit-state function).  Reads the
 * scratch of the encode lane that coded the block, so it answers only while that scratch still holds
 * this block's last encode: FQGPU_E_ARG when b is not a block of ctx or was never encoded, when the
 * lane has coded another block since, and after fqgpu_ctx_set_lanes, fqgpu_ctx_reserve or
 * fqgpu_ctx_fill_scratch until b is encoded again. */
int fqgpu_dblock_qual_segment_classes(fqgpu_ctx *ctx, const fqgpu_dblock *b, size_t counts[4]);
/* diagnostics, for tests: the same segments one by one, in the order of the chain kernels' segment numbers (contexts
 * ascending, the segments of a context in encode order).  cls_out[i]: 1 transparent, 2 .. 64 anchored (the number of
 * candidates), 0xFF uniform, 0 opaque; anchor_out[i]: the offset inside the segment of its first reset symbol or its anchor
 * symbol, the symbol of a uniform segment, 0xFFFFFFFF for an opaque one; ctx_out[i]: the segment's quality context.  cap:
 * entries each array holds; *n_out: how many segments there are, also when cap is too small (FQGPU_E_OVERFLOW, nothing
 * written; cap 0 with NULL arrays asks for the number alone).  Host code only: it copies what the kernels left.  Same
 * guards and refusals as fqgpu_dblock_qual_segment_classes. */
int fqgpu_dblock_qual_segments(fqgpu_ctx *ctx, const fqgpu_dblock *b, uint8_t *cls_out, uint32_t *anchor_out, uint32_t *ctx_out,
                               size_t cap, size_t *n_out);
/* diagnostics, for tests of "no result depends on what the scratch held before": waits for the handle (fqgpu_sync) and sets
 * every byte of every device scratch buffer the handle owns -- the encode lanes, the decode scratch, the device parser's,
 * header coder's and chunk decoder's, the checksum, summary and selection scratch, and the staging block of the host-pointer
 * calls, inputs and outputs alike -- to `byte`, up to each buffer's capacity.  Exempt are the buffers that carry state from
 * call to call on purpose (the table beside the implementation names them).  *n_buffers / *n_bytes (either may be NULL): how
 * many buffers and bytes were filled.  Afterwards the staging block holds no chunk and no index (fqgpu_chunk_* and
 * fqgpu_encode_index / fqgpu_decode_index answer FQGPU_E_ARG until the next host-pointer call), and
 * fqgpu_dblock_qual_segment_classes of a block coded before is meaningless.  FQGPU_E_ARG while a block of fqgpu_encode_begin
 * or its header fields are still to be collected.  Nothing in the product calls it. */
int fqgpu_ctx_fill_scratch(fqgpu_ctx *ctx, unsigned char byte, size_t *n_buffers, size_t *n_bytes);
/* diagnostics, for tests that must prove which decode kernel they ran: the forms the handle's last decode launch used
 * (every decode call -- blocks, chunks, ranges, FASTA -- is one launch; a call refused before it launches leaves the last
 * answer standing), one bit per kernel form.  The placement rules choose by the handle's compute units: one launch for
 * both streams up to n_cus blocks, separate launches beyond, the compact quality walk beyond 2 * n_cus quality chains
 * (whole streams) or quality strides (indexed blocks).  *qual_chains: the blocks walked from their streams' ends,
 * *qual_strides: the quality strides walked from snapshots; any pointer may be NULL.  Nothing in the product calls it. */
#define FQGPU_DEC_FORM_BOTH 0x001u                 /* k_decode_both: a quality and a sequence chain side by side */
#define FQGPU_DEC_FORM_QUAL_RESIDENT 0x002u        /* k_decode<Qual>, entries and table offsets in LDS */
#define FQGPU_DEC_FORM_QUAL_COMPACT 0x004u         /* k_decode<Qual>, entries alone in LDS */
#define FQGPU_DEC_FORM_SEQ 0x008u                  /* k_decode<Seq> */
#define FQGPU_DEC_FORM_CHUNKS_QUAL_RESIDENT 0x010u /* k_decode_chunks<Qual>, resident */
#define FQGPU_DEC_FORM_CHUNKS_QUAL_COMPACT 0x020u  /* k_decode_chunks<Qual>, compact */
#define FQGPU_DEC_FORM_CHUNKS_SEQ 0x040u           /* k_decode_chunks<Seq> */
#define FQGPU_DEC_FORM_SNAP 0x100u                 /* the whole-stream forms above took snapshots (indexing decode) */
int fqgpu_ctx_decode_forms(const fqgpu_ctx *ctx, unsigned *forms, unsigned *qual_chains, unsigned *qual_strides, unsigned *n_cus);
/* copies results to the host (synchronous); any pointer may be NULL */
int fqgpu_dblock_fetch(fqgpu_ctx *ctx, const fqgpu_dblock *b, uint8_t *seq_out, uint8_t *qual_out,
                       uint16_t *readlens_out, uint16_t *n_count_out, uint16_t *n_pos_out,
                       uint8_t *raw_out);
/* decode index of one stream (0 = sequence, 1 = quality) of the last encode with
 * FQGPU_F_DECODE_INDEX: size, copy to the host, and the way back for a later decode.  An index
 * is only valid together with the streams it was made for (load it after the streams). */
int fqgpu_ctx_set_index_stride(fqgpu_ctx *ctx, unsigned symbols); /* default 1 Mi, multiple of 64 Ki */
int fqgpu_dblock_index_bytes(const fqgpu_dblock *b, int stream, size_t *bytes);
int fqgpu_dblock_fetch_index(fqgpu_ctx *ctx, const fqgpu_dblock *b, int stream, void *out, size_t cap);
int fqgpu_dblock_load_index(fqgpu_ctx *ctx, fqgpu_dblock *b, int stream, const void *data, size_t len);
/* replaces the block's coded streams with host data (decode of foreign archives) */
int fqgpu_dblock_load_streams(fqgpu_ctx *ctx, fqgpu_dblock *b, const uint8_t *seq, size_t seq_len,
                              const uint8_t *qual, size_t qual_len, const uint16_t *n_count,
                              const uint16_t *n_pos, size_t n_pos_len);

/* Device time per kernel group, measured with HIP events on the streams the kernels are
 * launched on, accumulated from fqgpu_ctx_enable_timing(ctx, 1) until read: kernel_ms =
 * summed duration, kernel_calls = number of launches; total_ms = first start to last end. */
typedef struct {
  float total_ms;
  float kernel_ms[32];
  int kernel_calls[32];
  const char *kernel_name[32];
  int n_kernels;
} fqgpu_timing;
int fqgpu_ctx_enable_timing(fqgpu_ctx *ctx, int on);
int fqgpu_ctx_last_timing(fqgpu_ctx *ctx, fqgpu_timing *out);
/* Restricts the events to the kernel group of that name (NULL or "" = all groups again): two
 * events per launch of that group instead of two per launch of every group -- the events between
 * the kernels of a stream cost about 7 % of a step of 256 MiB blocks. */
int fqgpu_ctx_timing_only(fqgpu_ctx *ctx, const char *name);

/* ---- host helpers of the path's callers (not GPU code) ------------------
 * Minimal 4-line FASTQ parser with the reference's semantics
 * (FastqReader::parseRecords, src/fastq_io.cpp:67-125): returns the number of
 * complete records found (writes at most cap of them) or a negative error. */
long fqgpu_parse_fastq(const uint8_t *raw, size_t len, fqgpu_rec *recs, size_t cap);
/* Deterministic synthetic FASTQ for the BASELINE.json configs:
 * mode 1: 150 bp, N w.p. 0.001, all quals 'I'; mode 2: 150 bp uniform ACGT,
 * Phred ~ round(N(34,5)) clipped to [2,41]; mode 4: length U[50,300], N w.p. 0.01
 * with quality '#'.  Two more modes are NOT BASELINE configs; they probe how the path depends on
 * the data (bench.py: encode_binned_MBps, encode_constant_MBps): mode 3: mode 2's bases with binned
 * qualities -- '#', '-', '8', 'F' at 5/10/15/70 %, the previous position's level kept w.p. 0.85 (no
 * symbol with a single table cell, long runs of one context); mode 5: every base 'A', every quality
 * 'F' (one context per stream); mode 6: mode 2's bases, two quality levels '-' / 'F' i.i.d. at 30/70 %
 * (every quality segment needs its full entry-state -> exit-state function).  Writes whole records
 * only; returns bytes written. */
size_t fqgpu_synth_fastq(uint8_t *dst, size_t cap, int mode, uint64_t seed, uint64_t first_read_id,
                         uint64_t *n_reads_out);


/* ---- chunk decode: both passes of DecompressionWorkspace::decodeChunk (src/workspace.cpp:47-88) on the device.
 * The read headers are decoded from their field streams (decodeHeader, src/workspace.cpp:128-157), the chunk is laid
 * out (header, '\n', sequence, "\n+\n", quality, '\n' per record; zeros behind the last record up to raw_len), the
 * record table is built and the sequence and quality lines are decoded: no skeleton goes up.
 * hdr: the format as fqgpu_encode_headers_begin takes it, the dataset's first header ('@' included), and per field
 * its three streams (isDifferentFlag, content, contentLength: streams[3 i .. 3 i + 2]) with their sizes.
 * recs_out (may be NULL) receives the record table; *laid_out_len the bytes up to the end of the last record.
 * Returns
 *   FQGPU_E_CORRUPT with *bad_record = the first record whose header the host decoder throws out_of_range on (a stream
 *                   exhausted, or the record ending behind raw_len); raw_out is not written
 *   FQGPU_E_CORRUPT with *bad_record = (size_t)-1: a damaged sequence / quality stream, as fqgpu_decode_block
 *   FQGPU_E_ARG     n_fields 0 or above FQGPU_HDR_MAX_FIELDS, raw_len >= 2^32, no records, a NULL where data is
 *                   required, a first header the host coder does not take
 * seq_index / qual_index: as fqgpu_decode_block_indexed (NULL / 0: none). */
typedef struct {
  const uint8_t *field_types;  /* n_fields: 0 = NUMERIC, 1 = STRING */
  const char *separators;      /* n_fields - 1 */
  unsigned n_fields;
  const uint8_t *first_header;
  size_t first_header_len;
  const fqgpu_field_sizes *sizes;  /* n_fields */
  const uint8_t *const *streams;   /* 3 n_fields */
} fqgpu_header_streams;
int fqgpu_decode_chunk(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                       const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                       const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                       const uint8_t *seq_index, size_t seq_index_len, const uint8_t *qual_index, size_t qual_index_len,
                       uint8_t *raw_out, size_t raw_len, fqgpu_rec *recs_out, size_t *laid_out_len, size_t *bad_record);

/* Extension: fqgpu_decode_chunk for a chunk without decode indexes, which builds them while it decodes (as
 * fqgpu_dblocks_decode_indexing; stride: fqgpu_ctx_set_index_stride).  The arguments of fqgpu_decode_chunk without the four
 * index arguments; raw_out == NULL: index only -- nothing of the chunk comes back, *laid_out_len, recs_out and *bad_record
 * as usual.  Afterwards fqgpu_decode_index(stream 0 / 1) hands the index of the chunk just decoded out, shaped like
 * fqgpu_encode_index (out == NULL: *len alone), until the handle's next host-pointer call.
 * Returns the codes of fqgpu_decode_chunk; after a failure no index is kept: fqgpu_decode_index then returns FQGPU_E_ARG
 * with *len = 0 (also for cap < *len). */
int fqgpu_decode_chunk_indexing(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                                const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                                const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                                uint8_t *raw_out, size_t raw_len, fqgpu_rec *recs_out, size_t *laid_out_len, size_t *bad_record);
int fqgpu_decode_index(fqgpu_ctx *ctx, int stream, uint8_t *out, size_t cap, size_t *len);

/* Extension: records [first, end) of a chunk -- exactly the bytes fqgpu_decode_chunk would lay out for them, and
 * nothing else.  Inputs as fqgpu_decode_chunk; raw_len is the chunk's recorded size and judges the layout as there.
 * out == NULL: only *out_len (the range's size) is reported, after the layout passes, and no stream is decoded.
 * recs_out (may be NULL): end - first records, offsets relative to out.  With both decode indexes, only the strides
 * that hold symbols of the range are decoded; without them, every stream is walked whole (the format's pace).
 * Returns
 *   FQGPU_E_ARG       first >= end, end > n_recs, or any argument fqgpu_decode_chunk refuses
 *   FQGPU_E_OVERFLOW  out_cap below the range's size: nothing is written to out, *out_len holds the size needed
 *   the other codes as fqgpu_decode_chunk (the layout is judged over the whole chunk: same rc, same *bad_record).
 * A decoded stride must consume exactly its bits and a patched record must keep its N positions inside the read;
 * a damaged stride that is not decoded goes unseen (a whole-chunk decode still finds it).  Uses the handle's
 * staging block like the other host-pointer calls: one call per handle at a time. */
int fqgpu_decode_chunk_range(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                             const uint8_t *seq, size_t seq_len, const uint8_t *qual, size_t qual_len,
                             const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                             const uint8_t *seq_index, size_t seq_index_len, const uint8_t *qual_index, size_t qual_index_len,
                             size_t raw_len, size_t first, size_t end, uint8_t *out, size_t out_cap, size_t *out_len,
                             fqgpu_rec *recs_out, size_t *bad_record);

/* Extension: records [first, end) of a chunk as FASTA -- per record ">hdr\nSEQ\n": the FASTQ header line byte for byte
 * except for its first byte, the sequence on one line, N restored as N -- from the sequence stream alone.  The call takes
 * no quality argument: the quality stream is not uploaded, not decoded and not looked at, so DAMAGE TO THE QUALITY STREAM
 * IS NEVER SEEN here (a FASTQ decode of the chunk still finds it).  first = 0, end = n_recs is the whole chunk.
 * Shaped like fqgpu_decode_chunk_range:
 *   raw_len    the chunk's recorded FASTQ size.  The chunk is judged on its FASTQ layout exactly as fqgpu_decode_chunk
 *              judges it: same rc, same *bad_record for the same header streams and readlens.
 *   out == NULL: only *out_len (the FASTA size of the range) is reported, after the layout passes; no stream goes up.
 *   recs_out (may be NULL): end - first records, seq_off relative to out (into the FASTA bytes), len, qual_off = 0.
 *   seq_index  the chunk's sequence decode index (NULL / 0: none).  With it only the strides that hold symbols of the
 *              range are decoded; without it the sequence stream is walked whole.
 * Returns
 *   FQGPU_E_ARG       first >= end, end > n_recs, or any argument fqgpu_decode_chunk_range refuses
 *   FQGPU_E_OVERFLOW  out_cap below the range's size: nothing is written to out, *out_len holds the size needed
 *   FQGPU_E_CORRUPT   with *bad_record: the layout, as fqgpu_decode_chunk; with *bad_record = (size_t)-1: a damaged sequence
 *                     stride that was decoded, or (behind the layout's verdict) a damaged index
 *   FQGPU_E_NO_DEVICE without a GPU, whatever the arguments.
 * A FASTA piece is never digested (the digests describe FASTQ bytes): fqgpu_chunk_crc32 afterwards returns FQGPU_E_ARG with
 * *crc = 0, *len = 0.  Uses the handle's staging block like the other host-pointer calls: one call per handle at a time. */
int fqgpu_decode_chunk_fasta(fqgpu_ctx *ctx, const fqgpu_header_streams *hdr, const uint16_t *readlens, size_t n_recs,
                             const uint8_t *seq, size_t seq_len,
                             const uint16_t *n_count, size_t n_count_len, const uint16_t *n_pos, size_t n_pos_len,
                             const uint8_t *seq_index, size_t seq_index_len,
                             size_t raw_len, size_t first, size_t end,
                             uint8_t *out, size_t out_cap, size_t *out_len, fqgpu_rec *recs_out, size_t *bad_record);

/* ---- Extension (nothing in the reference, whose format has no content checksum): CRC-32 of a chunk, taken where the
 * chunk lies already -- in HBM.  The digest is the CRC-32 of zlib / gzip (reflected polynomial 0xEDB88320, initial value
 * and final xor 0xFFFFFFFF: Python's zlib.crc32) of the chunk's CANONICAL bytes, which are exactly what fqgpu_decode_chunk
 * lays out for it: per record the header line with its '\n', the sequence, "\n+\n", the quality line, '\n'.  For input
 * whose '+' lines are bare these are the input bytes up to the end of the last complete record; text behind a '+', which
 * the parsers accept and the format drops, is not part of the digest, so the digest of a chunk about to be encoded and
 * that of the chunk restored from its streams agree.  N bases are digested as N (what a restore yields).
 *   fqgpu_chunk_crc32    the chunk on the handle's staging block.  Valid (a) from fqgpu_encode_begin until the handle's
 *                        next host-pointer call (fqgpu_encode_cancel ends it too): the chunk in flight, digested on the
 *                        handle's copy stream beside the lane's encode, as the header fields are; *len = the canonical
 *                        length (= *used_len for bare '+' lines).  The host-pointer encode never patches the device copy,
 *                        so FQGPU_F_WRITE_BACK_N does not change the digest.  (b) after a SUCCESSFUL fqgpu_decode_chunk,
 *                        fqgpu_decode_chunk_indexing (*len = *laid_out_len), fqgpu_decode_block or fqgpu_decode_block_indexed
 *                        (*len = raw_len: the block as the caller laid it out, digested as it lies).  Everywhere else --
 *                        after a failed decode (a call refused for its arguments included: every host-pointer decode
 *                        ends the digest of the chunk before it), after fqgpu_decode_chunk_range or _fasta, with no chunk on the handle --
 *                        FQGPU_E_ARG with *crc = 0, *len = 0.
 *   fqgpu_dblock_crc32   waits for the block's last operation as fqgpu_dblock_status does, then digests the canonical bytes
 *                        of its raw block by its record table -- of WHATEVER the raw block holds when asked: after
 *                        fqgpu_dblock_encode with FQGPU_F_WRITE_BACK_N that is 'A' where the input had 'N'; take the
 *                        digest before such an encode (or after a decode) if it is to match a restore.
 *   fqgpu_crc32_combine  host helper: the digest of A || B from those of A and B and the length of B.  A file's digest is
 *                        its chunks' digests combined in chunk order.
 *   fqgpu_ctx_set_check_only  on != 0: fqgpu_decode_chunk accepts raw_out == NULL -- everything is decoded and judged,
 *                        nothing of the chunk comes back (recs_out, *laid_out_len, *bad_record as always), the digest is
 *                        there to be asked for.  Off (the default) the call refuses NULL.
 * Without a GPU the two digest calls return FQGPU_E_NO_DEVICE; the combine helper works. */
int fqgpu_chunk_crc32(fqgpu_ctx *ctx, uint32_t *crc, size_t *len);
int fqgpu_dblock_crc32(fqgpu_ctx *ctx, const fqgpu_dblock *b, uint32_t *crc, size_t *len);
uint32_t fqgpu_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int fqgpu_ctx_set_check_only(fqgpu_ctx *ctx, int on);

/* ---- Extension (nothing in the reference): a read summary of a chunk, taken where the chunk lies already -- in HBM -- in
 * one pass over its sequence and quality lines by its record table (fqgpu_rec; header lines and text behind a '+' play no
 * part).  A summary is a flat block of fqgpu_stats_words(P) = 176 + 70 (P + 1) uint64_t counters; P = `positions`,
 * 1 .. 65535, is the caller's choice.  Tables "by position" have P + 1 rows: row p < P is position p of a read (0-based),
 * row P collects every position >= P, so that nothing is dropped:
 *   word 0 n_records | 1 n_bases | 2 min_len | 3 max_len | 4 reads_with_n (reads with at least one N) | 5 positions | 6, 7 zero
 *   8 .. 71    meanq_hist[64]   reads by floor(sum of Phred over the read / len), Phred = quality byte - 33
 *   72 .. 172  gc_hist[101]     reads by floor(100 (#G + #C) / len); N counts in len
 *   173 .. 175 zero
 *   then P + 1       len_hist   reads by min(len, P)
 *   then 5 (P + 1)   base_pos[row][A, C, G, T, N]
 *   then 64 (P + 1)  qual_pos[row][Phred 0 .. 63]
 * Integer arithmetic throughout: the summary is a pure function of the chunk's records.  A sequence byte outside ACGTN, a
 * quality byte outside 33 .. 96 (as the analysis and the encoder judge them), a record that does not lie inside the chunk
 * or a record of length 0 (which no parser here makes; it has no mean quality): FQGPU_E_ARG with `out` zeroed.
 *   fqgpu_stats_words   host only: the size of a summary; 0 for positions == 0 or > 65535
 *   fqgpu_chunk_stats   the chunk on the handle's staging block, in the states in which fqgpu_chunk_crc32 is valid: (a) from
 *                       fqgpu_encode_begin until the handle's next host-pointer call, on the handle's copy stream beside the
 *                       lane's encode, by the record table given or built by the device parser -- the host-pointer encode
 *                       never patches the device copy, so N is counted as N with FQGPU_F_WRITE_BACK_N too; (b) after a
 *                       SUCCESSFUL fqgpu_decode_chunk (check-only with raw_out == NULL included), fqgpu_decode_chunk_indexing,
 *                       fqgpu_decode_block or fqgpu_decode_block_indexed.  Everywhere else -- after a failed or refused decode,
 *                       after fqgpu_decode_chunk_range or _fasta, after fqgpu_encode_cancel, with no chunk on the handle --
 *                       FQGPU_E_ARG with `out` zeroed.  May be called together with fqgpu_chunk_crc32, in either order.
 *   fqgpu_dblock_stats  waits for the block's last operation as fqgpu_dblock_crc32 does, then summarises WHATEVER the raw
 *                       block holds when asked: after fqgpu_dblock_encode with FQGPU_F_WRITE_BACK_N that is 'A' where the
 *                       input had 'N'; take the summary before such an encode (or after a decode) if N is to be counted.
 *   fqgpu_stats_merge   host only: dst += src.  Counters add, min_len / max_len take the min / max; a dst whose n_records
 *                       is 0 (a block of zeros included) is empty and becomes a copy of src.  Different `positions`, or a
 *                       length that is not fqgpu_stats_words(positions): FQGPU_E_ARG.
 * cap_words below the size needed: FQGPU_E_OVERFLOW, nothing is written.  Bad positions or a NULL pointer: FQGPU_E_ARG.
 * Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any argument is looked at; the two host helpers work. */
size_t fqgpu_stats_words(unsigned positions);
int fqgpu_chunk_stats(fqgpu_ctx *ctx, unsigned positions, uint64_t *out, size_t cap_words);
int fqgpu_dblock_stats(fqgpu_ctx *ctx, const fqgpu_dblock *b, unsigned positions, uint64_t *out, size_t cap_words);
int fqgpu_stats_merge(uint64_t *dst, size_t dst_words, const uint64_t *src, size_t src_words);

/* ---- Extension (nothing in the reference): the reads of a chunk that pass a filter, selected where the chunk lies already
 * -- in HBM -- so that only the kept bytes come down.  A read is judged by its length, its number of N, the sum of its
 * Phred values (quality byte - 33) and the number of its Phred values below a level, the quantities the read summary
 * counts; integer arithmetic throughout, so the result is a pure function of the chunk's records.  The output is the
 * CANONICAL bytes of the kept records in input order (per record the header line with its '\n', the sequence, "\n+\n", the
 * quality line, '\n': what fqgpu_chunk_crc32 digests and a restore lays out); text behind a '+' is dropped, N stays N.
 *   report  FQGPU_FILTER_REPORT_WORDS uint64_t: 0 n_records | 1 n_kept | 2 bases_in | 3 bases_kept | 4 bytes_kept |
 *           5 dropped_short | 6 dropped_long | 7 dropped_n | 8 dropped_mean_q | 9 dropped_low_q | 10 .. 15 zero.  A dropped
 *           read is counted once, under its first failing criterion in that order.  Reports of several chunks add word by word.
 *   out == NULL           size query: *out_len, report and keep_out are filled, nothing is copied
 *   out_cap < *out_len    FQGPU_E_OVERFLOW: nothing is written to out, *out_len holds the size needed, report is valid
 *   keep_out              NULL, or (n_recs + 7) / 8 bytes: bit r & 7 of byte r >> 3 is set iff record r is kept
 * Only the lines a criterion needs are read: the sequence lines when max_n is on, the quality lines when min_mean_q or low_q
 * is on; a length-only filter touches the record table alone.  The bytes of the lines that ARE read are judged as the read
 * summary judges them -- a sequence byte outside ACGTN, a quality byte outside 33 .. 96: FQGPU_E_ARG -- and a byte of a line
 * that is not read is not looked at.  A record that does not lie inside the chunk, or of length 0: FQGPU_E_ARG.  A filter
 * fqgpu_filter_check refuses (min_len > max_len, min_mean_q > 63, low_q > 64, max_low_pct > 100, reserved not zero), a
 * NULL where data is expected: FQGPU_E_ARG.  Every FQGPU_E_ARG comes with *out_len = 0 and a zeroed report.
 *   fqgpu_filter_check   host only: FQGPU_OK or FQGPU_E_ARG
 *   fqgpu_chunk_filter   the chunk on the handle's staging block, in exactly the states in which fqgpu_chunk_stats is valid,
 *                        on the same stream; everywhere else FQGPU_E_ARG.  It leaves the chunk as it is: digest and summary
 *                        taken before or after it are the same.  `out` receives ONE copy of *out_len bytes; nothing else of
 *                        the chunk comes down.
 *   fqgpu_dblock_filter  waits for the block's last operation as fqgpu_dblock_stats does, then selects from WHATEVER the raw
 *                        block holds when asked.
 * Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any argument is looked at; fqgpu_filter_check works. */
#define FQGPU_FILTER_NONE 0xFFFFFFFFu
typedef struct {
  uint32_t min_len, max_len;   /* keep min_len <= len <= max_len; max_len FQGPU_FILTER_NONE = no upper limit */
  uint32_t max_n;              /* keep #N <= max_n; FQGPU_FILTER_NONE = off */
  uint32_t min_mean_q;         /* keep sum(Phred) >= min_mean_q * len, i.e. floor(mean) >= q as the summary bins it; 0 = off; <= 63 */
  uint32_t low_q, max_low_pct; /* keep 100 * #(Phred < low_q) <= max_low_pct * len; low_q 0 = off; low_q <= 64, pct <= 100 */
  uint32_t reserved[2];        /* zero */
} fqgpu_filter;
#define FQGPU_FILTER_REPORT_WORDS 16
int fqgpu_filter_check(const fqgpu_filter *f);
int fqgpu_chunk_filter(fqgpu_ctx *ctx, const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len,
                       uint64_t *report, uint8_t *keep_out);
int fqgpu_dblock_filter(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_filter *f, uint8_t *out, size_t out_cap,
                        size_t *out_len, uint64_t *report, uint8_t *keep_out);

/* ---- Extension (nothing in the reference): the reads of a chunk TRIMMED, then filtered, where the chunk lies already -- in
 * HBM.  What every QC tool does beside dropping reads: cut a fixed number of bases from either end, cut low-quality ends by
 * the running-sum rule (BWA -q, cutadapt -q), crop to a maximum length; the criteria of an fqgpu_filter are then applied to
 * what is left.  For a read of length L with Phred values p[i] = quality byte - 33, integer arithmetic throughout:
 *   1 fixed cuts     f = min(cut_front, L), t = min(cut_tail, L - f): the interval [f, L - t)
 *   2 front (q_front on)  start = f; walk i = f .. L-t-1 with s = 0, best = 0: s += q_front - p[i]; s < 0: stop;
 *                    s > best (strictly): best = s, start = i + 1
 *   3 tail (q_tail on)    stop = L - t; walk i = L-t-1 .. f downwards with s = 0, best = 0: s += q_tail - p[i]; s < 0: stop;
 *                    s > best (strictly): best = s, stop = i
 *   4 the two walks are independent, both over the interval of step 1.  start >= stop: the read is EMPTY, its window (0, 0).
 *                    Otherwise n = min(stop - start, crop) and the read's window is (start, n)
 *   5 the filter     judged on the trimmed read: its length n, the N of seq[start, start+n), Phred sum and low count of
 *                    qual[start, start+n); comparisons and order of the first failing criterion as fqgpu_chunk_filter.  A NULL
 *                    filter keeps everything.  An emptied read is always dropped: counted under dropped_short whatever
 *                    min_len is, and under reads_emptied
 * The output, in input order, per kept record: the header line byte for byte with its '\n', seq[start, start+n), "\n+\n",
 * qual[start, start+n), '\n'; text behind a '+' is dropped, N stays N.  With a trim that cuts nothing (all fields off) the
 * output, report words 0 .. 9 and the keep bits are those of fqgpu_*_filter with the same filter.
 *   report  FQGPU_TRIM_REPORT_WORDS uint64_t: 0 .. 9 as the filter's report (bases_in counts untrimmed lengths, bases_kept the
 *           n of kept reads) | 10 reads_trimmed (n != L, kept or not) | 11 bases_cut_front (sum of start) | 12 bases_cut_tail
 *           (sum of L - start - n; all L of an emptied read) | 13 reads_emptied | 14, 15 zero.  Words 11 and 12 run over ALL
 *           records: bases_in = word 11 + word 12 + the sum of n over all records.  Reports of several chunks add word by word.
 *   out == NULL, out_cap < *out_len, keep_out   as fqgpu_chunk_filter
 *   win_out               NULL, or n_recs words: start | n << 16 of every record, kept or not
 * The sequence line is read iff max_n is on, the quality line iff q_front, q_tail, min_mean_q or low_q is on; a line that is
 * read is judged over ALL L bytes, the cut ones too, by the filter's rules (ACGTN; 33 .. 96: FQGPU_E_ARG), a line that is not
 * read is not looked at: fixed cuts and crop with length criteria alone touch the record table only.  A record outside the
 * chunk, or of length 0: FQGPU_E_ARG.  A trim fqgpu_trim_check refuses (a cut above 65535, a cutoff above 64, crop 0,
 * reserved not zero), a filter fqgpu_filter_check refuses, a NULL where data is expected: FQGPU_E_ARG.  Every FQGPU_E_ARG
 * comes with *out_len = 0, a zeroed report and -- where the chunk itself is refused -- zeroed keep bits and windows.
 *   fqgpu_trim_check    host only: FQGPU_OK or FQGPU_E_ARG
 *   fqgpu_chunk_trim    the chunk on the handle's staging block, in exactly the states in which fqgpu_chunk_filter is valid,
 *                       on the same stream.  It leaves the chunk as it is: digest, summary and a plain filter before or after
 *                       give the same results (every call is waited for before it returns).
 *   fqgpu_dblock_trim   waits for the block's last operation as fqgpu_dblock_filter does.
 * Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any argument is looked at; fqgpu_trim_check works. */
typedef struct {
  uint32_t cut_front, cut_tail;  /* bases removed from the 5' / 3' end first; each <= 65535 */
  uint32_t q_front, q_tail;      /* running-sum quality trim of the 5' / 3' end; 0 = off; <= 64 */
  uint32_t crop;                 /* keep at most this many bases, counted from the new front; FQGPU_FILTER_NONE = off; 0 refused */
  uint32_t reserved[3];          /* zero */
} fqgpu_trim;
#define FQGPU_TRIM_REPORT_WORDS 16
int fqgpu_trim_check(const fqgpu_trim *t);
int fqgpu_chunk_trim(fqgpu_ctx *ctx, const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len,
                     uint64_t *report, uint8_t *keep_out, uint32_t *win_out);
int fqgpu_dblock_trim(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out, size_t out_cap,
                      size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out);

/* ---- Extension (nothing in the reference): a 3' ADAPTER clipped from the reads of a chunk, then trimmed, then filtered,
 * where the chunk lies already -- in HBM.  What fastp, cutadapt and Trimmomatic do to a short-insert read whose 3' end runs
 * into the sequencing adapter: find the adapter and cut the read there.  An adapter is a string A[0, m) over ACGT,
 * 1 <= m <= FQGPU_ADAPTER_MAX, with a min_overlap in 1 .. m and a max_err_pct in 0 .. 50.  For a read with the sequence line
 * s[0, L), integer arithmetic throughout:
 *   0 the clip       at every place p in 0 .. L-1: ov = min(m, L - p), mism(p) = the number of j < ov with s[p + j] != A[j]
 *                    (an N in the read is a mismatch; there are no indels).  p is a HIT iff ov >= min_overlap and
 *                    100 * mism(p) <= max_err_pct * ov.  The clip place a is the SMALLEST hit -- the leftmost one wins even
 *                    when a later place matches better (fastp's rule for a given adapter), which makes the result independent
 *                    of how the work is split -- and a = L when there is none.  The search runs over the whole untrimmed line
 *   1 .. 4           the steps of fqgpu_chunk_trim, on the read as if its length were a: f = min(cut_front, a),
 *                    t = min(cut_tail, a - f), the two walks over [f, a - t), crop.  A NULL trim cuts nothing beyond the clip
 *   5 the filter     on the window that is left, as fqgpu_chunk_trim.  a == 0 gives an emptied read: dropped, counted under
 *                    dropped_short and reads_emptied, its window (0, 0)
 * Output, keep bits and windows are those of fqgpu_chunk_trim.
 *   report  FQGPU_TRIM_REPORT_WORDS uint64_t: 0 .. 13 as the trim's report -- word 12, bases_cut_tail, stays the sum of
 *           L - start - n and so includes the clipped bases; bases_in = word 11 + word 12 + the sum of n over all records keeps
 *           holding | 14 reads_with_adapter (a < L, kept or not) | 15 bases_cut_adapter (the sum of L - a over all records)
 *   out == NULL, out_cap < *out_len, keep_out, win_out   as fqgpu_chunk_trim
 * The sequence line is read iff max_n is on OR an adapter is given, and is then judged over all L bytes by the filter's rule
 * (a byte outside ACGTN: FQGPU_E_ARG); the quality line is read by the trim's rule alone.  An adapter fqgpu_adapter_check
 * refuses (len outside 1 .. 64, a byte of seq[0, len) outside upper-case ACGT, a byte behind len that is not zero,
 * min_overlap outside 1 .. len, max_err_pct above 50, reserved not zero), a trim or filter their checks refuse:
 * FQGPU_E_ARG, with *out_len = 0, a zeroed report and -- where the chunk itself is refused -- zeroed keep bits and windows.
 *   fqgpu_adapter_check  host only: FQGPU_OK or FQGPU_E_ARG
 *   fqgpu_chunk_clip     the chunk on the handle's staging block, in exactly the states in which fqgpu_chunk_trim is valid, on
 *                        the same stream; it leaves the chunk as it is and is waited for before it returns.  a == NULL: exactly
 *                        fqgpu_chunk_trim with the same t and f (a NULL t is then refused as it is there)
 *   fqgpu_dblock_clip    waits for the block's last operation as fqgpu_dblock_trim does; a == NULL: exactly fqgpu_dblock_trim.
 * Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any argument is looked at; fqgpu_adapter_check works. */
#define FQGPU_ADAPTER_MAX 64
typedef struct {
  uint8_t seq[FQGPU_ADAPTER_MAX];                    /* A[0, len) in "ACGT" (upper case), zero behind */
  uint32_t len, min_overlap, max_err_pct, reserved;  /* 1 .. 64 | 1 .. len | 0 .. 50 | zero */
} fqgpu_adapter;
int fqgpu_adapter_check(const fqgpu_adapter *a);
int fqgpu_chunk_clip(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_trim *t, const fqgpu_filter *f, uint8_t *out, size_t out_cap,
                     size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out);
int fqgpu_dblock_clip(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_trim *t, const fqgpu_filter *f,
                      uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out);

/* ---- Extension (nothing in the reference): POLY-X TAILS and a SLIDING-WINDOW quality cut taken from the 3' end of the reads
 * of a chunk, between the adapter clip and the trim's steps, where the chunk lies already -- in HBM.  A two-colour instrument
 * reads "no signal" as G, so a read that runs off its fragment ends in a run of G with a few errors in it and often high
 * qualities (fastp trims these by default on such data); Trimmomatic SLIDINGWINDOW:W:Q and fastp --cut_right are the window
 * rule.  For a read with the sequence line s[0, L) and Phred values p[i] = quality byte - 33, integer arithmetic throughout:
 *   0  the clip      fqgpu_chunk_clip's step 0, unchanged: a0.  A NULL adapter: a0 = L
 *   0b the poly tail over s[0, a0) (poly_bases on).  For a base X of the set and i = 1 .. a0: b_i = s[a0 - i]; mism_X(i) is the
 *                    number of j in 1 .. i with b_j != X (an N is a mismatch for every X); ok_X(i) holds iff
 *                    mism_X(i) <= min(i / poly_every, poly_max_mism).  v_X is the smallest i with !ok_X(i), a0 + 1 when there
 *                    is none: the walk stops at the FIRST violation, a place behind it never counts, however well it matches.
 *                    t_X is the largest i < v_X with b_i == X (the tail that is cut begins with an X), 0 when there is none;
 *                    t_X < poly_min_len gives t_X = 0.  t is the largest t_X over the set and a1 = a0 - t.  Off: a1 = a0
 *   1  fixed cuts    on the read as if its length were a1: f = min(cut_front, a1), e = a1 - min(cut_tail, a1 - f).  A NULL trim
 *                    cuts nothing
 *   1b the window    over [f, e) (window_len = W on, window_q = Q).  For p = f, f+1, ... while p + W <= e:
 *                    S(p) = p[p] + ... + p[p+W-1]; take the smallest p with S(p) < Q * W; e2 is the smallest i >= p with
 *                    p[i] < Q -- it exists and lies inside that window: the good bases at the window's front are kept, as fastp
 *                    does.  No such p, e - f < W, or off: e2 = e
 *   2 .. 4           the two running-sum walks of fqgpu_chunk_trim over [f, e2), then the crop
 *   5  the filter    on the window that is left, exactly as fqgpu_chunk_trim: an emptied read is dropped, counted under
 *                    dropped_short and reads_emptied
 * Output, keep bits and windows have the forms of fqgpu_chunk_trim.
 *   report  FQGPU_TAIL_REPORT_WORDS uint64_t: 0 .. 15 as fqgpu_chunk_clip's report -- word 12 stays the sum of L - start - n,
 *           and bases_in = word 11 + word 12 + the sum of n keeps holding | 16 reads_with_poly_tail (a1 < a0, kept or not) |
 *           17 bases_cut_poly (the sum of a0 - a1) | 18 reads_window_cut (e2 < e) | 19 bases_cut_window (the sum of e - e2) |
 *           20 .. 23 zero (word 20 is fqgpu_chunk_select_marked's).  Reports of several chunks add word by word
 *   places_out   NULL, or 4 uint16_t per record, kept or not: a0, a1, e, e2
 *   out == NULL, out_cap < *out_len, keep_out, win_out   as fqgpu_chunk_clip
 * The sequence line is read iff max_n is on, an adapter is given, or poly_bases != 0; the quality line iff the trim's rule
 * says so or window_len != 0.  A line that is read is judged over all L bytes (ACGTN; 33 .. 96: FQGPU_E_ARG), a line that is
 * not read is not looked at.  A tail fqgpu_tail_check refuses (poly_bases above 15; a poly_max_mism above 255; with poly_bases
 * on a poly_min_len outside 1 .. 65535 or a poly_every outside 2 .. 255, with it off either of the two not zero; window_len
 * above 32; with window_len on a window_q outside 1 .. 64, with it off a window_q not zero; reserved not zero), an adapter,
 * trim or filter its own check refuses, a record outside the chunk or of length 0, a NULL where data is expected: FQGPU_E_ARG,
 * with *out_len = 0, a zeroed report and -- where the chunk itself is refused -- zeroed keep bits, windows and places.
 *   fqgpu_tail_check      host only: FQGPU_OK or FQGPU_E_ARG
 *   fqgpu_chunk_tailtrim  the chunk on the handle's staging block, in exactly the states in which fqgpu_chunk_clip is valid, on
 *                         the same stream; it leaves the chunk as it is and is waited for before it returns.  x == NULL, or a
 *                         tail with both rules off: output, report words 0 .. 15, keep bits and windows are those of
 *                         fqgpu_chunk_clip with the same a, t, f (a NULL a then follows that call's rules), words 16 .. 23
 *                         zero, the places a0 = a1 and e = e2
 *   fqgpu_dblock_tailtrim waits for the block's last operation as fqgpu_dblock_clip does; x == NULL: as above.
 * Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any argument is looked at; fqgpu_tail_check works. */
typedef struct {
  uint32_t poly_bases;     /* bit 0 A, 1 C, 2 G, 3 T; 0 = poly trim off; above 15 refused */
  uint32_t poly_min_len;   /* shortest tail that is cut; 1 .. 65535 when poly_bases != 0, else 0 */
  uint32_t poly_every;     /* one mismatch allowed per this many tail bases; 2 .. 255 when on, else 0 */
  uint32_t poly_max_mism;  /* and never more than this many; 0 .. 255 */
  uint32_t window_len;     /* W; 0 = window cut off; 1 .. 32 */
  uint32_t window_q;       /* Q; 1 .. 64 when window_len != 0, else 0 */
  uint32_t reserved[2];    /* zero */
} fqgpu_tail;
#define FQGPU_TAIL_REPORT_WORDS 24
int fqgpu_tail_check(const fqgpu_tail *x);
int fqgpu_chunk_tailtrim(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t, const fqgpu_filter *f,
                         uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out,
                         uint16_t *places_out);
int fqgpu_dblock_tailtrim(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t,
                          const fqgpu_filter *f, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out,
                          uint32_t *win_out, uint16_t *places_out);

/* ---- Extension (nothing in the reference): PAIRED chunks -- a selection restricted to a RECORD RANGE of a chunk and to a MARK,
 * and the READ IDS of two chunks compared, where the chunks lie already -- in HBM.  Paired-end reads come as two files whose
 * record i are mates; a restore that drops reads must drop a pair when either mate fails, and the chunks of two archives are
 * cut by bytes, so that the mates of one chunk's records lie in a range of one to three chunks of the other archive.  The two
 * calls are what a paired restore is made of: judge mate 1 (a size query: its keep bits), judge the matching range of mate 2
 * with those bits as the mark (its keep bits are the pair's), gather mate 1 with the pair's bits as the mark.
 *   fqgpu_chunk_select_marked   records [first, end) of the chunk alone are judged, counted and written; first < end <= n_recs,
 *                  else FQGPU_E_ARG.  Steps 0 to 5 are exactly those of fqgpu_chunk_tailtrim; each of a, x, t, f may be NULL,
 *                  which means "off", and all four NULL keeps every read.  report[0], keep_out, win_out, places_out, the
 *                  offsets inside out and the bits of mark_in are all relative to `first`: record first + i is bit i & 7 of
 *                  byte i >> 3, word i of win_out, row i of places_out.
 *   mark_in        NULL (every record is marked), or (end - first + 7) / 8 bytes in keep_out's layout.  A record whose bit is 0
 *                  is dropped whatever its own verdict.  The bits of the last byte behind `end` are not looked at.
 *   report  FQGPU_TAIL_REPORT_WORDS uint64_t, the tail calls' report of the range: words 5 .. 19 are the records' own -- what
 *           each criterion dropped and what was cut; the mark does not change them -- | 1 n_kept, 3 bases_kept, 4 bytes_kept count
 *           the records that are kept AND marked | 20 dropped_unmarked: the records that pass every criterion and whose mark bit
 *           is 0 | 21 .. 23 zero.  n_records = n_kept + words 5 .. 9 + word 20 always.  Reports add word by word.
 *   keep_out       the final bit: the record's own verdict AND its mark
 *   out == NULL, out_cap < *out_len, win_out, places_out, the lines that are read and judged, what is refused and what a
 *   refusal zeroes: as fqgpu_chunk_tailtrim, over the range.  Valid in exactly the states in which fqgpu_chunk_tailtrim is
 *   valid, on the same stream; it leaves the chunk as it is and is waited for before it returns, so several calls on one
 *   staged chunk are allowed.  With first = 0, end = n_recs, mark_in = NULL and arguments fqgpu_chunk_tailtrim accepts, every
 *   output is that call's, byte for byte (word 20 is zero).
 *   fqgpu_dblock_select_marked  waits for the block's last operation as fqgpu_dblock_tailtrim does.
 * The READ ID of a record is the bytes of its header line behind the '@', up to the first ' ', '\t' or '\n'; if they end in
 * "/1" or "/2", those two bytes are not part of it -- judged for each mate on its own, so "x/1" and "x" have one id.
 *   fqgpu_chunk_pair_names   compares the ids of record first_a + i of the chunk staged on ctx_a and record first_b + i of the
 *                  chunk staged on ctx_b (each where fqgpu_chunk_stats is valid) for i < count.  *mismatch = the smallest i whose
 *                  ids differ in length or in any byte, (size_t)-1 when there is none: a mismatch still returns FQGPU_OK, the
 *                  caller decides what to make of it.  Both handles must be of one device, else FQGPU_E_ARG; every stream of
 *                  both is waited for first, then ONE kernel runs on ctx_a's stream and is waited for.  ctx_a == ctx_b is allowed
 *                  (a chunk against itself).  count == 0, a range outside either chunk, a header line that does not lie
 *                  inside its chunk (a table that is not the chunk's), a NULL: FQGPU_E_ARG with *mismatch = (size_t)-1.
 *   fqgpu_dblock_pair_names  two blocks of ctx's device; waits for each block's last operation as fqgpu_dblock_stats does, the
 *                  owners of blocks of other handles included.  A block of another device: FQGPU_E_ARG.
 *   fqgpu_read_id_len        host only, the rule's statement: the id's length for a header line of `len` bytes that starts
 *                  with its '@' (the line's end counts as an end when no ' ', '\t' or '\n' stands in front of it); 0 for NULL.
 * Without a GPU the four device calls return FQGPU_E_NO_DEVICE before any argument is looked at; fqgpu_read_id_len works. */
int fqgpu_chunk_select_marked(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t, const fqgpu_filter *f,
                              size_t first, size_t end, const uint8_t *mark_in, uint8_t *out, size_t out_cap, size_t *out_len,
                              uint64_t *report, uint8_t *keep_out, uint32_t *win_out, uint16_t *places_out);
int fqgpu_dblock_select_marked(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t,
                               const fqgpu_filter *f, size_t first, size_t end, const uint8_t *mark_in, uint8_t *out, size_t out_cap,
                               size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out, uint16_t *places_out);
int fqgpu_chunk_pair_names(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, size_t *mismatch);
int fqgpu_dblock_pair_names(fqgpu_ctx *ctx, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b, size_t count,
                            size_t *mismatch);
size_t fqgpu_read_id_len(const uint8_t *header_line, size_t len);

/* ---- Extension (nothing in the reference): ADAPTER CONTENT -- which 3' adapters the reads of a chunk hold, in how many reads
 * and where, counted where the chunk lies already -- in HBM.  FastQC's "Adapter Content" module, and the question in front
 * of fqgpu_chunk_clip: which sequence to clip, and what that would cut.  A probe set is n probes, 1 <= n <=
 * FQGPU_PROBES_MAX, each an fqgpu_adapter with its own min_overlap and max_err_pct; P = `positions`, 1 .. 65535, is the
 * number of rows.  For a read of length L, a_k is the clip place of step 0 of fqgpu_chunk_clip for probe k alone (L when
 * there is no hit) and a = min over k of a_k: for every probe the pass reports exactly what a clip with that adapter would
 * do.  Nothing else is applied -- no trim, no filter.  Integer arithmetic throughout; the result is a pure function of the
 * chunk's records and adds over chunks.
 *   out  fqgpu_probe_words(n, P) = 8 + (n + 1) (8 + P + 1) uint64_t:
 *        head   0 n_records | 1 n_bases | 2 n_probes | 3 positions | 4 the probe set's fingerprint: zlib's CRC-32 of the
 *               80 n bytes of probe[0 .. n) | 5 .. 7 zero
 *        then n + 1 tables: table k for probe k, table n for "any", which uses a.  A table is 8 words and P + 1 rows:
 *               0 reads_with (a_k < L) | 1 bases_behind (the sum of L - a_k) | 2 reads_whole (a_k + m_k <= L, m_k probe k's
 *               length: the hit shows the whole probe; zero in the "any" table) | 3 reads_emptied (a_k == 0) | 4 .. 7 zero |
 *               row i: the reads with a_k < L and min(a_k, P) == i -- the rows sum to word 0
 *   places_out   NULL, or n uint16_t per record: places_out[r * n + k] = a_k of record r
 * Only the sequence lines are read; they are judged over all their bytes (a byte outside ACGTN: FQGPU_E_ARG), the quality
 * lines are not looked at.  A record outside the chunk, or of length 0: FQGPU_E_ARG.  Every FQGPU_E_ARG zeroes `out`, and
 * where the chunk itself is refused places_out as well.  Counts of rows up to 319 (and of row P) are summed on the chip;
 * rows between 320 and P are added in global memory one by one -- correct, slow, and rare with reads of some hundred bases.
 *   fqgpu_probe_words    host only: the size of a result; 0 for n outside 1 .. 16 or positions outside 1 .. 65535
 *   fqgpu_probes_check   host only: FQGPU_OK iff n is in 1 .. 16, reserved is zero, every probe[k < n] passes
 *                        fqgpu_adapter_check and every byte of probe[k >= n] is zero.  Equal probes are allowed
 *   fqgpu_chunk_probe    the chunk on the handle's staging block, in exactly the states in which fqgpu_chunk_stats is valid,
 *                        on the same stream; it leaves the chunk as it is -- digest, summary and any selection give the same
 *                        result before it and after it -- and is waited for before it returns
 *   fqgpu_dblock_probe   waits for the block's last operation as fqgpu_dblock_stats does
 *   fqgpu_probe_merge    host only: dst += src.  Head words 2, 3 and 4 must be equal and both lengths fqgpu_probe_words of
 *                        them, else FQGPU_E_ARG; a dst whose n_records is 0 is empty (a dst of all zeros counts as empty)
 *                        and becomes a copy of src: fqgpu_stats_merge's rule
 * cap_words below the size needed: FQGPU_E_OVERFLOW, nothing is written.  A probe set its check refuses, bad positions or a
 * NULL where data is expected: FQGPU_E_ARG.  Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any
 * argument is looked at; the three host helpers work. */
#define FQGPU_PROBES_MAX 16
typedef struct {
  uint32_t n, reserved[3];                /* 1 .. 16 | zero */
  fqgpu_adapter probe[FQGPU_PROBES_MAX];  /* probe[k >= n]: all bytes zero */
} fqgpu_probes;
size_t fqgpu_probe_words(unsigned n_probes, unsigned positions);
int fqgpu_probes_check(const fqgpu_probes *p);
int fqgpu_chunk_probe(fqgpu_ctx *ctx, const fqgpu_probes *p, unsigned positions, uint64_t *out, size_t cap_words, uint16_t *places_out);
int fqgpu_dblock_probe(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_probes *p, unsigned positions, uint64_t *out, size_t cap_words,
                       uint16_t *places_out);
int fqgpu_probe_merge(uint64_t *dst, size_t dst_words, const uint64_t *src, size_t src_words);

/* ---- Extension (nothing in the reference): MATE OVERLAP -- where the two mates of a pair stop agreeing, found where both
 * chunks lie already -- in HBM -- and a per-record LIMIT that a selection takes in front of its other steps.  When a fragment is
 * shorter than the reads, each mate runs through the fragment's far end into the adapter; over the fragment the mates are
 * reverse complements of each other, so the fragment's end is found without knowing the adapter (fastp's PE mode does this by
 * default), and the same comparison gives the insert size of every overlapping pair.  For a pair with the sequence lines
 * s1[0, L1) (mate 1) and s2[0, L2) (mate 2), let r[j] = comp(s2[L2 - 1 - j]), comp mapping A<->T, C<->G and N to N.  Integer
 * arithmetic throughout:
 *   candidates   an integer shift d puts r[0] beside s1[d]: the overlap covers s1[lo, hi), lo = max(0, d), hi = min(L1, d + L2),
 *                ov = hi - lo.  mism(d) = the number of i in [lo, hi) with s1[i] != r[i - d]; an N in either read is a
 *                mismatch, there are no indels.  d is a HIT iff ov >= min_overlap, mism(d) <= max_mism and
 *                100 * mism(d) <= max_err_pct * ov
 *   the choice   the candidates are tried in the order d = 0, 1, 2, ..., then d = -1, -2, ..., and the FIRST hit wins (fastp's
 *                order): the chosen d minimises d >= 0 ? d : 512 + |d|.  A later shift that matches better does not count,
 *                which -- like the adapter clip's leftmost hit -- makes the result independent of how the work is split
 *   a hit        the insert size is I = d + L2 (>= ov >= 1); limit1 = min(L1, I) and limit2 = min(L2, I) are the bases of each
 *                mate that lie inside the fragment.  No hit: I = 0, limit1 = L1, limit2 = L2
 *   the cap      a pair with L1 or L2 above FQGPU_OVERLAP_MAX_LEN is NOT ANALYSED: a pair without a hit, counted in word 5, its
 *                lines not looked at
 * The sequence lines of an analysed pair are judged over all their bytes (a byte outside ACGTN: FQGPU_E_ARG); a record outside
 * its chunk or of length 0: FQGPU_E_ARG.  Every FQGPU_E_ARG zeroes `out` and the three arrays.
 *   out  FQGPU_OVERLAP_WORDS uint64_t: 0 n_pairs | 1 pairs_overlapped | 2 pairs_read_through (limit1 < L1 or limit2 < L2) |
 *        3 bases_behind_a (the sum of L1 - limit1) | 4 bases_behind_b | 5 pairs_not_analysed | 6 mismatches (the sum of mism at
 *        the chosen d) | 7 overlap_bases (the sum of ov) | 8 zlib's CRC-32 of the 32 bytes of the fqgpu_overlap | 9 .. 15 zero |
 *        then 1024 rows: the overlapped pairs by I (I <= 1023 always: the rows sum to word 1)
 *   limit_a_out, limit_b_out, insert_out   each NULL, or `count` uint16_t: limit1, limit2 and I of pair i
 *   fqgpu_overlap_check       host only: min_overlap in 1 .. 512, max_mism in 0 .. 65535, max_err_pct in 0 .. 50, reserved zero:
 *                             FQGPU_OK, else FQGPU_E_ARG
 *   fqgpu_chunk_pair_overlap  record first_a + i of the chunk staged on ctx_a (mate 1) against record first_b + i of the chunk
 *                             staged on ctx_b (mate 2), i < count: shaped and validated exactly like fqgpu_chunk_pair_names --
 *                             valid in the same states, both handles of one device, every stream of both waited for, then ONE
 *                             kernel on ctx_a's stream, waited for; ctx_a == ctx_b is allowed
 *   fqgpu_dblock_pair_overlap as fqgpu_dblock_pair_names
 *   fqgpu_overlap_merge       host only: dst += src.  Both lengths FQGPU_OVERLAP_WORDS and word 8 equal, else FQGPU_E_ARG; a dst
 *                             whose n_pairs is 0 is empty (a dst of all zeros counts as empty) and becomes a copy of src:
 *                             fqgpu_stats_merge's rule
 * cap_words below FQGPU_OVERLAP_WORDS: FQGPU_E_OVERFLOW, nothing is written.  A spec its check refuses, count == 0, a range
 * outside either chunk, a NULL where data is expected: FQGPU_E_ARG.  Without a GPU the two device calls return
 * FQGPU_E_NO_DEVICE before any argument is looked at; the two host helpers work.
 *
 * THE LIMIT.  fqgpu_chunk_select_limited / fqgpu_dblock_select_limited are the marked calls with one more input:
 *   limit_in   NULL, or end - first uint16_t relative to `first`.  Step 0 becomes a0 = min(a_adapter, limit[i]), a_adapter the
 *              adapter's clip place, or L without an adapter; everything behind step 0 is unchanged.  A limit causes no line
 *              to be read
 *   report     words 14 / 15 keep counting a0 < L / L - a0 | 21 reads_cut_limit (limit < a_adapter) | 22 bases_cut_limit (the
 *              sum of a_adapter - a0) | 23 zero
 * With limit_in == NULL every output is the marked call's, byte for byte. */
#define FQGPU_OVERLAP_MAX_LEN 512
#define FQGPU_OVERLAP_ROWS 1024
#define FQGPU_OVERLAP_WORDS (16 + FQGPU_OVERLAP_ROWS)
typedef struct {
  uint32_t min_overlap, max_mism, max_err_pct;  /* 1 .. 512 | 0 .. 65535 | 0 .. 50 */
  uint32_t reserved[5];                         /* zero */
} fqgpu_overlap;
int fqgpu_overlap_check(const fqgpu_overlap *o);
int fqgpu_chunk_pair_overlap(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, const fqgpu_overlap *o,
                             uint64_t *out, size_t cap_words, uint16_t *limit_a_out, uint16_t *limit_b_out, uint16_t *insert_out);
int fqgpu_dblock_pair_overlap(fqgpu_ctx *ctx, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b, size_t count,
                              const fqgpu_overlap *o, uint64_t *out, size_t cap_words, uint16_t *limit_a_out, uint16_t *limit_b_out,
                              uint16_t *insert_out);
int fqgpu_overlap_merge(uint64_t *dst, size_t dst_words, const uint64_t *src, size_t src_words);
int fqgpu_chunk_select_limited(fqgpu_ctx *ctx, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t, const fqgpu_filter *f,
                               size_t first, size_t end, const uint8_t *mark_in, const uint16_t *limit_in, uint8_t *out, size_t out_cap,
                               size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out, uint16_t *places_out);
int fqgpu_dblock_select_limited(fqgpu_ctx *ctx, const fqgpu_dblock *b, const fqgpu_adapter *a, const fqgpu_tail *x, const fqgpu_trim *t,
                                const fqgpu_filter *f, size_t first, size_t end, const uint8_t *mark_in, const uint16_t *limit_in,
                                uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report, uint8_t *keep_out, uint32_t *win_out,
                                uint16_t *places_out);

/* ---- Extension (nothing in the reference): OVERLAP CORRECTION -- where the mates of a pair disagree inside their overlap and
 * one base is confident while the other is poor, the poor one is replaced (fastp's --correction).  THESE ARE THE CALLS THAT
 * CHANGE A CHUNK: every other call on a staged chunk or a block leaves the chunk as it is; these two patch sequence and quality
 * bytes of both chunks in HBM.  Digest, summary, probe and every selection taken afterwards see the corrected bytes.  A chunk
 * staged by fqgpu_encode_begin has finished its encode by then: the streams fqgpu_encode_end delivers describe the UNCORRECTED
 * chunk, and a block's streams and status likewise describe what its last encode saw.
 * For a pair with the sequence lines s1[0, L1), s2[0, L2), the quality lines q1, q2 and an insert size I -- insert_out's
 * meaning: I = d + L2, or 0 for "no hit" --, comp mapping A<->T, C<->G and N to N.  Integer arithmetic throughout:
 *   I == 0       the pair is untouched and none of its four lines is looked at
 *   I != 0       L1 <= 512, L2 <= 512 and 1 <= I <= L1 + L2 - 1 are required, else FQGPU_E_ARG: the inserts are the caller's
 *                data and not trusted.  d = I - L2, lo = max(0, d), hi = min(L1, I): the overlap, hi - lo >= 1.  Place i in
 *                [lo, hi) of mate 1 stands beside place j = I - 1 - i of mate 2, which lies in [0, L2)
 *   a place      b1 = s1[i], b2 = s2[j], p1 = q1[i] - 33, p2 = q2[j] - 33.  It DISAGREES iff b1 == 'N' or b2 == 'N' or
 *                b1 != comp(b2): the overlap rule's mismatch.  Mate 1 wins iff it disagrees, b1 != 'N', p1 >= good_q and
 *                p2 <= bad_q: s2[j] := comp(b1), q2[j] := q1[i].  Mate 2 wins iff it disagrees, b2 != 'N', p2 >= good_q and
 *                p1 <= bad_q: s1[i] := comp(b2), q1[i] := q2[j].  Otherwise nothing changes.  bad_q < good_q, so the two
 *                exclude each other.  A winner is never N; a loser may be: an N beside a confident base becomes that base
 *   independence every place is decided from the uncorrected bytes of its own four bytes alone, and no byte belongs to two
 *                places: the result does not depend on how the work is split, and a second call with the same inserts
 *                corrects nothing
 * Only the overlap's bytes of the four lines are read and judged: a sequence byte outside ACGTN or a quality byte outside
 * 33 .. 96 there is FQGPU_E_ARG, and so is a record with I != 0 that has length 0 or lies outside its chunk.
 *   report  FQGPU_CORRECT_REPORT_WORDS uint64_t: 0 n_pairs | 1 pairs_with_insert (I != 0) | 2 pairs_corrected (at least one
 *           base changed) | 3 bases_corrected_a (mate 2 won, mate 1 changed) | 4 bases_corrected_b (mate 1 won, mate 2 changed) |
 *           5 n_resolved (corrected places whose old base was N, either mate) | 6 mismatches_seen (disagreeing places before
 *           the correction) | 7 overlap_bases (the sum of hi - lo).  Reports add word by word.  With the inserts of
 *           fqgpu_*_pair_overlap over the same records, words 1, 6 and 7 equal that summary's words 1, 6 and 7
 *   insert_in    count uint16_t, as insert_out
 *   fixed_a_out, fixed_b_out   each NULL, or `count` uint16_t: the places changed in mate 1 and in mate 2 of pair i
 *   fqgpu_correct_check       host only: good_q in 1 .. 63, bad_q in 0 .. 62 and below good_q, reserved zero: FQGPU_OK, else
 *                             FQGPU_E_ARG
 *   fqgpu_chunk_pair_correct  shaped and validated like fqgpu_chunk_pair_overlap -- valid in the same states, both handles of
 *                             one device, every stream of both waited for, then the kernels on ctx_a's stream, waited for --
 *                             but ctx_a == ctx_b is refused: a record would be patched as both mate 1 and mate 2
 *   fqgpu_dblock_pair_correct as fqgpu_dblock_pair_overlap, its waits for the blocks' owners included; ba == bb is refused
 * A spec its check refuses, count == 0, a range outside either chunk, a NULL where data is expected: FQGPU_E_ARG.  EVERY
 * FQGPU_E_ARG LEAVES BOTH CHUNKS EXACTLY AS THEY WERE and zeroes the report and the two arrays: the call judges and counts
 * first and stores only when nothing was refused.  Without a GPU the two device calls return FQGPU_E_NO_DEVICE before any
 * argument is looked at; the check works. */
#define FQGPU_CORRECT_REPORT_WORDS 8
typedef struct {
  uint32_t good_q, bad_q;  /* 1 .. 63 | 0 .. 62, bad_q < good_q */
  uint32_t reserved[6];    /* zero */
} fqgpu_correct;
int fqgpu_correct_check(const fqgpu_correct *c);
int fqgpu_chunk_pair_correct(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, const uint16_t *insert_in,
                             const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out, uint16_t *fixed_b_out);
int fqgpu_dblock_pair_correct(fqgpu_ctx *ctx, fqgpu_dblock *ba, size_t first_a, fqgpu_dblock *bb, size_t first_b, size_t count,
                              const uint16_t *insert_in, const fqgpu_correct *c, uint64_t *report, uint16_t *fixed_a_out,
                              uint16_t *fixed_b_out);

/* ---- Extension (nothing in the reference): MATE MERGING -- the two mates of an overlapping pair written as ONE read, the
 * fragment from its first base to its last (fastp's --merge, FLASH, PEAR), built where both chunks lie: in HBM.  THE CALLS LEAVE
 * BOTH CHUNKS AS THEY ARE: digest, summary and every selection give the same result before and after.
 * For a pair with the lines s1, q1 of length L1 (mate 1), s2, q2 of length L2 (mate 2) and an insert size I -- insert_out's
 * meaning: I = d + L2, or 0 for "no hit" --, comp the overlap rule's complement.  Integer arithmetic throughout:
 *   eligibility  a pair is MERGED iff I != 0, its mark bit is set (no mark: every pair counts as marked) and I >= min_len.
 *                Every other pair is left alone and none of its lines is looked at
 *   the inserts  every pair with I != 0, marked or not, needs L1 <= 512, L2 <= 512 and 1 <= I <= L1 + L2 - 1, else FQGPU_E_ARG:
 *                the inserts are the caller's data, as in the correction
 *   the length   the merged read has exactly I bases (I <= 1023)
 *   place p      in [0, I): j = I - 1 - p, in1 = (p < L1), in2 = (j < L2); at least one holds.  The bases of either mate at or
 *                behind I belong to neither mate's fragment (adapter) and are dropped
 *   one mate     in1 alone: base s1[p], quality q1[p].  in2 alone: base comp(s2[j]), quality q2[j]
 *   both mates   b1 = s1[p], b2 = comp(s2[j]), p1 = q1[p] - 33, p2 = q2[j] - 33.  b1 == b2 and neither is N: b1, Phred
 *                max(p1, p2).  Both N: N, Phred min(p1, p2).  Exactly one N: the other mate's base and Phred.  Two bases that
 *                differ: the base with the higher Phred, mate 1's on a tie, Phred max(p_winner - p_loser, floor_q) (FLASH's
 *                rule).  After fqgpu_*_pair_correct a corrected place agrees, so the two steps compose
 *   the record   mate 1's header line byte for byte with its '\n' | the I bases | "\n+\n" | the I quality bytes | '\n'
 *   the order    merged records appear in pair order; every byte is a function of the pair's own lines and I, so the result
 *                does not depend on how the work is split
 * For merged pairs only, s1, q1 are read and judged over [0, min(L1, I)) and s2, q2 over [0, min(L2, I)): a base outside ACGTN or
 * a quality byte outside 33 .. 96 there is FQGPU_E_ARG, and so is a merged pair's record of length 0 or outside its chunk.
 *   insert_in   count uint16_t, as insert_out
 *   mark_in     NULL, or (count + 7) / 8 bytes in the selection's bit order, relative to the range
 *   merged_out  NULL, or the same size: bit i set iff pair i was merged
 *   out         NULL: everything is judged and counted, *out_len is set, nothing is copied.  Else *out_len bytes, when out_cap
 *               holds them; out_cap < *out_len: FQGPU_E_OVERFLOW, nothing is written to out, *out_len, the report and
 *               merged_out are valid.  *out_len NEVER EXCEEDS the canonical bytes of the two ranges together (a record is its
 *               header line and 2 I + 4 <= 2 L1 + 4 + 2 L2 + 4 bytes): a buffer of that size always holds the result
 *   report      FQGPU_MERGE_REPORT_WORDS uint64_t: 0 n_pairs | 1 pairs_with_insert | 2 pairs_merged | 3 bases_merged (the sum of
 *               I) | 4 bytes_out | 5 overlap_bases (places with both mates, merged pairs only) | 6 places_disagree (the two bases
 *               differ) | 7 places_n (at least one N among both-mate places) | 8 bases_dropped_a (the sum of L1 - min(L1, I)
 *               over merged pairs) | 9 bases_dropped_b | 10 pairs_unmarked (I != 0, mark 0) | 11 pairs_too_short (marked,
 *               0 < I < min_len) | 12 .. 15 zero.  Reports add word by word
 *   fqgpu_merge_check        host only: floor_q in 0 .. 63, min_len in 1 .. 1023, reserved zero: FQGPU_OK, else FQGPU_E_ARG
 *   fqgpu_chunk_pair_merge   shaped and validated exactly like fqgpu_chunk_pair_overlap -- valid in the same states, both
 *                            handles of one device, every stream of both waited for, the kernels on ctx_a's stream, waited for;
 *                            ctx_a == ctx_b is allowed, for nothing is patched
 *   fqgpu_dblock_pair_merge  as fqgpu_dblock_pair_overlap; ba == bb is allowed
 * A spec its check refuses, count == 0, a range outside either chunk, a NULL where data is expected (insert_in, m, out_len,
 * report): FQGPU_E_ARG.  EVERY FQGPU_E_ARG leaves `out` untouched and zeroes *out_len, the report and merged_out.  Without a GPU
 * the two device calls return FQGPU_E_NO_DEVICE before any argument is looked at; the check works. */
#define FQGPU_MERGE_REPORT_WORDS 16
typedef struct {
  uint32_t floor_q, min_len;  /* 0 .. 63 | 1 .. 1023 */
  uint32_t reserved[6];       /* zero */
} fqgpu_merge;
int fqgpu_merge_check(const fqgpu_merge *m);
int fqgpu_chunk_pair_merge(fqgpu_ctx *ctx_a, size_t first_a, fqgpu_ctx *ctx_b, size_t first_b, size_t count, const uint16_t *insert_in,
                           const uint8_t *mark_in, const fqgpu_merge *m, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *report,
                           uint8_t *merged_out);
int fqgpu_dblock_pair_merge(fqgpu_ctx *ctx, const fqgpu_dblock *ba, size_t first_a, const fqgpu_dblock *bb, size_t first_b, size_t count,
                            const uint16_t *insert_in, const uint8_t *mark_in, const fqgpu_merge *m, uint8_t *out, size_t out_cap,
                            size_t *out_len, uint64_t *report, uint8_t *merged_out);

/* Pinned (page-locked) host memory for the buffers that cross PCIe: the shim's FastqChunk::raw_data
 * and CompressedBuffers::seq/qual live in it, so that fqgpu_encode_block / fqgpu_decode_block copy
 * at the full link rate and asynchronously.  Without a usable GPU the memory is ordinary heap
 * memory (host-only tools and tests still run); there is still no compute fallback.
 * fqgpu_host_free keeps pinned blocks in a cache (hipHostFree waits until the device is idle: a
 * worker thread freeing a buffer would wait for every other worker's kernels); fqgpu_host_trim
 * returns the cache to the system (bytes freed).  Limit of the cache: FQGPU_PINNED_CACHE_MB (8192). */
void *fqgpu_host_alloc(size_t bytes);
void fqgpu_host_free(void *p);
size_t fqgpu_host_trim(void);

/* memcompress / memdecompress (src/memcompress.h:5-28) for the misc streams -- readlens, n_count,
 * n_pos and the header field streams, src/workspace.cpp:176-256.  The reference uses libbsc
 * (third party, source absent): the compressed BYTES are this library's own format and out of
 * parity scope; the contract is the reference's: dst holds src_size + 28 bytes
 * (extra_csize_misc, src/workspace.h:18), empty in = empty out, the original size travels in the
 * container.  fqgpu_memdecompress returns dst_size, 0 for an empty input, (size_t)-1 if malformed. */
size_t fqgpu_memcompress_bound(size_t src_size);
size_t fqgpu_memcompress(uint8_t *dst, size_t dst_cap, const uint8_t *src, size_t src_size);
size_t fqgpu_memdecompress(uint8_t *dst, size_t dst_size, const uint8_t *src, size_t src_size);

#ifdef __cplusplus
}
#endif
#endif
