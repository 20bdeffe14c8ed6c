/*
 * oracle/ref/shim/common/bitstream.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * zstd's bit-stream names, as the reference uses them, over oracle/fse_oracle.h (see fse.h
 * beside this file).  The reader of fse_oracle.c is positional -- it refetches its window on
 * every read -- so BIT_reloadDStream has nothing to do.
 */
#ifndef FQC_REF_SHIM_BITSTREAM_H
#define FQC_REF_SHIM_BITSTREAM_H

#include <stddef.h>

#include "fse_oracle.h"

typedef fo_bitw BIT_CStream_t;
typedef fo_bitr BIT_DStream_t;

/* 0 on success, an error code (non-zero) if the buffer cannot hold the writer's window */
static inline size_t BIT_initCStream(BIT_CStream_t *bitC, void *dstBuffer, size_t dstCapacity) {
  return fo_bitw_init(bitC, dstBuffer, dstCapacity) == 0 ? 0 : (size_t)-1;
}
static inline void BIT_addBits(BIT_CStream_t *bitC, size_t value, unsigned nbBits) { fo_bitw_add(bitC, value, nbBits); }
static inline void BIT_flushBitsFast(BIT_CStream_t *bitC) { fo_bitw_flush_fast(bitC); }
static inline void BIT_flushBits(BIT_CStream_t *bitC) { fo_bitw_flush(bitC); }
static inline size_t BIT_closeCStream(BIT_CStream_t *bitC) { return fo_bitw_close(bitC); }

/* srcSize on success, an error code otherwise */
static inline size_t BIT_initDStream(BIT_DStream_t *bitD, const void *srcBuffer, size_t srcSize) {
  return fo_bitr_init(bitD, srcBuffer, srcSize) == 0 ? srcSize : (size_t)-1;
}
static inline void BIT_reloadDStream(BIT_DStream_t *bitD) { (void)bitD; } /* nothing to reload; the reference ignores the result */
static inline unsigned BIT_endOfDStream(const BIT_DStream_t *bitD) { return (unsigned)fo_bitr_finished(bitD); }

#endif
