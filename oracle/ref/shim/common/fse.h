/*
 * oracle/ref/shim/common/fse.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Stands where zstd's common/fse.h stands on the reference's include path, so that the
 * reference's own sources compile unmodified into oracle/_ref/ref_tool (oracle/Makefile,
 * target `ref`).  It carries the names the reference uses (src/fse_common.hpp and the two
 * coders) and forwards each to oracle/fse_oracle.{h,c}: the arithmetic behind them is
 * fse_oracle.c's, pinned to libzstd 1.4.8 by tests/test_oracle_zstd.py; everything above
 * it -- contexts, symbol order, flush order, N handling, headers, container -- is the
 * reference's compiled code.  Nothing of zstd is linked.
 *
 * The size macros follow zstd 1.5's formulas (lib/common/fse.h); tests/test_reference_pin.py
 * checks them against what libzstd's FSE_build{C,D}Table_wksp accept.
 */
#ifndef FQC_REF_SHIM_FSE_H
#define FQC_REF_SHIM_FSE_H

#include "bitstream.h"

typedef unsigned FSE_CTable;
typedef unsigned FSE_DTable;
typedef unsigned char FSE_FUNCTION_TYPE;

#define FSE_MAX_MEMORY_USAGE 14
#define FSE_MAX_TABLELOG (FSE_MAX_MEMORY_USAGE - 2)
#define FSE_TABLELOG_ABSOLUTE_MAX 15

#define FSE_CTABLE_SIZE_U32(maxTableLog, maxSymbolValue) \
  (1 + (1 << ((maxTableLog)-1)) + (((maxSymbolValue) + 1) * 2))
#define FSE_DTABLE_SIZE_U32(maxTableLog) (1 + (1 << (maxTableLog)))

#define FSE_BUILD_CTABLE_WORKSPACE_SIZE_U32(maxSymbolValue, tableLog) \
  (((maxSymbolValue + 2) + (1ull << (tableLog))) / 2 + sizeof(unsigned long long) / sizeof(unsigned))
#define FSE_BUILD_CTABLE_WORKSPACE_SIZE(maxSymbolValue, tableLog) \
  (sizeof(unsigned) * FSE_BUILD_CTABLE_WORKSPACE_SIZE_U32(maxSymbolValue, tableLog))

#define FSE_BUILD_DTABLE_WKSP_SIZE(maxTableLog, maxSymbolValue) \
  (sizeof(short) * (maxSymbolValue + 1) + (1ULL << maxTableLog) + 8)
#define FSE_BUILD_DTABLE_WKSP_SIZE_U32(maxTableLog, maxSymbolValue) \
  ((FSE_BUILD_DTABLE_WKSP_SIZE(maxTableLog, maxSymbolValue) + sizeof(unsigned) - 1) / sizeof(unsigned))

/* zstd reports errors as (size_t)-code; the reference only compares against 0 or the expected value */
#define FQC_REF_SHIM_ERROR ((size_t)-1)

static inline unsigned FSE_optimalTableLog(unsigned maxTableLog, size_t srcSize, unsigned maxSymbolValue) {
  return fo_optimal_table_log(maxTableLog, srcSize, maxSymbolValue);
}

static inline size_t FSE_normalizeCount(short *normalizedCounter, unsigned tableLog, const unsigned *count,
                                        size_t srcSize, unsigned maxSymbolValue, unsigned useLowProbCount) {
  const int r = fo_normalize_count(normalizedCounter, tableLog, count, srcSize, maxSymbolValue, (int)useLowProbCount);
  return r < 0 ? FQC_REF_SHIM_ERROR : (size_t)r;
}

static inline size_t FSE_buildCTable_wksp(FSE_CTable *ct, const short *normalizedCounter, unsigned maxSymbolValue,
                                          unsigned tableLog, void *workSpace, size_t wkspSize) {
  (void)workSpace;
  if (wkspSize < FSE_BUILD_CTABLE_WORKSPACE_SIZE(maxSymbolValue, tableLog)) return FQC_REF_SHIM_ERROR;
  return fo_build_ctable(ct, normalizedCounter, maxSymbolValue, tableLog) == 0 ? 0 : FQC_REF_SHIM_ERROR;
}

static inline size_t FSE_buildDTable_wksp(FSE_DTable *dt, const short *normalizedCounter, unsigned maxSymbolValue,
                                          unsigned tableLog, void *workSpace, size_t wkspSize) {
  (void)workSpace;
  if (wkspSize < FSE_BUILD_DTABLE_WKSP_SIZE(tableLog, maxSymbolValue)) return FQC_REF_SHIM_ERROR;
  return fo_build_dtable(dt, normalizedCounter, maxSymbolValue, tableLog) == 0 ? 0 : FQC_REF_SHIM_ERROR;
}

typedef fo_cstate FSE_CState_t;
typedef fo_dstate FSE_DState_t;

static inline void FSE_initCState(FSE_CState_t *statePtr, const FSE_CTable *ct) { fo_cstate_init(statePtr, ct); }
static inline void FSE_encodeSymbol(BIT_CStream_t *bitC, FSE_CState_t *statePtr, unsigned symbol) {
  fo_encode_symbol(bitC, statePtr, symbol);
}
static inline void FSE_flushCState(BIT_CStream_t *bitC, const FSE_CState_t *statePtr) { fo_cstate_flush(bitC, statePtr); }

static inline void FSE_initDState(FSE_DState_t *DStatePtr, BIT_DStream_t *bitD, const FSE_DTable *dt) {
  fo_dstate_init(DStatePtr, bitD, dt);
}
static inline unsigned char FSE_decodeSymbol(FSE_DState_t *DStatePtr, BIT_DStream_t *bitD) {
  return (unsigned char)fo_decode_symbol(DStatePtr, bitD);
}

#endif
