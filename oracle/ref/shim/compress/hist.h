/*
 * oracle/ref/shim/compress/hist.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The reference includes zstd's compress/hist.h (src/fse_common.hpp) and calls nothing of it:
 * its two models count symbols themselves.  This file only has to exist.
 */
#ifndef FQC_REF_SHIM_HIST_H
#define FQC_REF_SHIM_HIST_H
#endif
