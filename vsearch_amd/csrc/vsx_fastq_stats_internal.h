// vsx_fastq_stats_internal.h -- shared between the read-summary kernels (vsx_fastq_stats.hip) and their host side (vsx_fastq_stats.cpp).
#ifndef VSX_FASTQ_STATS_INTERNAL_H
#define VSX_FASTQ_STATS_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/vsx_fastq_stats.h"
#include "vsx_eestats_internal.h"          // VsxEestatsItem and the ordered-sum kernel, used as they are

#define VSX_FQS_THREADS   VSX_EESTATS_THREADS      // both kernels: one lane per read, 256 reads per workgroup
#define VSX_FQS_TILE      64                       // positions a workgroup brings into LDS at a time
#define VSX_FQS_ROW_WORDS 17                       // LDS row of a read's tile: 64 bytes + one word, so that lanes fall on different banks
#define VSX_FQS_SYMS      VSX_FASTQ_STATS_SYMBOLS
#define VSX_FQS_FIRST     VSX_FASTQ_STATS_FIRST_SYMBOL
#define VSX_FQS_NO_SYMBOL 0xFFFFFFFFu              // minmax of a read without a symbol

struct VsxFastqStatsParams {
  int32_t  ascii;
  uint32_t stride;                    // reads per row of the matrix
  uint32_t len_max;
  uint32_t pad;
  const double * q2e;                 // 256, by quality symbol: 10^(-score/10), score = symbol - ascii, 0 below ascii
  uint32_t * symbol_counts;           // [len_max][94]
  uint32_t * prefix_hist;             // [8][len_max + 1]: reads by the length of the prefix on which a threshold holds; rows 0 .. 3 the
                                      // expected-error thresholds 1.0, 0.5, 0.25, 0.1, rows 4 .. 7 the score thresholds 5, 10, 15, 20
  double *   matrix;                  // [len_max][stride]: the running expected error of the window's read r at position i
};

// what the chars kernel accumulates over the windows of a call
struct VsxFastqCharsAcc {
  unsigned long long seq[256], qual[256], tail[256];
  int32_t  maxrun[256];
  uint32_t qmin_n, qmax_n;            // 255 and 0 before the first N
};

#ifdef __cplusplus
extern "C" {
#endif
// stats walk: per read the lowest and highest quality character (low | high << 8, VSX_FQS_NO_SYMBOL for an empty read) go to
// d_minmax; counts go to the tables of P by integer atomics, the running expected error to P.matrix
hipError_t vsx_launch_fastq_stats_walk(const VsxEestatsItem * d_items, uint32_t n_items, const uint8_t * d_qual, VsxFastqStatsParams P,
                                       uint32_t * d_minmax, hipStream_t st);
// chars: per read 1 goes to d_err when it holds a quality byte outside 33 ... 126, 0 otherwise; tail: 1 .. 2^31
hipError_t vsx_launch_fastq_chars(const VsxEestatsItem * d_items, uint32_t n_items, const uint8_t * d_seq, const uint8_t * d_qual,
                                  uint32_t tail, VsxFastqCharsAcc * d_acc, uint32_t * d_err, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
