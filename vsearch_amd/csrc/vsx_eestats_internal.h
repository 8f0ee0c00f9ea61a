// vsx_eestats_internal.h -- shared between the read-statistics kernels (vsx_eestats.hip) and their host side (vsx_eestats.cpp).
#ifndef VSX_EESTATS_INTERNAL_H
#define VSX_EESTATS_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/vsx_eestats.h"

#define VSX_EESTATS_THREADS   256        // walk kernel: one lane per read, 256 reads per workgroup
#define VSX_EESTATS_TILE      64         // positions a workgroup brings into LDS at a time
#define VSX_EESTATS_ROW_WORDS 17         // LDS row of a read's tile: 64 bytes + one word, so that lanes fall on different banks
#define VSX_EESTATS_MAX_COLS  96         // qmax + 2 <= 126 - 33 + 2
#define VSX_EESTATS_SUM_POS   16         // ordered-sum kernel: positions (chains) per workgroup
#define VSX_EESTATS_SUM_READS 256        //                     reads staged through LDS per step
#define VSX_EESTATS_RESOLUTION 1000      // bins per expected error of the reference's histogram
#define VSX_EESTATS_NO_ERROR  0xFFFFFFFFu
// Positions below this one combine equal histogram bins inside the wave before the atomic (early positions see a handful of
// distinct bins); from it on every lane issues its own.  A multiple of the tile.  Measured: DESIGN.md 7.z.
#ifndef VSX_EESTATS_COMBINE_BELOW
#define VSX_EESTATS_COMBINE_BELOW 64
#endif

// one read of a window: where it lies in the staged quality span (the caller's offset, rebased)
struct VsxEestatsItem {
  uint32_t off, len;
};

struct VsxEestatsParams {
  int32_t  ascii, qmin, qmax;
  int32_t  cols;                      // qmax + 2
  int32_t  want_tables, want_cutoffs;
  int32_t  shortest, increment;       // eestats2: position i is a cutoff position when i + 1 == shortest + x * increment, x < len_steps
  int32_t  len_steps, n_cutoffs;
  uint32_t stride;                    // reads per row of the matrix
  uint32_t pad;
  const double * q2e;                 // 128, by quality symbol: 10^(-max(q, 0)/10) for ascii + qmin .. ascii + qmax, 0 elsewhere
  const double * cutoffs;             // n_cutoffs
  uint32_t * qual_counts;             // [len_max][cols]
  uint32_t * hist;                    // ee_start(len_max) counters, row i at ee_start(i) with 1000 * (i + 1) + 1 bins
  uint32_t * cutoff_counts;           // [len_steps][n_cutoffs]
  double *   matrix;                  // [len_max][stride]: the running expected error of the window's read r at position i
};

#ifdef __cplusplus
extern "C" {
#endif
// walk: per read the first out-of-range position or VSX_EESTATS_NO_ERROR goes to d_err; counts go to the tables of P by integer atomics
hipError_t vsx_launch_eestats_walk(const VsxEestatsItem * d_items, uint32_t n_items, const uint8_t * d_qual, VsxEestatsParams P,
                                   uint32_t * d_err, hipStream_t st);
// ordered sum: d_sum[i] += matrix[i][r] for r = 0 .. n_items - 1 in that order, reads shorter than i adding +0.0
hipError_t vsx_launch_eestats_sum(const double * d_matrix, uint32_t stride, const VsxEestatsItem * d_items, uint32_t n_items,
                                  uint32_t len_max, double * d_sum, hipStream_t st);
// quantiles: d_bins[i][5] = Min, Low, Med, Hi, Max bin of row i of the histogram
hipError_t vsx_launch_eestats_quantile(const uint32_t * d_hist, const uint64_t * d_reads_at, uint32_t len_max, int64_t * d_bins,
                                       hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
