// vsx_filter_internal.h -- shared between the filter kernel (vsx_filter.hip) and its host side (vsx_filter.cpp).
#ifndef VSX_FILTER_INTERNAL_H
#define VSX_FILTER_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/vsx_filter.h"

#define VSX_FILTER_WAVES   4          // one wavefront per read, four reads per workgroup
#define VSX_FILTER_THREADS (64 * VSX_FILTER_WAVES)
#define VSX_FILTER_PAD     64         // bytes behind each staged span on the device

// what the kernel needs of vsx_fastx_filter_opts, plus the table (device pointer)
struct VsxFilterParams {
  int64_t stripleft, stripright, trunclen, trunclen_keep, truncqual, minqual, minlen, maxlen, maxns;
  double  maxee, maxee_rate, truncee, truncee_rate;
  int32_t ascii, qmin, qmax;
  int32_t has_qual;                   // 0: FASTA input, the quality walk and the expected-error filters are skipped
  const double * q2e;                 // 128, by quality symbol: 10^(-q/10) for offset + qmin .. offset + qmax, 0 elsewhere
};

// one read of a window: where it lies in the staged span (the caller's offset, rebased)
struct VsxFilterItem {
  uint32_t off, len;
};

// vsx_fastx_filter_record with the kernel's error report in its padding
struct VsxFilterDevRec {
  int32_t start, length;
  double  ee;
  uint8_t discarded, truncated;
  uint8_t qerr;                       // 0, or 1: quality below qmin, 2: above qmax (the first one in the reference's reading order)
  uint8_t pad;
  int32_t qerr_value;
};

// vsx_filter.hip: one wavefront per item.  d_seq / d_qual: the staged spans (d_qual unused without has_qual)
#ifdef __cplusplus
extern "C"
#endif
hipError_t vsx_launch_filter(const VsxFilterItem * d_items, uint32_t n_items, const uint8_t * d_seq, const uint8_t * d_qual,
                             VsxFilterParams P, VsxFilterDevRec * d_recs, hipStream_t st);

#endif
