// vsx_hitout_internal.h -- shared between the hit-text kernels (vsx_hitout.hip) and their host side (vsx_hitout.cpp).
// Run words are the library's ((length << 2) | op, op 0 = M, 1 = I, 2 = D; include/vsx.h), here in TEXT order: the run of the
// alignment's first column first.  The host has checked every job: the runs sum to ncols columns, qlen query and tlen target symbols,
// no run is empty, [c0, c0 + ilen) lies inside [0, ncols), and every offset has its bytes.
#ifndef VSX_HITOUT_INTERNAL_H
#define VSX_HITOUT_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#define VSX_HITJOB_NO 0xFFFFFFFFFFFFFFFFull  // a row nobody asked for

struct VsxHitJob {
  uint64_t q_off;        // the hit's strand (plus, or the separately masked reverse complement) in the query text: qrow, MD
  uint64_t qp_off;       // the plus strand's masked text: a minus-strand hit's --alnout row reads it backwards, complemented
  uint64_t t_off;        // the target in the database text
  uint64_t run_off;      // first run word
  uint64_t qrow_off, trow_off, sym_off, aln_off;   // into the row buffer, ilen bytes each, or VSX_HITJOB_NO
  uint32_t nruns;
  uint32_t qlen;
  uint32_t ncols;        // columns of the untrimmed alignment
  uint32_t c0, ilen;     // the trimmed columns
  uint32_t minus;
};

#ifdef __cplusplus
extern "C" {
#endif
// one wavefront per hit: qrow, trow, the symbol row and the --alnout query row over the trimmed columns
hipError_t vsx_launch_hitout_rows(const VsxHitJob * d_jobs, uint32_t n, const uint8_t * d_qtext, const uint8_t * d_dbtext, const uint32_t * d_runs,
                                  uint8_t * d_rows, int n_mismatch, hipStream_t st);
// one wavefront per hit: the byte length of its MD string
hipError_t vsx_launch_hitout_md_count(const VsxHitJob * d_jobs, uint32_t n, const uint8_t * d_qtext, const uint8_t * d_dbtext, const uint32_t * d_runs,
                                      uint32_t * d_md_len, hipStream_t st);
// exclusive sum of the lengths, in 64 bits; temp NULL: the temporary bytes only
hipError_t vsx_launch_hitout_md_scan(void * temp, size_t * temp_bytes, const uint32_t * d_md_len, uint64_t * d_md_off, uint32_t n, hipStream_t st);
// one wavefront per hit: the MD string at d_md + d_md_off[hit]
hipError_t vsx_launch_hitout_md_fill(const VsxHitJob * d_jobs, uint32_t n, const uint8_t * d_qtext, const uint8_t * d_dbtext, const uint32_t * d_runs,
                                     const uint64_t * d_md_off, uint8_t * d_md, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
