// vsx_merge_internal.h -- shared between the merge kernel (vsx_merge.hip) and its host side (vsx_merge.cpp).
#ifndef VSX_MERGE_INTERNAL_H
#define VSX_MERGE_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "../../include/vsx_merge.h"

#define VSX_MERGE_THREADS 64          // one wavefront per pair

// what the kernel needs of vsx_merge_opts, plus the tables (device pointers).  Quality SYMBOLS index the tables, as in the
// reference; `tlo`/`tdim` is the symbol range the call can produce (qmin..qmax and the symbol N's are forced to).
struct VsxMergeParams {
  int64_t truncqual, maxns, minlen, maxlen, minovlen, maxdiffs, minmergelen, maxmergelen;
  double  maxdiffpct, maxee, minscore;
  int32_t ascii, qmin, qmax, mindiagcount, allowstagger, tlo, tdim, pad;
  const double *  match;              // tdim x tdim
  const double *  mism;               // tdim x tdim
  const uint8_t * qual_same;          // tdim x tdim: merged quality symbol, symbols agree
  const uint8_t * qual_diff;          // tdim x tdim: symbols disagree, first index = the higher quality
  const double *  q2p;                // 128, by symbol
};

// one pair of a window: where its bytes lie in the packed input (fwd seq, fwd qual, rev seq, rev qual, back to back)
// and where its merged sequence / quality go (capacity flen + rlen each)
struct VsxMergeItem {
  uint64_t in_off;
  uint64_t out_off;
  uint32_t flen, rlen;                // both 0 with host == 1
  uint32_t host;                      // 1: not for the kernel (a read above VSX_MERGE_MAX_LEN)
  uint32_t pad;
};

struct VsxMergeDevRec {
  int32_t merged, reason, fwd_trunc, rev_trunc, merged_length, fwd_errors, rev_errors;
  int32_t qerr;                       // 0, or 1: quality below qmin, 2: above qmax (the first one in the reference's reading order)
  int32_t qerr_value;
  int32_t ndiag;                      // diagonals scored
  double  ee_merged, ee_fwd, ee_rev;
};

// vsx_merge.hip: one wavefront per item; items with host == 1 are skipped
#ifdef __cplusplus
extern "C"
#endif
hipError_t vsx_launch_merge(const VsxMergeItem * d_items, uint32_t n_items, const uint8_t * d_blob, VsxMergeParams P,
                            VsxMergeDevRec * d_recs, uint8_t * d_oseq, uint8_t * d_oqual, hipStream_t st);

#ifdef __HIPCC__
#define VSX_MG_HD __host__ __device__ inline
#else
#define VSX_MG_HD inline
#endif

// the FASTQ reader's symbol map: letters upper-cased, everything else N
VSX_MG_HD uint8_t vsx_mg_upcase(uint8_t c)
{
  if (c >= 'a' && c <= 'z') return (uint8_t) (c - 32);
  if (c >= 'A' && c <= 'Z') return c;
  return 'N';
}

// IUPAC complement of an upper-case symbol; letters that are no nucleotide code give N
VSX_MG_HD uint8_t vsx_mg_complement(uint8_t c)
{
  switch (c)
    {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': case 'U': return 'A';
    case 'R': return 'Y'; case 'Y': return 'R'; case 'K': return 'M'; case 'M': return 'K';
    case 'B': return 'V'; case 'V': return 'B'; case 'D': return 'H'; case 'H': return 'D';
    case 'S': return 'S'; case 'W': return 'W';
    default:  return 'N';
    }
}

// 2-bit code of an unambiguous symbol (T and U share one), `ambig` for every other symbol
VSX_MG_HD uint8_t vsx_mg_code(uint8_t c, uint8_t ambig)
{
  switch (c)
    {
    case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': case 'U': return 3;
    default:  return ambig;
    }
}

#endif
