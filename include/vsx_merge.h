/* vsx_merge.h -- paired-end read merging (the reference's --fastq_mergepairs core: process -> optimize -> merge) on the GPU.
 *
 * Reads go in as host blobs (the blob / offset / length convention of vsx_search_batch), one record per pair comes out,
 * plus a blob of merged sequences and a blob of merged quality strings.  Results are bit-identical to the reference:
 * the score tables are built on the host exactly as precompute_qual builds them, and the device only adds and compares
 * doubles in the reference's order.
 *
 * Symbols are taken as the reference's FASTQ reader delivers them to the merge core: upper-cased, every byte that is not a
 * letter read as 'N'.  FASTQ parsing and writing, the command's file-level statistics and labels stay with the caller.
 */
#ifndef VSX_MERGE_H
#define VSX_MERGE_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Reads longer than this (after nothing but the length checks) are answered by the host restatement of the same functions.
 * The kernel keeps a pair's symbols, qualities, 2-bit codes, merged quality and diagonal list in LDS: 12 bytes per base of
 * the longer read + 1 KiB, i.e. 7 KiB per one-wave workgroup at 512. */
#define VSX_MERGE_MAX_LEN 512

/* the Parameters fields process / optimize / merge / precompute_qual read (defaults: the reference's, src/vsearch.h) */
typedef struct vsx_merge_opts {
  int64_t fastq_ascii;             /* 33 */
  int64_t fastq_qmin;              /* 0 */
  int64_t fastq_qmax;              /* 41 */
  int64_t fastq_qminout;           /* 0 */
  int64_t fastq_qmaxout;           /* 41 */
  int64_t fastq_minovlen;          /* 10; values below 5 are read as 5; below 9 the diagonal-count and score thresholds relax */
  int64_t fastq_maxdiffs;          /* 10 */
  double  fastq_maxdiffpct;        /* 100.0 */
  int64_t fastq_minmergelen;       /* 0 */
  int64_t fastq_maxmergelen;       /* 1000000 */
  double  fastq_maxee;             /* DBL_MAX */
  int64_t fastq_truncqual;         /* LONG_MIN */
  int64_t fastq_maxns;             /* INT64_MAX */
  int64_t fastq_minlen;            /* 1 */
  int64_t fastq_maxlen;            /* INT64_MAX */
  int32_t fastq_allowmergestagger; /* 0 */
  int32_t pad;
  int64_t window;                  /* pairs per pipeline window; 0: the built-in size.  Results do not depend on it. */
} vsx_merge_opts;

/* the reference's Reason values that process() can leave behind */
enum {
  VSX_MERGE_OK = 0, VSX_MERGE_MINLEN, VSX_MERGE_MAXLEN, VSX_MERGE_MAXNS, VSX_MERGE_MINOVLEN, VSX_MERGE_MAXDIFFS,
  VSX_MERGE_MAXDIFFPCT, VSX_MERGE_STAGGERED, VSX_MERGE_REPEAT, VSX_MERGE_MINMERGELEN, VSX_MERGE_MAXMERGELEN,
  VSX_MERGE_MAXEE, VSX_MERGE_MINSCORE, VSX_MERGE_NOKMERS, VSX_MERGE_N_REASONS
};

/* one pair.  merged, reason, fwd_trunc, rev_trunc are always set; the rest only where merged == 1 (zero otherwise;
 * a pair rejected by maxee keeps its zeros too). */
typedef struct vsx_merge_record {
  int32_t  merged;          /* 0 / 1 */
  int32_t  reason;          /* VSX_MERGE_* */
  int32_t  fwd_trunc;
  int32_t  rev_trunc;
  int32_t  merged_length;
  int32_t  overlap_length;  /* fwd_trunc + rev_trunc - merged_length */
  int32_t  fwd_errors;
  int32_t  rev_errors;
  double   ee_merged;
  double   ee_fwd;
  double   ee_rev;
  uint64_t blob_off;        /* start of this pair's merged_length bytes in seq_blob and in qual_blob */
} vsx_merge_record;

typedef struct vsx_merge_out {
  uint64_t           n;
  vsx_merge_record * rec;          /* n records, input order */
  char *             seq_blob;     /* merged sequences, back to back in input order */
  char *             qual_blob;    /* merged quality strings, same offsets */
  uint64_t           blob_bytes;
} vsx_merge_out;

typedef struct vsx_merge_stats {
  double   seconds_stage;          /* packing the windows + H2D */
  double   seconds_kernel;         /* device time of the merge kernel (events) */
  double   seconds_unpack;         /* D2H + building the output */
  double   seconds_total;
  uint64_t pairs;
  uint64_t windows;
  uint64_t diagonals_scored;       /* candidate diagonals that passed the 5-mer census and were scored */
  uint64_t pairs_host;             /* pairs answered by the host restatement (long reads, VSX_MERGE=host) */
} vsx_merge_stats;

void vsx_merge_opts_default(vsx_merge_opts * o);

/* Merge n read pairs.  fwd / rev: sequence and quality blobs with offsets (into both the sequence and the quality blob of
 * that side) and lengths.  ctx may be NULL only when the environment has VSX_MERGE=host (every pair through the host
 * restatement).  A quality value outside [qmin, qmax] where the reference reads it fails the call with VSX_EINVAL and
 * vsx_last_error() names the value and the bound; nothing is returned then. */
int vsx_merge_pairs(vsx_ctx * ctx, const vsx_merge_opts * opts, uint64_t n,
                    const char * fwd_seq, const char * fwd_qual, uint64_t fwd_bytes, const uint64_t * fwd_off, const uint32_t * fwd_len,
                    const char * rev_seq, const char * rev_qual, uint64_t rev_bytes, const uint64_t * rev_off, const uint32_t * rev_len,
                    vsx_merge_out * out);
void vsx_merge_out_free(vsx_merge_out * out);

/* figures of this thread's last vsx_merge_pairs call */
void vsx_merge_last_stats(vsx_merge_stats * out);

#ifdef __cplusplus
}
#endif
#endif
