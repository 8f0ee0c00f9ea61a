/* vsx_filter.h -- read quality filtering (the analysis core of the reference's --fastq_filter / --fastx_filter, --reverse
 * pairs included) on the GPU.
 *
 * Reads go in as host blobs (the blob / offset / length convention of vsx_merge_pairs); one record per read comes out:
 * (start, length) of the substring of the caller's own read that survives stripping and truncation, its expected error and
 * the verdict.  Nothing is copied back but the records.  Results are bit-identical to the reference: the table of
 * 10^(-q/10) is built on the host, and the device only adds, subtracts, divides and compares doubles in the reference's order.
 *
 * Symbols and qualities are taken as the reference's reader delivers them to `analyse` (case preserved: only 'N' and 'n'
 * count as N).  FASTQ / FASTA parsing and writing, relabelling and the size / length / sample annotations stay with the
 * caller, who also resolves the abundances (--sizein, or 1).
 */
#ifndef VSX_FILTER_H
#define VSX_FILTER_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the Parameters fields `analyse` reads (defaults: the reference's, src/vsearch.h) */
typedef struct vsx_fastx_filter_opts {
  int64_t ascii;          /* 33 */
  int64_t qmin;           /* 0 */
  int64_t qmax;           /* 41 */
  int64_t stripleft;      /* 0 */
  int64_t stripright;     /* 0 */
  int64_t trunclen;       /* -1: not set */
  int64_t trunclen_keep;  /* -1: not set */
  int64_t truncqual;      /* LONG_MIN: not set */
  int64_t minqual;        /* 0 */
  int64_t minlen;         /* 1 */
  int64_t maxlen;         /* INT64_MAX */
  int64_t maxns;          /* INT64_MAX */
  int64_t minsize;        /* 0 */
  int64_t maxsize;        /* INT64_MAX */
  double  maxee;          /* DBL_MAX */
  double  maxee_rate;     /* DBL_MAX */
  double  truncee;        /* DBL_MAX */
  double  truncee_rate;   /* DBL_MAX */
  int64_t window;         /* reads per staging window; 0: the built-in size.  Results do not depend on it. */
} vsx_fastx_filter_opts;

/* one side of the input: the forward reads, or the reads of --reverse */
typedef struct vsx_fastx_reads {
  const char *     seq;        /* sequence blob */
  const char *     qual;       /* quality blob, same offsets; NULL: FASTA input (no quality walk, ee = -1.0) */
  uint64_t         bytes;      /* size of each blob */
  const uint64_t * off;        /* n offsets */
  const uint32_t * len;        /* n lengths, each <= INT32_MAX */
  const uint64_t * abundance;  /* n abundances; NULL: every read has abundance 1 */
} vsx_fastx_reads;

/* one read: [start, start + length) of the input read is what the command would print */
typedef struct vsx_fastx_filter_record {
  int32_t start;
  int32_t length;
  double  ee;             /* expected error of the printed part; -1.0 for FASTA input */
  uint8_t discarded;
  uint8_t truncated;      /* length < the read's length */
  uint8_t pad[6];
} vsx_fastx_filter_record;

typedef struct vsx_fastx_filter_out {
  uint64_t                  n;
  vsx_fastx_filter_record * fwd;             /* n records, input order */
  vsx_fastx_filter_record * rev;             /* n records, or NULL without reverse reads */
  uint8_t *                 pair_discarded;  /* n: the read (the pair, if either of its reads) is discarded */
  uint64_t                  kept;            /* the three totals the command prints */
  uint64_t                  kept_truncated;
  uint64_t                  discarded;
} vsx_fastx_filter_out;

typedef struct vsx_fastx_filter_stats {
  double   seconds_stage;        /* host: planning the windows, copying their spans into pinned memory, enqueueing */
  double   seconds_h2d;          /* device time of the host-to-device copies (events), summed over the windows */
  double   seconds_kernel;       /* device time of the filter kernel (events), summed over the windows */
  double   seconds_d2h_output;   /* waiting for the records + building the output */
  double   seconds_total;
  uint64_t reads;                /* forward + reverse */
  uint64_t windows;
  uint64_t reads_host;           /* reads answered by the host restatement (VSX_FILTER=host) */
} vsx_fastx_filter_stats;

void vsx_fastx_filter_opts_default(vsx_fastx_filter_opts * o);

/* Analyse n reads (rev == NULL) or n read pairs.  ctx may be NULL only when the environment has VSX_FILTER=host (every read
 * through the host restatement).  Option values the reference's check_parameters refuses, a quality offset with
 * offset + qmin or offset + qmax outside 0..127, a read beyond its blob or longer than INT32_MAX give VSX_EINVAL.  A quality
 * value outside [qmin, qmax] where the reference reads it fails the call with VSX_EINVAL too; vsx_last_error() names the
 * value and the bound of the first one in the reference's order (read 0 forward, read 0 reverse, read 1 forward, ...). */
int vsx_fastx_filter(vsx_ctx * ctx, const vsx_fastx_filter_opts * opts, uint64_t n,
                     const vsx_fastx_reads * fwd, const vsx_fastx_reads * rev, vsx_fastx_filter_out * out);
void vsx_fastx_filter_out_free(vsx_fastx_filter_out * out);

/* figures of this thread's last vsx_fastx_filter call */
void vsx_fastx_filter_last_stats(vsx_fastx_filter_stats * out);

#ifdef __cplusplus
}
#endif
#endif
