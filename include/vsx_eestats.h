/* vsx_eestats.h -- read quality statistics (the analysis core of the reference's --fastq_eestats and --fastq_eestats2) on the GPU.
 *
 * One accumulation call walks every quality symbol of every read and returns the tables both commands print from: integer
 * counts, and per position one double, the sum over the reads in input order of the running expected error.  The counts are
 * accumulated in any order; the double is formed in the reference's order (position order within a read, read order within a
 * position), so every printed figure is bit-identical to the reference.  The table of 10^(-q/10) is built on the host; the
 * device only adds, multiplies by 1000.0, truncates and compares doubles.
 *
 * Reads go in as host blobs (the vsx_fastx_reads convention of vsx_filter.h); only `qual`, `bytes`, `off` and `len` are read.
 * FASTQ parsing and the printing of the tables stay with the caller (vsearch_amd/eestats.py has both formatters).
 */
#ifndef VSX_EESTATS_H
#define VSX_EESTATS_H

#include "vsx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_EESTATS_WANT_EESTATS  1u     /* reads_at, qual_counts, sum_ee, ee_bins */
#define VSX_EESTATS_WANT_EESTATS2 2u     /* cutoff_counts */

/* The expected-error histogram of --fastq_eestats (1000 * (i + 1) + 1 bins for position i) stays on the device as 32-bit
 * counters; a call whose histogram would pass this many bytes (read length above about 1 460) runs on the host as a whole. */
#define VSX_EESTATS_HIST_BUDGET_BYTES ((uint64_t) 4 << 30)

/* the Parameters fields the two commands read (defaults: the reference's, src/vsearch.h) */
typedef struct vsx_fastq_eestats_opts {
  int64_t        ascii;          /* 33 */
  int64_t        qmin;           /* 0 */
  int64_t        qmax;           /* 41 */
  int64_t        len_shortest;   /* 50   --length_cutoffs shortest,longest,increment */
  int64_t        len_longest;    /* INT_MAX (the '*' of --length_cutoffs) */
  int64_t        len_increment;  /* 50 */
  const double * ee_cutoffs;     /* {0.5, 1.0, 2.0}   --ee_cutoffs, used in this order */
  uint64_t       n_ee_cutoffs;   /* 3 */
  uint32_t       want;           /* VSX_EESTATS_WANT_*; default: both */
  uint32_t       pad;
  int64_t        window;         /* reads per staging window; 0: the built-in size.  Results do not depend on it. */
  uint64_t       hist_budget;    /* for tests: a histogram budget below VSX_EESTATS_HIST_BUDGET_BYTES; 0: the built-in one */
} vsx_fastq_eestats_opts;

typedef struct vsx_fastq_eestats_out {
  uint64_t   n;               /* reads */
  uint64_t   symbols;         /* sum of their lengths */
  uint64_t   len_min;         /* 0 without reads */
  uint64_t   len_max;
  /* VSX_EESTATS_WANT_EESTATS (NULL otherwise, and when len_max is 0) */
  uint64_t   qual_cols;       /* qmax + 2, the width of a qual_counts row */
  uint64_t * reads_at;        /* [len_max]: reads longer than i */
  uint64_t * qual_counts;     /* [len_max][qual_cols], by max(symbol - ascii, 0) */
  double *   sum_ee;          /* [len_max]: sum over the reads, in input order, of the running expected error at i */
  int64_t *  ee_bins;         /* [len_max][5]: Min, Low, Med, Hi, Max bin of the 1/1000 histogram (before (bin + 0.5) / 1000) */
  /* VSX_EESTATS_WANT_EESTATS2 */
  uint64_t   len_steps;       /* 0 when no read has a symbol */
  uint64_t   n_ee_cutoffs;
  uint64_t * cutoff_counts;   /* [len_steps][n_ee_cutoffs]: reads of at least shortest + x * increment symbols whose running
                                 expected error there is <= ee_cutoffs[y] */
} vsx_fastq_eestats_out;

typedef struct vsx_fastq_eestats_stats {
  double   seconds_stage;        /* host: scanning the lengths, planning windows, copying spans into pinned memory, enqueueing */
  double   seconds_h2d;          /* device time of the host-to-device copies (events), summed over the windows */
  double   seconds_walk;         /* device time of the walk kernel (events), summed over the windows */
  double   seconds_sum;          /* device time of the ordered-sum kernel (events), summed over the windows */
  double   seconds_quantile;     /* device time of the quantile kernel */
  double   seconds_d2h_output;   /* waiting for the windows, copying the tables back, building the output */
  double   seconds_total;
  uint64_t reads;
  uint64_t windows;
  uint64_t reads_host;           /* reads answered by the host restatement: 0, or all of them */
} vsx_fastq_eestats_stats;

void vsx_fastq_eestats_opts_default(vsx_fastq_eestats_opts * o);

/* Accumulate the tables over n reads.  ctx may be NULL only when the environment has VSX_EESTATS=host (the whole call
 * through the host restatement).  Option values the reference refuses (ascii not 33 or 64, qmin > qmax, ascii + qmin < 33,
 * ascii + qmax > 126, shortest < 1, shortest > longest, increment < 1, a cutoff <= 0), qmax < -1 (the reference's table has
 * no column then), a read beyond its blob or longer than INT32_MAX give VSX_EINVAL.  The commands read every position of
 * every read: a quality value outside [qmin, qmax] fails the call with VSX_EINVAL, and vsx_last_error() names the first one in
 * read order, then position order.  A call with more than UINT32_MAX reads, or whose histogram passes the budget, runs on
 * the host as a whole (reads_host == n): a partial host route would break the read order of sum_ee. */
int vsx_fastq_eestats(vsx_ctx * ctx, const vsx_fastq_eestats_opts * opts, uint64_t n, const vsx_fastx_reads * reads,
                      vsx_fastq_eestats_out * out);
void vsx_fastq_eestats_out_free(vsx_fastq_eestats_out * out);

/* figures of this thread's last vsx_fastq_eestats call */
void vsx_fastq_eestats_last_stats(vsx_fastq_eestats_stats * out);

#ifdef __cplusplus
}
#endif
#endif
