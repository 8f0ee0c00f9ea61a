/* vsx_fastq_stats.h -- read summary statistics (the analysis cores of the reference's --fastq_stats and --fastq_chars) on the GPU.
 *
 * vsx_fastq_stats walks every quality symbol of every read and returns the tables --fastq_stats prints from: integer counts, and
 * per position one double, the sum over the reads in input order of the running expected error (formed in the reference's order,
 * so every printed figure is bit-identical).  vsx_fastq_chars walks sequence and quality together and returns the inventory
 * --fastq_chars prints.  Reads go in as host blobs (vsx_fastx_reads of vsx_filter.h); vsx_fastq_stats reads only `qual`, `bytes`,
 * `off` and `len`.  FASTQ parsing and the printing stay with the caller (vsearch_amd/fastq_stats.py has both formatters).
 */
#ifndef VSX_FASTQ_STATS_H
#define VSX_FASTQ_STATS_H

#include "vsx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_FASTQ_STATS_SYMBOLS      94     /* quality characters 33 ... 126: the width of a symbol_counts row */
#define VSX_FASTQ_STATS_FIRST_SYMBOL 33

/* The running expected error of a window's reads lies on the device as matrix[position][read] until the ordered sum has read it;
 * a call whose window (at least 256 reads) would need more than this for the matrix runs on the host as a whole. */
#define VSX_FASTQ_STATS_MATRIX_BUDGET_BYTES ((uint64_t) 1 << 30)

/* the Parameters fields --fastq_stats reads (defaults: the reference's, src/vsearch.h) */
typedef struct vsx_fastq_stats_opts {
  int64_t ascii;          /* 33 */
  int64_t qmin;           /* 0 */
  int64_t qmax;           /* 41 */
  int64_t window;         /* reads per staging window; 0: the built-in size.  Results do not depend on it. */
} vsx_fastq_stats_opts;

typedef struct vsx_fastq_stats_out {
  uint64_t   n;               /* reads */
  uint64_t   symbols;         /* sum of their lengths */
  uint64_t   len_min;         /* 0 without reads */
  uint64_t   len_max;
  uint64_t * length_counts;   /* [len_max + 1]: reads of length L */
  /* NULL when len_max is 0 */
  uint64_t * symbol_counts;   /* [len_max][94], by quality character 33 ... 126 */
  double *   sum_ee;          /* [len_max]: sum over the reads, in input order, of the running expected error at i */
  uint64_t * ee_counts;       /* [len_max][4]: reads whose running expected error at i is <= 1.0, 0.5, 0.25, 0.1 */
  uint64_t * q_counts;        /* [len_max][4]: reads whose lowest score up to i is > 5, 10, 15, 20 */
} vsx_fastq_stats_out;

typedef struct vsx_fastq_stats_stats {
  double   seconds_stage;        /* host: scanning the lengths, planning windows, copying spans into pinned memory, enqueueing */
  double   seconds_h2d;          /* device time of the host-to-device copies (events), summed over the windows */
  double   seconds_walk;         /* device time of the walk kernel (events), summed over the windows */
  double   seconds_sum;          /* device time of the ordered-sum kernel (events), summed over the windows */
  double   seconds_d2h_output;   /* waiting for the windows, copying the tables back, building the output */
  double   seconds_total;
  uint64_t reads;
  uint64_t windows;
  uint64_t reads_host;           /* reads answered by the host restatement: 0, or all of them */
} vsx_fastq_stats_stats;

void vsx_fastq_stats_opts_default(vsx_fastq_stats_opts * o);

/* Accumulate the tables over n reads.  ctx may be NULL only when the environment has VSX_FASTQ_STATS=host (the whole call
 * through the host restatement).  The score of a symbol is symbol - ascii, and 0 for every symbol below ascii.  VSX_EINVAL: option
 * values the reference refuses (ascii not 33 or 64, qmin > qmax, ascii + qmin < 33, ascii + qmax > 126), a negative window, a
 * quality byte outside 33 ... 126, a read beyond its blob or longer than INT32_MAX, and a read whose lowest or highest score,
 * compared as unsigned, lies outside [(unsigned) qmin, (unsigned) qmax]: vsx_last_error() names the value and the range of the
 * first such read in input order (the lowest score if it is out of range, otherwise the highest).  A call with more than
 * UINT32_MAX reads, or whose matrix passes the budget, runs on the host as a whole (reads_host == n): a partial host route would
 * break the read order of sum_ee. */
int vsx_fastq_stats(vsx_ctx * ctx, const vsx_fastq_stats_opts * opts, uint64_t n, const vsx_fastx_reads * reads,
                    vsx_fastq_stats_out * out);
void vsx_fastq_stats_out_free(vsx_fastq_stats_out * out);

/* figures of this thread's last vsx_fastq_stats call */
void vsx_fastq_stats_last_stats(vsx_fastq_stats_stats * out);

/* the Parameters fields --fastq_chars reads */
typedef struct vsx_fastq_chars_opts {
  int64_t tail;           /* 4   --fastq_tail */
  int64_t window;         /* reads per staging window; 0: the built-in size.  Results do not depend on it. */
} vsx_fastq_chars_opts;

typedef struct vsx_fastq_chars_out {
  uint64_t n;                  /* reads */
  uint64_t total_chars;        /* sum of their lengths */
  uint64_t seq_counts[256];    /* by sequence symbol after mapping: letters to upper case, every other byte to N */
  uint64_t qual_counts[256];   /* by quality character */
  uint64_t tail_counts[256];   /* reads of at least `tail` symbols whose last `tail` quality characters all equal this one */
  int32_t  maxrun[256];        /* by sequence symbol: the longest run within a read, minus one */
  uint8_t  qmin_n, qmax_n;     /* lowest and highest quality character seen under N (255 and 0 without one) */
  uint8_t  pad[6];
} vsx_fastq_chars_out;

typedef struct vsx_fastq_chars_stats {
  double   seconds_stage;
  double   seconds_h2d;
  double   seconds_kernel;       /* device time of the chars kernel (events), summed over the windows */
  double   seconds_d2h_output;
  double   seconds_total;
  uint64_t reads;
  uint64_t windows;
  uint64_t reads_host;           /* 0, or all of them */
} vsx_fastq_chars_stats;

void vsx_fastq_chars_opts_default(vsx_fastq_chars_opts * o);

/* ctx may be NULL only under VSX_FASTQ_STATS=host.  tail < 1, a negative window, seq == NULL or qual == NULL with n > 0, a
 * quality byte outside 33 ... 126, a read beyond its blob or longer than INT32_MAX give VSX_EINVAL.  More than UINT32_MAX reads
 * run on the host as a whole. */
int vsx_fastq_chars(vsx_ctx * ctx, const vsx_fastq_chars_opts * opts, uint64_t n, const vsx_fastx_reads * reads,
                    vsx_fastq_chars_out * out);
void vsx_fastq_chars_out_free(vsx_fastq_chars_out * out);
void vsx_fastq_chars_last_stats(vsx_fastq_chars_stats * out);

#ifdef __cplusplus
}
#endif
#endif
