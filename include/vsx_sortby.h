/* vsx_sortby.h -- the reference's sort orders (--sortbysize, --sortbylength, and the orders Database::sortbyabundance /
 * sortbylength / sortbylength_shortest_first give the clustering and chimera commands) on the GPU.
 *
 * The caller passes n headers (blob / offset / length, as the reference's parser would hand them on), n sequence lengths and n
 * abundances (the caller parses ;size=, as for every other call of the library).  No sequence text is needed.  Each order is a
 * total order whose last key is the input position:
 *
 *   VSX_SORTBY_SIZE         abundance descending, header ascending, input position    (commands/sortbysize.cpp, core/db.cpp:471-485)
 *   VSX_SORTBY_LENGTH       length descending, abundance descending, header, position (commands/sortbylength.cpp, core/db.cpp:433-450)
 *   VSX_SORTBY_LENGTH_ASC   length ascending, abundance descending, header, position  (core/db.cpp:452-469)
 *
 * Headers compare as strcmp compares them: unsigned bytes, a proper prefix first, equal headers in input order.  A header with a
 * NUL byte cannot be compared the way the reference would (its strcmp stops there) and is refused.
 *
 *   selection   VSX_SORTBY_SIZE keeps minsize <= abundance <= maxsize (before the sort, as create_deck does); the length orders
 *               keep everything, as --sortbylength ignores both options
 *   median      find_median_abundance / find_median_length over the kept deck before topn: the middle key, or the mean of the
 *               two middle keys (a round value or one with a remainder of .5); 0.0 for an empty deck
 *   topn        the first topn of the sorted deck
 *
 * FASTA parsing and writing stay with the caller (vsearch_amd/sortby.py has the writers and the log line).
 */
#ifndef VSX_SORTBY_H
#define VSX_SORTBY_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_SORTBY_SIZE        0
#define VSX_SORTBY_LENGTH      1
#define VSX_SORTBY_LENGTH_ASC  2

#define VSX_SORTBY_MAX_ROUNDS    32   /* label rounds of 8 bytes on the device: groups that share more go to the host comparator */
#define VSX_SORTBY_STAT_ROUNDS   8    /* rounds whose active items the statistics keep */

typedef struct vsx_sortby_opts {
  int32_t order;              /* VSX_SORTBY_* */
  int32_t threads;            /* host restatement: 0 = the usable CPUs, at most 16 */
  int64_t minsize;            /* default 0; VSX_SORTBY_SIZE only */
  int64_t maxsize;            /* default INT64_MAX; VSX_SORTBY_SIZE only */
  int64_t topn;               /* default INT64_MAX */
} vsx_sortby_opts;

typedef struct vsx_sortby_out {
  uint64_t   n;
  uint64_t   n_kept;          /* the deck after minsize / maxsize, before topn */
  uint64_t   n_out;           /* min(n_kept, topn) */
  uint64_t * order;           /* n_out input numbers in output order; the ordinal --relabel prints is index + 1 */
  double     median;
} vsx_sortby_out;

typedef struct vsx_sortby_stats {
  double   seconds_stage;        /* host: the checks */
  double   seconds_h2d;          /* uploading headers and keys */
  double   seconds_numeric;      /* selection, numeric keys, their sort and the tie groups */
  double   seconds_refine;       /* the label rounds */
  double   seconds_host_finish;  /* groups left at the round cap, through the host comparator */
  double   seconds_output;       /* copying the order back, median and topn; the whole host restatement on a host route */
  double   seconds_total;
  uint64_t items;
  uint64_t kept;
  uint64_t label_bytes;
  uint64_t rounds;               /* label rounds the device ran */
  uint64_t max_rounds;           /* the cap the call used */
  uint64_t active_numeric;       /* items in a tie group of more than one member after the numeric key */
  uint64_t active[VSX_SORTBY_STAT_ROUNDS];   /* items still in an open group after label round 0, 1, ... */
  uint64_t capped_items;         /* items the host comparator finished */
  uint64_t host_no_context;      /* the host routes: 1 when the call took it */
  uint64_t host_environment;     /* VSX_SORTBY=host */
  uint64_t host_count;           /* more than UINT32_MAX - 1 items */
  uint64_t host_memory;          /* headers and work arrays do not fit the device */
  uint64_t host_long_prefix;     /* 1 when groups were still open at the round cap (the rest of the call ran on the device) */
} vsx_sortby_stats;

void vsx_sortby_opts_default(vsx_sortby_opts * o);

/* Sort n records.  ctx may be NULL: the call then runs the host restatement (counted in the statistics), as it does under
 * VSX_SORTBY=host.  VSX_EINVAL: an unknown order, a negative topn or thread count, a header beyond the blob, an abundance of 0, a
 * NUL byte in a header.  VSX_SORTBY_MAX_ROUNDS (0 .. 32: the round cap), VSX_SORTBY_DEVICE_COUNT (the count limit of the device
 * route) and VSX_SORTBY_PRETEND_BYTES (what the call pretends to need of the device) are testing aids, read per call. */
int vsx_sortby(vsx_ctx * ctx, const vsx_sortby_opts * opts, uint64_t n, const char * label_blob, uint64_t blob_bytes,
               const uint64_t * label_offsets, const uint32_t * label_lengths, const uint32_t * seq_lengths, const uint32_t * sizes,
               vsx_sortby_out * out);
void vsx_sortby_out_free(vsx_sortby_out * out);

/* figures of this thread's last vsx_sortby call */
void vsx_sortby_last_stats(vsx_sortby_stats * out);

#ifdef __cplusplus
}
#endif
#endif
