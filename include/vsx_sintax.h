/* vsx_sintax.h -- SINTAX taxonomy classification (--sintax) on a searcher (vsx_sintax.cpp / vsx_sintax.hip).
 *
 * Restated from the reference (commands/sintax.cpp, core/tax.cpp, utils/random.{hpp,cpp}, core/unique.cpp):
 *   words     the database is the searcher's (--dbmask, --hardmask, --wordlength; every distinct word once per sequence); a query
 *             strand's words are its distinct words in FIRST-OCCURRENCE order, only ambiguous symbols poison a word (Masking::none)
 *   sampling  one SplitMix64 stream per query, seeded from (randseed, query number); it runs through the plus strand's 100 rounds
 *             and on into the minus strand's.  A strand with fewer than 32 words is skipped and draws nothing.  A round makes 32
 *             bounded draws (Lemire multiply-shift with rejection); a repeated index is dropped
 *   round     the database sequence with the most sampled words, ties to the shorter, then to the lower number; kept iff that
 *             count is above 1.  Kept rounds append their winner to the strand's candidate list
 *   strand    plus, or with strand_both the larger best count, then the longer candidate list, then plus
 *   vote      classified iff the chosen strand has at least 50 candidates; rank by rank (d k p c o f g s t) the name most
 *             candidates carry wins (the first in candidate order on a tie; a missing rank is the empty name) and the
 *             candidates with another name leave the vote of the lower ranks
 * The result carries database sequence numbers and counts; names and text are cut from the labels by the caller.
 *
 * Routes.  The kernels serve word lengths 3..8 in the default tie-break mode with database sequences shorter than
 * VSX_SINTAX_MAX_DBLEN.  sintax_random (ties drawn from the query's stream, once per database sequence in scan order -- serial by
 * construction), word lengths 9..15 and longer database sequences go to the host restatement, which is exact and slow; so does
 * every query under VSX_SINTAX=host.  vsx_sintax_stats counts each route.
 */
#ifndef VSX_SINTAX_H
#define VSX_SINTAX_H

#include "vsx_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_SINTAX_RANKS       9           /* d k p c o f g s t */
#define VSX_SINTAX_ROUNDS      100         /* bootstrap_count */
#define VSX_SINTAX_SUBSET      32          /* subset_size */
#define VSX_SINTAX_NONE        0xffffffffu /* no sequence: a rank of an unclassified query, an unused candidate slot */
#define VSX_SINTAX_MAX_DBLEN   (1u << 24)  /* the selection key keeps 24 bits of a database sequence's length */

typedef struct vsx_sintax_opts {
  int32_t  strand_both;      /* --strand both */
  int32_t  sintax_random;    /* --sintax_random: host route */
  int32_t  want_candidates;  /* also return the round winners of both strands */
  int32_t  pad;
  uint64_t randseed;         /* --randseed; 0 is refused (the reference would seed from the OS) */
  int64_t  window;           /* queries per device window; 0 = 4 096 */
} vsx_sintax_opts;
void vsx_sintax_opts_default(vsx_sintax_opts * o);

/* one record per query */
typedef struct vsx_sintax_record {
  int32_t  strand;                             /* the chosen strand: 0 plus, 1 minus */
  int32_t  classified;                         /* boot_count[strand] >= 50 */
  uint32_t boot_count[2];                      /* kept rounds per strand */
  uint32_t best_count[2];                      /* the largest winning count per strand */
  uint32_t rank_seq[VSX_SINTAX_RANKS];         /* per rank: the winning candidate's database sequence (VSX_SINTAX_NONE: unclassified) */
  uint32_t rank_count[VSX_SINTAX_RANKS];       /* ... and how many candidates shared its name */
} vsx_sintax_record;

typedef struct vsx_sintax_result {
  uint64_t n_queries;
  uint64_t n_classified;
  vsx_sintax_record * rec;                     /* n_queries */
  uint32_t * candidates;                       /* want_candidates: n_queries x 2 x VSX_SINTAX_ROUNDS, round order, unused = VSX_SINTAX_NONE */
} vsx_sintax_result;
void vsx_sintax_result_free(vsx_sintax_result * r);

typedef struct vsx_sintax_stats {
  uint64_t queries_device;
  uint64_t queries_host_random;                /* sintax_random */
  uint64_t queries_host_wordlength;            /* word length 9..15 */
  uint64_t queries_host_dblen;                 /* a database sequence of VSX_SINTAX_MAX_DBLEN symbols or more */
  uint64_t queries_host_forced;                /* VSX_SINTAX=host, or a searcher without a device */
  uint64_t windows, strands_sampled, rounds_counted, tiles;
  double   seconds_stage, seconds_sample, seconds_count, seconds_vote, seconds_output, seconds_index, seconds_total;
} vsx_sintax_stats;
void vsx_sintax_last_stats(vsx_sintax_stats * out);

/* Query k has number first_query_no + k, or query_no[k] when query_no is given (the reference numbers the queries of a file from 0).
   The searcher's labels (vsx_searcher_set_meta) carry the taxonomy: VSX_EINVAL without them, and for randseed == 0.
   The first call builds the searcher's k-mer index if no search has, and the name ids of the labels; one call at a time per
   searcher (the window buffers live in it). */
int vsx_sintax(vsx_searcher * s, const vsx_sintax_opts * opts, uint64_t n_queries, const char * qblob, uint64_t qbytes,
               const uint64_t * offsets, const uint32_t * lengths, uint64_t first_query_no, const uint64_t * query_no,
               vsx_sintax_result * out);

/* The same computation on the CPU, no device: the database as text with its labels; of `search` the masking options
   (soft_mask, hardmask bit 0), wordlength and threads are read.  The test oracle, and the host route of vsx_sintax. */
int vsx_internal_sintax_host(const vsx_search_opts * search, const vsx_sintax_opts * opts, uint64_t n, const char * blob,
                             uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths, const char * const * labels,
                             uint64_t n_queries, const char * qblob, uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen,
                             uint64_t first_query_no, const uint64_t * query_no, vsx_sintax_result * out);

/* For tests: the nine per-rank name ids of each label, ids[9 * i + k]; id 0 is the empty name, and two labels share an id at a
   rank iff their names there are equal as (length, bytes).  start/len (may be NULL): where each name lies in its label. */
int vsx_internal_sintax_intern(uint64_t n, const char * const * labels, uint32_t * ids, int32_t * start, int32_t * len);

#ifdef __cplusplus
}
#endif
#endif
