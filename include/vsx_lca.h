/* vsx_lca.h -- the last common ancestor of a query's hits, --lcaout with --lca_cutoff (the reference's results_show_lcaout,
 * core/results.cpp:545-687, over tax_parse / tax_split of core/tax.cpp), on the GPU.
 *
 * The database labels are split once into their nine rank names (d k p c o f g s t) and every (label, level) gets a number that
 * stands for the names of levels 0 .. level together: two labels carry the same number at level k iff their names of levels 0 .. k
 * agree in length and bytes (a rank the label does not name has length 0 and agrees with another missing rank).  That is a
 * vsx_lca_index.  vsx_lca then takes the hits of any search call and gives, per query, what --lcaout prints.
 *
 * The reference runs a Boyer-Moore majority vote per level over the top hits in their order and counts the candidate's matches in a
 * second pass; level j is printed while 1.0 * matches[j] / n_top >= lca_cutoff.  The CLI admits 0.5 < lca_cutoff <= 1.0 only, so a
 * printed level holds a strict majority of the top hits, which Boyer-Moore always finds: the printed text depends on the multiset
 * of top hits alone.  The device votes without walking the hits in order; the host restatement keeps the literal loops.
 *
 * A label is a span: it behaves as the reference's NUL-terminated header would if it ended at the span's end.  Every search of
 * tax_split is bounded by the span's end -- and by nothing else: the comma that ends a name is looked for beyond the ';' that ends
 * the tax= field, as in the reference.
 */
#ifndef VSX_LCA_H
#define VSX_LCA_H

#include "vsx_search.h"
#include "vsx_otutab.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_LCA_LEVELS 9
#define VSX_LCA_NONE   0xFFFFFFFFu

/* the database labels, split and numbered once */
typedef struct vsx_lca_index vsx_lca_index;

typedef struct vsx_lca_opts {
  double   lca_cutoff;       /* --lca_cutoff, default 1.0; must lie in (0.5, 1.0] */
  int64_t  maxhits;          /* --maxhits: only a query's first maxhits hits take part; 0 = all */
  int32_t  top_hits_only;    /* --top_hits_only: the hits before the first one whose id is below the first hit's */
  int32_t  threads;          /* host threads of the host restatement and the host steps; 0: what the process may use, 16 at most */
  uint64_t window;           /* queries per pass over the device; 0: the library's choice.  The result does not depend on it */
} vsx_lca_opts;

/* Per query q: n_top[q] is the reference's tophitcount (after maxhits and top_hits_only); depth[q] the first level at which the
 * cutoff fails -- 9 if none fails, 0 for a query without hits.  Per (q, level j < depth[q]), at [9 q + j]: matches = the top hits
 * whose names of levels 0 .. j agree with the majority's; target = the database label of the top hit with the LOWEST hit index
 * among them; the name to print is label[target][start .. start + len) (len 0: the rank is not named, nothing is printed).
 * At levels >= depth[q]: matches, start and len are 0 and target is VSX_LCA_NONE. */
typedef struct vsx_lca_result {
  uint64_t   n_queries;
  uint32_t * n_top;          /* n_queries */
  uint32_t * depth;          /* n_queries */
  uint32_t * matches;        /* 9 n_queries */
  uint32_t * target;         /* 9 n_queries */
  uint32_t * start;          /* 9 n_queries */
  uint32_t * len;            /* 9 n_queries */
} vsx_lca_result;

typedef struct vsx_lca_stats {
  /* the index this call used (or, after vsx_lca_index_create, the index just made) */
  double   seconds_index_stage;     /* checks, the blob's upload */
  double   seconds_index_split;     /* the split kernel and the download of start / len; host route: the host's split */
  double   seconds_index_number;    /* sort, head flags, verification; or the host's numbering */
  double   seconds_index_total;
  /* the call */
  double   seconds_stage;           /* checks, the hits' targets and ids gathered from the hit records */
  double   seconds_h2d;
  double   seconds_vote;            /* the vote kernel, from its launch to its completion */
  double   seconds_d2h;
  double   seconds_output;          /* host: the cutoff test, the result arrays; host route: the whole restatement */
  double   seconds_total;
  uint64_t labels;
  uint64_t labels_device;           /* labels the split kernel served */
  uint64_t labels_host;
  uint64_t windows;
  uint64_t queries_device, queries_host;
  uint64_t hits_device, hits_host;
  /* why the host answered.  The first four send the index AND every call on it to the host restatement; host_collision sends only
     the numbering of the index to the host (the vote stays on the device) */
  uint64_t host_no_context;         /* the index was made without a context */
  uint64_t host_environment;        /* VSX_LCA=host, at index creation or at the call */
  uint64_t host_count;              /* more than UINT32_MAX - 1 entries of 9 per label, or more than UINT32_MAX - 1 hits or queries */
  uint64_t host_memory;             /* the arrays do not fit the device's free memory */
  uint64_t host_collision;          /* two different name prefixes met in one run of equal hashes: verified, never merged */
} vsx_lca_stats;

void vsx_lca_opts_default(vsx_lca_opts * o);

/* Split and number the labels.  ctx NULL: a host index; every call on it runs the host restatement.  The index keeps copies of
 * nothing but its own arrays: the labels are read during this call only.
 *
 * Testing aids, read per call: VSX_LCA=host; VSX_LCA_HASH_BITS=n (1 .. 64) keeps the low n bits of every prefix hash;
 * VSX_LCA_DEVICE_COUNT lowers the count above which the host answers; VSX_LCA_PRETEND_BYTES replaces the device memory the call is
 * taken to need.
 *
 * VSX_EINVAL: a null argument, a label span outside its blob, a label that holds a NUL byte. */
int  vsx_lca_index_create(vsx_ctx * ctx, const vsx_labels * targets, vsx_lca_index ** out);
void vsx_lca_index_destroy(vsx_lca_index * index);

/* The last common ancestors of the hits of one search call (vsx_search_batch, vsx_search_exact, vsx_multi_search_batch, ...).
 * Only first, hit[].target and hit[].id are read.
 * VSX_EINVAL: a null argument; lca_cutoff outside (0.5, 1.0] or NaN (the CLI's fatal: "The argument to lca_cutoff must be larger
 * than 0.5, but not larger than 1.0"); maxhits or threads below 0; a `first` that does not ascend from 0 to n_hits; a hit whose
 * target is not below the number of labels. */
int  vsx_lca(vsx_lca_index * index, const vsx_lca_opts * opts, const vsx_hits * hits, vsx_lca_result * out);
void vsx_lca_result_free(vsx_lca_result * out);

/* figures of this thread's last vsx_lca_index_create or vsx_lca call */
void vsx_lca_last_stats(vsx_lca_stats * out);

/* The exact host restatement: the reference's Boyer-Moore loop and its second counting pass, literally, over the shared tax_split;
 * only the representative is normalised to the matching top hit of the lowest index.  No context; opts->threads host threads.
 * Same refusals and result as vsx_lca_index_create + vsx_lca. */
int  vsx_internal_lca_host(const vsx_lca_opts * opts, const vsx_labels * targets, const vsx_hits * hits, vsx_lca_result * out);

/* the split of an index, for the tests: start[9 n], len[9 n] as the index holds them (from the split kernel on a device index) */
int  vsx_internal_lca_index_split(const vsx_lca_index * index, uint64_t n, int32_t * start, int32_t * len);

#ifdef __cplusplus
}
#endif
#endif
