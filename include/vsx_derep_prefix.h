/* vsx_derep_prefix.h -- prefix dereplication (the reference's --derep_prefix, src/commands/derep_prefix.cpp) on the GPU.
 *
 * Reads go in as in include/vsx_derep.h: host blobs (vsx_fastx_reads of vsx_filter.h), labels as a blob with
 * offsets.  Out come the clusters in the command's output order with their members in the order of the --uc file.
 *
 * A read joins the cluster of a read it equals or is a prefix of.  Equality is the equality of vsx_search_exact / vsx_derep: the
 * same 4-bit code (chrmap_4bit) at every position, so it is case-blind, U equals T and an ambiguity code equals only itself.
 * The command sorts its input first (length ascending, abundance descending, label, input order) and walks it in that order;
 * what the walk computes is restated here as one order-independent rule (DESIGN, "Prefix dereplication"):
 *
 *   the distinct sequences are nodes; a node's head is its first read in sorted order, its rank the head's sorted position;
 *   a node P is absorbed by the lowest-ranked node that properly extends it; the clusters are the chains these links form;
 *   a cluster's representative is the head of the chain's longest node.
 *
 * reads->abundance is the header's size annotation (NULL: 1 each).  It is ALWAYS the second key of the sort, as in the reference;
 * sizein decides whether it is also what a cluster's size sums (--sizein) or every read counts 1.
 *
 * The reference keeps a cluster's size in 32 bits and wraps.  This library does not restate the wrap: a call whose summed sizes
 * reach 2^32 is refused with VSX_EINVAL, and so is a single abundance of 2^32 or more, or of 0.  The command has no --strand both.
 */
#ifndef VSX_DEREP_PREFIX_H
#define VSX_DEREP_PREFIX_H

#include "vsx.h"
#include "vsx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsx_derep_prefix_opts {
  int32_t sizein;          /* 0: every read counts 1; 1: --sizein, the abundances are summed */
  int32_t pad;
  int64_t minseqlength;    /* 32 */
  int64_t maxseqlength;    /* 50000 */
  int64_t minuniquesize;   /* 1 */
  int64_t maxuniquesize;   /* INT64_MAX */
  int64_t topn;            /* INT64_MAX */
  int64_t window;          /* reads per staging window; 0: the built-in size.  Results do not depend on it. */
} vsx_derep_prefix_opts;

typedef struct vsx_derep_prefix_out {
  uint64_t   n;                 /* reads given */
  /* the counts behind the command's log lines */
  uint64_t   kept;              /* reads within [minseqlength, maxseqlength] */
  uint64_t   nucleotides;       /* of the kept reads */
  uint64_t   shortest;          /* 0 when nothing is kept */
  uint64_t   longest;
  uint64_t   discarded_short;
  uint64_t   discarded_long;
  uint64_t   sumsize;           /* sum of the cluster sizes: the kept reads' abundances (sizein) or their number */
  uint64_t   maxsize;           /* largest cluster size */
  double     median;            /* of the cluster sizes */
  uint64_t   selected;          /* min(clusters with minuniquesize <= size <= maxuniquesize, topn): what --output prints */
  /* the clusters, ordered by size descending, then strcmp of the representative's label, then the representative's sorted rank */
  uint64_t   n_clusters;
  uint64_t * rep;               /* n_clusters: input index of the representative */
  uint64_t * size;              /* n_clusters */
  uint64_t * count;             /* n_clusters: number of members */
  /* CSR member list: cluster c owns member[member_start[c] .. member_start[c + 1]), the order of the --uc file's H records,
   * the representative first */
  uint64_t * member_start;      /* n_clusters + 1 */
  uint64_t * member;            /* kept: input indices */
  /* n: a kept read's position in the command's sorted order (0 .. kept - 1), UINT64_MAX for a discarded read */
  uint64_t * rank;
} vsx_derep_prefix_out;

typedef struct vsx_derep_prefix_stats {
  double   seconds_rank;         /* host: the four-key sort */
  double   seconds_stage;        /* host: planning the windows and copying their reads into pinned memory */
  double   seconds_h2d;          /* device time of the host-to-device copies (events) */
  double   seconds_hash;         /* device time of the code-word and prefix-sum kernels (events) */
  double   seconds_group;        /* find-or-insert of equal reads, the nodes' heads */
  double   seconds_claim;        /* the claim kernel */
  double   seconds_resolve;      /* chain tops, sizes, counts, the member sort and its download */
  double   seconds_output;       /* host: cluster order, member list, output arrays */
  double   seconds_total;
  uint64_t windows;
  uint64_t nodes;                /* distinct sequences */
  uint64_t distinct_lengths;
  uint64_t probes;               /* table slots the claim pass read */
  uint64_t candidates_compared;  /* prefixes the claim pass compared word for word (host: symbol for symbol) */
  uint64_t reads_host;           /* reads answered by the host restatement */
  /* why the host restatement answered (at most one is 1) */
  uint64_t host_no_context;      /* ctx was NULL */
  uint64_t host_environment;     /* VSX_DEREP_PREFIX=host */
  uint64_t host_read_count;      /* more than UINT32_MAX - 1 kept reads */
  uint64_t host_memory;          /* the code words do not fit the device's free memory */
} vsx_derep_prefix_stats;

void vsx_derep_prefix_opts_default(vsx_derep_prefix_opts * o);

/* Dereplicate n reads.  labels: blob of n labels, label k = label_blob[label_off[k] .. label_off[k + 1]) (no terminators needed;
 * n + 1 offsets); they break ties of the sort and of the cluster order.
 *
 * ctx NULL, or VSX_DEREP_PREFIX=host in the environment: the whole call runs through the host restatement.  So does a call with
 * more than UINT32_MAX - 1 kept reads, and one whose code words do not fit the device's free memory.
 *
 * Testing aids: VSX_DEREP_PREFIX_DEVICE_READS lowers the number of kept reads above which the host answers,
 * VSX_DEREP_PREFIX_PRETEND_BYTES replaces the device memory the call is taken to need.
 *
 * VSX_EINVAL: a negative window; a read beyond its blob or label offsets that decrease; an abundance of 0 or of 2^32 or more;
 * cluster sizes summing to 2^32 or more. */
int vsx_derep_prefix(vsx_ctx * ctx, const vsx_derep_prefix_opts * opts, uint64_t n, const vsx_fastx_reads * reads,
                     const char * label_blob, const uint64_t * label_off, vsx_derep_prefix_out * out);
void vsx_derep_prefix_out_free(vsx_derep_prefix_out * out);

/* figures of this thread's last vsx_derep_prefix call */
void vsx_derep_prefix_last_stats(vsx_derep_prefix_stats * out);

#ifdef __cplusplus
}
#endif
#endif
