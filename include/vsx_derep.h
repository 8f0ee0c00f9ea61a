/* vsx_derep.h -- full-length dereplication (the core of the reference's --derep_fulllength, --fastx_uniques and --derep_id,
 * src/core/derep.cpp: derep()) on the GPU.
 *
 * Reads go in as host blobs (vsx_fastx_reads of vsx_filter.h), labels as a blob with offsets.  Out come the clusters in the
 * command's output order with their members, strands and -- for FASTQ input -- the merged quality strings.
 *
 * Equality is the equality of vsx_search_exact: same length and the same 4-bit code (chrmap_4bit) at every position, so it is
 * case-blind, U equals T and an ambiguity code equals only itself.  With strand_both a cluster is the class {S, rc(S)}; its
 * representative is the member with the lowest input index, and a member's strand is '-' exactly when its codes differ from the
 * representative's (a reverse palindrome is '+').  by_label (--derep_id) additionally requires equal labels.
 *
 * The reference keeps a cluster's size in 32 bits and wraps.  This library does not restate the wrap: a call whose kept reads'
 * abundances sum to 2^32 or more is refused with VSX_EINVAL.  An abundance of 0 is refused too (the reference's reader never
 * delivers one).
 *
 * FASTA / FASTQ parsing and writing, --notrunclabels, relabelling and the abundance annotations stay with the caller.
 */
#ifndef VSX_DEREP_H
#define VSX_DEREP_H

#include "vsx.h"
#include "vsx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsx_derep_opts {
  int32_t strand_both;     /* 0: --strand plus */
  int32_t by_label;        /* 0; 1: --derep_id */
  int32_t want_quality;    /* 0; 1: merge the members' quality strings (--fastqout); needs reads->qual */
  int32_t qout_max;        /* 0: size-weighted average of the error probabilities; 1: --fastq_qout_max */
  int64_t minseqlength;    /* 32 (--derep_fulllength, --derep_id; --fastx_uniques: 1) */
  int64_t maxseqlength;    /* 50000 */
  int64_t minuniquesize;   /* 1 */
  int64_t maxuniquesize;   /* INT64_MAX */
  int64_t topn;            /* INT64_MAX */
  int64_t ascii;           /* 33 */
  int64_t asciiout;        /* 33 */
  int64_t qminout;         /* 0 */
  int64_t qmaxout;         /* 41 */
  int64_t window;          /* reads per staging window; 0: the built-in size.  Results do not depend on it. */
} vsx_derep_opts;

typedef struct vsx_derep_out {
  uint64_t   n;                 /* reads given */
  /* the counts behind the command's log lines */
  uint64_t   kept;              /* reads within [minseqlength, maxseqlength] */
  uint64_t   nucleotides;       /* of the kept reads */
  uint64_t   shortest;          /* 0 when nothing is kept */
  uint64_t   longest;
  uint64_t   discarded_short;
  uint64_t   discarded_long;
  uint64_t   sumsize;           /* sum of the kept reads' abundances */
  uint64_t   maxsize;           /* largest cluster size */
  double     median;            /* of the cluster sizes */
  uint64_t   selected;          /* min(clusters with minuniquesize <= size <= maxuniquesize, topn): what the FASTA / FASTQ writers print */
  /* the clusters, ordered by size descending, then strcmp of the representative's label, then representative index */
  uint64_t   n_clusters;
  uint64_t * rep;               /* n_clusters: input index of the representative */
  uint64_t * size;              /* n_clusters: sum of the members' abundances */
  uint64_t * count;             /* n_clusters: number of members */
  /* CSR member list: cluster c owns member[member_start[c] .. member_start[c + 1]), input order, the representative first */
  uint64_t * member_start;      /* n_clusters + 1 */
  uint64_t * member;            /* kept: input indices */
  uint8_t *  strand;            /* kept: 0 '+', 1 '-' */
  /* want_quality: cluster c's merged quality string is qual_blob[qual_off[c] .. qual_off[c + 1]); else NULL */
  uint64_t * qual_off;          /* n_clusters + 1 */
  char *     qual_blob;
  uint64_t   qual_bytes;
} vsx_derep_out;

typedef struct vsx_derep_stats {
  double   seconds_stage;        /* host: planning the windows and copying their reads into pinned memory */
  double   seconds_h2d;          /* device time of the host-to-device copies (events) */
  double   seconds_hash;         /* device time of the hash kernel (events) */
  double   seconds_group;        /* canonical strand + find-or-insert */
  double   seconds_account;      /* representatives, sizes, counts, the member sort and its download */
  double   seconds_quality;      /* uploading the quality strings, the merge kernel, its download */
  double   seconds_output;       /* host: cluster order, member list, output arrays */
  double   seconds_total;
  uint64_t windows;
  uint64_t slots_visited;        /* table slots the grouping kernel (or nothing, on the host) visited */
  uint64_t candidates_compared;  /* owners compared word for word */
  uint64_t reads_host;           /* reads answered by the host restatement */
} vsx_derep_stats;

void vsx_derep_opts_default(vsx_derep_opts * o);

/* Dereplicate n reads.  labels: blob of n labels, label k = label_blob[label_off[k] .. label_off[k + 1]) (no terminators needed;
 * n + 1 offsets); they break ties of the cluster order and, with by_label, are part of the key.  reads->abundance NULL: 1 each.
 *
 * ctx NULL, or VSX_DEREP=host in the environment: the whole call runs through the host restatement.  So does a call with more
 * than UINT32_MAX - 1 kept reads, and one whose code words do not fit the device's free memory.
 *
 * VSX_EINVAL: a quality byte outside 33 .. 126 (with want_quality); ascii outside 0 .. 127, qminout > qmaxout or asciiout +
 * qminout / qmaxout outside 0 .. 127; a read beyond its blob or label offsets that decrease; want_quality without reads->qual;
 * an abundance of 0; abundances of the kept reads summing to 2^32 or more. */
int vsx_derep(vsx_ctx * ctx, const vsx_derep_opts * opts, uint64_t n, const vsx_fastx_reads * reads,
              const char * label_blob, const uint64_t * label_off, vsx_derep_out * out);
void vsx_derep_out_free(vsx_derep_out * out);

/* figures of this thread's last vsx_derep call */
void vsx_derep_last_stats(vsx_derep_stats * out);

/* testing aid: T[v], v = 0 .. 128, the largest double p with trunc(-10 * log10(p)) >= v (the quality kernel's thresholds) */
void vsx_internal_derep_thresholds(double * out129);

#ifdef __cplusplus
}
#endif
#endif
