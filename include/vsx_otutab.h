/* vsx_otutab.h -- the OTU / ASV table of --otutabout, --biomout and --mothur_shared_out (the reference's core/otutable.cpp) on the GPU.
 *
 * The table is built from ADDS (query label or none, target label or none, abundance), as the reference's otutable_add() takes
 * them from --usearch_global, --search_exact and the four --cluster_* commands.  This call takes the adds of one command at once:
 *
 *   query k with q_target[k] = t        adds (query label k, target label t, q_abundance[k])
 *   query k with q_target[k] = NONE     adds (query label k, none, q_abundance[k]): its sample appears, with no counts
 *   then, when t_matched is given, every target t with t_matched[t] == 0 adds (none, target label t, 0), in target order
 *
 * A search passes the first reported hit per query and dbmatched per target; a clustering passes every sequence as a query with
 * its centroid (or the centroid's new label under --relabel) as target and t_matched NULL (vsearch_amd/otutab.py: from_search,
 * from_clusters).
 *
 * Names, restated from the reference's three regular expressions without any:
 *   sample    the leftmost p with (p == 0 or label[p - 1] == ';') where "sample=" or "barcodelabel=" starts: the name runs from behind
 *             the '=' to the next ';' or the end (it may be empty).  No such p: the longest prefix of [A-Za-z0-9_] (it may be empty).
 *   OTU       the same with "otu="; no such p: the prefix up to the first ';', or the whole label.
 *   taxonomy  the same with "tax="; no such p: the target says nothing about taxonomy.  tax[OTU name] is the value of the LAST add in
 *             call order whose target carries one.
 * Bytes are bytes: case-sensitive, no terminator needed, none honoured.  A name is entered whenever its label is present, even
 * when it is empty.  count[OTU][sample] += abundance iff both labels are present and the abundance is not 0 (64-bit, wrapping).
 * Samples and OTUs are in memcmp order on unsigned bytes, the shorter first on a tie (std::set<std::string>).
 */
#ifndef VSX_OTUTAB_H
#define VSX_OTUTAB_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_OTUTAB_NONE 0xFFFFFFFFu

/* n labels: label k = blob[offsets[k] .. offsets[k] + lengths[k]).  The spans may overlap, repeat and come in any order. */
typedef struct vsx_labels {
  uint64_t         n;
  const char *     blob;
  uint64_t         bytes;
  const uint64_t * offsets;
  const uint32_t * lengths;
} vsx_labels;

typedef struct vsx_otutab_opts {
  int32_t threads;         /* host threads of the host restatement and of the host steps; 0: what the process may use, 16 at most */
  int32_t pad;
} vsx_otutab_opts;

typedef struct vsx_otutab_result {
  uint64_t   n_queries, n_targets;
  uint64_t   n_samples, n_otus;
  int32_t    has_tax;            /* some add's target carried tax=: the writers print the taxonomy column / metadata */
  int32_t    pad;
  /* the names, sorted: name r = blob[off[r] .. off[r] + len[r]) */
  char *     sample_blob;  uint64_t sample_bytes;  uint64_t * sample_off;  uint32_t * sample_len;
  char *     otu_blob;     uint64_t otu_bytes;     uint64_t * otu_off;     uint32_t * otu_len;
  /* per OTU its taxonomy: tax_len[r] == VSX_OTUTAB_NONE when no add gave it one (an empty value has length 0) */
  char *     tax_blob;     uint64_t tax_bytes;     uint64_t * tax_off;     uint32_t * tax_len;
  /* the non-zero cells ordered by (OTU, sample): the order in which all three writers walk them */
  uint64_t   n_cells;
  uint32_t * nz_otu;
  uint32_t * nz_sample;
  uint64_t * nz_count;
  uint32_t * q_sample;           /* n_queries: the sample rank of every query */
  uint32_t * t_otu;              /* n_targets: the OTU rank of every target that took part in an add, else VSX_OTUTAB_NONE */
} vsx_otutab_result;

typedef struct vsx_otutab_stats {
  double   seconds_stage;        /* host: checking the spans, the list of targets that take part, the uploads */
  double   seconds_scan;         /* the two scan launches, from their start to their completion; host route: the label scan */
  double   seconds_group;        /* sort by hash, head flags, prefix sum, representatives (both sides) */
  double   seconds_rank;         /* host: download of the representatives, their sort and merge, upload of the ranks */
  double   seconds_accumulate;   /* key kernel, sort, the two reductions, the downloads */
  double   seconds_output;       /* host: the result arrays */
  double   seconds_total;
  uint64_t query_groups;         /* groups the device formed (>= n_samples: a split costs a group, never a merge) */
  uint64_t target_groups;
  uint64_t targets_in_adds;      /* targets that took part in an add */
  uint64_t adds_sorted;          /* elements of the accumulate sort: the queries and the unmatched targets */
  uint64_t labels_device;        /* labels the scan kernel served */
  uint64_t labels_host;          /* labels the host restatement served */
  /* why the host restatement answered (at most one is 1) */
  uint64_t host_no_context;      /* ctx was NULL */
  uint64_t host_environment;     /* VSX_OTUTAB=host */
  uint64_t host_label_count;     /* more than UINT32_MAX - 1 labels on a side (or on both together: an add is numbered in 32 bits) */
  uint64_t host_memory;          /* blobs and per-label arrays do not fit the device's free memory */
} vsx_otutab_stats;

void vsx_otutab_opts_default(vsx_otutab_opts * o);

/* Build the table.  q_abundance NULL: 1 each.  q_target[k]: a target number or VSX_OTUTAB_NONE (no hit); NULL only without queries.
 * t_matched NULL: no unmatched pass (clustering).
 *
 * ctx NULL, or VSX_OTUTAB=host in the environment: the whole call runs through the host restatement.  So does a call with more
 * than UINT32_MAX - 1 labels, and one whose blobs do not fit the device's free memory.  The device route serves any label length.
 *
 * Testing aids, read per call: VSX_OTUTAB_HASH_BITS=n (1 .. 64) keeps the low n bits of every name hash; VSX_OTUTAB_DEVICE_LABELS
 * lowers the label count above which the host answers; VSX_OTUTAB_PRETEND_BYTES replaces the device memory the call is taken to need.
 *
 * VSX_EINVAL: a null argument, a q_target that is neither below targets->n nor VSX_OTUTAB_NONE, a span outside its blob. */
int vsx_otutab(vsx_ctx * ctx, const vsx_otutab_opts * opts, const vsx_labels * queries, const uint64_t * q_abundance,
               const uint32_t * q_target, const vsx_labels * targets, const uint8_t * t_matched, vsx_otutab_result * out);
void vsx_otutab_result_free(vsx_otutab_result * out);

/* figures of this thread's last vsx_otutab call */
void vsx_otutab_last_stats(vsx_otutab_stats * out);

/* The exact host restatement: the host route of vsx_otutab and the oracle of its tests.  No regular expressions; opts->threads host
 * threads.  Same arguments, refusals and result as vsx_otutab. */
int vsx_internal_otutab_host(const vsx_otutab_opts * opts, const vsx_labels * queries, const uint64_t * q_abundance,
                             const uint32_t * q_target, const vsx_labels * targets, const uint8_t * t_matched, vsx_otutab_result * out);

#ifdef __cplusplus
}
#endif
#endif
