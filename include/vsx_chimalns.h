/* vsx_chimalns.h -- the --uchimealns alignment block of chimera records (vsx_chimalns.cpp / vsx_chimalns.hip).
   The reference prints the block serially under its output lock (core/chimera.cpp:1699-1808): the three-row alignment of the query
   with its two parents, the rows Diffs / Votes / Model, and per output line the positions the three sequences have reached.  Here
   every selected record of a finished vsx_uchime_ref / vsx_uchime_denovo is rendered by one workgroup of a kernel of its own, in
   column space; the scoring kernel (vsx_chimera.hip) never builds the three rows and is not touched.
   The renderer takes (query, parent_a, parent_b) AS THE RECORD NAMES THEM, i.e. after the reference's A / B flip.  In that order the
   reference's forward branch wins the column scan (the flipped h expressions are the same doubles, the visit order and the strict
   '>' are the same), so the block is a pure function of the three texts, the two alignments, xn and dn.  Both branches are still
   computed: a record whose recomputed winner is the reverse branch, or whose recomputed h (bit pattern) or left / right counts
   differ from the record, fails the call (VSX_EINVAL) -- it was not produced by this library from these sequences. */
#ifndef VSX_CHIMALNS_H
#define VSX_CHIMALNS_H

#include "vsx_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_CHIMALNS_Y          1u   /* select: records with flag 'Y' (what the reference prints) */
#define VSX_CHIMALNS_BORDERLINE 2u   /*         flag '?' */
#define VSX_CHIMALNS_N          4u   /*         scored records with flag 'N' */
#define VSX_CHIMALNS_MAX_COLS   8192 /* longest alignment the kernel takes (its LDS layout); queries above VSX_CHIMERA_MAX_QLEN and longer
                                        alignments: host restatement */

typedef struct vsx_chimalns_opts {
  double   xn, dn;          /* the detection's --xn / --dn (h is recomputed) */
  int32_t  alignwidth;      /* --alignwidth: columns per output line; 0 = one line per record.  Default 80 */
  uint32_t select;          /* mask of VSX_CHIMALNS_*; 0 = VSX_CHIMALNS_Y */
  int64_t  window;          /* selected records per device pass; 0 = 4 096.  The result does not depend on it */
  int32_t  threads;         /* host threads of the host restatement; 0 = the usable CPUs */
  int32_t  pad;
} vsx_chimalns_opts;
void vsx_chimalns_opts_default(vsx_chimalns_opts * o);

/* Rendered record j (j < n, in the order of the records): record[j] = its index in `records`; its six rows A, Q, B, Diffs, Votes,
   Model are alnlen[j] bytes each, row r at text + text_off[j] + r * alnlen[j] (no terminators).  Its output lines are
   line_first[j] .. line_first[j + 1] - 1; line l ends at positions line_end[3 l + 0 / 1 / 2] of A / Q / B (the reference's p + nt:
   symbols printed up to and including that line), so line l starts at the previous line's end + 1.  best_i[j], h[j] and
   counts[6 j ..] = left_yes, left_no, left_abstain, right_yes, right_no, right_abstain are the recomputed values.
   Free with vsx_chimalns_out_free. */
typedef struct vsx_chimalns_out {
  uint64_t   n;
  uint64_t   text_bytes, n_lines;
  uint64_t * record;
  uint32_t * alnlen;
  uint64_t * text_off;
  char     * text;
  uint64_t * line_first;      /* n + 1 */
  uint32_t * line_end;        /* 3 * n_lines */
  int32_t  * best_i;
  double   * h;
  int32_t  * counts;          /* 6 * n */
} vsx_chimalns_out;
void vsx_chimalns_out_free(vsx_chimalns_out * o);

/* records[k] = the record of query k of a finished vsx_uchime_ref over the same n queries (qblob / qoff / qlen as given there), or,
   with qblob == NULL, of sequence k of a finished vsx_uchime_denovo (n = the searcher's sequence count; the queries are the
   searcher's own sequences).  Every selected record's query is re-aligned with parent_a and parent_b in one plan per window (the
   aligner is deterministic per pair: these are the alignments the detection saw).  Host restatement, counted: a pair the 16-bit
   aligner refuses (realigned with vsx_lma_align), a query longer than VSX_CHIMERA_MAX_QLEN, an alignment longer than
   VSX_CHIMALNS_MAX_COLS, and every record under VSX_CHIMALNS=host. */
int vsx_chimera_alns(vsx_searcher * s, const vsx_chimalns_opts * opts, uint64_t n, const char * qblob, uint64_t qbytes,
                     const uint64_t * qoff, const uint32_t * qlen, const vsx_chimera_result * records, vsx_chimalns_out * out);

/* accounting of the calling thread's last vsx_chimera_alns */
typedef struct vsx_chimalns_stats {
  double   seconds_align;     /* re-alignment: plan + export + download of hit records and run words */
  double   seconds_kernel;    /* upload of the jobs, the rendering kernel */
  double   seconds_download;  /* rows, line ends and per-record values back to the host */
  double   seconds_host;      /* the host restatement */
  double   seconds_total;
  uint64_t windows, records_selected, records_kernel, records_host, sentinel_pairs;
  uint64_t host_long_query, host_long_alignment, host_forced;      /* why a record took the host route (a sentinel pair: the rest) */
} vsx_chimalns_stats;
void vsx_chimalns_last_stats(vsx_chimalns_stats * out);

/* For tests / tooling: the host restatement on ONE (query, parent_a, parent_b) triple given as text with the two alignments as CIGAR
   text (query against parent, as vsx_lma_align writes it); no device.  out: one rendered record (record[0] = 0).  VSX_EINVAL when a
   CIGAR does not span its two sequences or no column gives an h score. */
int vsx_internal_chimalns_host(const char * q, uint32_t qlen, const char * a, uint32_t alen, const char * b, uint32_t blen,
                               const char * cigar_a, const char * cigar_b, const vsx_chimalns_opts * opts, vsx_chimalns_out * out);

/* For tests / tooling: the KERNEL on n such triples (one workgroup each), in one launch on the context's device.  VSX_EINVAL also for a
   triple beyond the kernel (query above VSX_CHIMERA_MAX_QLEN, alignment above VSX_CHIMALNS_MAX_COLS). */
int vsx_internal_chimalns_device(vsx_ctx * ctx, uint64_t n, const char * const * q, const uint32_t * qlen, const char * const * a,
                                 const uint32_t * alen, const char * const * b, const uint32_t * blen, const char * const * cigar_a,
                                 const char * const * cigar_b, const vsx_chimalns_opts * opts, vsx_chimalns_out * out);

#ifdef __cplusplus
}
#endif
#endif
