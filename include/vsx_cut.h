/* vsx_cut.h -- in-silico restriction digest (the analysis core of the reference's --cut) on the GPU.
 *
 * Sequences go in as one host blob (the blob / offset / length convention of vsx_fastx_mask).  One IUPAC pattern is tested at every
 * position of every sequence; the pattern carries one '^' (where the forward strand is cut) and one '_' (the reverse strand).
 *
 *   match at i (0 <= i <= L - P)   for every j: code(pattern[j]) & code(seq[i + j]) != 0, code = the reference's chrmap_4bit
 *                                  (IUPAC, either case, U = T; any other byte has code 0 and matches nothing).  Overlaps all count.
 *   forward fragments              the cut points c = i + cut_fwd split [0, L) into [0, c_0), [c_0, c_1), ... [c_last, L); an empty
 *                                  piece (only the first and the last can be) is left out.  Sequences without a match give none.
 *   reverse fragments              the same pieces from d = i + cut_rev, in the same order; their TEXT is the piece reverse-complemented
 *                                  (chrmap_complement: case kept, unknown -> N).  Records stay in forward coordinates.
 *   uncut                          the sequences without a match, in input order.
 *
 * A fragment's ordinal (what --relabel prints) is its index in its list + 1: the lists run over the whole input, in output order.
 * Forward pieces are substrings of the caller's input and are not copied.  With a text bit the reverse-complemented pieces come back
 * in one packed blob: first the reverse fragments (VSX_CUT_WANT_REV_TEXT) in list order, then the uncut sequences whole
 * (VSX_CUT_WANT_DISCARDED_REV_TEXT) in list order, each kind with n + 1 offsets into the blob.
 * FASTA parsing and writing, relabelling and the size annotations stay with the caller (vsearch_amd/cut.py has the writers).
 */
#ifndef VSX_CUT_H
#define VSX_CUT_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_CUT_WANT_FWD                1u   /* the forward fragment list */
#define VSX_CUT_WANT_REV                2u   /* the reverse fragment list */
#define VSX_CUT_WANT_REV_TEXT           4u   /* the text of the reverse fragments (returns the reverse list too) */
#define VSX_CUT_WANT_DISCARDED_REV_TEXT 8u   /* the uncut sequences, reverse-complemented */

#define VSX_CUT_DEVICE_MAX_PATTERN 64        /* a longer pattern (without its marks) runs through the host restatement */

/* what vsx_cut_pattern_check found, in the order the reference looks */
#define VSX_CUT_PATTERN_OK        0
#define VSX_CUT_PATTERN_NO_FWD    1          /* "No forward sequence cut site (^) found in pattern" */
#define VSX_CUT_PATTERN_NO_REV    2          /* "No reverse sequence cut site (_) found in pattern" */
#define VSX_CUT_PATTERN_MULTIPLE  3          /* "Multiple cut sites not supported" */
#define VSX_CUT_PATTERN_EMPTY     4          /* "Empty cut pattern string" */
#define VSX_CUT_PATTERN_ILLEGAL   5          /* "Illegal character in cut pattern" */

typedef struct vsx_cut_opts {
  const char * pattern;       /* the raw pattern with its two marks, e.g. "G^AATT_C" */
  uint64_t     pattern_len;
  uint32_t     want;          /* VSX_CUT_WANT_* bits; default all four */
  int32_t      threads;       /* host restatement: 0 = the usable CPUs, at most 16 */
  int64_t      window;        /* sequences per launch of the match kernel; 0: the built-in size.  Results do not depend on it. */
} vsx_cut_opts;

typedef struct vsx_cut_fragment {
  uint64_t seq;               /* input number of the sequence */
  uint32_t start;             /* forward coordinates, also for a reverse fragment */
  uint32_t length;            /* > 0 */
} vsx_cut_fragment;

typedef struct vsx_cut_out {
  uint64_t           n;
  uint32_t *         matches;       /* n: matches per sequence */
  uint64_t           n_fwd;
  vsx_cut_fragment * fwd;           /* n_fwd records in output order, or NULL without WANT_FWD (n_fwd is counted regardless) */
  uint64_t           n_rev;
  vsx_cut_fragment * rev;           /* n_rev records, or NULL without WANT_REV / WANT_REV_TEXT */
  uint64_t           n_uncut;
  uint64_t *         uncut;         /* n_uncut sequence numbers, rising */
  char *             text;          /* text_bytes of reverse-complemented pieces, or NULL without a text bit */
  uint64_t           text_bytes;
  uint64_t *         rev_off;       /* n_rev + 1 offsets into text, or NULL without WANT_REV_TEXT */
  uint64_t *         discarded_off; /* n_uncut + 1 offsets into text, or NULL without WANT_DISCARDED_REV_TEXT */
  uint64_t           cut;           /* the three totals the command prints: sequences with a match, */
  uint64_t           uncut_total;   /* sequences without, */
  uint64_t           total_matches; /* matches */
} vsx_cut_out;

typedef struct vsx_cut_stats {
  double   seconds_stage;          /* host: checks, the block and work-item tables, packing scattered input */
  double   seconds_h2d;            /* uploading text and tables */
  double   seconds_match;          /* the match kernel */
  double   seconds_rank;           /* the scan over the block counts and the compaction */
  double   seconds_fragments;      /* per-sequence counts, their scans, the fragment and uncut kernels */
  double   seconds_emit;           /* piece offsets and the reverse-complement kernel */
  double   seconds_output;         /* copying the results back; the whole host restatement on a host route */
  double   seconds_total;
  uint64_t sequences;
  uint64_t symbols;
  uint64_t blocks;                 /* 64-position blocks of the device route */
  uint64_t items;                  /* work items (sequence, tile) */
  uint64_t tile;                   /* positions per work item the call used */
  uint64_t pattern_length;
  uint64_t host_no_context;        /* the host routes: 1 when the call took it */
  uint64_t host_environment;       /* VSX_CUT=host */
  uint64_t host_count;             /* more than UINT32_MAX - 1 sequences or possible fragments (symbols + sequences) */
  uint64_t host_memory;            /* text and tables do not fit the device */
  uint64_t host_pattern_length;    /* a pattern longer than VSX_CUT_DEVICE_MAX_PATTERN */
} vsx_cut_stats;

void vsx_cut_opts_default(vsx_cut_opts * o);

/* Which of the reference's five refusals applies to a raw pattern, or VSX_CUT_PATTERN_OK.  On OK: *plen = the length without the
 * marks, stripped (when not NULL; room for len bytes) = the pattern without them, *cut_fwd / *cut_rev = the index of '^' after '_' is
 * removed / of '_' after '^' is removed, both in 0 .. *plen. */
int vsx_cut_pattern_check(const char * pattern, uint64_t len, char * stripped, uint64_t * plen, int32_t * cut_fwd, int32_t * cut_rev);

/* Cut n sequences.  ctx may be NULL: the call then runs the host restatement (counted in the statistics), as it does under VSX_CUT=host.
 * VSX_EINVAL: a pattern vsx_cut_pattern_check refuses (the error text carries the reference's message), an unknown want bit, a negative
 * window or thread count, a sequence beyond the blob or longer than INT32_MAX (the reference holds lengths as int).
 * VSX_CUT_TILE (positions per work item, a multiple of 64), VSX_CUT_PRETEND_BYTES (what the call pretends to need of the device) and
 * VSX_CUT_DEVICE_COUNT (the count limit of the device route) are testing aids, read per call. */
int vsx_cut(vsx_ctx * ctx, const vsx_cut_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
            const uint64_t * offsets, const uint32_t * lengths, vsx_cut_out * out);
void vsx_cut_out_free(vsx_cut_out * out);

/* figures of this thread's last vsx_cut call */
void vsx_cut_last_stats(vsx_cut_stats * out);

#ifdef __cplusplus
}
#endif
#endif
