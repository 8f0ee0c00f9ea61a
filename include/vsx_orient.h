/* vsx_orient.h -- sequence orientation (--orient) on a searcher (vsx_orient.cpp / vsx_orient.hip).
 *
 * Restated from the reference (commands/orient.cpp:116-441, core/dbindex.cpp:121-148, core/unique.cpp:155-352, cli.cc:4185-4196):
 *   database  the searcher's text as indexed (--dbmask, --hardmask, --wordlength).  mc[word] = the number of database sequences
 *             that contain `word` at least once; a word is valid iff none of its symbols is ambiguous and, in every mask mode
 *             but none, none is lower case.  U = T.  The command's own default word length is 12
 *   query     only the forward strand is walked, over its distinct valid words, and the text is taken AS GIVEN: the reference
 *             neither DUST-masks nor hard-masks the query of this command.  qmask none: only ambiguity poisons a word; soft or
 *             dust (the default): lower case does too
 *   word      hf = mc[word], hr = mc[rc(word)] (2-bit reverse complement at the word length).  hf > 8u * hr: count_fwd + 1;
 *             else hr > 8u * hf: count_rev + 1.  32-bit unsigned arithmetic as written there
 *   verdict   + iff count_fwd >= 1 and count_fwd >= 4u * count_rev; else - iff count_rev >= 1 and count_rev >= 4u * count_fwd;
 *             else ?
 *   text      + and ? reads as given; - reads reverse-complemented (chrmap_complement: IUPAC, case kept), qualities reversed
 *
 * Routes.  The kernels serve word lengths 3..12 (the match-count table is mc[4^w] of uint32, 64 MB at 12) and queries of up to
 * VSX_ORIENT_MAX_QLEN symbols.  Word lengths 13..15 (a direct table of 256 MB .. 4 GB), longer queries, VSX_ORIENT=host and a
 * searcher without a device go to the exact host restatement.  vsx_orient_stats counts each route.
 */
#ifndef VSX_ORIENT_H
#define VSX_ORIENT_H

#include "vsx_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_ORIENT_MAX_QLEN    16384       /* the largest distinct-word set the count kernel keeps in LDS */
#define VSX_ORIENT_MAX_DEVICE_WORDLENGTH 12
#define VSX_ORIENT_CLASSES     3           /* length classes of the count kernel: queries of up to 512 / 4 096 / 16 384 symbols */

typedef struct vsx_orient_opts {
  int32_t qmask;             /* 0 none, 1 soft, 2 dust (dust = soft here: the query is never DUST-masked) */
  int32_t want_text;         /* also return the oriented text (and qualities) */
  int64_t window;            /* queries per device window; 0 = 65 536 */
} vsx_orient_opts;
void vsx_orient_opts_default(vsx_orient_opts * o);     /* qmask 2, want_text 0, window 0 */

typedef struct vsx_orient_record {
  uint32_t count_fwd, count_rev;
  int32_t  strand;                                     /* 0 +, 1 -, 2 ? */
} vsx_orient_record;

typedef struct vsx_orient_result {
  uint64_t n_queries, n_fwd, n_rev, n_none;
  vsx_orient_record * rec;                             /* n_queries */
  char * text;                                         /* want_text: qbytes bytes, query k at the caller's offsets[k]; - reads */
  char * qual;                                         /* reverse-complemented / reversed, the others copied.  qual: NULL without qualities */
} vsx_orient_result;
void vsx_orient_result_free(vsx_orient_result * r);

typedef struct vsx_orient_stats {
  uint64_t queries_device;
  uint64_t queries_host_wordlength;                    /* word length 13..15 */
  uint64_t queries_host_qlen;                          /* longer than VSX_ORIENT_MAX_QLEN */
  uint64_t queries_host_forced;                        /* VSX_ORIENT=host, or a searcher without a device */
  uint64_t queries_class[VSX_ORIENT_CLASSES];          /* device queries per length class */
  uint64_t windows;
  uint64_t words_distinct;                             /* distinct valid words looked up, over all queries */
  uint64_t build_chunks, build_keys;                   /* the table build of this call (0 when the table existed) */
  double   seconds_build, seconds_stage, seconds_count, seconds_emit, seconds_output, seconds_total;
} vsx_orient_stats;
void vsx_orient_last_stats(vsx_orient_stats * out);

/* The first call builds the match-count table and keeps it in the searcher; the k-mer postings index is not built.  qualblob
   (may be NULL) holds the qualities at the same offsets.  One call at a time per searcher (the window buffers live in it).
   With want_text, queries must not overlap in the blob. */
int vsx_orient(vsx_searcher * s, const vsx_orient_opts * opts, uint64_t n_queries, const char * qblob, uint64_t qbytes,
               const uint64_t * offsets, const uint32_t * lengths, const char * qualblob, vsx_orient_result * out);

/* The same computation on the CPU, no device: the database as text; of `search` the masking options (soft_mask, hardmask bit 0),
   wordlength and threads are read.  The test oracle, and the host route of vsx_orient. */
int vsx_internal_orient_host(const vsx_search_opts * search, const vsx_orient_opts * opts, uint64_t n, const char * blob,
                             uint64_t blob_bytes, const uint64_t * offsets, const uint32_t * lengths, uint64_t n_queries,
                             const char * qblob, uint64_t qbytes, const uint64_t * qoff, const uint32_t * qlen, const char * qualblob,
                             vsx_orient_result * out);

/* For tests: counts[i] = the device table's entry for words[i] (built if no call has); VSX_EINVAL for a searcher the device
   route does not serve or a word of more than 2 * wordlength bits. */
int vsx_internal_orient_matchcounts(vsx_searcher * s, const uint32_t * words, uint64_t n, uint32_t * counts);

#ifdef __cplusplus
}
#endif
#endif
