/* vsx_hitout.h -- what the search writers need from a hit list, on the GPU: the gapped query and target rows, the symbol row of
 * --alnout and SAM's MD:Z: string (the reference's core/showalign.cpp: get_alignment_row, putop, get_aligment_symbol, and
 * core/results.cpp: build_sam_strings).  Everything else --alnout, --samout, --blast6out, --fastapairs, --qsegout, --tsegout and
 * --userout print is a printf over fields vsx_hit already carries (vsearch_amd/hitout.py).
 *
 * Callers: the results of vsx_search_batch(_meta), vsx_search_exact and vsx_multi_search_batch (render with replica 0).  NOT covered:
 * the hits of vsx_allpairs_* and vsx_cluster_fast -- their queries are database sequences, which this call does not take.  The
 * chimera commands' --uchimealns block is a call of its own: vsx_chimera_alns (vsx_chimalns.h); so is --lcaout: vsx_lca (vsx_lca.h).
 *
 * Query text.  The call masks the queries itself with the code the search uses -- the plus strand and, under strand_both, the
 * reverse complement, each on its own (core/search.cpp:294-303): --qmask dust leaves the DUST intervals in lower case, --hardmask
 * turns them into 'N'.  For a minus-strand hit qrow, the MD string, --fastapairs and --qsegout read the separately masked reverse
 * complement, while --alnout walks the PLUS strand's masked text backwards through the complement table
 * (showalign.cpp:179-185,345): such a hit gets an --alnout query row of its own.
 * Target text: vsx_searcher_db_text, uploaded to the device by the searcher's first render call and kept.
 *
 * Columns.  A CIGAR is the project's: 'M' takes a symbol of both, 'D' of the query only (gap in the target row), 'I' of the target
 * only (gap in the query row); a run without a count is 1.  The rows cover the columns [trim_q_left + trim_t_left, + internal_alignmentlength)
 * (results.cpp:459-481, :100-155); the MD string is built over the UNtrimmed alignment.
 */
#ifndef VSX_HITOUT_H
#define VSX_HITOUT_H

#include "vsx_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_HITOUT_ROWS    1u      /* qrow, trow                                      */
#define VSX_HITOUT_SYMBOLS 2u      /* the symbol row and the --alnout query row       */
#define VSX_HITOUT_SAM     4u      /* the MD:Z: string                                */
#define VSX_HITOUT_NONE    0xFFFFFFFFFFFFFFFFull   /* an offset of something that was not asked for */

typedef struct vsx_hitout_opts {
  uint32_t want;           /* mask of VSX_HITOUT_*; nothing is computed or allocated for a bit that is not set */
  int32_t  threads;        /* host threads (masking, CIGAR parsing, the host restatement); 0: what the process may use, 16 at most */
  uint64_t window;         /* hits per device pass; 0 = 262 144.  The result does not depend on it */
} vsx_hitout_opts;

/* All arrays are malloc()'d (release with vsx_hit_text_free); an array whose bit is not set in `want` is NULL.
 * row_blob holds, hit after hit: qrow, trow (ROWS), the symbol row and -- for a minus-strand hit, or when ROWS is not set -- the
 * --alnout query row (SYMBOLS); each row_len[h] = internal_alignmentlength bytes, no terminator.  A plus-strand hit shares its
 * qrow with --alnout: aln_off[h] == qrow_off[h].  md_blob holds the MD strings back to back in hit order. */
typedef struct vsx_hit_text {
  uint64_t   n_queries, n_hits;
  uint32_t   want;
  uint32_t   both;                                       /* the minus strands' texts are present */
  char *     row_blob;   uint64_t row_bytes;
  uint32_t * row_len;                                    /* n_hits (always) */
  uint64_t * qrow_off, * trow_off;                       /* ROWS */
  uint64_t * sym_off, * aln_off;                         /* SYMBOLS */
  char *     md_blob;    uint64_t md_bytes;              /* SAM */
  uint64_t * md_off;     uint32_t * md_len;
  /* the masked query texts (SAM's SEQ, --qsegout): plus strand of query q at qtext[qplus_off[q] .. + qlen[q]); under strand_both
     its separately masked reverse complement at qminus_off[q], else qminus_off is NULL */
  char *     qtext;      uint64_t qtext_bytes;
  uint64_t * qplus_off, * qminus_off;
} vsx_hit_text;

typedef struct vsx_hitout_stats {
  double   seconds_mask;         /* host: the strands' texts, masked */
  double   seconds_stage;        /* host: CIGAR parse into run words, trimmed ranges, output offsets */
  double   seconds_h2d;          /* uploads (database text on the first call, query text, run words, jobs) */
  double   seconds_rows;         /* the row kernel */
  double   seconds_md_count;     /* the MD count kernel and the offset scan */
  double   seconds_md_fill;      /* the MD fill kernel */
  double   seconds_d2h;          /* downloads */
  double   seconds_host;         /* the host restatement */
  double   seconds_total;
  uint64_t windows;
  uint64_t hits_device, hits_host;   /* rendered by the kernels / by the host restatement */
  uint64_t db_text_uploaded;     /* this call put the database text on the device */
  /* why the host restatement answered (at most one is 1) */
  uint64_t host_no_context;      /* the searcher has no context (or the call was vsx_internal_hits_render_host) */
  uint64_t host_environment;     /* VSX_HITOUT=host */
  uint64_t host_hit_count;       /* more than UINT32_MAX - 1 hits */
  uint64_t host_memory;          /* the texts and one window's blobs do not fit the device's free memory */
} vsx_hitout_stats;

void vsx_hitout_opts_default(vsx_hitout_opts * o);       /* want = all three */

/* The queries exactly as they were handed to the search call, and the vsx_hits that call returned.
 * VSX_EINVAL: a null argument, a query span outside its blob, n_queries that differs from hits->n_queries, a `first` that does not
 * ascend to n_hits, a hit whose query or target is out of range or whose vsx_hit.query is not the query it is listed under, a
 * cigar_off outside the blob, a CIGAR with an unknown operation or an empty run, a CIGAR whose runs do not sum to the two lengths,
 * trimmed columns that do not lie inside the alignment, a minus-strand hit of a searcher without strand_both.
 * Testing aids, read per call: VSX_HITOUT=host; VSX_HITOUT_DEVICE_HITS lowers the hit count above which the host answers;
 * VSX_HITOUT_PRETEND_BYTES replaces the device memory the call is taken to need.  Two calls give identical bytes. */
int vsx_hits_render(vsx_searcher * s, const vsx_hitout_opts * o, uint64_t n_queries, const char * qblob, uint64_t qblob_bytes,
                    const uint64_t * qoffsets, const uint32_t * qlengths, const vsx_hits * hits, vsx_hit_text * out);
void vsx_hit_text_free(vsx_hit_text * t);
/* figures of this thread's last vsx_hits_render / vsx_internal_hits_render_host */
void vsx_hits_render_last_stats(vsx_hitout_stats * out);

/* For tests / tooling: the exact host restatement on a database given as text AS INDEXED (it is not masked again); no device, no
 * context.  Of `sopts` the masking of the queries (soft_mask, qmask, hardmask) and strand_both are read, of `scoring` n_mismatch. */
int vsx_internal_hits_render_host(const vsx_scoring * scoring, const vsx_search_opts * sopts, const vsx_hitout_opts * o,
                                  uint64_t n_db, const char * db_text, uint64_t db_bytes, const uint64_t * db_offsets, const uint32_t * db_lengths,
                                  uint64_t n_queries, const char * qblob, uint64_t qblob_bytes, const uint64_t * qoffsets,
                                  const uint32_t * qlengths, const vsx_hits * hits, vsx_hit_text * out);

#ifdef __cplusplus
}
#endif
#endif
