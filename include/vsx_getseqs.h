/* vsx_getseqs.h -- sequence extraction by label (the reference's --fastx_getseqs, --fastx_getseq and --fastx_getsubseq,
 * core/getseq.cpp) on the GPU.
 *
 * A HEADER is the byte span the caller passes: what the reference's parser hands on (cut at the first blank unless
 * --notrunclabels).  Exactly one mode per call; the single-needle modes take exactly one needle:
 *
 *   mode     substr  field   a header matches when
 *   LABEL    0       -       it has the needle's length and its bytes, after folding a-z to upper case
 *   LABEL    1       -       the folded needle occurs in the folded header; an EMPTY needle matches every non-empty header
 *   LABELS   0 / 1   -       the same against any label of the list
 *   WORD     -       absent  some occurrence of the needle (exact bytes) is bounded on both sides by the header's start / end
 *                            or a byte outside [0-9A-Za-z]
 *   WORD     -       given   some occurrence of field '=' needle is bounded on both sides by the header's start / end or ';'
 *   WORDS    -       any     the WORD rule against any label of the list
 *
 * Folding is ASCII a-z only; bytes >= 0x80 fold to themselves and are no alphanumerics.  Every occurrence counts, overlapping
 * ones too.  substr is ignored by the word modes, field by LABEL / LABELS.  An empty list matches nothing.
 *
 * With subseq_start / subseq_end (--fastx_getsubseq) a MATCHED sequence of length len gives the piece [start - 1, end) with
 * start = max(subseq_start, 1), end = min(subseq_end, len); it is empty, at offset 0, when end < start.  Unmatched sequences
 * are always whole.  Nothing is copied: the writers cut the caller's text and qualities with (start, length).
 * FASTA / FASTQ parsing and writing stay with the caller (vsearch_amd/getseqs.py has the writers and the labels-file reader).
 */
#ifndef VSX_GETSEQS_H
#define VSX_GETSEQS_H

#include "vsx.h"
#include "vsx_otutab.h"       /* vsx_labels */

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_GETSEQS_LABEL  0
#define VSX_GETSEQS_LABELS 1
#define VSX_GETSEQS_WORD   2
#define VSX_GETSEQS_WORDS  3

/* the longest needle (field '=' included) and, in the modes that look for occurrences, the longest header the device serves */
#define VSX_GETSEQS_DEVICE_MAX_BYTES 2047

typedef struct vsx_getseqs_opts {
  int32_t      mode;           /* VSX_GETSEQS_LABEL / _LABELS / _WORD / _WORDS */
  int32_t      substr;         /* 0 or 1: --label_substr_match */
  const char * field;          /* --label_field, or NULL */
  uint64_t     field_len;
  int64_t      subseq_start;   /* both 0: not a --fastx_getsubseq call; else both >= 1 and start <= end */
  int64_t      subseq_end;
  int64_t      window;         /* headers per match launch; 0: the built-in size.  Results do not depend on it. */
  int32_t      threads;        /* host threads of the host restatement; 0: what the process may use, 16 at most */
  int32_t      pad;
} vsx_getseqs_opts;

typedef struct vsx_getseqs_record {
  uint32_t matched;            /* 0 / 1 */
  uint32_t ordinal;            /* 1-based count among the sequences of the same verdict up to and including this one */
  uint32_t start;              /* the piece to print: [start, start + length) of the sequence */
  uint32_t length;
} vsx_getseqs_record;

typedef struct vsx_getseqs_out {
  uint64_t             n;
  vsx_getseqs_record * rec;    /* n records, input order */
  uint64_t             kept;
  uint64_t             discarded;
} vsx_getseqs_out;

typedef struct vsx_getseqs_stats {
  double   seconds_stage;      /* host: the checks, composing field '=' label, the uploads */
  double   seconds_table;      /* the needle table: zeroing, hashing and inserting (host route: building the host table) */
  double   seconds_match;      /* the match launches (host route: the match loop) */
  double   seconds_ordinals;   /* the scan over the verdicts and the record kernel (host route: the serial count) */
  double   seconds_output;     /* the download of the records */
  double   seconds_total;
  uint64_t headers_device;
  uint64_t headers_host;
  /* why the host restatement answered (at most one is 1) */
  uint64_t host_no_context;    /* ctx was NULL */
  uint64_t host_environment;   /* VSX_GETSEQS=host */
  uint64_t host_count;         /* more than UINT32_MAX - 1 headers */
  uint64_t host_memory;        /* blobs and per-header arrays do not fit the device's free memory */
  uint64_t host_needle_length; /* a needle of more than VSX_GETSEQS_DEVICE_MAX_BYTES bytes */
  uint64_t host_header_length; /* an occurrence mode with a header of more than VSX_GETSEQS_DEVICE_MAX_BYTES bytes */
  uint64_t host_lengths;       /* more distinct needle lengths than VSX_GETSEQS_MAX_LENGTHS allows (unset: no limit) */
  uint64_t labels_in_table;    /* needles entered (duplicates included) */
  uint64_t distinct_lengths;
  uint64_t table_slots;
  uint64_t probes;             /* (position, length) pairs looked up */
  uint64_t verifications;      /* byte comparisons of a slot whose length and hash agreed */
} vsx_getseqs_stats;

void vsx_getseqs_opts_default(vsx_getseqs_opts * o);

/* Decide every header.  seq_lengths (n values) is read only for the subsequence arithmetic and may be NULL without headers.
 *
 * ctx NULL, or VSX_GETSEQS=host in the environment: the whole call runs through the host restatement (the same hashed rule on
 * opts->threads host threads).  So does a call with more than UINT32_MAX - 1 headers, one whose blobs do not fit the
 * device's free memory, one with a needle longer than VSX_GETSEQS_DEVICE_MAX_BYTES and, in the occurrence modes, one with a
 * header longer than that.
 *
 * Testing aids, read per call: VSX_GETSEQS_HASH_BITS=n (1 .. 63) keeps the low n bits of every hash; VSX_GETSEQS_DEVICE_HEADERS
 * lowers the count above which the host answers; VSX_GETSEQS_PRETEND_BYTES replaces the device memory the call is taken to need;
 * VSX_GETSEQS_MAX_LENGTHS sends a call with more distinct needle lengths to the host.
 *
 * VSX_EINVAL: a null argument; an unknown mode; substr other than 0 / 1; a negative window or threads; field_len without field;
 * more than 2^30 needles; a single-needle mode with another count than one needle; an empty needle in a word mode; an empty label in a
 * list; a NUL byte in a needle, a label or field; subseq values below 1 (unless both are 0) or start > end; a span outside
 * its blob. */
int vsx_getseqs(vsx_ctx * ctx, const vsx_getseqs_opts * opts, const vsx_labels * headers, const uint32_t * seq_lengths,
                const vsx_labels * needles, vsx_getseqs_out * out);
void vsx_getseqs_out_free(vsx_getseqs_out * out);

/* figures of this thread's last vsx_getseqs call */
void vsx_getseqs_last_stats(vsx_getseqs_stats * out);

#ifdef __cplusplus
}
#endif
#endif
