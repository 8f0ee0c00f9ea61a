/* vsx_mask.h -- sequence masking (the analysis core of the reference's --fastx_mask and --maskfasta) on the GPU.
 *
 * Sequences go in as one host blob (the blob / offset / length convention of vsx_fastx_filter); out come, in input order, one
 * record per sequence (the count of unmasked symbols and the verdict of --min_unmasked_pct / --max_unmasked_pct), the masked text
 * of every sequence PACKED (sequence k at the sum of the lengths before it) and the mask bitmap over that packed text.
 *
 *   qmask  hardmask  text out                                                   `unmasked` counts
 *   none   any       unchanged                                                  len
 *   soft   0         unchanged                                                  symbols 'A' .. 'Z'
 *   soft   1         every byte with bit 0x20 set -> 'N'                        symbols != 'N'
 *   dust   0         upper-cased, DUST intervals = original | 0x20              symbols 'A' .. 'Z'
 *   dust   1         case kept, DUST intervals -> 'N'                           symbols != 'N'
 *
 * The DUST words come from the ORIGINAL text through the reference's 2-bit map (case ignored, U = T, everything else 0).
 * Bit i of the bitmap (bit i % 8 of byte i / 8) is set when packed symbol i does NOT count as unmasked; qmask none gives no bit.
 * FASTA / FASTQ parsing and writing, relabelling and the size annotations stay with the caller (vsearch_amd/mask.py has the writers).
 */
#ifndef VSX_MASK_H
#define VSX_MASK_H

#include "vsx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSX_MASK_NONE 0
#define VSX_MASK_SOFT 1
#define VSX_MASK_DUST 2

#define VSX_MASK_WANT_TEXT 1u
#define VSX_MASK_WANT_BITS 2u

#define VSX_MASK_KEPT 0
#define VSX_MASK_DISCARDED_LESS 1      /* 100.0 * unmasked / len <  min_unmasked_pct */
#define VSX_MASK_DISCARDED_MORE 2      /* 100.0 * unmasked / len >  max_unmasked_pct (and not less) */

typedef struct vsx_fastx_mask_opts {
  int32_t  qmask;             /* VSX_MASK_NONE / _SOFT / _DUST; default dust, the reference's */
  int32_t  hardmask;          /* 0 or 1 */
  double   min_unmasked_pct;  /* 0.0 */
  double   max_unmasked_pct;  /* 100.0 */
  uint32_t want;              /* VSX_MASK_WANT_TEXT | VSX_MASK_WANT_BITS; default both */
  uint32_t pad;
  int64_t  window;            /* sequences per staging window; 0: the built-in size.  Results do not depend on it. */
} vsx_fastx_mask_opts;

typedef struct vsx_fastx_mask_record {
  uint32_t unmasked;
  uint32_t verdict;           /* VSX_MASK_KEPT / _DISCARDED_LESS / _DISCARDED_MORE; a sequence of length 0 (NaN per cent) is kept */
} vsx_fastx_mask_record;

typedef struct vsx_fastx_mask_out {
  uint64_t                n;
  vsx_fastx_mask_record * rec;             /* n records, input order */
  char *                  text;            /* text_bytes of packed masked text, or NULL without WANT_TEXT */
  uint8_t *               bits;            /* (text_bytes + 7) / 8 bytes, or NULL without WANT_BITS */
  uint64_t                text_bytes;      /* the sum of the lengths */
  uint64_t                kept;            /* the three totals the command prints */
  uint64_t                discarded_less;
  uint64_t                discarded_more;
} vsx_fastx_mask_out;

typedef struct vsx_fastx_mask_stats {
  double   seconds_stage;          /* host: planning the windows, packing them into pinned memory, enqueueing */
  double   seconds_h2d;            /* device time of the host-to-device copies (events), summed over the windows */
  double   seconds_mask;           /* device time of the DUST kernels of both routes (events) */
  double   seconds_apply;          /* device time of the apply kernel (events) */
  double   seconds_d2h_output;     /* waiting for the results + building the output, host-route sequences included */
  double   seconds_total;
  uint64_t sequences;
  uint64_t sequences_short;        /* DUST by one wavefront per sequence */
  uint64_t sequences_long;         /* DUST by a window at every position + the chain resolution */
  uint64_t sequences_device_plain; /* on the device without DUST (qmask none / soft) */
  uint64_t sequences_host_forced;  /* VSX_MASK=host */
  uint64_t sequences_host_memory;  /* a staging window that does not fit the device */
  uint64_t sequences_host_long;    /* a long-route sequence whose working set does not fit */
  uint64_t windows;                /* staging windows */
  uint64_t dust_windows;           /* DUST windows evaluated (device and host) */
  uint64_t long_min;               /* the route threshold and the segment length the call used */
  uint64_t segment;
} vsx_fastx_mask_stats;

void vsx_fastx_mask_opts_default(vsx_fastx_mask_opts * o);

/* Mask n sequences.  ctx may be NULL only when the environment has VSX_MASK=host (every sequence through the host restatement).
 * VSX_EINVAL: an option value the reference refuses (a percentage outside 0 .. 100, min > max), an unknown qmask / hardmask / want
 * bit, a negative window, a sequence beyond the blob or longer than INT32_MAX, two sequences that share blob bytes.
 * VSX_MASK_LONG_MIN / VSX_MASK_SEGMENT (tests) replace the built-in route threshold and segment length. */
int vsx_fastx_mask(vsx_ctx * ctx, const vsx_fastx_mask_opts * opts, uint64_t n, const char * blob, uint64_t blob_bytes,
                   const uint64_t * offsets, const uint32_t * lengths, vsx_fastx_mask_out * out);
void vsx_fastx_mask_out_free(vsx_fastx_mask_out * out);

/* figures of this thread's last vsx_fastx_mask call */
void vsx_fastx_mask_last_stats(vsx_fastx_mask_stats * out);

#ifdef __cplusplus
}
#endif
#endif
