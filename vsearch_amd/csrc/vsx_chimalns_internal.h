// vsx_chimalns_internal.h -- shared between the --uchimealns kernel (vsx_chimalns.hip) and its host side (vsx_chimalns.cpp).
// Run words are the library's ((length << 2) | op, op 0 = M, 1 = target only, 2 = query only; include/vsx.h) as a plan exports them:
// the run of the alignment's LAST column first.  The host has checked every job it sends: each alignment's runs sum to qlen query
// symbols and to the parent's length, no run is empty, no two target-only runs are adjacent, qlen <= VSX_CHIMERA_MAX_QLEN and
// alnlen (query length + the longer target-only run in front of each position) <= VSX_CHIMALNS_MAX_COLS.
#ifndef VSX_CHIMALNS_INTERNAL_H
#define VSX_CHIMALNS_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

struct VsxChimAlnJob {
  uint64_t q_off;              // the query in the query text (the database text for the de novo form)
  uint64_t a_off, b_off;       // the parents in the database text
  uint64_t runs_a, runs_b;     // first stored run word of (query, parent_a) / (query, parent_b)
  uint64_t text_off;           // the record's six rows in the text buffer: A, Q, B, Diffs, Votes, Model, alnlen bytes each
  uint64_t line_off;           // its first output line (three end positions per line: A, Q, B)
  uint32_t nruns_a, nruns_b;
  uint32_t qlen, alen, blen;
  uint32_t alnlen;
  uint32_t width;              // columns per output line, >= 1
  uint32_t pad;
};

#define VSX_CHIMALN_OK        0u
#define VSX_CHIMALN_NO_SCORE  1u   // no column gave an h score
#define VSX_CHIMALN_BAD_JOB   2u   // the job's lengths do not match what the kernel found (nothing was rendered)

// what the kernel recomputed of one record
struct VsxChimAlnRec {
  double   h;
  int32_t  best_i;
  int32_t  counts[6];          // left_yes, left_no, left_abstain, right_yes, right_no, right_abstain (of the winning branch)
  uint32_t alnlen;
  uint32_t reverse;            // 1: the reverse branch won (the parents were not given in the record's order)
  uint32_t status;             // VSX_CHIMALN_*
};

#ifdef __cplusplus
extern "C" {
#endif
// one workgroup per job
hipError_t vsx_launch_chimalns(const VsxChimAlnJob * d_jobs, uint32_t n, const uint8_t * d_qtext, uint64_t qtext_bytes, const uint8_t * d_dbtext,
                               uint64_t dbtext_bytes, const uint32_t * d_runs, uint64_t n_runs, double xn, double dn, uint8_t * d_text,
                               uint32_t * d_line_end, VsxChimAlnRec * d_rec, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
