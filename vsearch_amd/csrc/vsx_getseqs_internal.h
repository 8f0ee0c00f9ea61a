// vsx_getseqs_internal.h -- shared between the extraction kernels (vsx_getseqs.hip) and their host side (vsx_getseqs.cpp).
//
// The hash of a byte string s[0, n) is  P(s) = sum over k of (fold(s[k]) + 1) * B^k  (mod 2^64), B odd.  With the prefix sums
// F[i] = P(s[0, i)) the hash of s[p, p + l) is (F[p + l] - F[p]) * B^-p: B is odd, so B^-1 exists mod 2^64.  A table key is
// mix(P ^ l * M) cut to hash_mask; a slot holds the key, the needle's length and its number + 1 (0: empty).
#ifndef VSX_GETSEQS_INTERNAL_H
#define VSX_GETSEQS_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>
#include "vsx_symbols.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define VSX_GS_HD __host__ __device__
#else
#define VSX_GS_HD
#endif

#define VSX_GS_BASE       vsxsym::kGolden              // odd
#define VSX_GS_LENGTH_MUL vsxsym::kLengthMul

#define VSX_GS_BOUND_NONE  0u                          // LABEL / LABELS
#define VSX_GS_BOUND_ALNUM 1u                          // WORD / WORDS
#define VSX_GS_BOUND_SEMI  2u                          // WORD / WORDS with a field

VSX_GS_HD inline uint64_t vsx_gs_key(uint64_t poly, uint32_t len, uint64_t hash_mask)
{
  return vsxsym::mix64(poly ^ ((uint64_t) len * VSX_GS_LENGTH_MUL)) & hash_mask;
}
VSX_GS_HD inline uint64_t vsx_gs_pow(uint64_t b, uint64_t e)
{
  uint64_t r = 1;
  for (; e; e >>= 1, b *= b) if (e & 1) r *= b;
  return r;
}
VSX_GS_HD inline uint32_t vsx_gs_fold(uint32_t c, uint32_t fold) { return (fold && c - 'a' < 26u) ? c - 32u : c; }
VSX_GS_HD inline bool vsx_gs_alnum(uint32_t c) { return (c - '0' < 10u) || (c - 'A' < 26u) || (c - 'a' < 26u); }

struct VsxGetseqsSlot {
  uint64_t key;
  uint32_t id1;            // needle number + 1; 0: empty
  uint32_t len;
};

// the needles and their table
struct VsxGetseqsTable {
  uint32_t         n;            // needles
  const uint8_t *  blob;         // (field '=' label in the field modes: composed by the host)
  const uint64_t * off;
  const uint32_t * len;
  VsxGetseqsSlot * slots;        // zeroed by the call
  uint32_t         slot_mask;    // slots - 1; slots is a power of two, >= 64 and >= 2 n
  uint32_t         fold;
  uint64_t         hash_mask;
};

// one match launch: headers [first, first + count)
struct VsxGetseqsMatch {
  uint32_t         first, count;
  const uint8_t *  blob;
  const uint64_t * off;
  const uint32_t * len;
  VsxGetseqsTable  T;
  const uint32_t * lengths;      // the distinct needle lengths, ascending
  uint32_t         n_lengths;
  uint32_t         bound;        // VSX_GS_BOUND_*
  uint32_t         exact;        // the whole header against the table (LABEL / LABELS without substr)
  uint32_t         empty_needle; // LABEL + substr with the empty needle: every non-empty header
  uint32_t         lds_entries;  // prefix sums per wavefront: the longest header + 1 (occurrence modes)
  uint64_t         base_inv;     // B^-1
  uint32_t *       verdict;      // per header, 0 / 1
  unsigned long long * counters; // [0] probes, [1] verifications
};

#ifdef __cplusplus
extern "C" {
#endif
// one wavefront per needle: hash, then insert by compare-and-swap
hipError_t vsx_launch_getseqs_insert(VsxGetseqsTable T, hipStream_t st);
// one wavefront per header
hipError_t vsx_launch_getseqs_match(VsxGetseqsMatch M, hipStream_t st);
// inclusive sum of the verdicts; temp NULL: the temporary bytes only
hipError_t vsx_launch_getseqs_scan(void * temp, size_t * temp_bytes, const uint32_t * d_verdict, uint32_t * d_incl, uint32_t n, hipStream_t st);
// the 16-byte records: matched, ordinal, start, length
hipError_t vsx_launch_getseqs_records(uint32_t n, const uint32_t * d_verdict, const uint32_t * d_incl, const uint32_t * d_seqlen, int64_t subseq_start,
                                      int64_t subseq_end, uint32_t * d_rec, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
