// vsx_derep_internal.h -- shared between the dereplication kernels (vsx_derep.hip) and their host side (vsx_derep.cpp).
#ifndef VSX_DEREP_INTERNAL_H
#define VSX_DEREP_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#include "vsx_exact_internal.h"

#define VSX_DEREP_EMPTY      0xFFFFFFFFu     // a free table slot, and a cluster without a representative yet
#define VSX_DEREP_THRESHOLDS 129             // T[0 .. 128]
#define VSX_DEREP_QBLOCK     64              // quality positions one wavefront merges

// the per-read arrays of the kept reads (device), written before the grouping launch and only read by it
struct VsxDerepReads {
  uint32_t         n;
  const uint32_t * len;
  const uint64_t * hash_plus;    // of the plus strand's words (vsx_launch_exact_hash)
  const uint64_t * hash_minus;   // of the reverse complement's; NULL: plus strand only
  const uint64_t * woff_plus;    // where the strands' code words begin
  const uint64_t * woff_minus;
  const uint32_t * label;        // interned label ids; NULL: labels are not part of the key
  const uint64_t * words;
};

// counters of the grouping launch (device, 64-bit)
struct VsxDerepCounters {
  unsigned long long slots_visited, candidates_compared;
};

// one task of the quality merge: a block of 64 positions of one cluster with at least two members
struct VsxDerepQTask {
  uint64_t first;       // of the cluster's members in the sorted member list
  uint64_t out;         // of the cluster's merged string in the output blob
  uint32_t members;
  uint32_t len;
  uint32_t block;       // positions 64 * block ...
  uint32_t pad;
};

struct VsxDerepQParams {
  const double *   prob;        // 128: error probability by quality symbol
  const uint64_t * threshold;   // VSX_DEREP_THRESHOLDS bit patterns, descending
  int32_t qout_max, asciiout, qminout, qmaxout;
};

#ifdef __cplusplus
extern "C" {
#endif
// per read: the smaller of (hash, words) over its strands becomes the key (equal words: a palindrome, plus); the label id is mixed
// into the key's hash (cut to hash_mask again); flag = 1: the key is the minus strand
hipError_t vsx_launch_derep_key(VsxDerepReads R, uint64_t hash_mask, uint64_t * d_khash, uint64_t * d_kwoff, uint8_t * d_flag, hipStream_t st);
// find-or-insert: d_root[read] = the read owning the slot of its key (itself when it claimed one).  d_table: table_size slots of
// VSX_DEREP_EMPTY.
hipError_t vsx_launch_derep_group(VsxDerepReads R, const uint64_t * d_khash, const uint64_t * d_kwoff, uint32_t * d_table, uint64_t table_size,
                                  uint32_t * d_root, VsxDerepCounters * d_counters, hipStream_t st);
// per cluster (indexed by its root): lowest member, abundance sum, member count.  d_rep: VSX_DEREP_EMPTY, d_size / d_count: zero.
hipError_t vsx_launch_derep_account(uint32_t n, const uint32_t * d_root, const uint64_t * d_abundance, uint32_t * d_rep, uint64_t * d_size,
                                    uint32_t * d_count, hipStream_t st);
// the member list: keys (representative << 32 | read) sorted ascending in d_keys_out.  temp == NULL: only *temp_bytes is set.
hipError_t vsx_launch_derep_members(uint32_t n, const uint32_t * d_root, const uint32_t * d_rep, uint64_t * d_keys_in, uint64_t * d_keys_out,
                                    void * temp, size_t * temp_bytes, hipStream_t st);
// the merged quality strings of the tasks' clusters.  d_qoff[read]: where the read's quality string begins in d_qual.
hipError_t vsx_launch_derep_quality(const VsxDerepQTask * d_tasks, uint32_t n_tasks, const uint64_t * d_members, const uint8_t * d_qual,
                                    const uint64_t * d_qoff, const uint64_t * d_abundance, VsxDerepQParams P, uint8_t * d_out, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
