// vsx_lca_internal.h -- what vsx_lca.cpp and vsx_lca.hip share: the launchers of the index build (split, number, verify) and of the
// vote.  Entry e = 9 * label + level stands for the names of levels 0 .. level of that label.
#ifndef VSX_LCA_INTERNAL_H
#define VSX_LCA_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/vsx_lca.h"

#define LCA_LEVELS VSX_LCA_LEVELS

// what the vote kernel writes per query
struct VsxLcaVote {
  uint32_t n_top;
  uint32_t matches[LCA_LEVELS];
  uint32_t first[LCA_LEVELS];      // the lowest top hit (counted from the query's first hit) that matches, VSX_LCA_NONE without one
};

#ifdef __cplusplus
extern "C" {
#endif

// one wavefront per label: start[9 n], len[9 n] (int32, 0 for a rank the label does not name) and the chained prefix hashes
// key[9 n] (AND hash_mask); idx[e] = e
hipError_t vsx_launch_lca_split(uint32_t n, const uint8_t * d_blob, const uint64_t * d_off, const uint32_t * d_len, uint64_t hash_mask,
                                int32_t * d_start, int32_t * d_name_len, uint64_t * d_key, uint32_t * d_idx, hipStream_t st);
// rocPRIM (temp == NULL: the size of the temporary storage): the stable sort of (key, idx), the inclusive maximum
hipError_t vsx_launch_lca_sort(void * temp, size_t * temp_bytes, const uint64_t * d_kin, uint64_t * d_kout, const uint32_t * d_vin, uint32_t * d_vout,
                               uint32_t count, uint32_t end_bit, hipStream_t st);
hipError_t vsx_launch_lca_scan_max(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint32_t count, hipStream_t st);
// mark[i] = i where a run of equal keys begins in the sorted list, else 0
hipError_t vsx_launch_lca_heads(uint32_t count, const uint64_t * d_sorted_key, uint32_t * d_mark, hipStream_t st);
// (head = the inclusive maximum of the marks)  id[idx[i]] = head[i]: the number of the run.  Every entry's names of levels 0 .. k
// are compared, length and bytes, with those of its run's first entry; a difference stores 1 to *d_differ (zeroed by the caller)
hipError_t vsx_launch_lca_verify(uint32_t count, const uint32_t * d_sorted_idx, const uint32_t * d_head, const uint8_t * d_blob, const uint64_t * d_off,
                                 const int32_t * d_start, const int32_t * d_name_len, uint32_t * d_id, uint32_t * d_differ, hipStream_t st);
// one wavefront per query of the window [q0, q0 + nq): first (the whole call's, first[q] - hit0 indexes d_target / d_hit_id),
// d_hit_id NULL without top_hits_only
hipError_t vsx_launch_lca_vote(uint32_t nq, const uint64_t * d_first, uint64_t hit0, const uint32_t * d_target, const double * d_hit_id,
                               const uint32_t * d_id, uint64_t maxhits, VsxLcaVote * d_vote, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif
