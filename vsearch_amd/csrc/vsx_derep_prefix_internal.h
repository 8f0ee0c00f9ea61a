// vsx_derep_prefix_internal.h -- shared between the prefix-dereplication kernels (vsx_derep_prefix.hip) and their host side
// (vsx_derep_prefix.cpp).  On the device a read is named by its rank: its position in the command's sorted order.
#ifndef VSX_DEREP_PREFIX_INTERNAL_H
#define VSX_DEREP_PREFIX_INTERNAL_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#include "vsx_derep_internal.h"

#define VSX_DEREP_PREFIX_NONE 0xFFFFFFFFu    // a node nobody holds

// counters of the claim launch (device, 64-bit)
struct VsxDerepPrefixCounters {
  unsigned long long probes, candidates_compared;
};

// what the claim kernel reads (all of it written by earlier launches) and the one array it updates, with atomicMin only
struct VsxDerepPrefixClaim {
  uint32_t         n;            // reads, in rank order
  uint32_t         n_lengths;    // distinct lengths
  const uint32_t * len;          // n, ascending
  const uint32_t * length_index; // n: how many distinct lengths lie below the read's own
  const uint32_t * lengths;      // n_lengths, ascending: the lengths that occur
  const uint64_t * woff;         // n: where a read's code words, and its prefix sums, begin
  const uint64_t * words;
  const uint64_t * sums;         // beside words: sums[woff + c] = the mixed full words 0 .. c - 1 added up
  const uint64_t * hash;         // n: the prefix hash at the read's own length, cut to hash_mask
  const uint32_t * node;         // n: the head (lowest rank) of the read's node
  const uint32_t * table;        // the grouping launch's table: an owner per distinct sequence, VSX_DEREP_EMPTY elsewhere
  uint64_t         table_size;
  uint64_t         hash_mask;
  uint32_t *       holder;       // n, VSX_DEREP_PREFIX_NONE: per head, the lowest rank of a node that properly extends it
  VsxDerepPrefixCounters * counters;
};

#ifdef __cplusplus
extern "C" {
#endif
// per read: the exclusive prefix sums of its position-tagged mixed full words, and the prefix hash at its own length.
// The words are those vsx_launch_exact_hash wrote in an earlier launch.
hipError_t vsx_launch_derep_prefix_scan(uint32_t n, const uint32_t * d_len, const uint64_t * d_woff, const uint64_t * d_words,
                                        uint64_t hash_mask, uint64_t * d_sums, uint64_t * d_hash, hipStream_t st);
// d_node[r] = d_rep[d_root[r]]: the head of the read's node (root, rep: the grouping and account launches of vsx_derep.hip)
hipError_t vsx_launch_derep_prefix_nodes(uint32_t n, const uint32_t * d_root, const uint32_t * d_rep, uint32_t * d_node, hipStream_t st);
// one wavefront per head: atomicMin(holder[P], rank) for every node P that is a proper prefix of the head's sequence
hipError_t vsx_launch_derep_prefix_claim(VsxDerepPrefixClaim P, hipStream_t st);
// d_next[r] = the read's node when it is no head, its holder when it has one, itself otherwise
hipError_t vsx_launch_derep_prefix_link(uint32_t n, const uint32_t * d_node, const uint32_t * d_holder, uint32_t * d_next, hipStream_t st);
// one round of pointer jumping: d_out[r] = d_in[d_in[r]]
hipError_t vsx_launch_derep_prefix_jump(uint32_t n, const uint32_t * d_in, uint32_t * d_out, hipStream_t st);
#ifdef __cplusplus
}
#endif

#endif
