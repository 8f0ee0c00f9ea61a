// vsx_rank.hip -- hit compaction on the device: of all pairs of a plan only those the accept filter kept
// leave the GPU.
//
// Reference: hits are kept if accepted (or weak) and ordered per query by identity descending, then target ascending
// (hit_compare_byid_typed, src/core/searchcore.cpp:133-179; allpairs_hit_compare_typed, src/commands/allpairs_global.cpp:
// 116-138; search_joinhits :1028-1052 and the qsort at allpairs_global.cpp:522).  The pair list of a plan is grouped by
// query with ascending targets inside a query, so "target ascending" is "pair order".  The identity is the double the
// accept filter compares (vsx_accept.h), so ties are exactly the reference's ties.
//
// The traceback's epilogue lists the kept pairs with their identities (vsx_device.hip rank_note); the kernel below gathers
// their statistics / verdict / id / text offset into compact arrays that cross PCIe, and the host puts the few entries in
// report order (vsx_fetch.cpp fetch_ranked_lists).
#include <hip/hip_runtime.h>
#include "vsx_internal.h"

typedef unsigned int u32;

__global__ void __launch_bounds__(256)
vsx_rank_gather_kernel(const u32 * __restrict__ ranked, const double * __restrict__ key, u32 kept, const VsxPairOut * __restrict__ out,
                       const uint64_t * __restrict__ text_off, VsxRankedOut r)
{
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= kept) return;
  const u32 pid = ranked[j];
  const VsxPairOut o = out[pid];
  r.pair[j] = pid;
  r.score[j] = o.score; r.aligned[j] = o.aligned; r.matches[j] = o.matches; r.mismatches[j] = o.mismatches; r.gaps[j] = o.gaps;
  r.verdict[j] = (uint8_t) o.pad;
  r.id[j] = key[j];
  r.text_off[j] = text_off[pid];
}

// r06: the kept pairs of a ranked plan as the traceback's epilogue listed them (arrival order; VsxFilterDev::kept_pair / kept_id) ->
// the compact arrays; the host orders the few entries (fetch_ranked_lists, vsx_fetch.cpp)
extern "C" hipError_t vsx_rank_gather_list(const uint32_t * d_kept_pair, const double * d_kept_id, uint32_t kept, const VsxPairOut * d_out,
                                           const uint64_t * d_text_off, VsxRankedOut r, hipStream_t st)
{
  if (kept)
    hipLaunchKernelGGL(vsx_rank_gather_kernel, dim3((kept + 255) / 256), dim3(256), 0, st, d_kept_pair, d_kept_id, kept, d_out, d_text_off, r);
  return hipGetLastError();
}
