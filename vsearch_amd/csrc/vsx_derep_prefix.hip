// vsx_derep_prefix.hip -- prefix dereplication on gfx950 (--derep_prefix): what is new on top of the exact-search and
// full-length dereplication kernels.  The code words come from vsx_exact.hip's hash kernel, equal reads are grouped by
// vsx_derep.hip's find-or-insert kernel and its account kernel finds every node's head; both unchanged.  Reads are staged in the
// command's sorted order, so a read's number IS its rank.
//
//   scan      one wavefront per read.  A hash that can be evaluated at every prefix length: with w_c the read's code words (16
//             codes each), m(c) = mix64(w_c ^ (c + 1) G) and j = floor(l / 16),
//                 H(l) = mix64((m(0) + ... + m(j - 1) + mix64(partial ^ (j + 1) G ^ T)) ^ l C)
//             where partial is word j cut to its first l mod 16 codes (zero when there are none).  The wave scans m over the
//             read's full words and stores the exclusive sums beside the words; H at the read's own length is the key under which
//             the grouping kernel files it.  A prefix of length l of ANY read then costs one sum, one word and two mixes.
//   claim     one wavefront per node (the waves of reads that are not their node's head leave at once).  The lanes take the
//             candidate prefix lengths: the lengths that occur in the input and lie below the node's own, from the host's
//             ascending list of them.  A lane evaluates H(l), walks the grouping launch's table from that slot until a free one,
//             and where hash and length agree compares floor(l / 16) full words and the masked last word; on equality it does
//             atomicMin(holder[head of that node], own rank) and stops (a sequence is filed once).  The table, the per-read
//             arrays and the words were all written by earlier launches; within this launch nothing is read that this launch
//             writes -- holder is touched by atomicMin only and read by the next launch.  Whatever the order of the waves, holder[P]
//             ends as the lowest rank among P's proper extensions.
//   link,     next[r] = r's node (a duplicate), else its holder, else itself; ceil(log2(distinct lengths + 1)) rounds of
//   jump      next = next[next] between two buffers (a round reads one and writes the other) leave every read at its chain's top.
//
// Sizes, counts and the member sort are vsx_derep.hip's account and members launches with the tops as roots.
// Integer code only; no kernel waits for another workgroup.
#include <hip/hip_runtime.h>
#include "vsx_derep_prefix_internal.h"
#include "vsx_devutil.h"
#include "vsx_symbols.h"

namespace {

typedef unsigned long long u64;
using vsxd::shfl64;
using vsxd::shfl_up64;
using vsxd::shfl_xor64;
using vsxsym::kGolden;
using vsxsym::kLengthMul;
using vsxsym::mix64;

#define PREFIX_WAVES   4
#define PREFIX_THREADS (64 * PREFIX_WAVES)

constexpr u64 kPartialTag = 0xD6E8FEB86659FD93ull;

// H(l) from the sum of the mixed full words below word j = l / 16 and word j cut to l mod 16 codes
__device__ inline u64 prefix_hash(u64 sum, u64 partial, uint32_t j, uint32_t l, u64 hash_mask)
{
  return mix64((sum + mix64(partial ^ ((u64) (j + 1) * kGolden) ^ kPartialTag)) ^ ((u64) l * kLengthMul)) & hash_mask;
}

__global__ __launch_bounds__(PREFIX_THREADS)
void vsx_derep_prefix_scan_kernel(uint32_t n, const uint32_t * __restrict__ len, const u64 * __restrict__ woff, const u64 * __restrict__ words,
                                  u64 hash_mask, u64 * __restrict__ sums, u64 * __restrict__ hash)
{
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * PREFIX_WAVES + (threadIdx.x >> 6));
  if (r >= n) return;
  const int lane = threadIdx.x & 63;
  const uint32_t L = len[r], nfull = L / VSX_EXACT_CHUNK, rem = L % VSX_EXACT_CHUNK, nwords = nfull + (rem ? 1u : 0u);
  const u64 * const w = words + woff[r];
  u64 * const s = sums + woff[r];
  u64 carry = 0;
  for (uint32_t base = 0; base < nwords; base += 64)
    {
      const uint32_t c = base + (uint32_t) lane;
      const u64 v = c < nfull ? mix64(w[c] ^ ((u64) (c + 1) * kGolden)) : 0ull;      // the partial word is no part of the sums
      u64 incl = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1)
        {
          const u64 t = shfl_up64(incl, d);
          if (lane >= d) incl += t;
        }
      if (c < nwords) s[c] = carry + incl - v;
      carry += shfl64(incl, 63);
    }
  if (lane == 0) hash[r] = prefix_hash(carry, rem ? w[nfull] : 0ull, nfull, L, hash_mask);       // the hash kernel zeroed the unused codes
}

__global__ __launch_bounds__(256)
void vsx_derep_prefix_nodes_kernel(uint32_t n, const uint32_t * __restrict__ root, const uint32_t * __restrict__ rep, uint32_t * __restrict__ node)
{
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  node[r] = rep[root[r]];
}

__global__ __launch_bounds__(PREFIX_THREADS)
void vsx_derep_prefix_claim_kernel(VsxDerepPrefixClaim P)
{
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * PREFIX_WAVES + (threadIdx.x >> 6));
  if (r >= P.n) return;
  if (P.node[r] != r) return;                                 // a duplicate: its node's head claims
  const int lane = threadIdx.x & 63;
  const uint32_t ncand = P.length_index[r];                   // the lengths below the read's own
  const u64 * const w = reinterpret_cast<const u64 *>(P.words) + P.woff[r];
  const u64 * const s = reinterpret_cast<const u64 *>(P.sums) + P.woff[r];
  const u64 mask = P.table_size - 1;
  u64 probes = 0, compared = 0;
  for (uint32_t i = (uint32_t) lane; i < ncand; i += 64)
    {
      const uint32_t l = P.lengths[i], j = l / VSX_EXACT_CHUNK, rem = l % VSX_EXACT_CHUNK;       // l < len[r]: word j is the read's own
      const u64 partial = rem ? w[j] & ~(~0ull << (4 * rem)) : 0ull;
      const u64 h = prefix_hash(s[j], partial, j, l, P.hash_mask);
      u64 slot = h & mask;
      // at most 2/3 of the slots are taken: a free one comes up
      for (u64 step = 0; step < P.table_size; ++step, slot = (slot + 1) & mask)
        {
          const uint32_t o = P.table[slot];
          ++probes;
          if (o == VSX_DEREP_EMPTY) break;
          if (P.hash[o] != h || P.len[o] != l) continue;
          const u64 * const t = reinterpret_cast<const u64 *>(P.words) + P.woff[o];
          bool differ = false;
          for (uint32_t c = 0; c < j; ++c) differ |= w[c] != t[c];
          if (rem) differ |= partial != t[j];
          ++compared;
          if (differ) continue;
          atomicMin(&P.holder[P.node[o]], r);
          break;                                              // equal sequences share one owner: there is no second
        }
    }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { probes += shfl_xor64(probes, m); compared += shfl_xor64(compared, m); }
  if (lane == 0)
    {
      if (probes) atomicAdd(&P.counters->probes, probes);
      if (compared) atomicAdd(&P.counters->candidates_compared, compared);
    }
}

__global__ __launch_bounds__(256)
void vsx_derep_prefix_link_kernel(uint32_t n, const uint32_t * __restrict__ node, const uint32_t * __restrict__ holder, uint32_t * __restrict__ next)
{
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const uint32_t head = node[r], held = holder[r];
  next[r] = head != r ? head : (held != VSX_DEREP_PREFIX_NONE ? held : r);
}

__global__ __launch_bounds__(256)
void vsx_derep_prefix_jump_kernel(uint32_t n, const uint32_t * __restrict__ in, uint32_t * __restrict__ out)
{
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const uint32_t a = in[r];
  out[r] = a < n ? in[a] : a;                                 // (a link beyond the reads is left for the host to refuse)
}

}  // namespace

extern "C" hipError_t vsx_launch_derep_prefix_scan(uint32_t n, const uint32_t * d_len, const uint64_t * d_woff, const uint64_t * d_words,
                                                   uint64_t hash_mask, uint64_t * d_sums, uint64_t * d_hash, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_prefix_scan_kernel, dim3((n + PREFIX_WAVES - 1) / PREFIX_WAVES), dim3(PREFIX_THREADS), 0, st, n, d_len,
                     reinterpret_cast<const u64 *>(d_woff), reinterpret_cast<const u64 *>(d_words), (u64) hash_mask,
                     reinterpret_cast<u64 *>(d_sums), reinterpret_cast<u64 *>(d_hash));
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_prefix_nodes(uint32_t n, const uint32_t * d_root, const uint32_t * d_rep, uint32_t * d_node, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_prefix_nodes_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_root, d_rep, d_node);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_prefix_claim(VsxDerepPrefixClaim P, hipStream_t st)
{
  if (P.n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_prefix_claim_kernel, dim3((P.n + PREFIX_WAVES - 1) / PREFIX_WAVES), dim3(PREFIX_THREADS), 0, st, P);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_prefix_link(uint32_t n, const uint32_t * d_node, const uint32_t * d_holder, uint32_t * d_next, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_prefix_link_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_node, d_holder, d_next);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_prefix_jump(uint32_t n, const uint32_t * d_in, uint32_t * d_out, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_prefix_jump_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_in, d_out);
  return hipGetLastError();
}
