// vsx_derep.hip -- full-length dereplication on gfx950 (--derep_fulllength, --fastx_uniques, --derep_id): what is new on top of
// the exact-search kernels.  The code words and hashes of both strands come from vsx_exact.hip's hash kernel, unchanged.
//
//   key       one thread per read.  With both strands the key is the smaller of (hash, words) over the read's two strands, so S and
//             rc(S) get the same key whichever comes first; equal words mean a reverse palindrome, which stays plus.  The words are
//             compared only where the hashes agree.  The label id (--derep_id) is mixed into the key's hash.
//   group     one wavefront per read: find-or-insert in an open-addressing table whose slots hold nothing but a 32-bit read number,
//             claimed with compare-and-swap.  A read that meets an owner compares hash, length, label and code words with it and
//             joins or probes on.  Within this launch NOTHING is read through the table but the value the atomic itself returns:
//             the owner's hash, length and words lie in the per-read arrays an earlier launch wrote.  So no fence between XCDs is
//             needed, and none is used.  Which member owns a slot varies from run to run; only the partition leaves this kernel.
//   account   one thread per read, integer atomics only: per cluster the lowest member (the representative), the 64-bit abundance
//             sum and the member count.  Deterministic whatever the order.
//   members   keys (representative << 32 | read), sorted by rocPRIM: the member list ordered by (cluster, input index).
//   quality   one wavefront per (cluster of two or more members, block of 64 positions), one lane per position, the members in
//             input order.  The chain q -> p -> q is serial in the members; the members' symbols do not depend on it and are
//             loaded eight members ahead.  p(symbol) is a host-built table; min, *, +, / on doubles are exact on both sides (no FP
//             contraction); the device's log10 is never called: trunc(-10 log10 p) is found by comparing p's bit pattern with the
//             host-built thresholds T[v] = largest p with trunc(-10 log10 p) >= v.
//
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "vsx_derep_internal.h"
#include "vsx_symbols.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
using vsxsym::mix64;

#define DEREP_WAVES   4
#define DEREP_THREADS (64 * DEREP_WAVES)
#define DEREP_AHEAD   8                      // members whose symbols the quality kernel loads ahead of the chain

__device__ inline uint32_t words_in(uint32_t len) { return (len + VSX_EXACT_CHUNK - 1) / VSX_EXACT_CHUNK; }

__global__ __launch_bounds__(256)
void vsx_derep_key_kernel(VsxDerepReads R, u64 hash_mask, u64 * __restrict__ khash, u64 * __restrict__ kwoff, uint8_t * __restrict__ flag)
{
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= R.n) return;
  u64 h = R.hash_plus[k], w = R.woff_plus[k];
  uint32_t minus = 0;
  if (R.hash_minus)
    {
      const u64 hm = R.hash_minus[k], wm = R.woff_minus[k];
      if (hm < h) minus = 1;
      else if (hm == h)
        {
          // the first word that differs decides, as unsigned numbers; no difference: a palindrome, plus
          const u64 * const a = reinterpret_cast<const u64 *>(R.words) + w;
          const u64 * const b = reinterpret_cast<const u64 *>(R.words) + wm;
          const uint32_t nw = words_in(R.len[k]);
          for (uint32_t i = 0; i < nw; ++i)
            {
              const u64 x = a[i], y = b[i];
              if (x != y) { minus = y < x; break; }
            }
        }
      if (minus) { h = hm; w = wm; }
    }
  if (R.label) h = mix64(h ^ ((u64) (R.label[k] + 1u) * vsxsym::kGolden)) & hash_mask;
  khash[k] = h; kwoff[k] = w; flag[k] = (uint8_t) minus;
}

__global__ __launch_bounds__(DEREP_THREADS)
void vsx_derep_group_kernel(VsxDerepReads R, const u64 * __restrict__ khash, const u64 * __restrict__ kwoff, uint32_t * table, u64 table_size,
                            uint32_t * __restrict__ root, VsxDerepCounters * counters)
{
  const uint32_t read = __builtin_amdgcn_readfirstlane(blockIdx.x * DEREP_WAVES + (threadIdx.x >> 6));
  if (read >= R.n) return;
  const int lane = threadIdx.x & 63;
  const u64 h = khash[read], mask = table_size - 1;
  const uint32_t len = R.len[read], lab = R.label ? R.label[read] : 0u;
  const uint32_t npairs = (words_in(len) + 1) / 2;
  const uint4 * const q4 = reinterpret_cast<const uint4 *>(reinterpret_cast<const u64 *>(R.words) + kwoff[read]);
  u64 visited = 0, compared = 0;
  uint32_t mine = read;
  u64 j = h & mask;
  // at most 2/3 of the slots are ever taken: a free one comes up
  for (u64 step = 0; step < table_size; ++step, j = (j + 1) & mask)
    {
      uint32_t old = 0;
      if (lane == 0) old = atomicCAS(&table[j], VSX_DEREP_EMPTY, read);
      old = (uint32_t) __shfl((int) old, 0);
      ++visited;
      if (old == VSX_DEREP_EMPTY) break;                      // claimed: this read founds a cluster
      // the owner's key: arrays of an earlier launch, never anything stored in this one
      if (khash[old] != h || R.len[old] != len || (R.label && R.label[old] != lab)) continue;
      const uint4 * const t4 = reinterpret_cast<const uint4 *>(reinterpret_cast<const u64 *>(R.words) + kwoff[old]);
      bool differ = false;
      for (uint32_t p = lane; p < npairs; p += 64)
        {
          const uint4 a = q4[p], b = t4[p];
          differ |= (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w);
        }
      ++compared;
      if (__ballot(differ) == 0) { mine = old; break; }
    }
  if (lane == 0)
    {
      root[read] = mine;
      atomicAdd(&counters->slots_visited, visited);
      if (compared) atomicAdd(&counters->candidates_compared, compared);
    }
}

__global__ __launch_bounds__(256)
void vsx_derep_account_kernel(uint32_t n, const uint32_t * __restrict__ root, const u64 * __restrict__ abundance, uint32_t * rep, u64 * size,
                              uint32_t * count)
{
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t c = root[k];
  atomicMin(&rep[c], k);
  atomicAdd(&size[c], abundance ? abundance[k] : 1ull);
  atomicAdd(&count[c], 1u);
}

__global__ __launch_bounds__(256)
void vsx_derep_member_keys_kernel(uint32_t n, const uint32_t * __restrict__ root, const uint32_t * __restrict__ rep, u64 * __restrict__ keys)
{
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  keys[k] = ((u64) rep[root[k]] << 32) | k;
}

// trunc(-10 log10 p) limited to 0 .. 128: the largest v with p <= T[v].  T descends, T[0] > 1 >= p, and positive doubles order as
// their bit patterns do.
__device__ inline int quality_of(u64 pbits, const u64 * __restrict__ T)
{
  int lo = 0, hi = VSX_DEREP_THRESHOLDS - 1;
  while (lo < hi)
    {
      const int mid = (lo + hi + 1) >> 1;
      if (pbits <= T[mid]) lo = mid; else hi = mid - 1;
    }
  return lo;
}

__global__ __launch_bounds__(DEREP_THREADS)
void vsx_derep_quality_kernel(const VsxDerepQTask * __restrict__ tasks, uint32_t n_tasks, const u64 * __restrict__ members,
                              const uint8_t * __restrict__ qual, const u64 * __restrict__ qoff, const u64 * __restrict__ abundance,
                              VsxDerepQParams P, uint8_t * __restrict__ out)
{
  const uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * DEREP_WAVES + (threadIdx.x >> 6));
  if (t >= n_tasks) return;
  const VsxDerepQTask T = tasks[t];
  const uint32_t pos = T.block * VSX_DEREP_QBLOCK + (threadIdx.x & 63);
  if (pos >= T.len) return;
  const u64 * const m = members + T.first;
  const uint32_t first = (uint32_t) m[0];
  uint32_t q = qual[qoff[first] + pos];
  u64 s1 = abundance ? abundance[first] : 1ull;
  for (uint32_t i0 = 1; i0 < T.members; i0 += DEREP_AHEAD)
    {
      uint32_t sym[DEREP_AHEAD];
      u64 ab[DEREP_AHEAD];
#pragma unroll
      for (int a = 0; a < DEREP_AHEAD; ++a)
        {
          sym[a] = 0; ab[a] = 1;
          if (i0 + a < T.members)
            {
              const uint32_t r = (uint32_t) m[i0 + a];
              sym[a] = qual[qoff[r] + pos];
              if (abundance) ab[a] = abundance[r];
            }
        }
#pragma unroll
      for (int a = 0; a < DEREP_AHEAD; ++a)
        if (i0 + a < T.members)
          {
            const double p1 = P.prob[q & 127u], p2 = P.prob[sym[a] & 127u];
            const u64 s2 = ab[a], s3 = s1 + s2;
            double p3;
            if (P.qout_max) p3 = p1 < p2 ? p1 : p2;
            else p3 = (p1 * (double) s1 + p2 * (double) s2) / (double) s3;
            int v = quality_of((u64) __double_as_longlong(p3), reinterpret_cast<const u64 *>(P.threshold));
            v = v < P.qmaxout ? v : P.qmaxout;
            v = v > P.qminout ? v : P.qminout;
            q = (uint32_t) (v + P.asciiout);
            s1 = s3;
          }
    }
  out[T.out + pos] = (uint8_t) q;
}

}  // namespace

extern "C" hipError_t vsx_launch_derep_key(VsxDerepReads R, uint64_t hash_mask, uint64_t * d_khash, uint64_t * d_kwoff, uint8_t * d_flag, hipStream_t st)
{
  if (R.n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_key_kernel, dim3((R.n + 255u) / 256u), dim3(256), 0, st, R, (u64) hash_mask, reinterpret_cast<u64 *>(d_khash),
                     reinterpret_cast<u64 *>(d_kwoff), d_flag);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_group(VsxDerepReads R, const uint64_t * d_khash, const uint64_t * d_kwoff, uint32_t * d_table,
                                             uint64_t table_size, uint32_t * d_root, VsxDerepCounters * d_counters, hipStream_t st)
{
  if (R.n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_group_kernel, dim3((R.n + DEREP_WAVES - 1) / DEREP_WAVES), dim3(DEREP_THREADS), 0, st, R,
                     reinterpret_cast<const u64 *>(d_khash), reinterpret_cast<const u64 *>(d_kwoff), d_table, (u64) table_size, d_root, d_counters);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_account(uint32_t n, const uint32_t * d_root, const uint64_t * d_abundance, uint32_t * d_rep, uint64_t * d_size,
                                               uint32_t * d_count, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_account_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_root, reinterpret_cast<const u64 *>(d_abundance), d_rep,
                     reinterpret_cast<u64 *>(d_size), d_count);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_derep_members(uint32_t n, const uint32_t * d_root, const uint32_t * d_rep, uint64_t * d_keys_in, uint64_t * d_keys_out,
                                               void * temp, size_t * temp_bytes, hipStream_t st)
{
  if (!temp) return rocprim::radix_sort_keys(nullptr, *temp_bytes, (u64 *) d_keys_in, (u64 *) d_keys_out, (size_t) n, 0, 64, st);
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_member_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_root, d_rep, reinterpret_cast<u64 *>(d_keys_in));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return rocprim::radix_sort_keys(temp, *temp_bytes, (u64 *) d_keys_in, (u64 *) d_keys_out, (size_t) n, 0, 64, st);
}

extern "C" hipError_t vsx_launch_derep_quality(const VsxDerepQTask * d_tasks, uint32_t n_tasks, const uint64_t * d_members, const uint8_t * d_qual,
                                               const uint64_t * d_qoff, const uint64_t * d_abundance, VsxDerepQParams P, uint8_t * d_out, hipStream_t st)
{
  if (n_tasks == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_derep_quality_kernel, dim3((n_tasks + DEREP_WAVES - 1) / DEREP_WAVES), dim3(DEREP_THREADS), 0, st, d_tasks, n_tasks,
                     reinterpret_cast<const u64 *>(d_members), d_qual, reinterpret_cast<const u64 *>(d_qoff),
                     reinterpret_cast<const u64 *>(d_abundance), P, d_out);
  return hipGetLastError();
}
