// vsx_otutab.hip -- the OTU table on gfx950 (--otutabout, --biomout, --mothur_shared_out; include/vsx_otutab.h).
//
//   scan      one wavefront per label, 64 bytes per step, lane = byte.  The wave keeps the step's bytes and the NEXT step's, so the
//             mask of a keyword's k-th letter is (ballot(cur == letter) >> k) | (ballot(next == letter) << (64 - k)) and a keyword
//             that begins in a step's last bytes is seen whole; a hit at p is the AND of these over the letters, with bit p - 1 of
//             the ';' mask (carried from the step before) or p == 0.  All of it is wave-uniform.  The leftmost hit opens a value,
//             which runs to the first ';' at or behind its start, in this step or a later one, else to the label's end.  The
//             fallback prefix ends at the first byte that does not belong to it (the positions behind the label count as such, so
//             a prefix that fills a step to its last byte simply goes on).  Then the name's bytes are hashed: every lane mixes
//             (position in the name, byte), the lanes' values are ADDED by a butterfly -- the sum does not depend on order --
//             and the name's length is mixed in.
//   heads     one wavefront per position of the list sorted by (hash, item number): the item starts a group unless the one before
//             it has the same hash, the same length and the same bytes.  A group is a set of EQUAL names; equal names may end in
//             several groups (a collision between them, or a cut hash), which the host's rank step merges.
//   groups,   group numbers from the flags' inclusive sum, a group's first item as its representative; ranks back onto the items.
//   assign
//   keys,     one lane per add: key = OTU rank << 32 | sample rank, sorted with the add's number as value; in sorted order the
//   gather    abundances are summed per key (the cells, in the writers' order) and the numbers of the adds whose target carries
//             tax= are maximised per OTU (the last such add wins).  What is no cell (abundance 0, the unmatched pass) takes the
//             sample half VSX_OTUTAB_NO: it still stands in its OTU's run for the maximum.
//
// rocPRIM does the sorts, the inclusive sum and the two reductions by key.  Integer code only; no atomics; no kernel waits for
// another workgroup; nothing is read that the same launch writes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include "vsx_otutab_internal.h"
#include "vsx_devutil.h"
#include "vsx_symbols.h"

namespace {

typedef unsigned long long u64;
using vsxd::shfl_xor64;
using vsxsym::kGolden;
using vsxsym::kLengthMul;
using vsxsym::mix64;

#define OTUTAB_WAVES   4
#define OTUTAB_THREADS (64 * OTUTAB_WAVES)

// bit p: the keyword stands at byte p of the step (it may run into the next step's bytes)
template <int N>
__device__ inline u64 keyword_mask(const char (&kw)[N], uint32_t cur, uint32_t next)
{
  u64 m = ~0ull;
#pragma unroll
  for (int k = 0; k < N - 1; ++k)
    {
      const uint32_t c = (uint32_t) (unsigned char) kw[k];
      u64 w = (u64) __ballot(cur == c) >> k;
      if (k) w |= (u64) __ballot(next == c) << (64 - k);
      m &= w;
    }
  return m;
}

// one annotation: looked for, then its value followed to its end
struct Finder {
  int state = 0;               // 0: looking for the keyword; 1: in the value; 2: done
  u64 vstart = 0, vend = 0;
  // hits: keyword starts allowed by what precedes them; klen_of: the keyword's length at a hit; semi: the step's ';'
  template <typename F>
  __device__ inline void step(u64 base, u64 hits, F klen_of, u64 semi)
  {
    if (state == 0 && hits)
      {
        const int p = __ffsll((long long) hits) - 1;
        vstart = base + (u64) p + (u64) klen_of(p);
        state = 1;
      }
    if (state == 1 && vstart < base + 64)
      {
        const u64 from = vstart > base ? vstart - base : 0;           // < 64
        const u64 m = semi & (~0ull << from);
        if (m) { vend = base + (u64) (__ffsll((long long) m) - 1); state = 2; }
      }
  }
  __device__ inline void finish(u64 L) { if (state == 1) { vend = L; state = 2; } }
};

__device__ inline bool word_byte(uint32_t c)
{
  return (c - 'A' < 26u) || (c - 'a' < 26u) || (c - '0' < 10u) || c == '_';
}

template <bool TARGET>
__global__ __launch_bounds__(OTUTAB_THREADS)
void vsx_otutab_scan_kernel(VsxOtutabScan P)
{
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * OTUTAB_WAVES + (threadIdx.x >> 6));
  if (i >= P.n) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t k = P.list ? P.list[i] : i;
  const u64 label_off = P.off[k], L = P.len[k];
  const uint8_t * const s = P.blob + label_off;
  Finder name, tax;                      // name: sample= / barcodelabel= (queries), otu= (targets)
  u64 fallback_end = L;
  bool fallback_open = true;
  u64 before = 1;                        // bit 0: the byte before this step is ';', or there is none
  uint32_t cur = lane < L ? s[lane] : 0u;
  for (u64 base = 0; base < L; base += 64)
    {
      const u64 np = base + 64 + lane;
      const uint32_t next = np < L ? s[np] : 0u;                      // what lies behind the label reads as 0: no keyword holds one
      const u64 valid = (u64) __ballot(base + lane < L);
      const u64 semi = (u64) __ballot(cur == (uint32_t) ';') & valid;
      const u64 start_ok = (semi << 1) | before;
      if (TARGET)
        {
          name.step(base, keyword_mask("otu=", cur, next) & start_ok, [](int) { return 4; }, semi);
          tax.step(base, keyword_mask("tax=", cur, next) & start_ok, [](int) { return 4; }, semi);
          if (fallback_open && (semi | ~valid)) { fallback_end = base + (u64) (__ffsll((long long) (semi | ~valid)) - 1); fallback_open = false; }
          if (name.state == 2 && tax.state == 2) break;
        }
      else
        {
          const u64 a = keyword_mask("sample=", cur, next), b = keyword_mask("barcodelabel=", cur, next);
          name.step(base, (a | b) & start_ok, [a](int p) { return ((a >> p) & 1) ? 7 : 13; }, semi);
          const u64 bad = ~((u64) __ballot(word_byte(cur)) & valid);
          if (fallback_open && bad) { fallback_end = base + (u64) (__ffsll((long long) bad) - 1); fallback_open = false; }
          if (name.state == 2) break;
        }
      before = semi >> 63;
      cur = next;
    }
  name.finish(L); tax.finish(L);
  const u64 ns = name.state == 2 ? name.vstart : 0, nl = name.state == 2 ? name.vend - name.vstart : fallback_end;
  // the name's hash: a sum over its bytes of mix64(position, byte)
  u64 acc = 0;
  for (u64 j = lane; j < nl; j += 64) acc += mix64((((j + 1) << 8) | (u64) s[ns + j]) + kGolden);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor64(acc, m);
  if (lane == 0)
    {
      P.name_off[i] = label_off + ns;
      P.name_len[i] = (uint32_t) nl;
      P.hash[i] = mix64(acc ^ (nl * kLengthMul)) & P.hash_mask;
      if (TARGET)
        {
          P.tax_off[k] = label_off + (tax.state == 2 ? tax.vstart : 0);
          P.tax_len[k] = tax.state == 2 ? (uint32_t) (tax.vend - tax.vstart) : VSX_OTUTAB_NO;
        }
    }
}

__global__ __launch_bounds__(256)
void vsx_otutab_iota_kernel(uint32_t n, uint32_t * __restrict__ idx)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) idx[i] = i;
}

__global__ __launch_bounds__(OTUTAB_THREADS)
void vsx_otutab_heads_kernel(uint32_t n, const u64 * __restrict__ sorted_hash, const uint32_t * __restrict__ idx, const uint8_t * __restrict__ blob,
                             const u64 * __restrict__ name_off, const uint32_t * __restrict__ name_len, uint32_t * __restrict__ flag)
{
  const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * OTUTAB_WAVES + (threadIdx.x >> 6));
  if (i >= n) return;
  const uint32_t lane = threadIdx.x & 63;
  bool same = false;
  if (i > 0 && sorted_hash[i] == sorted_hash[i - 1])
    {
      const uint32_t a = idx[i], b = idx[i - 1];
      const uint32_t la = name_len[a];
      if (la == name_len[b])
        {
          const uint8_t * const sa = blob + name_off[a], * const sb = blob + name_off[b];
          same = true;
          for (u64 base = 0; base < la && same; base += 64)
            {
              const u64 j = base + lane;
              const bool differ = j < la && sa[j] != sb[j];
              if (__ballot(differ)) same = false;
            }
        }
    }
  if (lane == 0) flag[i] = same ? 0u : 1u;
}

__global__ __launch_bounds__(256)
void vsx_otutab_groups_kernel(uint32_t n, const uint32_t * __restrict__ flag, const uint32_t * __restrict__ incl, const uint32_t * __restrict__ idx,
                              const u64 * __restrict__ name_off, const uint32_t * __restrict__ name_len, uint32_t * __restrict__ group,
                              uint32_t * __restrict__ rep_item, u64 * __restrict__ rep_off, uint32_t * __restrict__ rep_len)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t item = idx[i], g = incl[i] - 1u;                      // flag[0] is 1: incl >= 1
  group[item] = g;
  if (flag[i]) { rep_item[g] = item; rep_off[g] = name_off[item]; rep_len[g] = name_len[item]; }
}

__global__ __launch_bounds__(256)
void vsx_otutab_assign_kernel(uint32_t n, const uint32_t * __restrict__ group, const uint32_t * __restrict__ rank, const uint32_t * __restrict__ list,
                              uint32_t * __restrict__ item_rank, uint32_t * __restrict__ label_rank)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = rank[group[i]];
  item_rank[i] = r;
  if (list) label_rank[list[i]] = r;
}

__global__ __launch_bounds__(256)
void vsx_otutab_keys_kernel(VsxOtutabAdds A, u64 * __restrict__ keys, uint32_t * __restrict__ vals)
{
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= A.nq + A.nu) return;
  u64 key;
  if (e < A.nq)
    {
      const uint32_t t = A.q_target[e];
      if (t == VSX_OTUTAB_NO) key = ((u64) A.n_otus << 32) | VSX_OTUTAB_NO;
      else
        {
          const u64 ab = A.q_ab ? A.q_ab[e] : 1ull;
          key = ((u64) A.t_otu[t] << 32) | (ab ? A.q_sample[e] : VSX_OTUTAB_NO);
        }
    }
  else key = ((u64) A.t_otu[A.unmatched[e - A.nq]] << 32) | VSX_OTUTAB_NO;
  keys[e] = key;
  vals[e] = e;
}

__global__ __launch_bounds__(256)
void vsx_otutab_gather_kernel(VsxOtutabAdds A, const u64 * __restrict__ sorted_keys, const uint32_t * __restrict__ sorted_vals, u64 * __restrict__ count,
                              uint32_t * __restrict__ otu, uint32_t * __restrict__ taxseq)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.nq + A.nu) return;
  const uint32_t e = sorted_vals[i];
  uint32_t t;
  u64 ab = 0;
  if (e < A.nq)
    {
      t = A.q_target[e];
      if (t != VSX_OTUTAB_NO) ab = A.q_ab ? A.q_ab[e] : 1ull;
    }
  else t = A.unmatched[e - A.nq];
  count[i] = ab;
  otu[i] = (uint32_t) (sorted_keys[i] >> 32);
  taxseq[i] = (t != VSX_OTUTAB_NO && A.t_tax_len[t] != VSX_OTUTAB_NO) ? e + 1u : 0u;
}

inline dim3 lanes(uint32_t n) { return dim3((n + 255u) / 256u); }
inline dim3 waves(uint32_t n) { return dim3((n + OTUTAB_WAVES - 1) / OTUTAB_WAVES); }

}  // namespace

extern "C" hipError_t vsx_launch_otutab_scan(VsxOtutabScan P, int targets, hipStream_t st)
{
  if (P.n == 0) return hipSuccess;
  if (targets) hipLaunchKernelGGL(vsx_otutab_scan_kernel<true>, waves(P.n), dim3(OTUTAB_THREADS), 0, st, P);
  else hipLaunchKernelGGL(vsx_otutab_scan_kernel<false>, waves(P.n), dim3(OTUTAB_THREADS), 0, st, P);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_iota(uint32_t n, uint32_t * d_idx, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_otutab_iota_kernel, lanes(n), dim3(256), 0, st, n, d_idx);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_sort(void * temp, size_t * temp_bytes, const uint64_t * d_keys_in, uint64_t * d_keys_out, const uint32_t * d_vals_in,
                                             uint32_t * d_vals_out, uint32_t n, uint32_t end_bit, hipStream_t st)
{
  return rocprim::radix_sort_pairs(temp, *temp_bytes, (const u64 *) d_keys_in, (u64 *) d_keys_out, d_vals_in, d_vals_out, (size_t) n, 0u, end_bit, st);
}

extern "C" hipError_t vsx_launch_otutab_heads(uint32_t n, const uint64_t * d_sorted_hash, const uint32_t * d_idx, const uint8_t * d_blob,
                                              const uint64_t * d_name_off, const uint32_t * d_name_len, uint32_t * d_flag, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_otutab_heads_kernel, waves(n), dim3(OTUTAB_THREADS), 0, st, n, (const u64 *) d_sorted_hash, d_idx, d_blob,
                     (const u64 *) d_name_off, d_name_len, d_flag);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_flagsum(void * temp, size_t * temp_bytes, const uint32_t * d_flag, uint32_t * d_incl, uint32_t n, hipStream_t st)
{
  return rocprim::inclusive_scan(temp, *temp_bytes, d_flag, d_incl, (size_t) n, rocprim::plus<uint32_t>(), st);
}

extern "C" hipError_t vsx_launch_otutab_groups(uint32_t n, const uint32_t * d_flag, const uint32_t * d_incl, const uint32_t * d_idx, const uint64_t * d_name_off,
                                               const uint32_t * d_name_len, uint32_t * d_group, uint32_t * d_rep_item, uint64_t * d_rep_off,
                                               uint32_t * d_rep_len, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_otutab_groups_kernel, lanes(n), dim3(256), 0, st, n, d_flag, d_incl, d_idx, (const u64 *) d_name_off, d_name_len, d_group,
                     d_rep_item, (u64 *) d_rep_off, d_rep_len);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_assign(uint32_t n, const uint32_t * d_group, const uint32_t * d_rank, const uint32_t * d_list, uint32_t * d_item_rank,
                                               uint32_t * d_label_rank, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_otutab_assign_kernel, lanes(n), dim3(256), 0, st, n, d_group, d_rank, d_list, d_item_rank, d_label_rank);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_keys(VsxOtutabAdds A, uint64_t * d_keys, uint32_t * d_vals, hipStream_t st)
{
  if (A.nq + A.nu == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_otutab_keys_kernel, lanes(A.nq + A.nu), dim3(256), 0, st, A, (u64 *) d_keys, d_vals);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_gather(VsxOtutabAdds A, const uint64_t * d_sorted_keys, const uint32_t * d_sorted_vals, uint64_t * d_count,
                                               uint32_t * d_otu, uint32_t * d_taxseq, hipStream_t st)
{
  if (A.nq + A.nu == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_otutab_gather_kernel, lanes(A.nq + A.nu), dim3(256), 0, st, A, (const u64 *) d_sorted_keys, d_sorted_vals, (u64 *) d_count,
                     d_otu, d_taxseq);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_otutab_reduce_cells(void * temp, size_t * temp_bytes, const uint64_t * d_keys, const uint64_t * d_count, uint32_t n,
                                                     uint64_t * d_unique, uint64_t * d_sum, uint32_t * d_n_unique, hipStream_t st)
{
  return rocprim::reduce_by_key(temp, *temp_bytes, (const u64 *) d_keys, (const u64 *) d_count, (size_t) n, (u64 *) d_unique, (u64 *) d_sum, d_n_unique,
                                rocprim::plus<u64>(), rocprim::equal_to<u64>(), st);
}

extern "C" hipError_t vsx_launch_otutab_reduce_tax(void * temp, size_t * temp_bytes, const uint32_t * d_otu, const uint32_t * d_taxseq, uint32_t n,
                                                   uint32_t * d_unique, uint32_t * d_max, uint32_t * d_n_unique, hipStream_t st)
{
  return rocprim::reduce_by_key(temp, *temp_bytes, d_otu, d_taxseq, (size_t) n, d_unique, d_max, d_n_unique, rocprim::maximum<uint32_t>(),
                                rocprim::equal_to<uint32_t>(), st);
}
