// vsx_lca.hip -- the last common ancestor of a query's hits on gfx950 (--lcaout, --lca_cutoff; include/vsx_lca.h).
//
//   split     one wavefront per label, 64 bytes per step, lane = byte, any length with the same loop.  The wave keeps the step's
//             bytes and the NEXT step's, so "tax=" is found from the ballots of its four letters shifted onto each other even
//             across a step's end; it counts where the byte before it is ';' or there is none, and the leftmost such place wins
//             (vsx_tax_split.h: the reference's loop finds the same).  The field ends at the first ';' at or behind its fifth
//             byte, else at the label's end.  A rank field begins at the field's first byte and behind every comma of the field
//             that still lies before its end; lane = that byte tests its rank letter (either case) and the ':' behind it.  Per
//             rank the LAST such field of a step wins and a later step overwrites: the reference's overwrite.  A name runs to the
//             next comma ANYWHERE in the label -- beyond the field's ';' too -- so a rank stays pending across steps until a step
//             holds a comma at or behind its start; what is pending at the label's end runs to the field's end.  Everything here
//             is wave-uniform (ballots).  Then the nine names are hashed: every lane mixes (position in the name, byte), the
//             lanes' values are ADDED by a butterfly (no dependence on how lanes and steps cut the name), the length is mixed in
//             and the level's hash is chained onto the level before: h_k stands for the names of levels 0 .. k.
//   number    rocPRIM's stable radix sort of the 9 n (h_k, 9 label + k); a run of equal hashes is numbered by the position of
//             its first entry (marks, an inclusive maximum).
//   verify    a lane per entry: its names of levels 0 .. k against those of its run's first entry, lengths and bytes.  Any
//             difference raises one flag (every writer stores the same 1), and the host then numbers the index itself: two
//             different prefixes never share a number and equal prefixes, having equal hashes, never get two.
//   vote      one wavefront per query, hits in lanes, 64 per step, counters carried across steps.  n_top from the lowest set bit
//             of ballot(id < id of the first hit): the reference breaks there, sorted or not.  Per level the candidate is the
//             bitwise majority of the top hits' 32-bit prefix numbers (32 ballots per step; lane b keeps the count of bit b): with
//             a strict majority that is its number, without one some value that at most half of the hits carry.  A second pass
//             counts the hits equal to the candidate and keeps the lowest.  A level without a strict majority ends the query:
//             no level above it can have one (its prefixes extend this level's), and lca_cutoff > 0.5 never prints it.
//
// Integer code (one double comparison), no atomics, no LDS: two calls give identical bytes.  Every result is written with plain
// vector stores.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "vsx_lca_internal.h"
#include "vsx_devutil.h"
#include "vsx_symbols.h"

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;
using vsxd::shfl_xor64;
using vsxsym::kGolden;
using vsxsym::kLengthMul;
using vsxsym::mix64;

#define LCA_WAVES   4
#define LCA_THREADS (64 * LCA_WAVES)

// bit i: position base + i is at or behind x
__device__ inline u64 ge_mask(u32 base, u32 x)
{
  if (x <= base) return ~0ull;
  if (x >= base + 64) return 0ull;
  return ~0ull << (x - base);
}

// bit p: "tax=" stands at byte p of the step (it may run into the next step's bytes)
__device__ inline u64 tax_mask(u32 cur, u32 next)
{
  const char kw[4] = { 't', 'a', 'x', '=' };
  u64 m = ~0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    {
      const u32 c = (u32) (unsigned char) kw[k];
      u64 w = (u64) __ballot(cur == c) >> k;
      if (k) w |= (u64) __ballot(next == c) << (64 - k);
      m &= w;
    }
  return m;
}

// the level of a rank letter in either case (d k p c o f g s t), or -1
__device__ inline int level_of(u32 c)
{
  if (c - 'A' < 26u) c |= 0x20u;
  const char ranks[LCA_LEVELS] = { 'd', 'k', 'p', 'c', 'o', 'f', 'g', 's', 't' };
  int r = -1;
#pragma unroll
  for (int k = 0; k < LCA_LEVELS; ++k) if (c == (u32) ranks[k]) r = k;
  return r;
}

__global__ __launch_bounds__(LCA_THREADS)
void vsx_lca_split_kernel(u32 n, const uint8_t * __restrict__ blob, const u64 * __restrict__ off, const u32 * __restrict__ len, u64 hash_mask,
                          int32_t * __restrict__ start_out, int32_t * __restrict__ len_out, u64 * __restrict__ key, u32 * __restrict__ idx)
{
  const u32 i = __builtin_amdgcn_readfirstlane(blockIdx.x * LCA_WAVES + (threadIdx.x >> 6));
  if (i >= n) return;
  const u32 lane = threadIdx.x & 63;
  const u32 L = len[i];                     // (the host refuses labels beyond INT32_MAX: positions fit 32 bits)
  const uint8_t * const s = blob + off[i];
  bool found = false, have_end = false;
  u32 p = 0, tax_end = 0;
  u64 before = 1;                        // bit 0: the byte before this step is ';', or there is none
  u64 carry = 0;                         // bit 0: the byte before this step is a comma of the field
  u32 st[LCA_LEVELS], ln[LCA_LEVELS];
  u32 pend = 0;                          // bit k: rank k has a start and waits for the comma that ends its name
#pragma unroll
  for (int k = 0; k < LCA_LEVELS; ++k) st[k] = ln[k] = 0;
  u32 cur = lane < L ? s[lane] : 0u;
  for (u32 base = 0; base < L; base += 64)
    {
      const u32 np = base + 64 + lane;
      const u32 next = np < L ? s[np] : 0u;                           // what lies behind the label reads as 0: no keyword, no ':' holds one
      const u64 valid = (u64) __ballot(base + lane < L);
      const u64 semi = (u64) __ballot(cur == (u32) ';') & valid;
      const u64 comma = (u64) __ballot(cur == (u32) ',') & valid;
      if (!found)
        {
          const u64 hits = tax_mask(cur, next) & ((semi << 1) | before);
          if (hits) { p = base + (u32) (__ffsll((long long) hits) - 1); found = true; }
        }
      if (found && !have_end)
        {
          const u64 m = semi & ge_mask(base, p + 4);
          if (m) { tax_end = base + (u32) (__ffsll((long long) m) - 1); have_end = true; }
        }
      if (found)
        {
          const u64 in_field = have_end ? ~ge_mask(base, tax_end) : ~0ull;      // no end yet: it lies behind this step
          const u64 cf = comma & ge_mask(base, p + 4);
          u64 fs = (cf << 1) | carry;
          if (p + 4 >= base && p + 4 < base + 64) fs |= 1ull << (p + 4 - base);
          fs &= in_field & valid;
          carry = cf >> 63;
          if (fs)
            {
              const u32 a = (u32) __shfl((int) cur, (int) ((lane + 1) & 63u)), n0 = (u32) __shfl((int) next, 0);
              const u32 after = lane < 63u ? a : n0;
              const bool field = ((fs >> lane) & 1ull) && after == (u32) ':';
              const int r = level_of(cur);
#pragma unroll
              for (int k = 0; k < LCA_LEVELS; ++k)
                {
                  const u64 mk = (u64) __ballot(field && r == k);
                  if (mk) { st[k] = base + (u32) (63 - __clzll((long long) mk)) + 2; ln[k] = 0; pend |= 1u << k; }
                }
            }
          if (pend)
            {
#pragma unroll
              for (int k = 0; k < LCA_LEVELS; ++k)
                if ((pend >> k) & 1u)
                  {
                    const u64 m = comma & ge_mask(base, st[k]);
                    if (m) { ln[k] = base + (u32) (__ffsll((long long) m) - 1) - st[k]; pend &= ~(1u << k); }
                  }
            }
        }
      before = semi >> 63;
      cur = next;
    }
  if (found && !have_end) tax_end = L;
#pragma unroll
  for (int k = 0; k < LCA_LEVELS; ++k) if ((pend >> k) & 1u) ln[k] = tax_end - st[k];
  // a name lies inside its label; were one not to, nothing is read through it and the host refuses the index (start < 0)
  bool inside = true;
#pragma unroll
  for (int k = 0; k < LCA_LEVELS; ++k) if (st[k] > L || ln[k] > L - st[k]) inside = false;
  if (!inside)
    {
#pragma unroll
      for (int k = 0; k < LCA_LEVELS; ++k) { st[k] = 0xFFFFFFFFu; ln[k] = 0; }
    }

  // the chained hashes; lane k keeps level k's values for the stores
  u64 h = 0, my_key = 0;
  int32_t my_st = 0, my_ln = 0;
#pragma unroll
  for (int k = 0; k < LCA_LEVELS; ++k)
    {
      u64 acc = 0;
      if (ln[k])                                                       // (wave-uniform)
        {
          for (u32 j = lane; j < ln[k]; j += 64) acc += mix64(((((u64) j + 1) << 8) | (u64) s[st[k] + j]) + kGolden);
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor64(acc, m);
        }
      h = mix64((h ^ mix64(acc ^ ((u64) ln[k] * kLengthMul))) + kGolden);
      if (lane == (u32) k) { my_key = h & hash_mask; my_st = (int32_t) st[k]; my_ln = (int32_t) ln[k]; }
    }
  if (lane < (u32) LCA_LEVELS)
    {
      const u64 e = (u64) i * LCA_LEVELS + lane;
      start_out[e] = my_st; len_out[e] = my_ln; key[e] = my_key; idx[e] = (u32) e;
    }
}

__global__ __launch_bounds__(256)
void vsx_lca_heads_kernel(u32 count, const u64 * __restrict__ sorted_key, u32 * __restrict__ mark)
{
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  mark[i] = (i > 0u && sorted_key[i] != sorted_key[i - 1u]) ? i : 0u;
}

__global__ __launch_bounds__(256)
void vsx_lca_verify_kernel(u32 count, const u32 * __restrict__ sorted_idx, const u32 * __restrict__ head, const uint8_t * __restrict__ blob,
                           const u64 * __restrict__ off, const int32_t * __restrict__ start, const int32_t * __restrict__ name_len,
                           u32 * __restrict__ id, u32 * __restrict__ differ)
{
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const u32 e = sorted_idx[i], hd = head[i], eh = sorted_idx[hd];
  id[e] = hd;
  if (e == eh) return;
  const u32 la = e / LCA_LEVELS, k = e % LCA_LEVELS, lb = eh / LCA_LEVELS;
  bool same = k == eh % LCA_LEVELS;
  const uint8_t * const sa = blob + off[la], * const sb = blob + off[lb];
  for (u32 j = 0; same && j <= k; ++j)
    {
      const u64 ea = (u64) la * LCA_LEVELS + j, eb = (u64) lb * LCA_LEVELS + j;
      const int32_t n = name_len[ea];
      if (n != name_len[eb]) { same = false; break; }
      const uint8_t * const a = sa + start[ea], * const b = sb + start[eb];
      for (int32_t x = 0; x < n; ++x) if (a[x] != b[x]) { same = false; break; }
    }
  if (!same) *differ = 1u;
}

__global__ __launch_bounds__(LCA_THREADS)
void vsx_lca_vote_kernel(u32 nq, const u64 * __restrict__ first, u64 hit0, const u32 * __restrict__ target, const double * __restrict__ hit_id,
                         const u32 * __restrict__ id, u64 maxhits, VsxLcaVote * __restrict__ out)
{
  const u32 q = __builtin_amdgcn_readfirstlane(blockIdx.x * LCA_WAVES + (threadIdx.x >> 6));
  if (q >= nq) return;
  const u32 lane = threadIdx.x & 63;
  const u64 h0 = first[q] - hit0, nh = first[q + 1] - first[q];
  const u64 toreport = (maxhits && maxhits < nh) ? maxhits : nh;
  u64 n_top = toreport;
  if (hit_id && toreport)
    {
      const double top = hit_id[h0];
      for (u64 b = 0; b < toreport; b += 64)
        {
          const u64 j = b + lane;
          const u64 m = (u64) __ballot(j < toreport && hit_id[h0 + j] < top);
          if (m) { n_top = b + (u64) (__ffsll((long long) m) - 1); break; }
        }
    }
  VsxLcaVote * const o = out + q;
  bool open = n_top > 0;
#pragma unroll 1
  for (int k = 0; k < LCA_LEVELS; ++k)
    {
      u32 matches = 0, firstm = VSX_LCA_NONE;
      if (open)
        {
          u32 cnt = 0;                                                   // lane b < 32: the top hits whose number has bit b
          for (u64 b = 0; b < n_top; b += 64)
            {
              const u64 j = b + lane;
              const u32 v = j < n_top ? id[(u64) target[h0 + j] * LCA_LEVELS + (u32) k] : 0u;
#pragma unroll
              for (u32 bit = 0; bit < 32u; ++bit)
                {
                  const u32 c = (u32) __popcll((u64) __ballot((v >> bit) & 1u));
                  if (lane == bit) cnt += c;
                }
            }
          const u32 cand = (u32) (u64) __ballot(lane < 32u && 2ull * cnt > n_top);
          for (u64 b = 0; b < n_top; b += 64)
            {
              const u64 j = b + lane;
              const bool hit = j < n_top && id[(u64) target[h0 + j] * LCA_LEVELS + (u32) k] == cand;
              const u64 m = (u64) __ballot(hit);
              if (m && firstm == VSX_LCA_NONE) firstm = (u32) (b + (u64) (__ffsll((long long) m) - 1));
              matches += (u32) __popcll(m);
            }
          if (2ull * matches <= n_top) { open = false; matches = 0; firstm = VSX_LCA_NONE; }
        }
      if (lane == 0) { o->matches[k] = matches; o->first[k] = firstm; }
    }
  if (lane == 0) o->n_top = (u32) n_top;
}

inline dim3 lanes(u32 n) { return dim3((u32) (((u64) n + 255u) / 256u)); }
inline dim3 waves(u32 n) { return dim3((u32) (((u64) n + LCA_WAVES - 1) / LCA_WAVES)); }

}  // namespace

extern "C" hipError_t vsx_launch_lca_split(uint32_t n, const uint8_t * d_blob, const uint64_t * d_off, const uint32_t * d_len, uint64_t hash_mask,
                                           int32_t * d_start, int32_t * d_name_len, uint64_t * d_key, uint32_t * d_idx, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_lca_split_kernel, waves(n), dim3(LCA_THREADS), 0, st, n, d_blob, (const u64 *) d_off, d_len, (u64) hash_mask, d_start, d_name_len,
                     (u64 *) d_key, d_idx);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_lca_sort(void * temp, size_t * temp_bytes, const uint64_t * d_kin, uint64_t * d_kout, const uint32_t * d_vin, uint32_t * d_vout,
                                          uint32_t count, uint32_t end_bit, hipStream_t st)
{
  if (end_bit == 0 || end_bit > 64) return hipErrorInvalidValue;
  return rocprim::radix_sort_pairs(temp, *temp_bytes, (const u64 *) d_kin, (u64 *) d_kout, d_vin, d_vout, (size_t) count, 0u, end_bit, st);
}

extern "C" hipError_t vsx_launch_lca_scan_max(void * temp, size_t * temp_bytes, const uint32_t * d_in, uint32_t * d_out, uint32_t count, hipStream_t st)
{
  return rocprim::inclusive_scan(temp, *temp_bytes, d_in, d_out, (size_t) count, rocprim::maximum<uint32_t>(), st);
}

extern "C" hipError_t vsx_launch_lca_heads(uint32_t count, const uint64_t * d_sorted_key, uint32_t * d_mark, hipStream_t st)
{
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_lca_heads_kernel, lanes(count), dim3(256), 0, st, count, (const u64 *) d_sorted_key, d_mark);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_lca_verify(uint32_t count, const uint32_t * d_sorted_idx, const uint32_t * d_head, const uint8_t * d_blob,
                                            const uint64_t * d_off, const int32_t * d_start, const int32_t * d_name_len, uint32_t * d_id,
                                            uint32_t * d_differ, hipStream_t st)
{
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_lca_verify_kernel, lanes(count), dim3(256), 0, st, count, d_sorted_idx, d_head, d_blob, (const u64 *) d_off, d_start, d_name_len,
                     d_id, d_differ);
  return hipGetLastError();
}

extern "C" hipError_t vsx_launch_lca_vote(uint32_t nq, const uint64_t * d_first, uint64_t hit0, const uint32_t * d_target, const double * d_hit_id,
                                          const uint32_t * d_id, uint64_t maxhits, VsxLcaVote * d_vote, hipStream_t st)
{
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(vsx_lca_vote_kernel, waves(nq), dim3(LCA_THREADS), 0, st, nq, (const u64 *) d_first, (u64) hit0, d_target, d_hit_id, d_id, (u64) maxhits,
                     d_vote);
  return hipGetLastError();
}
